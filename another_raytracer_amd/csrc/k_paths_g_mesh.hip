// k_paths_g_mesh.hip — the k_paths_g instantiations k_paths_g.h declares extern (cow: meshes with solid/checker
// textures whose BVH is not all in LDS), in their own object for the Makefile's MESH_SCHED scheduler.
#include "k_paths_g.h"

namespace art {
template __global__ void k_paths_g<kMeshG, kTexBasic, 0>(DevScene, PassGeom, CameraRec, Work, uint32_t*);
template __global__ void k_paths_g<kMeshG, kTexBasic, 2>(DevScene, PassGeom, CameraRec, Work, uint32_t*);
}  // namespace art

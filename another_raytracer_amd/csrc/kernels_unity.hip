// kernels_unity.hip — every kernel and the host code that reads the diagnostic device globals (g_art_stats,
// g_trace_*: one copy per object) in one translation unit: the Makefile's UNITY=1, for EXTRA=-DART_STATS / -DART_TRACE.
#include "kernels.hip"
#include "k_paths.hip"
#include "k_paths_g_mesh.hip"
#include "radiance_rays.hip"
#include "radiance_grad.hip"
#include "texel_grad.hip"
#include "tile_lists.hip"
#include "refit.hip"
#include "device_scene.hip"
#include "renderer.hip"

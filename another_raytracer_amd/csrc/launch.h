// launch.h — the host launchers the objects share.  The library is built without relocatable device code: a kernel
// lives in one object, and so does every host function that takes its address (hipLaunchKernelGGL, blocks_per_cu,
// static_lds_is_zero).  renderer.hip has no kernel of its own and launches through these.
#pragma once
#include <functional>

#include "device_scene.h"
#include "path_work.h"

namespace art {

// Extend variant: 0 = HBM scene, 1 = LDS scene, 2 = LDS scene with fused shading (no k_shade launches), 3 = persistent
// paths (k_paths: the fused LDS bounce loop in registers, one launch per pass), 4 = persistent paths over the HBM scene (k_paths_g).
enum ExtendVariant { EXT_GLOBAL = 0, EXT_LDS = 1, EXT_FUSED = 2, EXT_MEGA = 3, EXT_MEGA_G = 4 };
// The variant for this scene and these flags (RT_GLOBAL_SCENE / RT_SPLIT_SHADE / RT_WAVEFRONT force the general kernels).
int extend_variant(const DeviceScene& ds, int flags);
// Which persistent-path kernel a render ran (rt_stats.kernel_*): k_paths_g<F, TF, LM>, or k_paths as LM 3
struct KernelId {
    uint32_t f = 0, tf = 0;
    int lm = -1;
};

// kernels.hip
bool static_lds_is_zero(const void* kernel);
int blocks_per_cu(const void* kernel, int block, size_t lds);
KernelId launch_paths_g(uint32_t feat, bool tex_basic, bool tex_bary, bool codes16, uint32_t leaf_shift, int num_cu, hipStream_t st,
                        const DevScene& S, const PassGeom& g, const CameraRec& cam, const Work& w, uint32_t* next_slot);
void bounce(const DeviceScene& ds, int variant, int num_cu, hipStream_t st, const PassGeom& g, const CameraRec& cam,
            const Work& w, int d, const std::function<void()>& mark);
void launch_accum(hipStream_t st, const PassGeom& g, const Work& w, double* qsum, uint32_t m);  // qsum: k_accum_images, or null
void launch_finalize(hipStream_t st, const double* acc, uint8_t* rgb, uint32_t n, int spp);
void launch_adapt_corners(hipStream_t st, uint32_t* list, int W, int sqx, uint32_t nsq);
void launch_adapt_store(hipStream_t st, const uint32_t* list, uint32_t n, const double* acc, int spp, int32_t* work);
void launch_adapt_accum(hipStream_t st, const uint32_t* list, uint32_t cap, const ResRec* res, uint32_t k, int spp, int32_t* work);
void launch_adapt_level(hipStream_t st, int level, int32_t* work, int W, int sqx, uint32_t nsq, uint8_t* f0, uint8_t* f1, uint8_t* f2, uint32_t* list,
                        uint32_t* count);
void launch_adapt_fill(hipStream_t st, int32_t* work, uint8_t* rgb, int W, int rows, int sqx, const uint8_t* f0, const uint8_t* f1, const uint8_t* f2);
void launch_trace_rays(const DeviceScene& ds, bool global_scene, hipStream_t st, const double* rays, uint32_t n, double* t_out, double* n_out);
// rt_query_rays: closest hits with the record (hits: n x 12) / occlusion bytes; t_max may be null (+inf)
void launch_query_rays(const DeviceScene& ds, bool global_scene, hipStream_t st, const double* rays, const double* t_max, uint32_t n,
                       bool no_media, double* hits);
void launch_occlude_rays(const DeviceScene& ds, bool global_scene, hipStream_t st, const double* rays, const double* t_max, uint32_t n,
                         uint8_t* occluded);
void launch_guides(const DeviceScene& ds, int flags, hipStream_t st, const GuideGeom& g, const CameraRec& cam, double* guides,
                   double* rays);
// radiance_rays.hip
// One rt_radiance_rays call as its kernels see it.  Path p = i * spp + s (ray i, sample s) of P = n * spp <= kMaxPassSlots.
struct RadianceJob {
    const double* rays;            // n x 7
    const uint64_t* rng;           // P PCG states, or null: pcg_seed(seed, id_base + i, sample_base + s)
    double* radiance;              // n x 3; written by k_radiance_rays itself when res is null (spp == 1)
    ResRec* res;                   // P per-path records for k_radiance_sum (spp > 1), or null
    uint32_t* next;                // the claim counter, zeroed before the launch
    unsigned long long* segments;  // zeroed before the launch
    uint32_t P, spp, chunk;        // chunk: paths per claim (path_chunk)
    uint32_t sample_base, id_base;
    uint32_t stack;                // LDS traversal stack rows per lane (stack_rows)
    int32_t max_depth;
    uint64_t seed_mix;             // splitmix64(seed), as PassGeom::seed_mix
    FastDiv fd_spp;                // / spp
};
// The persistent path kernel over the job's paths with `background` on a miss (flags: RT_GLOBAL_SCENE), then the per-ray
// sums when job.res is set.
void launch_radiance_rays(const DeviceScene& ds, int flags, int num_cu, hipStream_t st, const RadianceJob& job, uint32_t n, const double background[3]);
// k_radiance_sum alone: radiance[i] = +0.0 + the spp records of ray i in sample order (rt_radiance_grad's sums)
void launch_radiance_sum(hipStream_t st, const ResRec* res, uint32_t n, uint32_t spp, double* radiance);
// One launch of rt_render_views as its kernels see it: a group of whole views of one W x H x spp frame.  Path
// p = ((v * npix + pixel) * spp + s) of P = views * npix * spp <= kMaxPassSlots, pixel = ly * W + lx (row-major: p is
// also the index of the path's record, and p / spp the pixel's place in the group's sums).
struct ViewRec {  // a view of the table: its camera and splitmix64(its seed), PassGeom::seed_mix per view
    CameraRec cam;
    uint64_t seed_mix;
};
struct ViewsJob {
    const ViewRec* views;          // the group's views
    double* radiance;              // the group's pixels x 3; written by k_radiance_views itself when res is null (spp == 1)
    ResRec* res;                   // P per-path records for k_radiance_sum (spp > 1), or null
    uint32_t* next;                // the claim counter, zeroed before the launch
    unsigned long long* segments;  // the kernel adds its segments: zeroed before the first group
    uint32_t P, spp, chunk;
    uint32_t npix;                 // W * H
    uint32_t stack;
    int32_t max_depth;
    int32_t W, H;
    double inv_w1, inv_h1;         // PassGeom's: RN(1 / (W - 1)), RN(1 / (H - 1))
    FastDiv fd_spp, fd_npix, fd_w;  // / spp, / npix, / W
};
// The persistent path kernel over the job's paths with `background` on a miss (flags: RT_GLOBAL_SCENE), then the sums
// of the job's npixels = views * npix pixels when job.res is set.
void launch_radiance_views(const DeviceScene& ds, int flags, int num_cu, hipStream_t st, const ViewsJob& job, uint32_t npixels, const double background[3]);
// radiance_grad.hip
// One vertex of a path as k_radiance_grad records it where the path scatters, for the walk back from the path's end:
// P = the throughput before the vertex (P_j), a = its attenuation (a_j), row = the accumulator row the attenuation came
// from (kGradNoRow: none).  Vertex j of the lane with grid-wide index g is verts[j * lanes + g].
struct GradVertex {
    double P[3], a[3];
    uint32_t row, pad[3];
};
static_assert(sizeof(GradVertex) == 64, "GradVertex is one 64-B line");
constexpr uint32_t kGradNoRow = 0xFFFFFFFFu;
constexpr uint32_t kGradRowLimbs = 10;   // a row of the accumulator: 3 colours x 3 limbs (grad_fixed.h), then the NaN flag
constexpr uint32_t kGradMaxCopies = 64;  // copies of the accumulator table, one per block index modulo the count
// One rt_radiance_grad call as its kernels see it: rt_radiance_rays' job (radiance and res may both be null: no radiance
// asked for), the adjoints and the accumulators.  Rows: texture t is row t, material m row n_texs + m, the background
// row n_texs + n_mats; rows = n_texs + n_mats + 1.
struct GradJob {
    RadianceJob path;
    const double* weights;         // n x 3
    GradVertex* verts;             // lanes x max(max_depth - 1, 1) records
    unsigned long long* acc;       // copies x rows x kGradRowLimbs, zeroed before the launch; null (and verts): radiance only
    uint32_t rows, copies, n_texs;
    uint32_t lanes;                // grid blocks x block size
};
// The persistent grid of the call's kernel (blocks of kBlock lanes): every block the CUs hold at once, or fewer when the
// job has fewer paths.  The workspace is sized by it.
uint32_t radiance_grad_grid(const DeviceScene& ds, int num_cu, uint32_t P, uint32_t stack);
// The path kernel over `grid` blocks (job.lanes = grid * kBlock) with `background` on a miss, the per-ray sums when
// job.path.res is set, then k_grad_finish: the accumulators, summed over the copies and rounded once, into the colour
// columns of grad_textures (n_texs x 4), grad_materials (n_mats x 5) and grad_background (3); the other columns +0.0.
// Any of the three may be null.
void launch_radiance_grad(const DeviceScene& ds, hipStream_t st, const GradJob& job, uint32_t grid, uint32_t n, const double background[3],
                          uint32_t n_mats, double* grad_textures, double* grad_materials, double* grad_background);
// k_grad_finish alone (nothing when the three outputs are null): what follows launch_texel_grad's path kernel too
void launch_grad_finish(hipStream_t st, const GradJob& job, uint32_t n_mats, double* grad_textures, double* grad_materials, double* grad_background);
// texel_grad.hip
// One rt_radiance_grad_texels call with a texel output as k_texel_grad sees it: rt_radiance_grad's job, and the texel
// rows.  Global texel t (art.h: first_k + j * w_k + i) is row g.rows + t of a GradVertex and row t of the texel table,
// which has its own copy count (Renderer::radiance_grad keeps the table within a byte budget); a block adds to copy
// blockIdx.x % texel_copies.  image_row[k] = g.rows + first_k, or kGradNoRow for an image with bpp < 3.
struct TexelJob {
    GradJob g;
    unsigned long long* texel_acc;  // texel_copies x n_texels x kGradRowLimbs, zeroed before the launch
    const uint32_t* image_row;      // one entry per image of the scene
    uint32_t n_texels, texel_copies;
};
constexpr size_t kTexelTableBudget = size_t(256) << 20;  // bytes of texel rows over all copies, unless one copy is more
// Whether the scene's kernel has a texel form (a scene of solid and checker textures only has no image: its call is
// launch_radiance_grad's), and that kernel's persistent grid, as radiance_grad_grid
bool texel_grad_kernel(const DeviceScene& ds);
uint32_t texel_grad_grid(const DeviceScene& ds, int num_cu, uint32_t P, uint32_t stack);
// k_texel_grad over `grid` blocks, the per-ray sums, k_grad_finish, then k_texel_finish: the texel table summed over
// its copies and rounded once into grad_texels (n_texels x 3; null: not launched)
void launch_texel_grad(const DeviceScene& ds, hipStream_t st, const TexelJob& job, uint32_t grid, uint32_t n, const double background[3],
                       uint32_t n_mats, double* grad_textures, double* grad_materials, double* grad_background, double* grad_texels);
// rt_camera_rays: entry (ly * W + lx) * g.k + j = cam_ray of local pixel (lx, ly), sample g.sample_base + j (rng may be null)
void launch_camera_rays(hipStream_t st, const PassGeom& g, const CameraRec& cam, double* rays, uint64_t* rng);
// k_paths.hip
void launch_paths(int num_cu, hipStream_t st, const DevScene& S, const PassGeom& g, const CameraRec& cam, const Work& w,
                  uint32_t* next_slot);
// tile_lists.hip: fills one TileRec (tile_lists.h) per 8x8 tile of g's frame geometry for `cam`; S holds an LDS scene
// image with representative slots (DeviceScene::tile_reps > 0)
void launch_tile_lists(hipStream_t st, const DevScene& S, const PassGeom& g, const CameraRec& cam, void* tiles);
// refit.hip
// One rt_scene_update_triangles call as k_update_tris sees it: new vertices p (9 doubles each) for triangles
// [first, first + n), written into every array of the uploaded scene that holds one.
struct UpdateJob {
    const double* p;
    uint32_t first, n;
    const uint32_t* primrefs;      // the device copy (pair-aligned where the scene runs an F_LEAF2 kernel)
    const ObjRec* objs;
    uint32_t n_slots, n_objs;
    TriRec* tris;
    TriRec* leaf_tris;
    TriRec112* leaf_tris112;
    PrimRec80* leaf_prims;
    PrimRec80* obj_prims;
    double* slot_box;              // 6 doubles per slot: the f64 box of its primitive (refit.h)
};
void launch_update_tris(hipStream_t st, const UpdateJob& j);
// One rt_scene_update_spheres call as k_update_spheres sees it: new (cx, cy, cz, r) s for spheres [first, first + n),
// written into every array of the uploaded scene that holds one, the LDS scene image (null: none) included.
struct SphereJob {
    const double* s;
    uint32_t first, n;
    const uint32_t* primrefs;
    const uint8_t* slot_pad;       // 1: slot i belongs to no leaf (DeviceScene::slot_pad)
    const ObjRec* objs;
    uint32_t n_slots, n_objs;
    SphereRec* spheres;
    PrimRec80* leaf_prims;
    PrimRec80* obj_prims;
    double* slot_box;
    uint8_t* image;
};
void launch_update_spheres(hipStream_t st, const SphereJob& j);
// k_image_nodes: the nine box planes of every node of the LDS scene image from the (refitted) nodes
void launch_image_nodes(hipStream_t st, uint8_t* image, const BvhNode* nodes, uint32_t n_nodes);
// One rt_scene_update_materials / rt_scene_update_textures call as its kernels see it.  k_update_materials (m: 5 doubles
// per material -- albedo, fuzz, ir) and k_update_textures (t: 4 per texture -- colour, scale) write the fields a record's
// type takes into records [first, first + n); k_derive_materials then runs over all n_mats materials: a MATF_SOLID
// record's albedo from its texture, and with an image the shading-table entries of every material that has one
// (entry: lds_image.h image_material_entries' codes on the device, null without an image).
struct AppearanceJob {
    const double* v;
    uint32_t first, n;
    MatRec* mats;
    TexRec* texs;
    uint32_t n_mats;
    const int32_t* entry;
    uint8_t* image;
};
void launch_update_materials(hipStream_t st, const AppearanceJob& j);
void launch_update_textures(hipStream_t st, const AppearanceJob& j);
// One rt_scene_update_rects / rt_scene_update_boxes call as k_update_rects / k_update_boxes see it: new values v (5
// doubles per rect -- a0, a1, b0, b1, k -- or 6 per box -- min xyz, max xyz) for records [first, first + n), written
// into every array of the uploaded scene that holds one (axis and mat stay).  A scene without a BVH has no slots:
// n_slots 0, and only the records and obj_prims are written.
struct RigidJob {
    const double* v;
    uint32_t first, n;
    const uint32_t* primrefs;
    const uint8_t* slot_pad;
    const ObjRec* objs;
    uint32_t n_slots, n_objs;
    RectRec* rects;                // k_update_rects
    BoxRec* boxes;                 // k_update_boxes
    PrimRec80* leaf_prims;
    PrimRec80* obj_prims;
    double* slot_box;
};
void launch_update_rects(hipStream_t st, const RigidJob& j);
void launch_update_boxes(hipStream_t st, const RigidJob& j);
// One rt_scene_update_objects call as k_update_objects sees it: new p (4 doubles each) for objects [first, first + n);
// a record takes what its kind uses (a translate p[0..2], a rotate_y p[0..1], a medium p[0]; a prim and a BVH nothing)
struct ObjectJob {
    const double* v;
    uint32_t first, n;
    ObjRec* objs;
};
void launch_update_objects(hipStream_t st, const ObjectJob& j);
// k_refit_level over every level [level_begin[l], level_begin[l + 1]) (refit.h refit_levels), the deepest first
void launch_refit_levels(hipStream_t st, BvhNode* nodes, uint32_t n_nodes, const double* slot_box, uint32_t n_slots,
                         const std::vector<uint32_t>& level_begin);
size_t pool_bytes(int variant, int num_cu);  // the path pools of `variant` (k_paths' PathPool, kPoolCap entries per wave; 0 for every other)

}  // namespace art

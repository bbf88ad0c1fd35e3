/* include/art.h — C ABI of the MI355X path tracer (libart.so).
 *
 * Drop-in boundary for the hot path of blackccpie/another_raytracer: what `src/main.cpp:29-46` does with the
 * reference's scene_manager / camera / engine classes maps onto these calls.  Plain pointers and sizes only; no C++,
 * torch or HIP types cross this boundary (a hipStream_t travels as void*).  No exceptions cross it: every call returns
 * RT_OK (0) or a negative RT_E* code, with a message in rt_last_error() (thread-local).
 *
 *   reference (file:line)                                        replacement
 *   scene scene_manager::build(scene_alias)  scene_manager.cpp:260  rt_scene_build(name, assets, device, &scene)
 *   struct scene {lookfrom, lookat, vfov, aperture, background}   rt_scene_info(scene, &info)
 *     scene_manager.h:6-14
 *   camera::camera(lookfrom, lookat, vup, vfov, aspect, aperture, rt_camera (POD, same 9 arguments)
 *     focus_dist, t0, t1)                camera.h:8-36
 *   engine<W,H,C>(const camera&, engine_mode)  engine.h:22        rt_params (W, H, spp, max_depth are runtime here:
 *   engine::set_scene(hittable_list, color)   engine.h:24-28       tracer_constants.h:6-14 made them compile-time)
 *   int engine::run(uint8_t* out)             engine.h:30-54      rt_render(scene, &cam, &params, out_rgb8, ...)
 *   write_color (gamma 2, clamp, quantize)    color.h:6-22        inside rt_render (f64 sums -> RGB8, row 0 = top)
 *   hittable constructors (sphere.h, moving_sphere.h, triangle.h, rt_graph_* (one call per constructor, same
 *     aarect.h, box.h, hittable_list.h, bvh.h, hittable.h,          arguments); rt_graph_compile -> rt_scene
 *     constant_medium.h, material.h, texture.h)
 *   bool mesh::parse(path)                    mesh.h:31-65        rt_mesh_parse(path, &triangles, &shapes)
 *   hittable_list mesh::build()               mesh.h:67-145       rt_mesh_build(graph, path, &first_id)
 *   imageio::load_image (stbi_load)          imageio.cpp:11-15   rt_image_load(path, &w, &h, &c, &pixels)
 *   engine::_run_parallel_stripes (threads)  engine.h:335-376    rt_multi_create + rt_render_multi (GPUs, RCCL)
 *   dynamic_gui refresh per row / square     gui.cpp:25-58,      rt_render_progressive(..., callback, user, ...)
 *                                            engine.h:88,307,353
 *   hittable_list::hit(r, 0.001, inf, rec)   hittable_list.cpp:5 rt_trace_rays(scene, rays, n, flags, t, normals)
 *   hittable_list::hit(r, t_min, t_max, rec)  hittable_list.cpp:5 rt_query_rays(scene, &q, rays, t_max, n, hits, occluded): the
 *     with the full hit_record                hittable.h:9-23       whole record per ray (t_min = 0.001), or any-hit occlusion
 *   _ray_color(r, background, world, depth)  engine.h:447-466    rt_radiance_rays(scene, &q, rays, rng, n, radiance, stats): the
 *     for a ray the caller made                                      recursion along caller-given rays, summed over spp samples
 *   _stochastic_sample's camera draws and     engine.h:58-68,     rt_camera_rays(&cam, &params, sample_base, device, rays, rng): the
 *     camera::get_ray                         camera.h:38-47        renderer's camera rays and post-camera RNG states as data
 *   one engine::run per camera of a scene     main.cpp:29-46      rt_render_views(scene, cams, seeds, nviews, &params, rgb8, accum,
 *     (an orbit, a cube map, a light field)                          stats): every view in one persistent launch, rt_render's bits
 *   (scene construction every run)           scene_manager.cpp,  rt_scene_save / rt_scene_load (flat-scene files)
 *                                            mesh.h, bvh.cpp
 *   (none: a scene is rebuilt every run)                          rt_scene_update_triangles (new vertices for a compiled
 *                                                                    scene's triangles, BVH boxes refitted on the device)
 *                                                                  rt_scene_update_spheres (new centres and radii; the BVH
 *                                                                    boxes and the LDS scene image refitted on the device)
 *                                                                  rt_scene_update_materials, rt_scene_update_textures
 *                                                                    (new colours, fuzz, ir, noise scale; every device
 *                                                                    copy of them refreshed, the image's shading table too)
 *                                                                  rt_scene_update_rects, rt_scene_update_boxes (new
 *                                                                    extents, BVH boxes refitted), rt_scene_update_objects
 *                                                                    (where a translate / rotate_y instance stands and how
 *                                                                    it is turned, a constant_medium's density)
 *   (none: engine_mode::adaptive interpolates     engine.h:96-333  rt_render_guides + rt_denoise, or rt_render_denoised
 *    untraced pixels; there is no denoiser)                          (first-hit guides, variance-guided a-trous filter)
 *   (none: tracer_constants::samples_per_pixel is   tracer_constants.h:12  rt_render_noise_target (per-pixel sample counts:
 *    one compile-time count for every pixel)                          every pixel is traced until its noise target, up to spp)
 *
 * RNG contract: the reference draws from one global std::mt19937 (tracer_utils.h:27-31).  Scene construction here
 * replays that generator exactly (seed 5489, same draw order), so scenes are bit-identical.  Rendering draws come
 * from PCG32 streams keyed by (seed, global pixel j*W+i, sample index): results depend on neither the tiling nor the
 * GPU count, and oracle/restate.cpp (ORC_PCG) replays the same streams on the CPU.
 */
#ifndef ART_H
#define ART_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 2: rt_params.fp_mode 0 = RT_FP64 (the only arithmetic: the reference's IEEE double), rt_scene_info's f32 byte count
 * dropped, rt_multi_* (multi-GPU render over RCCL), rt_render_progressive, rt_scene_save / rt_scene_load, rt_image_load.
 * ABI 3 (additive): rt_band_block_rows, rt_unpack_bands (the gather layout for callers that move the bands themselves,
 * e.g. one process per GPU over torch.distributed), rt_multi_ngpus, rt_multi_scene_info, rt_multi_device_stats.
 * ABI 4: rt_unpack_bands takes the byte sizes of both buffers and refuses a mismatch with the layout; rt_multi_times
 * (per-phase timing of the last rt_render_multi: renders, gather, unpack); rt_render_multi bounds its wait on the
 * collective (RT_E_DEVICE on an RCCL error or timeout, after which the rt_multi refuses further renders).
 * ABI 5: rt_option_set / rt_option_get (process-wide options; the library reads no environment knobs but the documented
 * ART_MULTI_TIMEOUT_MS); rt_stats.kernel_features / kernel_textures / kernel_lds_mode name the persistent kernel a
 * render ran; rt_multi_create uploads the scene to every device before it returns.
 * Additive since ABI 5 (the version stays 5): rt_render_guides, rt_denoise, rt_render_denoised, rt_denoise_params,
 * RT_GUIDE_DOUBLES, RT_DN_NO_DEMODULATE; rt_render_noise_target, rt_noise_params, rt_noise_result; rt_query_rays,
 * rt_query_params, RT_Q_ANY_HIT, RT_Q_NO_MEDIA, RT_HIT_DOUBLES (ray queries with the hit record, a per-ray t_max, occlusion
 * queries, device buffers and a caller's stream), option query.any_sorted; rt_radiance_rays, rt_radiance_params (path-traced
 * radiance along caller-given rays), rt_camera_rays (the renderer's camera rays and post-camera RNG states as data);
 * rt_render_views (many cameras of one scene in one persistent launch), option views.max_paths; rt_tile_candidates (the
 * per-tile sphere lists of a render, as counts), option render.tile_lists; rt_scene_update_triangles, rt_update_params,
 * rt_scene_triangles_get, rt_scene_bvh_get (new vertices for a compiled scene's triangles and a BVH refit on the device);
 * rt_scene_update_spheres, rt_scene_spheres_get, rt_scene_lds_image_get (new centres and radii for its spheres);
 * rt_scene_update_materials, rt_scene_update_textures, rt_scene_materials_get, rt_scene_textures_get, RT_MATERIAL_DOUBLES,
 * RT_TEXTURE_DOUBLES, RT_MAT_*, RT_TEX_* (new values for its materials and textures); rt_scene_update_rects,
 * rt_scene_update_boxes, rt_scene_update_objects, rt_scene_rects_get, rt_scene_boxes_get, rt_scene_objects_get,
 * RT_RECT_DOUBLES, RT_BOX_DOUBLES, RT_OBJECT_DOUBLES, RT_OBJ_* (new extents for its rects and boxes, new offsets, angles
 * and densities for its translate, rotate_y and constant_medium objects); rt_radiance_grad (the exact gradient of
 * rt_radiance_rays' radiance with respect to the solid texture colours, the metal albedos and the background). */
#define RT_ABI_VERSION 5

/* return codes */
#define RT_OK 0
#define RT_E_INVALID (-1)   /* bad argument */
#define RT_E_SCENE (-2)     /* scene build / compile failure (e.g. "Invalid input scene!", engine.h:32-36) */
#define RT_E_DEVICE (-3)    /* HIP runtime failure or no device */
#define RT_E_INTERNAL (-4)

/* rt_params.fp_mode: arithmetic of the leaf tests and shading.  RT_FP64 (= 0, so a zero-initialised rt_params gets it)
 * is the reference's own IEEE double and the only mode: ABI 1's experimental RT_FP32 self-intersected on the
 * reference's r = 1000 / r = 5000 spheres and is gone (any other value is RT_E_INVALID).  The BVH box tests are
 * conservative f32 in every mode; they never decide a hit. */
#define RT_FP64 0
/* rt_params.flags */
#define RT_OUT_DEVICE 1     /* out_rgb8 / out_accum are device pointers (on the scene's device) */
#define RT_PROFILE 2        /* time every extend/shade launch with HIP events (rt_stats.*_ms) */
#define RT_GLOBAL_SCENE 4   /* never use the LDS-resident scene variant of the extend kernel (A/B and parity tests) */
#define RT_SPLIT_SHADE 8    /* never fuse shading into the extend kernel: one k_shade launch per material (A/B, tests) */
#define RT_ADAPTIVE 16      /* engine_mode::adaptive (engine.h:96-333): trace the corners of 12/6/3-px squares, subdivide
                               where neighbouring corners differ by > 100 (squared gamma-corrected RGB), interpolate
                               the rest.  Width and local rows must be multiples of 12 (the reference throws
                               std::logic_error otherwise: RT_E_INVALID here), band_rows a multiple of 12 when
                               band_count > 1, and out_accum NULL (interpolated pixels have no radiance sums). */
#define RT_WAVEFRONT 32     /* LDS-scene renders: one fused extend launch per bounce depth (paths stored in HBM between
                               bounces) instead of the persistent-path kernel (A/B and parity tests) */
#define RT_PARALLEL_IMAGES 64 /* engine_mode::parallel_images (engine.h:378-445): four partial images of spp/4 samples
                               each (samples [q*spp/4, (q+1)*spp/4) of every pixel's streams), every pixel's partial
                               sum rounded to float (write_color_raw<float>), the four summed in double and written
                               with the full spp -- the reference's float rounding and its spp/4 truncation included.
                               out_accum receives that sum.  Not with RT_ADAPTIVE or progressive rendering. */

typedef struct rt_scene rt_scene;
typedef struct rt_graph rt_graph;

typedef struct rt_camera {      /* camera.h:8-18 constructor arguments */
    double lookfrom[3];
    double lookat[3];
    double vup[3];
    double vfov;                /* vertical field of view, degrees */
    double aspect;              /* aspect ratio (the reference hard-codes 4:3 in main.cpp:35) */
    double aperture;
    double focus_dist;          /* main.cpp:34 uses 10 */
    double time0, time1;        /* shutter; main.cpp:35 uses 0, 1 */
} rt_camera;

typedef struct rt_params {
    int32_t width, height;      /* full image */
    int32_t spp;                /* samples per pixel (tracer_constants.h:12) */
    int32_t max_depth;          /* bounce limit (tracer_constants.h:13; 50) */
    uint64_t seed;              /* render RNG seed */
    int32_t fp_mode;            /* RT_FP64 (0) */
    int32_t band_rows;          /* row-interleaved partition: global row y belongs to band (y / band_rows) and */
    int32_t band_count;         /*   is rendered here when band % band_count == band_index; (H, 1, 0) = whole image */
    int32_t band_index;
    int32_t samples_per_pass;   /* 0 = auto: the largest pass whose path state fits half of the free device memory */
    int32_t flags;              /* RT_OUT_DEVICE | RT_PROFILE | RT_GLOBAL_SCENE */
    void* stream;               /* hipStream_t to run on, or NULL for the scene's own stream */
    double background[3];       /* engine::set_scene(world, background) (engine.h:24-28): returned on a miss */
} rt_params;

typedef struct rt_stats {
    uint64_t segments;          /* rays traced through the world (world.hit calls): the metric's unit */
    uint64_t primary;           /* camera rays = local pixels * spp */
    double ms;                  /* device time, first kernel -> finalized RGB8 (HIP events) */
    double extend_ms, shade_ms; /* RT_PROFILE only: summed launch durations */
    uint64_t extend_launches, shade_launches;
    int32_t passes, samples_per_pass, local_rows;
    int32_t extend_variant;     /* 0: scene read from HBM; 1: LDS-resident scene (spheres-only scene that fits);
                                   2: LDS-resident scene with shading fused into the extend kernel (one launch per
                                   depth); 3: persistent paths (the fused bounce loop in registers, one launch per pass);
                                   4: persistent paths over the HBM scene (every other scene; k_paths_g) */
    uint32_t kernel_features;   /* the persistent kernel that ran (variants 3, 4): k_paths_g<kernel_features, */
    uint32_t kernel_textures;   /*   kernel_textures, kernel_lds_mode> (layout.h feature / texture bits; LDS mode 0: BVH */
    int32_t kernel_lds_mode;    /*   in HBM, 1: whole BVH in LDS, 2: its top levels in LDS), or k_paths (LDS mode 3, the */
                                /*   LDS scene image); -1 for the per-depth wavefront variants */
} rt_stats;

typedef struct rt_scene_info {  /* scene_manager.h:6-14 */
    double lookfrom[3], lookat[3];
    double vfov, aperture;
    double background[3];
    int64_t spheres, triangles, rects, boxes, bvh_nodes, objects, materials, textures;
    int32_t has_media, max_bvh_depth;
    uint64_t device_bytes_f64;  /* scene bytes uploaded to the device (0 before the first render) */
} rt_scene_info;

/* ---- library ---- */
int rt_abi_version(void);
const char* rt_last_error(void);
int rt_device_count(void);
/* Process-wide options, by name (every one is also readable with rt_option_get).  The library reads no environment
 * variables for them (only multi.timeout_ms falls back to ART_MULTI_TIMEOUT_MS while never set).  Unknown names and
 * values outside an option's range are RT_E_INVALID; name NULL resets every option to its default.
 *   compile.world_merge (2: 0 off, 1 BVH runs only), compile.hoist (1), bvh.collapse (0 greedy, 1 SAH-optimal DP),
 *   bvh.collapse_ci (0.6), bvh.dp_binary_leaf (1), bvh.sah_ci (1.5), bvh.sah_leaf (4), bvh.sbvh (1.5), bvh.sbvh_alpha
 *   (1e-5): scene compilation, for scenes built after the call (builder experiments; the defaults are what was measured
 *   best);
 *   render.codes16 (1; 0 = always the 32-bit-child-code kernels), render.leaf2 (1; 0 = no pair-aligned leaves: a mesh
 *   of more than 8192 references takes the 32-bit-code kernels), render.tex_bary (1; 0 = meshes whose only images are
 *   barycentric take the all-textures kernels), render.lds_nodes_max (diagnostic cap on LDS nodes): uploads and
 *   renders after the call (kernel-selection switches for A/B; images are identical either way);
 *   denoise.lds_iterations (2; how many of rt_denoise's first iterations -- tap spacings 1, 2 -- read their taps from an
 *   LDS tile instead of loading each directly; 0..2, the result is identical either way);
 *   query.any_sorted (0; rt_query_rays' any-hit walk takes a node's children in node order, without the closest search's
 *   sorting network; 1 = nearest first; the answers are identical either way, DESIGN.md 4.7 measured both);
 *   views.max_paths (0 = off; N caps the paths of one rt_render_views launch, so the views run in groups of
 *   floor(N / (width * height * spp)) views, at least one; diagnostic: the frames are identical either way);
 *   render.tile_lists (1; the batches of 64 camera rays of the LDS-scene path kernel test a per-tile list of the spheres
 *   their 8x8 tile can reach instead of walking the tree: 0 = off, 1 = when a pass holds at least 72 samples per pixel, so
 *   that the table's one launch per rt_render call is below 1 % of it, 2 = always; the frames are identical either way);
 *   render.accum_overlap (1; a whole-image pass of the LDS-scene path kernel runs as two launches and the first one's
 *   radiance records are summed on a second stream while the second, the pass's last 128 samples, traces: 0 = off, 1 =
 *   when those records are at least 8 GiB and samples_per_pass is 0, 2 = whenever a pass holds two samples or more; the
 *   frames are identical either way; rt_stats.passes and extend_launches count both launches of a split pass);
 *   grad.texel_copies (0; the copies of rt_radiance_grad_texels' texel accumulator table: 0 = as many as its 256 MiB
 *   budget holds, 1..64 = that many, never more than the call's grid has blocks; the gradients are identical either way);
 *   multi.timeout_ms (the RCCL deadline; inf = none), multi.rccl_blocking (0; 1 = blocking communicators, diagnosis:
 *   gives up the deadline and the error-path protection);
 *   test.fault_workspace_bytes (0 = off; N refuses workspace growth beyond N bytes), test.fault_gather_abort (0; 1 = the
 *   next gather fails in flight), test.fault_rccl_group (0; 1 / 2 = an error inside rt_multi_create's / the gather's
 *   RCCL group): fault points for the tests, each failing a later call exactly as the real fault would. */
int rt_option_set(const char* name, double value);
int rt_option_get(const char* name, double* value);

/* ---- scenes ---- */
/* Builtin scenes = scene_manager::build(alias): "1".."8" or "random", "two_spheres", "two_perlin_spheres", "earth",
 * "simple_light", "cornell_box", "cornell_smoke", "final"; plus "c1" (SURVEY Q7 3-sphere scene), "cow", "dino"
 * (SURVEY Q8 mesh scenes) and "9"/"mesh" (the capsule, the reference's default scene).  asset_dir holds earthmap.jpg
 * and models/{cow.obj, dino.obj, capsule/capsule.obj + .mtl + capsule.jpg}; images are decoded by rt_image_load's
 * decoder. */
int rt_scene_build(const char* name, const char* asset_dir, int device, rt_scene** out);
int rt_scene_info_get(const rt_scene* scene, rt_scene_info* info);
/* Canonical JSON of the scene graph (schema of oracle/ref_harness `dump`); returns the size needed incl. NUL. */
size_t rt_scene_dump(const rt_scene* scene, char* buf, size_t cap);
void rt_scene_destroy(rt_scene* scene);
/* Versioned flat-scene files (csrc/scenefile.h): the compiled scene -- primitive records, SAH BVH4, objects, materials,
 * textures and decoded texels, plus the scene_manager view -- written once and loaded (mmap) without re-parsing OBJ/MTL,
 * re-decoding images or rebuilding the BVH (the reference rebuilds every run: scene_manager.cpp:260-355, mesh.h:31-145,
 * bvh.cpp:3-42).  A loaded scene renders bit-identically to the one saved; it has no object graph (rt_scene_dump
 * fails).  Wrong magic, version, record layout, size or checksum: RT_E_SCENE with the reason. */
int rt_scene_save(const rt_scene* scene, const char* path);
int rt_scene_load(const char* path, int device, rt_scene** out);

/* ---- deforming a compiled scene (additive since ABI 5; the reference rebuilds a scene to move a vertex) ----
 * The scene's triangles as it holds them now: 9 doubles each (pt1, pt2, pt3), in compiled order -- the order the
 * triangles are met walking the world list, rt_scene_info.triangles of them.  Returns the count; p_out may be NULL (the
 * count only), else it holds cap >= count triangles (RT_E_INVALID otherwise).  Host buffer.  Needs no device unless the
 * scene has been updated. */
int64_t rt_scene_triangles_get(rt_scene* scene, double* p_out, int64_t cap);
typedef struct rt_update_params {   /* zero-initialised = host buffer, scene's stream */
    int32_t flags;                  /* RT_OUT_DEVICE: p is a device pointer on the scene's device */
    int32_t reserved;
    void* stream;                   /* hipStream_t (RT_OUT_DEVICE only), or NULL for the scene's own stream */
} rt_update_params;
/* rt_scene_update_triangles: new vertices for triangles [first, first + n) (9 doubles each, as rt_scene_triangles_get
 * orders them), then a refit of every BVH box on the device -- a cloth step, a morph target, a mesh whose vertices come
 * out of an optimiser -- where the only other way to move a vertex is a new graph, a full SAH build and a new upload.
 * Materials (rt_scene_update_materials / _textures change their values), texture coordinates and topology stay; spheres
 * move by rt_scene_update_spheres, rects, boxes and instances by rt_scene_update_rects / _boxes / _objects (below);
 * rt_multi is not covered.
 * Equality with a fresh compile: let scene A be compiled from triangles P0 and updated to P1, and scene B be compiled
 *   from the same graph with P1.  Every later call on A gives the bits it gives on B: rt_render, rt_render_views,
 *   rt_query_rays (all 12 doubles, prim included: the compiled triangle order is the same), rt_radiance_rays, and the
 *   segment counts -- closest hits do not depend on the tree, up to the exact-t ties any two trees can differ in.  A's
 *   tree keeps its topology, so rt_stats.kernel_* of A does not change; its boxes are the builder's own conservative
 *   boxes of what lies below them (a spatially split reference gets its triangle's whole box), so a refit tree is as
 *   tight as its topology allows but not re-optimised: after a large deformation a fresh compile traverses faster.
 * Streams and waiting: the work (one kernel that writes the vertices, then one small kernel per tree level) runs on
 *   u->stream, or on the scene's own stream when that is NULL (then the call waits).  On a caller's stream the call
 *   returns once enqueued when ms is NULL; with ms (HIP events around the kernels, milliseconds) it waits.
 * Ordering: the update writes the arrays the render kernels read.  Calls on one scene must be ordered by the caller --
 *   the same stream, or a synchronisation between them -- the rule the scene's workspace already imposes.
 * Upload: the first call uploads the scene if no render has done so yet (blocking), and makes the refit's own tables.
 * RT_E_INVALID, before any device work: scene or u NULL; first < 0, n < 0 or first + n above the triangle count; p NULL
 *   with n > 0; a flag bit other than RT_OUT_DEVICE; a stream without RT_OUT_DEVICE; a non-finite value in a host
 *   buffer (a device buffer is not inspected).  n = 0 is RT_OK and touches nothing; a scene without triangles accepts
 *   only n = 0.
 * Host copies: after an update rt_scene_triangles_get, rt_scene_bvh_get and rt_scene_save fetch what they need from the
 *   device first (the triangle records and the 24 box floats per node; they wait for the device), so a saved and loaded
 *   updated scene renders as the updated one.  rt_scene_dump fails (RT_E_SCENE) once a scene has been updated, as for
 *   a loaded scene: the graph no longer describes it. */
int rt_scene_update_triangles(rt_scene* scene, const rt_update_params* u, const double* p, int64_t first, int64_t n, double* ms);
/* Diagnostic, as rt_tile_candidates is: the device's BVH as it is now.  nodes_out: n_nodes x 128 bytes (four-child nodes
 * as uploaded: six float[4] planes lox, hix, loy, hiy, loz, hiz of the child boxes, int32 child[4] codes -- >= 0 an inner
 * node, -1 empty, else a leaf ~((count << 24) | first slot) -- and the 16-bit codes in int32 pad[4]); primrefs_out:
 * n_primrefs x uint32 (type:2 | index:30 per leaf slot; the device copy, pair-aligned where the scene runs an F_LEAF2
 * kernel).  Either may be NULL; the counts come back through n_nodes / n_primrefs (either may be NULL); a buffer smaller
 * than its count (node_cap / ref_cap entries) is RT_E_INVALID.  Uploads the scene if needed.  Host buffers, blocking. */
int rt_scene_bvh_get(rt_scene* scene, void* nodes_out, int64_t node_cap, uint32_t* primrefs_out, int64_t ref_cap, int64_t* n_nodes,
                     int64_t* n_primrefs);
/* The scene's spheres as it holds them now: 4 doubles each (cx, cy, cz, r; for a moving_sphere c is center0), in
 * compiled order -- the order the spheres are met walking the world list, rt_scene_info.spheres of them.  Returns the
 * count; s_out may be NULL (the count only), else it holds cap >= count spheres (RT_E_INVALID otherwise).  Host buffer.
 * Needs no device unless the scene has been updated. */
int64_t rt_scene_spheres_get(rt_scene* scene, double* s_out, int64_t cap);
/* rt_scene_update_spheres: new centres and radii for spheres [first, first + n) (4 doubles each, as
 * rt_scene_spheres_get orders them), then the refit of every BVH box and, for a scene that runs out of the LDS scene
 * image (the spheres-only scenes: the benchmark scene among them), of the image -- bouncing spheres, a particle or
 * physics step, a light or probe sphere an optimiser moves -- without a new graph, SAH build and upload.
 * What stays: materials and flags, and a moving sphere's motion (center1 - center0, time0, time1): it translates with
 *   its motion, which is also what keeps an image scene on its kernel.  Topology stays; rects, boxes and instances
 *   have calls of their own (rt_scene_update_rects below); rt_multi is not covered.
 * Everything else is rt_scene_update_triangles' contract with "sphere" for "triangle": scene A compiled with spheres S0
 *   and updated to S1 gives, in every later call, the bits scene B compiled from the same graph with S1 gives --
 *   rt_render in every variant, rt_render_views, rt_query_rays (all 12 doubles), rt_radiance_rays, rt_render_guides,
 *   rt_render_noise_target, rt_tile_candidates and the segment counts, up to exact-t ties; A's rt_stats.kernel_* and
 *   extend_variant do not change, whatever B would hoist or run.  rt_update_params, streams and waiting, ordering, the
 *   upload at the first call, ms, and the host copies (rt_scene_spheres_get, rt_scene_bvh_get and rt_scene_save fetch
 *   from the device first; rt_scene_dump refuses an updated scene) are as there.
 * RT_E_INVALID, before any device work: the rows of rt_scene_update_triangles, and in a host buffer a non-finite value
 *   or a radius <= 0.  A device buffer is not inspected: a radius <= 0 there gives the boxes sphere_box makes of it, as
 *   at compile.  n = 0 is RT_OK and touches nothing; a scene without spheres accepts only n = 0. */
int rt_scene_update_spheres(rt_scene* scene, const rt_update_params* u, const double* s, int64_t first, int64_t n, double* ms);
/* Diagnostic, as rt_scene_bvh_get is: the scene's LDS scene image (csrc/layout.h) with the tile representatives behind
 * it.  Returns its size in bytes, or 0 when the scene has none; out may be NULL (the size only), else it holds cap >=
 * size bytes (RT_E_INVALID otherwise).  rebuilt = 0: the device's bytes as they are now; rebuilt = 1: what the host
 * builder makes now from the scene as the device holds it (the fetched sphere records and node boxes) -- equal byte for
 * byte after any update.  Uploads the scene if needed.  Host buffer, blocking. */
int64_t rt_scene_lds_image_get(rt_scene* scene, int32_t rebuilt, uint8_t* out, int64_t cap);

/* ---- appearance: the values of a compiled scene's materials and textures ----
 * Indices: a compiled material index is the graph's material id (what rt_mat_* returned; for a builtin scene, creation
 * order), a compiled texture index the graph's texture id (rt_tex_*): compiling copies both lists in order and merges
 * nothing.  The material index is the `mat` value rt_query_rays reports.  The isotropic material rt_obj_constant_medium
 * creates is an ordinary entry, made when the medium is.  rt_scene_info.materials / .textures are the counts. */
#define RT_MATERIAL_DOUBLES 5   /* albedo r, g, b; fuzz; ir */
#define RT_TEXTURE_DOUBLES  4   /* colour r, g, b; scale */
#define RT_MAT_LAMBERTIAN    0
#define RT_MAT_METAL         1
#define RT_MAT_DIELECTRIC    2
#define RT_MAT_DIFFUSE_LIGHT 3
#define RT_MAT_ISOTROPIC     4
#define RT_TEX_SOLID      0
#define RT_TEX_CHECKER    1
#define RT_TEX_NOISE      2
#define RT_TEX_IMAGE      3
#define RT_TEX_BARY_IMAGE 4
/* The scene's materials / textures as it holds them now.  Both return the count.  Either out pointer may be NULL; one
 * that is given holds cap >= count rows (RT_E_INVALID otherwise).  Host buffers; no device is needed unless the scene
 * has been updated.  params_out rows: RT_MATERIAL_DOUBLES (albedo r, g, b; fuzz; ir) or RT_TEXTURE_DOUBLES (colour r, g,
 * b; scale) doubles; a field the record's type does not use comes back as the host record holds it.  desc_out rows: a
 * material's {RT_MAT_* type, texture index or -1 where the material has none (metal, dielectric)}; a texture's
 * {RT_TEX_* type, even, odd}, the two children's texture indices for a checker and -1, -1 otherwise. */
int64_t rt_scene_materials_get(rt_scene* scene, double* params_out, int32_t* desc_out, int64_t cap);
int64_t rt_scene_textures_get(rt_scene* scene, double* params_out, int32_t* desc_out, int64_t cap);
/* rt_scene_update_materials / rt_scene_update_textures: new values for materials / textures [first, first + n), rows as
 * the getters give them -- a light an optimiser drives, material parameters for inverse rendering, look-dev on the
 * material rt_query_rays reported, a flickering emitter across rt_render_views frames -- without a new graph, SAH build
 * and upload.  What a record takes from its row, by its type:
 *   metal                                   albedo; fuzz, stored as fuzz < 1 ? fuzz : 1 (material.h:47)   (ir ignored)
 *   dielectric                              ir                                                 (the rest ignored)
 *   lambertian / diffuse_light / isotropic  nothing: their colour is their texture's
 *   solid texture                           colour                                             (scale ignored)
 *   noise texture                           scale; the perlin table stays                      (colour ignored)
 *   checker / image / barycentric image     nothing
 * Ignored fields are left untouched, so a get followed by an update of the same rows changes no bit.  Types, texture
 *   links, checker children, images and texcoords never change.  Every device copy of a value follows: a solid colour
 *   shared by a lambertian, a light and a checker updates all three, whichever range the call named, and so does the
 *   LDS scene image's shading table.
 * Everything else is rt_scene_update_spheres' contract: scene A compiled with values V0 and updated to V1 gives, in
 *   every later call, the bits scene B compiled from the same graph call sequence with V1 gives -- rt_render in every
 *   variant, rt_render_views, rt_radiance_rays, rt_render_guides (albedo included), rt_render_noise_target,
 *   rt_query_rays and the segment counts; A's rt_stats.kernel_* and extend_variant do not change (no kernel choice
 *   depends on a value).  rt_update_params, streams and waiting, ordering, the blocking upload at the first call, ms and
 *   the host copies (the getters and rt_scene_save fetch from the device first; rt_scene_dump refuses an updated scene)
 *   are as there.  rt_multi is not covered.
 * RT_E_INVALID, before any device work: the rows of rt_scene_update_triangles; in a host buffer a non-finite value in
 *   any of a row's doubles, used or ignored.  A device buffer is not inspected.  n = 0 is RT_OK and touches nothing. */
int rt_scene_update_materials(rt_scene* scene, const rt_update_params* u, const double* m, int64_t first, int64_t n, double* ms);
int rt_scene_update_textures(rt_scene* scene, const rt_update_params* u, const double* t, int64_t first, int64_t n, double* ms);
/* ---- image texels (additive since ABI 5): the bytes of a scene's image textures, read, updated and (rt_radiance_grad_texels)
 * differentiated.  A compiled scene's images are the graph's, in rt_tex_image creation order, nothing merged; a mesh's
 * map_Kd images and a builtin scene's follow the same rule in the order the scene makes them.  Image k has w_k * h_k
 * texels; texel (i, j) of image k -- column i, row j counted from the top row, as the lookup computes them from u, v
 * (texture.h:90-117: i = int(clamp(u) * w), j = int((1 - clamp(v)) * h), each capped at w - 1 / h - 1) -- is global texel
 *   first_k + j * w_k + i,   first_k = sum of w_m * h_m over m < k,   N = the total.
 * rt_scene_images_get: returns the image count; desc_out rows {w, h, bpp}, first_texel_out first_k.  Either may be NULL;
 *   one that is given holds cap >= count rows (RT_E_INVALID otherwise).  Needs no device.
 * rt_scene_texture_images_get: one entry per texture (the rows of rt_scene_textures_get, whose desc rows cannot grow):
 *   the image index of an RT_TEX_IMAGE / RT_TEX_BARY_IMAGE texture, -1 otherwise.  Returns the texture count; image_out
 *   may be NULL, else holds cap >= count entries.  Needs no device.
 * rt_scene_texels_get: the image's bytes, h * w * bpp, top row first, as rt_tex_image took them and as the scene holds
 *   them now (fetched from the device first when the scene has been updated, like the other getters).  Returns the byte
 *   count; out may be NULL, else holds cap_bytes >= that.
 * rt_scene_update_texels: new bytes for rows [first_row, first_row + n_rows) of one image, n_rows * w * bpp of them in
 *   the same layout, from a host buffer or (RT_OUT_DEVICE) a device buffer.  The contract is rt_scene_update_textures':
 *   scene A updated to bytes V1 gives, in every later call, the bits a scene compiled from the same graph calls with
 *   V1 gives; kernel choice does not move (none depends on a byte); rt_scene_save and the getters see the new bytes;
 *   rt_scene_dump refuses an updated scene; rt_update_params, streams and waiting, ordering, the blocking upload at the
 *   first call and ms are as there; rt_multi is not covered.  The texel pool is the only device copy of the bytes, so
 *   the update is one copy on the call's stream.
 * RT_E_INVALID, before any device work: scene or u NULL; image not in [0, images); a row range outside [0, h]; a flag
 *   other than RT_OUT_DEVICE; a stream without it; texels NULL with n_rows > 0.  n_rows = 0 is RT_OK and touches nothing. */
int64_t rt_scene_images_get(rt_scene* scene, int32_t* desc_out, int64_t* first_texel_out, int64_t cap);
int64_t rt_scene_texture_images_get(rt_scene* scene, int32_t* image_out, int64_t cap);
int64_t rt_scene_texels_get(rt_scene* scene, int32_t image, uint8_t* out, int64_t cap_bytes);
int rt_scene_update_texels(rt_scene* scene, const rt_update_params* u, int32_t image, const uint8_t* texels, int64_t first_row, int64_t n_rows,
                           double* ms);

/* ---- rigid scenes: rects, boxes and the objects that place them (translate, rotate_y, constant_medium) ----
 * The Cornell box, the Cornell smoke box, the simple-light scene and the Next-Week final scene are made of these.
 * Indices: rects and boxes are numbered in compiled order, the order they are met walking the world list (a box under
 *   translate(rotate_y(...)) or inside a constant_medium included).  An object index is an index into the compiled
 *   object list: the world list walked in order, where a wrapper is numbered AFTER what it wraps -- for
 *   constant_medium(translate(rotate_y(box))) the box's prim object k, the rotate_y k + 1, the translate k + 2, the medium
 *   k + 3 -- and a run of consecutive world entries that world merging made one BVH is one object.  Only world-level
 *   objects and what they wrap are objects; primitives inside a bvh_node are not.
 * Getters, as rt_scene_materials_get: the count; either out pointer may be NULL, one that is given holds cap >= count
 *   rows.  values_out rows: RT_RECT_DOUBLES (a0, a1, b0, b1, k -- for an xy_rect x0, x1, y0, y1, k; xz_rect x0, x1, z0,
 *   z1, k; yz_rect y0, y1, z0, z1, k), RT_BOX_DOUBLES (min xyz, max xyz) or RT_OBJECT_DOUBLES (the object's four
 *   parameter doubles p: a translate's offset xyz in p[0..2]; a rotate_y's sin and cos of its angle in p[0..1]; a
 *   constant_medium's -1 / density in p[0]; what a kind does not use is 0).  desc_out rows: a rect's {axis (0 xy_rect,
 *   1 xz_rect, 2 yz_rect), material index}; a box's {material index}; an object's {RT_OBJ_* kind, a, b, world slot}: a
 *   is a prim's primitive reference (type:2 | index:30; type 2 a rect, 3 a box), a BVH's root node, a translate's, a
 *   rotate_y's and a medium's child object; b a medium's phase material, a BVH's hoisted-leaf code or -1; world slot the
 *   object's place in the world list, or -1 for an object that another one wraps. */
#define RT_RECT_DOUBLES   5
#define RT_BOX_DOUBLES    6
#define RT_OBJECT_DOUBLES 4
#define RT_OBJ_PRIM      0
#define RT_OBJ_BVH       1
#define RT_OBJ_TRANSLATE 2
#define RT_OBJ_ROTATE_Y  3
#define RT_OBJ_MEDIUM    4
int64_t rt_scene_rects_get(rt_scene* scene, double* values_out, int32_t* desc_out, int64_t cap);
int64_t rt_scene_boxes_get(rt_scene* scene, double* values_out, int32_t* desc_out, int64_t cap);
int64_t rt_scene_objects_get(rt_scene* scene, double* values_out, int32_t* desc_out, int64_t cap);
/* rt_scene_update_rects / rt_scene_update_boxes: new extents for rects / boxes [first, first + n), rows as the getters
 * give them -- a wall, the ceiling light, a box's size -- then the refit of every BVH box, as for triangles.  axis and
 * material stay.  Every device copy follows: the record, its copy in a BVH leaf, the copy of a loose primitive of the
 * world or of one under a transform chain (a constant_medium's boundary included).
 * rt_scene_update_objects: new parameters for objects [first, first + n), rows as rt_scene_objects_get gives them.  What
 * a record takes from its row, by its kind:
 *   RT_OBJ_TRANSLATE   p[0..2], the offset
 *   RT_OBJ_ROTATE_Y    p[0..1], sin and cos of the angle: to get the bits a compile gives, sin(d * pi / 180.0) and
 *                      cos(d * pi / 180.0) of libm for an angle of d degrees (hittable.cpp:27-29)
 *   RT_OBJ_MEDIUM      p[0], -1 / density (constant_medium.h:14)
 *   RT_OBJ_PRIM / RT_OBJ_BVH   nothing
 *   Ignored fields are left untouched, so a get followed by an update changes no bit.  Kinds and links never change.  A
 *   transformed object has no box anywhere -- a hit transforms the ray and tests the child -- so moving or turning an
 *   instance, a whole bvh_node mesh under translate(rotate_y(...)) included, refits nothing: it is one small launch, and
 *   the child's tree is the one a fresh compile builds.
 * Everything else is rt_scene_update_spheres' contract: scene A compiled with values V0 and updated to V1 gives, in
 *   every later call, the bits scene B compiled from the same graph call sequence with V1 gives, up to the exact-t ties
 *   any two trees can differ in (rects and boxes; an objects update keeps the very tree B has); A's rt_stats.kernel_*
 *   and extend_variant do not change.  rt_update_params, streams and waiting, ordering, the blocking upload at the first
 *   call, ms and the host copies (the getters and rt_scene_save fetch from the device first; rt_scene_dump refuses an
 *   updated scene) are as there.  rt_multi is not covered.
 * RT_E_INVALID, before any device work: the rows of rt_scene_update_triangles; in a host buffer a non-finite value in
 *   any of a row's doubles, used or ignored.  No other rule (the reference's constructors check none either: a rect with
 *   a0 > a1 is what it is at compile).  A device buffer is not inspected.  n = 0 is RT_OK and touches nothing. */
int rt_scene_update_rects(rt_scene* scene, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms);
int rt_scene_update_boxes(rt_scene* scene, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms);
int rt_scene_update_objects(rt_scene* scene, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms);

/* ---- render (engine::run; the engine_mode is in rt_params.flags: RT_ADAPTIVE, RT_PARALLEL_IMAGES, or neither for
 * single and parallel_stripes, which compute the same image) ----
 * out_rgb8: local_rows * width * 3 bytes (row-major, local row 0 = the first row this band set owns, top-most first);
 * out_accum (optional): local_rows * width * 3 f64 radiance sums (pixel_color before write_color).  Host pointers
 * unless RT_OUT_DEVICE.  Blocking. */
int rt_render(rt_scene* scene, const rt_camera* cam, const rt_params* params, uint8_t* out_rgb8, double* out_accum, rt_stats* stats);
/* Progressive rendering: the headless replacement for the reference's live preview (dynamic_gui_impl refreshed after
 * every row / square, gui.cpp:25-58, engine.h:88,307,353).  The frame is traced in passes of params->samples_per_pass
 * samples per pixel (0: ceil(spp / 8)); after each pass `cb` gets the samples traced so far and the frame write_color'ed
 * with that count, already in out_rgb8 (and the f64 sums in out_accum when non-NULL).  A non-zero return from `cb`
 * stops the render there (RT_OK; stats->primary counts the samples traced).  Every snapshot equals rt_render of that
 * many samples bit for bit, the last one rt_render's whole frame.  No RT_ADAPTIVE. */
typedef int (*rt_progress_fn)(void* user, int32_t samples_done, int32_t spp, const uint8_t* rgb8, const double* accum);
int rt_render_progressive(rt_scene* scene, const rt_camera* cam, const rt_params* params, uint8_t* out_rgb8, double* out_accum,
                          rt_progress_fn cb, void* user, rt_stats* stats);
/* Ray queries: the world's closest hit (hittable_list::hit, hittable_list.cpp:5-19, t in [0.001, inf)) of n rays
 * given as n x {ox, oy, oz, dx, dy, dz, time} doubles, through the renderer's own BVH traversal (the LDS scene image when
 * the scene has one, unless flags has RT_GLOBAL_SCENE).  t_out: n hit distances (+inf on a miss); normal_out (may be
 * NULL): n x 3 face normals as hit_record holds them (set_face_normal, hittable.h:18-22), 0 on a miss.  Ray i draws
 * its constant_medium uniforms from the PCG stream keyed (seed 0, pixel i, sample 0).  Host buffers; blocking. */
int rt_trace_rays(rt_scene* scene, const double* rays, int64_t n, int32_t flags, double* t_out, double* normal_out);
/* rt_query_rays (additive since ABI 5): hittable_list::hit(r, 0.001, t_max[i], rec) of n rays (rays as rt_trace_rays takes
 * them; t_max: n doubles, or NULL for +inf) with the whole hit_record, or as an occlusion query.  t_min is always 0.001
 * (the traversal's packed sort keys need a positive t_min).  A t_max below 0.001 finds nothing; a NaN t_max is undefined.
 * Closest mode (hits non-NULL, occluded NULL, no RT_Q_ANY_HIT): hits receives RT_HIT_DOUBLES per ray:
 *   [0]     t          hit distance; with t_max NULL and no RT_Q_NO_MEDIA, t and normal equal rt_trace_rays' bit for bit
 *   [1..3]  normal     hit_record::normal (set_face_normal, hittable.h:18-22: against the ray)
 *   [4..6]  point      hit_record::p
 *   [7, 8]  u, v       as the primitive's hit() sets them: a static sphere (get_sphere_uv, sphere.h:24-37, with glibc's
 *                      acos / atan2 restated), a triangle (barycentric, triangle.h:83-84), an aarect and each side of a
 *                      box (aarect.cpp:11-12, :29-30, :47-48) -- for every material, image-textured or not.  0 where the
 *                      reference sets none: a moving sphere (moving_sphere.h) and a constant_medium event
 *   [9]     front_face 1.0 or 0.0
 *   [10]    prim       the compiled primitive reference (type:2 | index:30) as an exact double: opaque, stable for one
 *                      rt_scene, equal for two rays iff they hit the same primitive; -2 for a constant_medium event
 *   [11]    mat        the compiled material index in [0, rt_scene_info.materials) (a medium event: its isotropic one)
 *   A miss: t = +inf, normal 0, point +inf, u = v = 0, front_face 0, prim = mat = -1.
 *   Ray i draws its constant_medium uniforms from the PCG stream keyed (seed 0, pixel i, sample 0), as rt_trace_rays.
 *   RT_Q_NO_MEDIA: constant_medium objects are skipped (and draw nothing): the closest surface.
 * Any-hit mode (RT_Q_ANY_HIT, occluded non-NULL, hits NULL): occluded[i] = 1 iff some non-medium primitive is accepted by
 *   its own hit test in [0.001, t_max[i]], else 0 -- shadow, visibility and ambient-occlusion rays.  Media never occlude.
 *   The walk stops at the first accepted primitive; which one that is depends on the tree, the byte does not.
 * Buffers: host pointers, and the call blocks (workspace and copies, as rt_trace_rays).  With RT_OUT_DEVICE rays, t_max,
 *   hits and occluded are device pointers on the scene's device, used in place (no workspace, no copy), and the kernel
 *   is enqueued on q->stream: the call returns once it is enqueued, WITHOUT waiting -- the results are ready when that
 *   stream reaches the point, and the buffers must stay alive until then.  With q->stream NULL it runs on the scene's own
 *   stream and the call waits for it; that stream is ordered after no other, so rays and t_max must be complete when
 *   the call is made.  The first call on a scene uploads it (blocking) in either case.
 * RT_GLOBAL_SCENE: never the LDS scene image (A/B and parity tests).  RT_E_INVALID, before any device work: scene or q
 * NULL; n < 0 or n > 2^30; rays NULL with n > 0; flag bits other than the four named; both of hits / occluded given, or
 * neither; RT_Q_ANY_HIT without occluded, or occluded without RT_Q_ANY_HIT.  n = 0 is RT_OK and touches nothing. */
#define RT_Q_ANY_HIT 512    /* occlusion query: stop at the first accepted hit */
#define RT_Q_NO_MEDIA 1024  /* constant_medium objects are skipped (implied by RT_Q_ANY_HIT) */
#define RT_HIT_DOUBLES 12   /* t, normal[3], point[3], u, v, front_face, prim, mat */
typedef struct rt_query_params { /* zero-initialised = closest hit, host buffers, scene's stream */
    int32_t flags;              /* RT_OUT_DEVICE | RT_GLOBAL_SCENE | RT_Q_ANY_HIT | RT_Q_NO_MEDIA */
    int32_t reserved;
    void* stream;               /* hipStream_t (RT_OUT_DEVICE only), or NULL for the scene's own stream */
} rt_query_params;
int rt_query_rays(rt_scene* scene, const rt_query_params* q, const double* rays, const double* t_max, int64_t n, double* hits,
                  uint8_t* occluded);
/* rt_radiance_rays (additive since ABI 5): the path-traced radiance that arrives along n caller-given rays (rays as
 * rt_trace_rays takes them) -- another camera model, light probes, lightmap texels, several cameras in one launch.
 * Paths: path (i, s), s in [0, spp), has index p = i * spp + s.  It starts at ray i with throughput 1 and runs _ray_color
 *   (engine.h:447-466) exactly as rt_render's persistent kernels do: a miss returns throughput * background; a
 *   diffuse_light hit returns its emission and ends the path; any other hit scatters while depth + 1 < max_depth (the
 *   path returns 0 once max_depth segments are traced).
 * RNG: the PCG state of path p is rng[p] when rng is given (n * spp states; seed, id_base and sample_base are then
 *   ignored), else the stream keyed (seed, pixel id_base + i, sample sample_base + s) -- rt_render's key, with the ray's
 *   stream id in the place of the global pixel.
 * Output: radiance[i] = +0.0 + L(i, 0) + L(i, 1) + ..., an f64 sum in sample order -- a sum like rt_render's out_accum, not
 *   a mean.  With rt_camera_rays (below): rt_render's out_accum of a pixel equals the in-order sum over its samples of
 *   rt_radiance_rays of its camera rays and states, bit for bit, and the segment counts are equal.
 * stats (may be NULL): segments counts world.hit calls as rt_render does, primary = n * spp, ms = HIP events around the
 *   kernel launches, passes = 1, samples_per_pass = spp; the other fields are 0 (extend_variant and kernel_lds_mode -1).
 * Limits: n <= 2^30 and n * spp <= 2^31 (kMaxPassSlots: path indices are 32 bits) per call; beyond that RT_E_INVALID.
 *   A caller with more work chunks the rays (id_base) or the samples (sample_base).
 * Buffers: host pointers; the call copies through the scene's workspace and blocks, as rt_query_rays.  With RT_OUT_DEVICE
 *   rays, rng, radiance are device pointers on the scene's device, used in place on q->stream (NULL: the scene's own
 *   stream, and the call waits; rays and rng must then be complete when the call is made).  On a caller's stream the call
 *   returns once the work is enqueued when stats is NULL; with stats it waits, because the segment count is read back.
 *   In both modes the claim counter and (spp > 1) the per-path records live in the scene's grow-only workspace, which
 *   every call on the scene shares: calls on one scene (rt_render, rt_query_rays on host buffers, this one) must be
 *   ordered by the caller -- the same stream, or a synchronisation between them.  The first call uploads the scene.
 * RT_E_INVALID, before any device work: scene or q NULL; n < 0 or above the limits; rays or radiance NULL with n > 0;
 *   max_depth < 1; spp < 0; a flag bit other than RT_OUT_DEVICE | RT_GLOBAL_SCENE; stream without RT_OUT_DEVICE;
 *   id_base + n > 2^32 when rng is NULL.  n = 0 is RT_OK and touches nothing. */
typedef struct rt_radiance_params { /* zero-initialised + max_depth = host buffers, seed 0, spp 1 */
    int32_t flags;              /* RT_OUT_DEVICE | RT_GLOBAL_SCENE, nothing else */
    int32_t spp;                /* samples per ray, >= 1 (0 is taken as 1) */
    int32_t max_depth;          /* >= 1, as rt_params.max_depth */
    uint32_t sample_base;       /* first sample index */
    uint64_t seed;
    uint64_t id_base;           /* stream id of ray 0; ray i has id_base + i; id_base + n <= 2^32 */
    void* stream;               /* hipStream_t (RT_OUT_DEVICE only), or NULL for the scene's own stream */
    double background[3];       /* returned on a miss, as rt_params.background */
} rt_radiance_params;
int rt_radiance_rays(rt_scene* scene, const rt_radiance_params* q, const double* rays, const uint64_t* rng, int64_t n, double* radiance,
                     rt_stats* stats);
/* rt_radiance_grad (additive since ABI 5): rt_radiance_rays' paths, and the gradient of
 *   phi = sum_i <weights[i], radiance[i]>
 * with respect to every solid texture colour, every metal albedo and the background -- one call whatever the number of
 * colours, measured at 1.4 to 4.3 times rt_radiance_rays on the same paths.  _ray_color has no Russian roulette and no scatter direction depends on a colour, so
 * with a fixed seed the radiance is a polynomial in these colours and the gradient below is its exact derivative.
 * rays, rng, n, every field of q, stats, the limits, the host / device buffer rules and the stream rules are
 *   rt_radiance_rays'.  weights (n x 3 f64) is the adjoint d loss / d radiance[i]; it applies to each of ray i's spp
 *   paths.  radiance (may be NULL) receives the bits rt_radiance_rays writes, and stats the same segment count.
 * Outputs, each of which may be NULL: grad_textures (T x RT_TEXTURE_DOUBLES) and grad_materials (M x
 *   RT_MATERIAL_DOUBLES) in the row layout of rt_scene_textures_get / rt_scene_materials_get, grad_background (3); so
 *   params -= lr * grad followed by rt_scene_update_* is a descent step.  Only the three colour columns are written with
 *   sums, and a row is non-zero only for an RT_TEX_SOLID texture or an RT_MAT_METAL material: the scale, fuzz and ir
 *   columns and the rows of every other type are +0.0.
 * Definition (w = weights[i], * the component-wise f64 product, each product rounded as written): a path scatters at
 *   vertices 0 .. k-1 with attenuations a_0 .. a_{k-1}, then ends at a diffuse_light with emission E, at a miss with E =
 *   background, or with nothing (the depth ran out, or the material absorbed): such a path adds to no row.
 *     P_0 = (1, 1, 1), P_{j+1} = P_j * a_j          (the renderer's throughput, in the order it multiplies it)
 *     Q_{k-1} = E,     Q_{j-1} = a_j * Q_j
 *     the end of the path adds  w * P_k             to the row E came from, or to grad_background;
 *     vertex j adds             (w * P_j) * Q_j     to the row a_j came from (skipped, being zero, when E is (0, 0, 0)).
 *   The row of a lambertian, isotropic or diffuse_light value is the solid texture it resolved to -- directly, or
 *   through checker levels; the row of a metal's is the metal's material row; a dielectric's attenuation and a noise or
 *   image value have no row.
 * Accumulation is exact, so the gradient's bits depend on neither the device, the grid nor the order of the rays: each
 *   f64 contribution c becomes the integer trunc(c * 2^96) (its magnitude truncated towards zero: |c| < 2^-96 adds
 *   nothing), the integers are summed in 192 bits with integer atomics, and each sum is rounded to f64 once, to nearest
 *   even.  A contribution that is not finite or has |c| >= 2^56 turns its row's three colours to NaN.
 * Workspace (the scene's grow-only one, as rt_radiance_rays'): beside that call's parts, the accumulators, copies x (T + M
 *   + 1) x 80 bytes with copies = min(blocks of the grid, 64), and a 64-byte record per scatter vertex, lanes of the grid
 *   x max(max_depth - 1, 1) x 64 bytes -- about 12 MiB per unit of max_depth on a 256-CU device.  A refused allocation
 *   is RT_E_DEVICE, and the next call allocates again.  With all three gradient outputs NULL the call records and adds
 *   nothing and needs neither: it is rt_radiance_rays on an HBM-scene kernel.
 * Scenes updated by rt_scene_update_*: the call reads the device's current values.
 * RT_E_INVALID, before any device work: every case of rt_radiance_rays (radiance may be NULL here), and weights NULL
 *   with n > 0.  n = 0, or all four outputs NULL, is RT_OK and touches nothing. */
int rt_radiance_grad(rt_scene* scene, const rt_radiance_params* q, const double* rays, const uint64_t* rng, const double* weights, int64_t n,
                     double* radiance, double* grad_textures, double* grad_materials, double* grad_background, rt_stats* stats);
/* rt_radiance_grad_texels (additive since ABI 5): rt_radiance_grad with one more output, grad_texels (N x 3 f64, may be
 * NULL; N and the global texel index as rt_scene_images_get states them): the gradient of phi with respect to the
 * texels of the scene's images -- what recovering a texture map needs.  The lookup is a nearest-texel one whose result
 * enters the path's product exactly where a solid colour does, and no scatter direction depends on it, so phi is the
 * same kind of polynomial in the texel values.  Everything rt_radiance_grad documents holds unchanged -- arguments,
 * definition, exact accumulation, buffer and stream rules, refusals -- with one definition changed:
 *   the row of a lambertian, isotropic or diffuse_light value that resolved (directly or through checker levels) to an
 *   RT_TEX_IMAGE or RT_TEX_BARY_IMAGE texture is the global texel the lookup read.
 * The derivative is with respect to the texel's value, byte / 255 per channel; the three columns are the texel's first
 *   three bytes (a fourth byte of a bpp 4 image is never read).  Texels of an image with bpp < 3 have no row and stay
 *   +0.0: the lookup reads neighbouring texels' bytes there, so no single texel owns the value.  Every texel no path
 *   read is +0.0.
 * With grad_texels NULL the call is rt_radiance_grad: the same kernels, the same bits in every output.  With it, a
 *   scene that has an image texture runs the texel form of its kernel (k_texel_grad), and the other outputs hold the
 *   bits rt_radiance_grad gives.
 * Workspace: beside rt_radiance_grad's parts, the texel accumulators, copies x N x 80 bytes, zeroed per call, with as
 *   many copies as 256 MiB hold -- at least one, at most the other table's count -- or as option grad.texel_copies
 *   says; no output bit depends on the count.  Allocated only when grad_texels is given.
 * RT_E_INVALID, before any device work: every case of rt_radiance_grad, and with grad_texels given a scene whose T + M +
 *   1 + N rows do not fit the 32-bit row of a vertex record (2^32 rows or more).  n = 0, or all five outputs NULL, is RT_OK
 *   and touches nothing. */
int rt_radiance_grad_texels(rt_scene* scene, const rt_radiance_params* q, const double* rays, const uint64_t* rng, const double* weights,
                            int64_t n, double* radiance, double* grad_textures, double* grad_materials, double* grad_background,
                            double* grad_texels, rt_stats* stats);
/* rt_camera_rays (additive since ABI 5): rt_render's own camera rays as data -- the starting point of a custom camera, and
 * what makes rt_radiance_rays checkable against rt_render.  Entry (ly * width + lx) * k + j of rays_out (7 doubles) and
 * rng_out (one PCG state; may be NULL) holds the ray of local pixel (lx, ly), sample sample_base + j, and the generator's
 * state after the camera's draws (engine.h:58-68, camera.h:38-47: pixel jitter, lens disk, shutter time), with k =
 * params->spp; local rows and the band partition as in rt_render.  Reads width, height (both >= 2), spp, seed, the band
 * fields, flags (RT_OUT_DEVICE only) and stream; needs no scene.  Host buffers (blocking), or with RT_OUT_DEVICE device
 * buffers on `device`, written on params->stream (the call returns once enqueued; NULL: the default stream, and the call
 * waits).  RT_E_INVALID also when the padded local pixels (8x8 tiles) times k exceed 2^31: fewer samples per call. */
int rt_camera_rays(const rt_camera* cam, const rt_params* params, uint32_t sample_base, int device, double* rays_out, uint64_t* rng_out);
/* rt_tile_candidates (additive since ABI 5): the tile lists rt_render(scene, cam, params, ...) would build (option
 * render.tile_lists), as data: counts_out[i] = the number of spheres the camera rays of 8x8 tile i of the local rows can
 * reach (tiles in row-major order, (width + 7) / 8 per row), or 0xFFFF for a tile with more than 15, whose batches walk
 * the tree.  Returns the number of tiles, or 0 when that render builds no lists: the scene is not a spheres-only scene
 * traced from LDS, the option is 0, the mode is RT_ADAPTIVE, or (option 1) a pass holds fewer than 72 samples per pixel.
 * counts_out may be NULL (the number only); otherwise it holds `cap` entries, RT_E_INVALID when that is fewer than the
 * tiles.  Host buffer, blocking.  The diagnostic of a caller whose scene gains nothing: many 0xFFFF tiles or none at all. */
int rt_tile_candidates(rt_scene* scene, const rt_camera* cam, const rt_params* params, uint16_t* counts_out, int64_t cap);
/* rt_render_views (additive since ABI 5): nviews whole frames of one scene in one call -- an orbit of a mesh, the six faces of
 * a cube map, a light field -- where a loop of rt_render pays a workspace reset, a launch per pass, the accumulation, a
 * host wait and a copy per frame.  Every view has params->width x height, spp, max_depth and background; view v looks
 * through cams[v] with seed seeds[v] (seeds NULL: params->seed for every view).
 * Contract: view v's out_rgb8 and out_accum equal, bit for bit, what rt_render(scene, &cams[v], params with seed =
 *   seeds[v], ...) writes, and stats->segments / primary equal the sums over those nviews calls.
 * Output: out_rgb8 is nviews x height x width x 3 bytes, view-major, row 0 of a view at the top; out_accum (optional) is
 *   nviews x height x width x 3 f64 radiance sums.
 * How: one persistent path kernel (rt_radiance_rays') whose path p = ((v * width * height + pixel) * spp + s) takes its
 *   camera ray from view v's camera in registers.  The views are cut into groups of whole views, one launch per group,
 *   so that a group's paths fit kMaxPassSlots = 2^31, half of the free device memory (24 bytes per path) and option
 *   views.max_paths; small views run as one launch.
 * stats (may be NULL): segments and primary as above, ms = HIP events around the device work, passes = launches of the
 *   path kernel, samples_per_pass = spp; the other fields are 0 (extend_variant and kernel_lds_mode -1).
 * Reads width, height, spp, max_depth, seed, background, flags (RT_OUT_DEVICE | RT_GLOBAL_SCENE, nothing else), stream and
 *   fp_mode; band_count must be 1 (the whole frame; band_rows is not read); samples_per_pass is ignored.
 * Buffers: host pointers; the call copies through the scene's workspace and blocks.  With RT_OUT_DEVICE out_rgb8 and
 *   out_accum are device pointers on the scene's device, written in place on params->stream (NULL: the scene's own
 *   stream, and the call waits).  On a caller's stream the call returns once the work is enqueued when stats is NULL;
 *   with stats it waits, because the segment count is read back.  In both modes the camera table, the claim counters
 *   and (spp > 1) the per-path records live in the scene's grow-only workspace, which every call on the scene shares:
 *   calls on one scene (rt_render, rt_radiance_rays, rt_query_rays on host buffers, this one) must be ordered by the
 *   caller -- the same stream, or a synchronisation between them.  The first call uploads the scene.
 * RT_E_INVALID, before any device work: scene, cams or params NULL; nviews < 0; out_rgb8 NULL with nviews > 0; width or
 *   height < 2; spp < 1; max_depth < 1; band_count != 1; a flag bit other than the two named; stream without
 *   RT_OUT_DEVICE; width * height * spp of one view above 2^31 (render such a frame with rt_render, which splits it into
 *   passes).  nviews = 0 is RT_OK and touches nothing.
 * For many small frames: 64 views of 128 x 128 x 16 take 0.13-0.19 of the time of 64 rt_render calls.  Large frames gain
 * nothing (1920 x 1080 x 16: 0.94-1.24 of the loop's time): render those with rt_render. */
int rt_render_views(rt_scene* scene, const rt_camera* cams, const uint64_t* seeds, int32_t nviews, const rt_params* params, uint8_t* out_rgb8,
                    double* out_accum, rt_stats* stats);
/* Number of rows a band partition owns, and optionally their global indices (rows_out may be NULL).  Global row y
 * belongs to band set (y / band_rows) % band_count; local row ly of set r is global row
 * (ly / band_rows) * band_rows * band_count + r * band_rows + ly % band_rows. */
int rt_local_rows(const rt_params* params, int32_t* rows_out);
/* Gather layout of an n-way band partition (what rt_render_multi's ncclGather moves): every band set sends one block of
 * rt_band_block_rows(height, band_rows, n) rows (the largest set's row count; a shorter set pads after its rows).
 * rt_unpack_bands places the n concatenated blocks (packed: n * block_rows * width * 3 bytes, block r = set r's rows in
 * local order) into the height-row frame (row 0 = top): device pointers and a kernel on `stream` (hipStream_t, NULL =
 * default) with RT_OUT_DEVICE, else host memory.  packed_bytes / frame_bytes are the sizes of the two buffers: unless
 * they are exactly n * block_rows * width * 3 and height * width * 3 the call is refused (RT_E_INVALID) before any byte
 * moves.  Replaces the reference's in-place stripe writes into one frame (engine.h:343-355). */
int rt_band_block_rows(int32_t height, int32_t band_rows, int32_t n);
int rt_unpack_bands(const uint8_t* packed, size_t packed_bytes, uint8_t* frame, size_t frame_bytes, int32_t width, int32_t height,
                    int32_t band_rows, int32_t n, int32_t flags, void* stream);

/* ---- denoising (additive since ABI 5; the reference has none) ----
 * rt_render_guides: the first-hit guide buffers of the local rows (ordered as in rt_render), RT_GUIDE_DOUBLES per pixel:
 * albedo[3], normal[3], position[3], t.  One ray per pixel with no render RNG draw: through the pixel centre
 * (s = (i + 0.5) / (W - 1), t = ((H - 1 - gy) + 0.5) / (H - 1)) of rt_render's camera basis, from `origin` (no lens
 * offset), d = llc + s * horizontal + t * vertical - origin, time = time0; its constant_medium draws come from the PCG
 * stream keyed (seed 0, global pixel gy * W + i, sample 0), so a whole frame's t and normal equal rt_trace_rays of
 * rays_out (optional: the 7 doubles of every ray) with ray index = pixel index.  position is the hit point as the
 * hit_record holds it.  albedo: the texture value at the hit for lambertian and isotropic, the albedo of a metal,
 * (1, 1, 1) for dielectric and diffuse_light.  A miss has t = +inf, normal 0, position +inf, albedo 1.
 * Honours width, height, the band fields, stream, RT_OUT_DEVICE and RT_GLOBAL_SCENE; ignores spp, seed, max_depth and
 * samples_per_pass; any other flag is RT_E_INVALID.  Blocking. */
#define RT_GUIDE_DOUBLES 10
int rt_render_guides(rt_scene* scene, const rt_camera* cam, const rt_params* params, double* guides, double* rays_out);
/* rt_denoise: a variance-guided edge-avoiding a-trous filter.  accum_a / accum_b: two rt_render out_accum frames of the
 * same whole width x height image (bands unpacked by the caller), spp_each samples each, rendered with different seeds
 * (independent estimates: their mean is the frame, their half difference squared its variance); guides: that frame's
 * rt_render_guides.  out_color: width * height * 3 filtered radiance (per sample, i.e. already divided by the sample
 * count); out_rgb8 (optional): write_color of it (gamma 2, clamp, quantize, as rt_render with spp = 1).  The mean is
 * divided by max(albedo, albedo_floor) before filtering and multiplied back after it unless RT_DN_NO_DEMODULATE.  Each of
 * the `iterations` passes (tap spacing 1, 2, 4, ...) is a 5x5 B3-spline average weighted by the normals
 * (max(0, n.n')^(2^normal_squarings)), the distance from the centre's tangent plane (sigma_plane), hit / miss, and the
 * colour difference against sigma_color^2 times the 3x3-blurred variance, which is filtered along.  All f64 + - * / in a
 * fixed order: tests/dn_reference.py restates it and the result equals it bit for bit.  Host buffers, or device buffers
 * on `device` with RT_OUT_DEVICE; ms (optional): device time of the filter kernels.  One call at a time per device. */
#define RT_DN_NO_DEMODULATE 256
typedef struct rt_denoise_params {   /* zero-initialised = defaults */
    int32_t width, height;
    int32_t iterations;         /* 0 -> 5; 1..8 */
    int32_t normal_squarings;   /* 0 -> 6 (normal weight = max(0, n.n')^(2^k)); 1..10 */
    double sigma_color;         /* 0 -> 1.0 */
    double sigma_plane;         /* 0 -> 0.1 */
    double albedo_floor;        /* 0 -> 0.5 (measured: smaller floors let a dark albedo channel's 1/A^2 dominate the weights) */
    int32_t flags;              /* RT_OUT_DEVICE | RT_DN_NO_DEMODULATE */
    void* stream;               /* hipStream_t to run on, or NULL for the library's own */
} rt_denoise_params;
int rt_denoise(int device, const rt_denoise_params* p, const double* accum_a, const double* accum_b, int32_t spp_each,
               const double* guides, double* out_color, uint8_t* out_rgb8, double* ms);
/* rt_render_denoised: two rt_render passes of spp / 2 samples (seeds `seed` and `seed + 1`), rt_render_guides and
 * rt_denoise in one call; the frames stay on the device until the final copy.  Needs the whole frame (band_count 1) and
 * an even spp >= 2; no RT_ADAPTIVE or RT_PARALLEL_IMAGES.  dn: NULL = defaults (its width / height are taken from
 * params; of its flags only RT_DN_NO_DEMODULATE is read, RT_OUT_DEVICE comes from params).  out_rgb8: W*H*3;
 * out_color (optional): W*H*3 f64.  stats: segments / primary / passes / launches summed over the two renders, the
 * kernel identity of the second; ms = host wall time of the whole call.  The result equals the same steps made through
 * the public calls, bit for bit. */
int rt_render_denoised(rt_scene* scene, const rt_camera* cam, const rt_params* params, const rt_denoise_params* dn, uint8_t* out_rgb8,
                       double* out_color, rt_stats* stats);

/* ---- noise-target rendering (additive since ABI 5; the reference gives every pixel the same sample count) ----
 * rt_render_noise_target traces every local pixel until the standard error of its mean luminance is within a relative
 * tolerance, up to params->spp samples (the per-pixel cap).
 *   1. Base pass: samples [0, min_spp) of every pixel.  Beside the radiance sums two luminance sums are kept per pixel,
 *      S1 += y and S2 += y*y with y = (0.2126*r + 0.7152*g) + 0.0722*b of each sample, f64, in sample order from +0.
 *   2. Test after n samples: mean = S1/n; var = (S2 - S1*mean)/(n-1), negative values set to 0; se2 = var/n;
 *      thr = rel_tol*(mean + lum_floor); converged iff se2 <= thr*thr (+ - * / and comparisons only).
 *   3. Rounds: a pixel stays active while it was active, has fewer than spp samples and is unconverged -- with dilate = 1,
 *      while any active pixel of its 3x3 neighbourhood (itself included) is unconverged.  Retirement is final.  Each
 *      round adds min(step_spp, spp - n) samples to every active pixel, continuing its sums in sample order.
 *   4. The render ends when no pixel is active or the active ones are at the cap; out_rgb8 is write_color of every
 *      pixel's sums with its own count.
 * A pixel that received n samples holds the out_accum and RGB8 that rt_render with spp = n and the same seed gives it,
 * bit for bit (tests/nt_reference.py restates the test and the active-set rule).  All buffers cover the local rows,
 * ordered as in rt_render; every one but out_rgb8 may be NULL: out_accum 3 f64 sums, out_count the samples, out_moments
 * {S1, S2} per pixel; host pointers, or device pointers with RT_OUT_DEVICE.  Honours seed, max_depth, background, stream,
 * samples_per_pass, the band fields, RT_OUT_DEVICE, RT_GLOBAL_SCENE and RT_PROFILE.  RT_E_INVALID, before any device
 * work: RT_ADAPTIVE, RT_PARALLEL_IMAGES, RT_WAVEFRONT, RT_SPLIT_SHADE; min_spp < 2 or > spp; step_spp < 1; negative or
 * non-finite tolerances; dilate outside 0 / 1, or dilate = 1 with band_count > 1 (the neighbourhood would depend on the
 * partition).  stats as for rt_render: primary = the sum of out_count, segments from the device counter, the kernel
 * identity of the persistent kernel, passes = path-kernel launches.  result (optional): the refinement rounds run, the
 * pixels the test retired (a pixel whose test passes exactly when it reaches the cap counts; one stopped by the cap alone
 * does not) and the samples traced.  Blocking. */
typedef struct rt_noise_params {   /* zero-initialised = defaults */
    int32_t min_spp;            /* 0 -> 32; every pixel gets this many (>= 2) */
    int32_t step_spp;           /* 0 -> 32; samples a refinement round adds to every still-active pixel (>= 1) */
    int32_t dilate;             /* 0 / 1: 1 also keeps the 3x3 neighbours of an unconverged pixel active (recommended for
                                   whole frames: a pixel whose first min_spp samples are all equal, e.g. all black under a
                                   small light, has var == 0 and would retire at once; measured in DESIGN.md 4.6) */
    double rel_tol;             /* 0 -> 0.05; target relative standard error of the pixel's mean luminance */
    double lum_floor;           /* 0 -> 0.01; added to the mean before the relative test (dark pixels) */
} rt_noise_params;
typedef struct rt_noise_result {
    int32_t rounds;
    int64_t converged_pixels;
    uint64_t samples;
} rt_noise_result;
int rt_render_noise_target(rt_scene* scene, const rt_camera* cam, const rt_params* params, const rt_noise_params* noise, uint8_t* out_rgb8,
                           double* out_accum, int32_t* out_count, double* out_moments, rt_stats* stats, rt_noise_result* result);

/* ---- images (imageio::load_image, imageio.cpp:11-15: stbi_load(path, &w, &h, &c, 0) of stb_image v2.27) ----
 * Decodes a JPEG (baseline or progressive) or PNG file to 8-bit samples, native channel count, row 0 = top, the bytes
 * stb_image returns (the JPEG inverse DCT, color transform and chroma upsampling follow its arithmetic).  *pixels is
 * allocated by the library (h * w * channels bytes); release it with rt_image_free.  image_texture (texture.h:67-118)
 * and map_Kd textures load their files through this decoder. */
int rt_image_load(const char* path, int32_t* width, int32_t* height, int32_t* channels, uint8_t** pixels);
void rt_image_free(uint8_t* pixels);

/* ---- multi-GPU (one process, one host thread per GPU, RCCL) ----
 * Replaces the reference's CPU-parallel drivers (engine.h:335-376 _run_parallel_stripes: 4 threads on 4 row stripes;
 * SURVEY.md §8(b) rt_render_multi).  An rt_multi holds the scene uploaded on every listed device and one RCCL
 * communicator per device (one group of ncclCommInitRankConfig, non-blocking), both made at creation: the first
 * rt_render_multi spends no time on the upload (the reference times engine::run only, main.cpp:44-46; the pass
 * workspace, sized by the render's W, H and spp, is still allocated by the first render of a size).
 * rt_render_multi renders the whole frame: device k
 * renders the row bands b (params->band_rows rows each) with b % ngpus == k -- params->band_count / band_index are
 * ignored -- packs them into one buffer, and a single ncclGather moves every device's block to devices[0], whose unpack
 * kernel writes the rows in image order.  out_rgb8: W*H*3 bytes, row 0 = top; host memory, or device memory on
 * devices[0] with RT_OUT_DEVICE.  The image is bit-identical to rt_render's for any device count (the RNG is keyed by
 * (seed, global pixel, sample)).  stats: segments/primary summed over the devices, ms = host wall time of the call.
 * Threading: one rt_multi per process at a time per device set; calls are blocking.
 * Failure behaviour: a device whose render fails makes the call return that error before any collective starts (the
 * rt_multi stays usable).  The communicators are non-blocking (ncclConfig_t.blocking = 0); their creation and the
 * gather are polled (ncclCommGetAsyncError, hipStreamQuery) against a deadline of multi.timeout_ms milliseconds
 * (rt_option_set; while unset, the environment's ART_MULTI_TIMEOUT_MS, default 120000).  An RCCL error or an expired
 * deadline aborts every communicator (ncclCommAbort) and returns RT_E_DEVICE; the rt_multi then refuses renders until
 * it is destroyed and created again.  Both RCCL groups (creation, gather) are closed on every error path and the
 * communicators aborted, so a failure never leaves the calling thread inside an open ncclGroupStart. */
typedef struct rt_multi rt_multi;
int rt_multi_create(const char* name, const char* asset_dir, const int* devices, int ngpus, rt_multi** out);
int rt_multi_from_graph(rt_graph* g, const int* devices, int ngpus, rt_multi** out);
void rt_multi_destroy(rt_multi* m);
int rt_render_multi(rt_multi* m, const rt_camera* cam, const rt_params* params, uint8_t* out_rgb8, rt_stats* stats);
int rt_multi_ngpus(const rt_multi* m);
/* The scene_manager view and sizes of the multi's scene (as rt_scene_info_get; device_bytes_f64 = bytes on each device). */
int rt_multi_scene_info(const rt_multi* m, rt_scene_info* info);
/* Stats of devices[k] alone in the last rt_render_multi: its segments, primaries, rows and (RT_PROFILE) its own kernel
 * times and launches; ms = that device's render time (before the gather). */
int rt_multi_device_stats(const rt_multi* m, int k, rt_stats* stats);
/* Phases of the last rt_render_multi, so a scaling shortfall can be attributed: every device's render (host wall time of
 * its thread: kernels + its own finalize), the gather (HIP events around the ncclGather on devices[0]'s stream) and the
 * unpack (k_unpack_bands + the host copy when out_rgb8 is host memory). */
typedef struct rt_multi_times {
    double total_ms;            /* the whole call (== rt_stats.ms) */
    double render_ms_max;       /* slowest device's render */
    double render_ms_min;       /* fastest device's render */
    double gather_ms;           /* ncclGather, as devices[0]'s stream sees it */
    double unpack_ms;           /* unpack kernel (+ device-to-host copy) */
    double wait_ms;             /* host time spent polling the gather */
    uint64_t collectives;       /* gathers this rt_multi has issued so far (failed renders issue none) */
    int32_t slowest_device;     /* index k (devices[k]) of render_ms_max */
    int32_t ngpus;
} rt_multi_times;
int rt_multi_times_get(const rt_multi* m, rt_multi_times* out);

/* ---- scene graph builder (one call per reference constructor; returns an id >= 0 or a negative code) ----
 * Scene-build randomness (noise textures' perlin tables, rt_graph_bvh's node draws) comes from the graph's own
 * mt19937 (seed 5489), in call order, exactly as the reference's global generator would produce it. */
rt_graph* rt_graph_new(void);
void rt_graph_free(rt_graph* g);
int rt_graph_random_double(rt_graph* g, double* out);              /* random_double() from the graph's generator */
int rt_tex_solid(rt_graph* g, double r, double gr, double b);       /* texture.h:16-29 */
int rt_tex_checker(rt_graph* g, int even, int odd);                 /* texture.h:31-50 */
int rt_tex_noise(rt_graph* g, double scale);                        /* texture.h:52-65 */
int rt_tex_image(rt_graph* g, int w, int h, int bpp, const uint8_t* texels); /* texture.h:67-118 */
/* barycentric_image_texture(a, b, c, image) (texture.h:135-154): uv = {ua, va, ub, vb, uc, vc}; image_tex from rt_tex_image */
int rt_tex_bary_image(rt_graph* g, const double uv[6], int image_tex);
int rt_mat_lambertian(rt_graph* g, int tex);                        /* material.h:20-43 */
int rt_mat_metal(rt_graph* g, double r, double gr, double b, double fuzz); /* material.h:45-61 */
int rt_mat_dielectric(rt_graph* g, double ir);                      /* material.h:63-99 */
int rt_mat_diffuse_light(rt_graph* g, int tex);                     /* material.h:101-118 */
int rt_obj_sphere(rt_graph* g, const double c[3], double r, int mat);                 /* sphere.h */
int rt_obj_moving_sphere(rt_graph* g, const double c0[3], const double c1[3], double t0, double t1, double r, int mat);
int rt_obj_triangle(rt_graph* g, const double p1[3], const double p2[3], const double p3[3], int mat); /* triangle.h */
int rt_obj_rect(rt_graph* g, int axis /*0 xy,1 xz,2 yz*/, double a0, double a1, double b0, double b1, double k, int mat);
int rt_obj_box(rt_graph* g, const double p0[3], const double p1[3], int mat);         /* box.cpp */
int rt_obj_list(rt_graph* g, int n, const int* items);                                /* hittable_list */
int rt_obj_bvh(rt_graph* g, int n, const int* items);                                 /* bvh_node(list, 0, 1) */
int rt_obj_translate(rt_graph* g, int child, const double offset[3]);                 /* hittable.cpp:3-23 */
int rt_obj_rotate_y(rt_graph* g, int child, double degrees);                          /* hittable.cpp:25-85 */
int rt_obj_constant_medium(rt_graph* g, int boundary, double density, int tex);       /* constant_medium.h */
int rt_graph_add_world(rt_graph* g, int obj);                                         /* world.add(obj) */
int rt_graph_clear_world(rt_graph* g);
int rt_graph_set_view(rt_graph* g, const double lookfrom[3], const double lookat[3], double vfov, double aperture,
                      const double background[3]);
/* ---- meshes (Wavefront OBJ + MTL, rapidobj v1.0.1 semantics: objmesh.h) ----
 * rt_mesh_parse = mesh::parse: parses and triangulates; reports the triangle and shape counts (either may be NULL).
 * rt_mesh_build = mesh::parse + mesh::build into the graph: one triangle per post-triangulation face with
 *   lambertian(color::random()) (no MTL; draws from the graph's generator), lambertian(Ka + Kd), or
 *   lambertian(barycentric_image_texture) for a map_Kd material, whose image (JPEG / PNG, next to the MTL) is decoded
 *   as rt_image_load does (stb_image's bytes; a raw texel file <stem>.rgb[.gz] is also accepted).  The triangle ids are
 *   *first_id .. *first_id + n - 1; returns n >= 0 or a negative code. */
int rt_mesh_parse(const char* obj_path, int64_t* triangles, int64_t* shapes);
int rt_mesh_build(rt_graph* g, const char* obj_path, int* first_id);
/* Compiles the graph (flat SoA + SAH BVH) and uploads it to `device`.  The graph stays owned by the caller. */
int rt_graph_compile(rt_graph* g, int device, rt_scene** out);

#ifdef __cplusplus
}
#endif
#endif /* ART_H */

// renderer.h — host-side device renderer (implemented in renderer.hip; no HIP types in this header).
#pragma once
#include <cstdint>
#include <functional>

#include "art.h"
#include "layout.h"
#include "noise_target.h"
#include "scene.h"
#include "update_kinds.h"

namespace art {

struct RenderParams {
    int width = 0, height = 0, spp = 1, max_depth = 50;
    uint64_t seed = 0;
    int fp_mode = RT_FP64;
    int band_rows = 1, band_count = 1, band_index = 0;
    int samples_per_pass = 0;
    int flags = 0;
    void* stream = nullptr;
    double background[3] = {0, 0, 0};
    // Progressive rendering (whole-image traces): called after every pass with the samples traced so far, once the
    // frame write_color'ed with that count (and the sums, when requested) are in the caller's buffers; returning
    // false ends the render there.
    std::function<bool(int samples_done)> on_pass;
};

struct RenderStats {
    uint64_t segments = 0, primary = 0;
    double ms = 0, extend_ms = 0, shade_ms = 0;
    uint64_t extend_launches = 0, shade_launches = 0;
    int passes = 0, samples_per_pass = 0, local_rows = 0;
    int extend_variant = 0;
    uint32_t kernel_features = 0, kernel_textures = 0;  // the persistent kernel: k_paths_g<F, TF, LM> / k_paths (LM 3)
    int kernel_lds_mode = -1;
};

struct RadianceParams {  // rt_radiance_params, checked (art.h)
    int spp = 1, max_depth = 50;
    uint32_t sample_base = 0;
    uint64_t seed = 0, id_base = 0;
    bool device = false, global_scene = false;
    void* stream = nullptr;
    double background[3] = {0, 0, 0};
};

class Renderer {
public:
    struct Impl;
    Renderer(FlatScene flat, int device);
    ~Renderer();
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;
    // Uploads the scene to the device now (render and trace_rays otherwise do it at their first call).
    void upload();
    void render(const CameraRec& cam, const RenderParams& p, uint8_t* out_rgb, double* out_acc, RenderStats& stats);
    // Closest hit of n rays (rays: n x {ox, oy, oz, dx, dy, dz, tm}) through the renderer's traversal: t (inf on a
    // miss) and the face normal (n x 3), host buffers; global_scene forces the HBM traversal on an LDS-image scene.
    void trace_rays(const double* rays, size_t n, bool global_scene, double* t_out, double* n_out);
    // rt_query_rays: closest hits with the record (hits: n x RT_HIT_DOUBLES) or, with any_hit, occlusion bytes, over
    // [0.001, t_max[i]] (t_max null: +inf).  device: every buffer is a device pointer and nothing is copied; the launch
    // goes to `stream` and the call returns without waiting for it, or to the scene's own stream (null) and waits.
    // Host buffers: workspace, copies and a wait, as trace_rays.
    void query_rays(const double* rays, const double* t_max, size_t n, bool device, bool global_scene, bool any_hit, bool no_media, void* stream,
                    double* hits, uint8_t* occluded);
    // rt_radiance_rays: radiance[i] = the in-order f64 sum of p.spp paths from ray i (rng: n * spp PCG states, or null).
    // device: the four buffers are device pointers used in place on `stream` (null: the scene's own, and the call waits);
    // the claim counter and the per-path records come from the workspace either way.  stats (may be null: then a device
    // call on the caller's stream returns once enqueued) receives segments, primary and ms.
    void radiance_rays(const RadianceParams& p, const double* rays, const uint64_t* rng, size_t n, double* radiance, RenderStats* stats);
    // rt_radiance_grad: radiance_rays' paths with the adjoint weights (n x 3), and the gradient of sum_i <weights[i],
    // radiance[i]> in the row layouts of the texture and material getters plus the background's three doubles (art.h).
    // radiance and the three gradient buffers may each be null.  Buffers and stream as radiance_rays.  The workspace holds,
    // beside radiance_rays' parts, the accumulator table, copies x (textures + materials + 1) x 80 bytes with copies =
    // min(grid blocks, 64), and the vertex records, grid lanes x max(max_depth - 1, 1) x 64 bytes.
    // grad_texels (rt_radiance_grad_texels; null: rt_radiance_grad, the same kernels and bits): one row of three doubles
    // per texel of the scene's images in image order.  With it the scene's kernel is k_texel_grad, and the workspace also
    // holds the texel table, copies x texels x 80 bytes, zeroed per call, with as many copies as 256 MiB hold (at least
    // one, at most the other table's count; option grad.texel_copies sets the count).  A scene without an image texture
    // runs k_radiance_grad and gets zeros.
    void radiance_grad(const RadianceParams& p, const double* rays, const uint64_t* rng, const double* weights, size_t n, double* radiance,
                       double* grad_textures, double* grad_materials, double* grad_background, double* grad_texels, RenderStats* stats);
    // rt_render_views: nviews whole frames of p's width x height x spp, view v through cams[v] with seed seeds[v] (seeds
    // null: p.seed), each equal to render()'s bit for bit.  out_rgb (nviews x H x W x 3 bytes) and out_acc (optional, the
    // f64 sums) are host buffers, or with RT_OUT_DEVICE device buffers written in place on p.stream; the camera table,
    // the claim counters, the per-path records of the largest group (view_plan.h) and whatever the caller's buffers do
    // not hold come from the workspace.  stats (may be null: then a device call on the caller's stream returns once
    // enqueued) receives segments, primary, ms and passes = the launches of the path kernel.
    void render_views(const CameraRec* cams, const uint64_t* seeds, size_t nviews, const RenderParams& p, uint8_t* out_rgb, double* out_acc,
                      RenderStats* stats);
    // rt_camera_rays: cam_ray (path_work.h) of every local pixel of p's frame and band partition, samples
    // [sample_base, sample_base + p.spp), entry (ly * W + lx) * p.spp + j; host buffers, or device ones on `device` with
    // RT_OUT_DEVICE (p.stream; null: the default stream).  rng_out may be null.  Needs no scene.  Blocking.
    static void camera_rays(int device, const CameraRec& cam, const RenderParams& p, uint32_t sample_base, double* rays_out, uint64_t* rng_out);
    // First-hit guide buffers of the local rows (k_guides): 10 doubles per pixel {albedo, normal, position, t} and,
    // when rays_out is non-NULL, the 7 doubles of every pixel-centre ray; host buffers, or device ones with RT_OUT_DEVICE.
    void render_guides(const CameraRec& cam, const RenderParams& p, double* guides, double* rays_out);
    // Noise-target rendering (rt_render_noise_target): p.spp is the per-pixel cap; every local pixel is traced until the
    // test of noise_target.hip retires it.  out_acc (3 f64), out_count (int32) and out_moments ({S1, S2} f64) per local
    // pixel are optional; host buffers, or device ones with RT_OUT_DEVICE.
    void render_noise_target(const CameraRec& cam, const RenderParams& p, const NoiseParams& np, uint8_t* out_rgb, double* out_acc,
                             int32_t* out_count, double* out_moments, RenderStats& stats, NoiseResult& result);
    // rt_tile_candidates: the tile lists render() would build for this camera and these parameters (tile_lists.h), as
    // one count per 8x8 tile of the local rows in tile order (kTileOverflow for a tile that walks the tree).  Returns
    // the number of tiles, or 0 when render() would build no lists (the scene, the option, the mode or the sample
    // count).  counts may be null (the number only); otherwise it holds at least `cap` >= tiles entries.
    int tile_candidates(const CameraRec& cam, const RenderParams& p, uint16_t* counts, size_t cap);
    // rt_scene_update_triangles / _spheres / _materials / _textures / _rects / _boxes / _objects (update_kinds.h): new values v for records
    // [first, first + n) of the kind's array in flat(), written into every device array that holds such a record.  device: v is a device pointer
    // read in place on `stream` (null: the scene's own, and the call waits); a host v goes through the workspace: a copy,
    // the kernels, a wait, as query_rays.  ms (may be null: then a device call on the caller's stream returns once
    // enqueued): HIP events around the kernels.  A scene's first update of a geometry kind, and of an appearance kind,
    // makes what the kind's kernels need beside the scene (blocking).  Leaves the host copy stale: generation() counts the
    // updates, current_flat() fetches before it answers.
    //   Triangles: 9 doubles, the vertices (k_update_tris); then a refit of every BVH box, one launch per tree level from
    //     the deepest up (k_refit_level; refit.h).  First: the slot boxes, the pad flags and the level table.
    //   Spheres: 4 doubles, cx, cy, cz, r, the LDS scene image's sphere planes included (k_update_spheres); then the same
    //     refit, then the image's box planes from the refitted nodes (k_image_nodes).  mat, flags and a moving sphere's
    //     d, t0, dt stay.  First: as Triangles (whichever comes first makes them for both).
    //   Materials (5 doubles: albedo, fuzz, ir), Textures (4: colour, scale): a record takes what its type uses
    //     (k_update_materials, k_update_textures); then every material of the scene gets its copies refreshed
    //     (k_derive_materials): the solid colour inlined into a MATF_SOLID record, and the image's shading-table entries.
    //     Types, links, boxes and the tree stay.  First: with an image, every material's entry code.
    //   Rects (5 doubles: a0, a1, b0, b1, k), Boxes (6: min xyz, max xyz): the records, their leaf-ordered copies and the
    //     prim objects' copies (k_update_rects, k_update_boxes); then the same refit.  axis and mat stay.  First: as
    //     Triangles.  A scene without a BVH has no slots and nothing to refit.
    //   Objects (4 doubles: ObjRec::p): a record takes what its kind uses -- a translate's offset, a rotate_y's sin and
    //     cos, a medium's neg_inv_density; a prim and a BVH nothing (k_update_objects).  Nothing is prepared or refitted:
    //     no box depends on them.
    void update(UpdateKind kind, const double* v, size_t first, size_t n, bool device, void* stream, double* ms);
    // rt_scene_update_texels: new bytes for rows [first_row, first_row + n_rows) of image `image` of flat().images (w x bpp
    // bytes per row), through update's runner -- buffers, stream, ms, generation() as there -- as one copy into the texel
    // pool, the only device copy of an image's bytes.  texel_generation() counts these calls: current_flat() fetches the
    // pool only after one.
    void update_texels(size_t image, const uint8_t* bytes, size_t first_row, size_t n_rows, bool device, void* stream, double* ms);
    uint64_t texel_generation() const;
    // rt_scene_lds_image_get: kLdsImageBytes + sizeof(TileReps), or 0 when the scene has no LDS image; out (may be null:
    // the size only) receives the device's bytes, or with `rebuilt` what build_lds_image makes of current_flat().
    size_t lds_image_get(bool rebuilt, uint8_t* out);
    uint64_t generation() const;
    // flat() with the sphere centres and radii, the triangle vertices, the 24 box floats of every node and the material and
    // texture fields an update can write (a metal's albedo and fuzz, a dielectric's ir, a solid texture's colour, a noise
    // texture's scale), a rect's a0, a1, b0, b1, k, a box's min and max and an object's p as the device holds them now (fetched when an update happened since the last fetch; waits for the
    // device).  Node order and child codes are the compiled ones.
    const FlatScene& current_flat();
    // rt_scene_bvh_get: the device's nodes (n_nodes x 128 bytes, as uploaded) and primitive references; either may be
    // null (both null: the counts only).  Uploads the scene if no call has yet; blocking.
    void bvh_get(void* nodes_out, uint32_t* primrefs_out, size_t& n_nodes, size_t& n_primrefs);
    int device() const;
    size_t scene_bytes() const;
    const FlatScene& flat() const;

private:
    Impl* impl_;
};

}  // namespace art

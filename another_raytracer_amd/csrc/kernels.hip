// kernels.hip — the wavefront path tracer for gfx950 (MI355X).
//
// The reference's recursive integrator (engine.h:58-68 _stochastic_sample + engine.h:447-466 _ray_color) is
// flattened into an iterative per-ray wavefront loop over a pool of P = k * npix paths (k samples of every local
// pixel per pass).  Per pass:
//   for depth d < max_depth:
//     k_extend<F>              closest hit over the world list (LDS-stack BVH traversal, f32 boxes, f64 leaf tests);
//                              at depth 0 it first generates the camera ray of every (pixel, sample) slot itself
//                              (PCG32 keyed by (seed, pixel, sample)); F = the scene's feature subset (layout.h),
//                              misses finish their path (L += T*background); hits are appended to one of five
//                              material queues (branch sorting for the shade stage)
//     k_shade<F, M, TF>        one launch per material type M present: emitted + scatter on that material's queue
//                              (branch-sorted shading); survivors go to the next active queue
//   k_accum                    adds the k per-slot radiances into the f64 pixel sums in sample order
// then k_finalize (write_color, color.h:6-22).  All queue sizes live on the device: extend/shade are persistent
// grids walking their input in a static grid-stride order, and appends go to kShards-way sharded queues, so no
// host round trip and no hot atomic word exists inside a render (path_work.h "work distribution").
//
// This file: the wavefront, accumulation, ray-query, guide and adaptive kernels, every k_paths_g instantiation but the
// two of k_paths_g_mesh.hip, and their launchers (launch.h).  k_paths has its own object (k_paths.hip); the host side
// is device_scene.hip and renderer.hip.
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "art.h"
#include "k_paths_g.h"
#include "launch.h"
#include "options.h"
#include "ray_launch.h"

#ifndef ART_EXTEND_MIN_WAVES
#define ART_EXTEND_MIN_WAVES 1  // __launch_bounds__ minimum waves per SIMD for k_extend (register budget knob)
#endif
namespace art {

// L: the scene is LDS-resident (DevScene::lds_image, spheres-only f64): nodes and leaf spheres are read from LDS.
// FUSE (L scenes with solid/checker textures, no media): every hit is shaded in place (shade_hit) and goes straight to
// the next depth's active queue -- no hit record, no material queues, no k_shade launches, one path-record round trip
// per bounce.
template <uint32_t F, bool L, bool FUSE>
__global__ __launch_bounds__(L ? kBlockL : kBlock, L ? 1 : ART_EXTEND_MIN_WAVES) void k_extend(DevScene S, PassGeom g, CameraRec cam, Work w, int d) {
    constexpr int B = L ? kBlockL : kBlock;
    // dynamic LDS: [scene image (L only)][traversal stack: g.stack entries x B lanes] (sized per scene at launch)
    // dynamic LDS only, so the scene image starts at LDS address 0 (device.h lds_f4)
    extern __shared__ __align__(16) uint8_t smem[];
    uint32_t* pre = reinterpret_cast<uint32_t*>(smem + extend_pre_offset(L, g.stack));
    const uint8_t* lds = smem;
    // row 0 of the stack region is this lane's sentinel (device.h traverse), entries start at row 1
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem + (L ? kLdsImageBytes : 0u)) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);

    // input: depth 0 = every slot (identity; padding slots are skipped), deeper = the kShards active shards
    uint32_t count;
    if (d == 0) {
        count = g.P;
    } else {
        block_prefix(pre, kShards, threadIdx.x < kShards ? *counter(w, d, 0, threadIdx.x) : 0u);
        count = pre[kShards];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(w.segments, static_cast<unsigned long long>(d == 0 ? g.live : count));
    if constexpr (L) {
        // deep bounces have few paths: blocks without a batch leave before paying for the image
        if (static_cast<uint64_t>(blockIdx.x) * B >= count) return;
        load_lds_image<B>(S.lds_image, smem);
        __syncthreads();
    }
    const uint32_t* in = w.active[d & 1];
    const uint32_t wave = blockIdx.x * (B / 64) + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * (B / 64);
    const int shard = static_cast<int>(wave % kShards);
#ifdef ART_STATS
    unsigned long long tm_load = 0, tm_trace = 0, tm_shade = 0, tm_app = 0, tm_prev = __builtin_amdgcn_s_memtime();
#endif
    for (uint32_t b = wave; b * 64u < count; b += nwaves) {
        const uint32_t i = b * 64u + __lane_id();
        int mtype = -1;
        bool cont = false;  // FUSE: the path continues at depth d + 1
        uint32_t q = 0;
        bool live = i < count;
        PathState st;
        if (live) {
            if (d == 0) {
                q = i;
                int lx, ly;
                uint32_t qi, j;
                slot_split(g, i, qi, j);
                live = slot_pixel(g, qi, lx, ly);
                if (live) gen_ray(g, cam, j, lx, ly, st);
            } else {
                const int s = find_segment(pre, kShards, i);
                q = in[s * g.cap + (i - pre[s])];
                // FUSE: the throughput/radiance line is needed after the traversal; issuing it with the ray line
                // puts its HBM latency under the traversal instead of after it
                load_path(w.paths, q, st, FUSE);
            }
        }
        ART_TICK(tm_load);
        if (FUSE) {
            double t;
            HitOut h{0, 0, kMatUnknown};
            const bool hitf = live && trace_world<F, B, L>(S, lds, st.ray, stk, st.rng, t, h);
            ART_TICK(tm_trace);
            if (hitf) {
                cont = shade_hit_lds(lds, h.obj >> 16, h.mt, t, d + 1 >= g.max_depth, st);
                if (cont) store_path(w.paths, q, st);
                else store_res(w.res, q, st.L);
            } else if (live) {  // engine.h:455-456: miss -> background
                st.L = st.L + st.T * mk(S.bg[0], S.bg[1], S.bg[2]);
                store_res(w.res, q, st.L);
            }
            ART_TICK(tm_shade);
        } else if (live) {
            double t;
            HitOut h{0, 0, kMatUnknown};
            if (trace_world<F, B, L>(S, lds, st.ray, stk, st.rng, t, h)) {
                w.hits[q] = HitRecD{t, h.prim, h.obj};
                if (L && h.mt != kMatUnknown) {
                    mtype = static_cast<int>(h.mt);  // from the LDS image: no dependent global loads
                } else {
                    uint32_t m;
                    if ((F & F_MEDIA) && h.prim == kMediumHit) {
                        m = static_cast<uint32_t>(S.objs[S.world[h.obj & 0xFFFFu]].b);
                    } else if (F == F_SPHERE) {
                        m = S.spheres[primref_index(h.prim)].mat;
                    } else {
                        const uint32_t idx = primref_index(h.prim);
                        switch (primref_type(h.prim)) {
                            case PRIM_SPHERE: m = S.spheres[idx].mat; break;
                            case PRIM_TRIANGLE: m = S.tris[idx].mat; break;
                            case PRIM_RECT: m = S.rects[idx].mat; break;
                            default: m = S.boxes[idx].mat; break;
                        }
                    }
                    mtype = static_cast<int>(S.mats[m].type);
                }
                if (d == 0) store_path(w.paths, q, st);
                else if (F & F_MEDIA) store_rng(w.paths, q, st.rng);
            } else {  // engine.h:455-456: miss -> background
                if (d != 0) load_path(w.paths, q, st, true);
                st.L = st.L + st.T * mk(S.bg[0], S.bg[1], S.bg[2]);
                store_res(w.res, q, st.L);
            }
        }
        if constexpr (FUSE) wave_append(cont, q, w.active[(d + 1) & 1] + static_cast<size_t>(shard) * g.cap, counter(w, d + 1, 0, shard));
        else append_by_material(mtype, q, w, g, d, shard);
        ART_TICK(tm_app);
    }
#ifdef ART_STATS
    if (__lane_id() == 0) {
        atomicAdd(&g_art_stats[8], tm_load);
        atomicAdd(&g_art_stats[9], tm_trace);
        atomicAdd(&g_art_stats[10], tm_shade);
        atomicAdd(&g_art_stats[11], tm_app);
    }
#endif
}

// Input: the kShards shards of material queue M at depth d (the extend stage sorted hits by material type).
template <uint32_t F, uint32_t M, uint32_t TF>
__global__ __launch_bounds__(kBlock) void k_shade(DevScene S, PassGeom g, Work w, int d) {
    __shared__ uint32_t pre[kShards + 1];
    block_prefix(pre, kShards, threadIdx.x < kShards ? *counter(w, d, 1 + static_cast<int>(M), threadIdx.x) : 0u);
    const uint32_t total = pre[kShards];
    const uint32_t* in = w.mq + static_cast<size_t>(M) * kShards * g.cap;
    const bool last = d + 1 >= g.max_depth;
    uint32_t* next = w.active[(d + 1) & 1];
    const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * (kBlock / 64);
    const int shard = static_cast<int>(wave % kShards);
    for (uint32_t b = wave; b * 64u < total; b += nwaves) {
        const uint32_t i = b * 64u + __lane_id();
        bool cont = false;
        uint32_t q = 0;
        if (i < total) {
            const int sg = find_segment(pre, kShards, i);
            q = in[static_cast<size_t>(sg) * g.cap + (i - pre[sg])];
            PathState st;
            load_path(w.paths, q, st, true);
            const HitRecD h = w.hits[q];
            Surf s;
            world_surface<F, (TF & TF_IMAGE) != 0>(S, HitOut{h.prim, h.obj, kMatUnknown}, st.ray, h.t, s, uv_table(S));
            const MatRec& mat = S.mats[s.mat];
            if (M == MAT_LIGHT) st.L = st.L + st.T * mat_tex_value<TF>(S, mat, s.u, s.v, s.p);  // material.h:114-116
            if (M != MAT_LIGHT && !last) {
                V3 att, dir;
                if (scatter<M, TF>(S, mat, s, st, att, dir)) {
                    st.T = st.T * att;
                    st.ray.o = s.p;
                    st.ray.d = dir;
                    store_path(w.paths, q, st);
                    cont = true;
                }
            }
            if (!cont) store_res(w.res, q, st.L);
        }
        wave_append(cont, q, next + static_cast<size_t>(shard) * g.cap, counter(w, d + 1, 0, shard));
    }
}

__global__ __launch_bounds__(256) void k_accum(PassGeom g, Work w) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= g.npix_pad) return;
    int lx, ly;
    if (!slot_pixel(g, qi, lx, ly)) return;
    // pixel sums: per local pixel, or per list entry in pixel-list mode
    double* a = w.acc + 3 * (g.list ? static_cast<size_t>(qi) : static_cast<size_t>(ly) * g.W + lx);
    double r = a[0], gg = a[1], b = a[2];
    for (uint32_t j = 0; j < g.k; ++j) {  // sample order == the reference's `pixel_color +=` order
        double x, y, z;
        load_res(w.res, j * g.npix_pad + qi, x, y, z);
        r += x;
        gg += y;
        b += z;
    }
    a[0] = r;
    a[1] = gg;
    a[2] = b;
}

// engine_mode::parallel_images (engine.h:378-445): sample s of a pixel belongs to partial image s / m (m = spp / 4).
// Its samples are summed in order into the quarter sum q (f64, as the reference's pixel_color); when the quarter's
// last sample is in, write_color_raw<float> rounds q to float and the running image sum takes it:
// acc = ((c1 + c2) + c3) + c4 in double, the reference's `pixel_color1 + ... + pixel_color4`.  q persists across passes.
__global__ __launch_bounds__(256) void k_accum_images(PassGeom g, Work w, double* qsum, uint32_t m) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= g.npix_pad) return;
    int lx, ly;
    if (!slot_pixel(g, qi, lx, ly)) return;
    const size_t pix = static_cast<size_t>(ly) * g.W + lx;
    double* a = w.acc + 3 * pix;
    double* q = qsum + 3 * pix;
    double ar = a[0], ag = a[1], ab = a[2], qr = q[0], qg = q[1], qb = q[2];
    for (uint32_t j = 0; j < g.k; ++j) {
        double x, y, z;
        load_res(w.res, j * g.npix_pad + qi, x, y, z);
        qr += x;
        qg += y;
        qb += z;
        if ((g.sample_base + j + 1) % m == 0) {
            ar += static_cast<double>(static_cast<float>(qr));
            ag += static_cast<double>(static_cast<float>(qg));
            ab += static_cast<double>(static_cast<float>(qb));
            qr = qg = qb = 0.0;
        }
    }
    a[0] = ar;
    a[1] = ag;
    a[2] = ab;
    q[0] = qr;
    q[1] = qg;
    q[2] = qb;
}

// Ray queries (rt_trace_rays): the world's closest hit (hittable_list::hit, hittable_list.cpp:5-19) of n caller-given
// rays through the renderer's own traversal -- the LDS image (L) or the HBM scene -- and the surface normal
// (hit_record::set_face_normal), so traversal edge cases (axis-parallel rays, origins on faces) can be checked one ray
// at a time against the oracle.  Ray i's medium draws come from the PCG stream pcg_seed(0, i, 0).
template <uint32_t F, bool L>
__global__ __launch_bounds__(L ? kBlockL : kBlock) void k_trace_rays(DevScene S, const double* rays, uint32_t n, uint32_t stack_rows,
                                                                       double* t_out, double* n_out) {
    constexpr int B = L ? kBlockL : kBlock;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem + (L ? kLdsImageBytes : 0u)) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    if constexpr (L) {
        load_lds_image<B>(S.lds_image, smem);
        __syncthreads();
    }
    (void)stack_rows;
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i >= n) return;
    const double* q = rays + 7 * static_cast<size_t>(i);
    Ray r;
    r.o = mk(q[0], q[1], q[2]);
    r.d = mk(q[3], q[4], q[5]);
    r.tm = q[6];
    uint64_t rng = pcg_seed(0, i, 0);
    double t = 0.0;
    HitOut h{0, 0, kMatUnknown};
    if (trace_world<F, B, L>(S, L ? smem : nullptr, r, stk, rng, t, h)) {
        Surf s;
        world_surface<F, false>(S, h, r, t, s);
        t_out[i] = t;
        n_out[3 * i] = s.n.x;
        n_out[3 * i + 1] = s.n.y;
        n_out[3 * i + 2] = s.n.z;
    } else {
        t_out[i] = __builtin_inf();
        n_out[3 * i] = n_out[3 * i + 1] = n_out[3 * i + 2] = 0.0;
    }
}

// Ray queries with the hit record (rt_query_rays, closest mode): k_trace_rays' search over [0.001, t_max[i]] (t_max null:
// +inf), constant_medium objects skipped when no_media, and the whole hit_record as world_surface rebuilds it.  Record per
// ray (RT_HIT_DOUBLES = 12): t, normal[3], point[3], u, v, front_face, prim, mat.  u, v: get_sphere_uv / the rect and
// triangle formulas for every material (prim_surface ALLUV; the trig table is uploaded with every scene); 0 where the
// reference's hit() sets none (moving spheres, media).  prim: the compiled primitive reference (type:2 | index:30), -2 for
// a medium scattering event; mat: the material index.  A miss: t = point = +inf, prim = mat = -1, everything else 0.
// With t_max null and no_media 0 the traversal is k_trace_rays' own: the same t and normal.
template <uint32_t F, bool L>
__global__ __launch_bounds__(L ? kBlockL : kBlock) void k_query_rays(DevScene S, const double* rays, const double* t_max, uint32_t n,
                                                                       uint32_t no_media, double* hits) {
    constexpr int B = L ? kBlockL : kBlock;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem + (L ? kLdsImageBytes : 0u)) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    if constexpr (L) {
        load_lds_image<B>(S.lds_image, smem);
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i >= n) return;
    const double* q = rays + 7 * static_cast<size_t>(i);
    Ray r;
    r.o = mk(q[0], q[1], q[2]);
    r.d = mk(q[3], q[4], q[5]);
    r.tm = q[6];
    const double inf = __builtin_inf();
    const double tm = t_max ? t_max[i] : inf;
    uint64_t rng = pcg_seed(0, i, 0);
    double t = 0.0;
    HitOut h{0, 0, kMatUnknown};
    double* o = hits + 12 * static_cast<size_t>(i);
    if (trace_world<F, B, L>(S, L ? smem : nullptr, r, stk, rng, t, h, tm, no_media != 0)) {
        Surf s;
        world_surface<F, true, true, true>(S, h, r, t, s, uv_table(S));
        o[0] = t;
        o[1] = s.n.x; o[2] = s.n.y; o[3] = s.n.z;
        o[4] = s.p.x; o[5] = s.p.y; o[6] = s.p.z;
        o[7] = s.u; o[8] = s.v;
        o[9] = s.ff ? 1.0 : 0.0;
        o[10] = h.prim == kMediumHit ? -2.0 : static_cast<double>(h.prim);
        o[11] = static_cast<double>(s.mat);
    } else {
        o[0] = inf;
        o[1] = o[2] = o[3] = 0.0;
        o[4] = o[5] = o[6] = inf;
        o[7] = o[8] = o[9] = 0.0;
        o[10] = o[11] = -1.0;
    }
}

// Occlusion queries (rt_query_rays with RT_Q_ANY_HIT): occluded[i] = 1 iff some non-medium primitive is accepted by its own
// hit test in [0.001, t_max[i]] (occlude_world: the any-hit traversal, the world walk stopping at the first occluder).  F
// carries no media bits; no RNG.  ANY: traverse's child order (1 sorted, 2 node order: option query.any_sorted; the node
// order is the default, DESIGN.md 4.7 measured both).
template <uint32_t F, bool L, int ANY>
__global__ __launch_bounds__(L ? kBlockL : kBlock) void k_occlude_rays(DevScene S, const double* rays, const double* t_max, uint32_t n,
                                                                         uint8_t* occluded) {
    constexpr int B = L ? kBlockL : kBlock;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem + (L ? kLdsImageBytes : 0u)) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    if constexpr (L) {
        load_lds_image<B>(S.lds_image, smem);
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * B + threadIdx.x;
    if (i >= n) return;
    const double* q = rays + 7 * static_cast<size_t>(i);
    Ray r;
    r.o = mk(q[0], q[1], q[2]);
    r.d = mk(q[3], q[4], q[5]);
    r.tm = q[6];
    const double tm = t_max ? t_max[i] : __builtin_inf();
    occluded[i] = occlude_world<F, B, L, ANY>(S, L ? smem : nullptr, r, stk, tm) ? 1 : 0;
}

// First-hit guide buffers (rt_render_guides): one ray per local pixel through the pixel centre -- no render RNG draw,
// no lens offset, time0 -- traced exactly as k_trace_rays traces it (ray index = global pixel gy * W + i, so a whole
// frame's t and normal equal rt_trace_rays of rays_out), plus the hit point (Surf::p) and the first hit's albedo:
// mat_tex_value for lambertian / isotropic, MatRec::albedo for metal, 1 for dielectric, diffuse_light and a miss.
// Record per local pixel (RT_GUIDE_DOUBLES = 10): albedo[3], normal[3], position[3], t; a miss has t = position = +inf.
template <uint32_t F, bool L, uint32_t TF>
__global__ __launch_bounds__(L ? kBlockL : kBlock) void k_guides(DevScene S, GuideGeom g, CameraRec cam, double* guides, double* rays_out) {
    constexpr int B = L ? kBlockL : kBlock;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem + (L ? kLdsImageBytes : 0u)) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    if constexpr (L) {
        load_lds_image<B>(S.lds_image, smem);
        __syncthreads();
    }
    const uint32_t lp = blockIdx.x * B + threadIdx.x;
    if (lp >= static_cast<uint32_t>(g.rows) * static_cast<uint32_t>(g.W)) return;
    const int ly = static_cast<int>(lp / static_cast<uint32_t>(g.W));
    const int lx = static_cast<int>(lp - static_cast<uint32_t>(ly) * static_cast<uint32_t>(g.W));
    const int gy = band_global_row(ly, g.band_rows, g.band_count, g.band_index);
    const double s = (static_cast<double>(lx) + 0.5) / static_cast<double>(g.W - 1);
    const double t_img = (static_cast<double>(g.H - 1 - gy) + 0.5) / static_cast<double>(g.H - 1);
    Ray r;
    r.o = ld3(cam.origin);
    r.d = ld3(cam.llc) + s * ld3(cam.horizontal) + t_img * ld3(cam.vertical) - ld3(cam.origin);
    r.tm = cam.time0;
    if (rays_out) {
        double* q = rays_out + 7 * static_cast<size_t>(lp);
        q[0] = r.o.x; q[1] = r.o.y; q[2] = r.o.z;
        q[3] = r.d.x; q[4] = r.d.y; q[5] = r.d.z;
        q[6] = r.tm;
    }
    uint64_t rng = pcg_seed(0, static_cast<uint32_t>(gy) * static_cast<uint32_t>(g.W) + static_cast<uint32_t>(lx), 0);
    double t = 0.0;
    HitOut h{0, 0, kMatUnknown};
    const double inf = __builtin_inf();
    V3 alb = mk(1.0, 1.0, 1.0), nrm = mk(0.0, 0.0, 0.0), pos = mk(inf, inf, inf);
    double t_hit = inf;
    if (trace_world<F, B, L>(S, L ? smem : nullptr, r, stk, rng, t, h)) {
        Surf sf;
        world_surface<F, (TF & TF_IMAGE) != 0, (TF & (TF_IMAGE | TF_BARY)) != 0>(S, h, r, t, sf, uv_table(S));
        const MatRec& m = S.mats[sf.mat];
        if (m.type == MAT_LAMBERTIAN || m.type == MAT_ISOTROPIC) alb = mat_tex_value<TF>(S, m, sf.u, sf.v, sf.p);
        else if (m.type == MAT_METAL) alb = ld3(m.albedo);
        nrm = sf.n;
        pos = sf.p;
        t_hit = t;
    }
    double* o = guides + 10 * static_cast<size_t>(lp);
    o[0] = alb.x; o[1] = alb.y; o[2] = alb.z;
    o[3] = nrm.x; o[4] = nrm.y; o[5] = nrm.z;
    o[6] = pos.x; o[7] = pos.y; o[8] = pos.z;
    o[9] = t_hit;
}

__global__ void k_finalize(const double* acc, uint8_t* rgb, uint32_t n, int spp) {  // color.h:6-22
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double scale = 1.0 / spp;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double x = sqrt(scale * acc[3 * i + c]);
        x = x < 0.0 ? 0.0 : (x > 0.999 ? 0.999 : x);
        rgb[3 * i + c] = static_cast<uint8_t>(256 * x);
    }
}

// ------------------------------------------------------------------------------------------------ adaptive mode
// engine_mode::adaptive (engine.h:96-333) as four traced levels over the local image, whose rows group into 12-px
// "big squares" (6-px mid and 3-px small squares inside).  Level 0 traces every big square's 4 corners; level L+1
// traces the new corners (12 per square) of the sub-squares of every level-L square whose corner heuristic fired, and
// level 3 the 5 remaining pixels of each subdivided small square; k_adapt_fill then interpolates every pixel no level
// traced from the corners of the deepest square that was not subdivided.  The work image is the reference's int frame
// (-1 = not yet written); every traced pixel's value depends only on its (pixel, sample) streams, so a corner shared by
// two levels is traced once.

// write_color<int> (color.h:6-22) of list entry e's pixel sums into the work image.
__global__ void k_adapt_store(const uint32_t* list, uint32_t n, const double* acc, int spp, int32_t* work) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const double scale = 1.0 / spp;
    int32_t* o = work + 3 * static_cast<size_t>(list[e]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double x = sqrt(scale * acc[3 * static_cast<size_t>(e) + c]);
        x = x < 0.0 ? 0.0 : (x > 0.999 ? 0.999 : x);
        o[c] = static_cast<int32_t>(256 * x);
    }
}

// list_mode 1 (the device-counted levels): the pixel sums of every list entry -- its k samples on consecutive slots,
// summed in sample order from +0.0 as k_accum sums them into the zeroed accumulator (engine.h:58-68) -- written into
// the work image as k_adapt_store writes them.  The entry count is list[-1].
// One wave per entry (r6o): the entry's k records are consecutive (entry-major slots), so the wave reads 64 of them
// per coalesced load into LDS and lanes 0-2 (one per channel) add them in sample order from LDS.  One thread per
// entry, 100 records each, left every level's accumulation latency-bound at ~62 us whatever its size (rocprofv3
// kernel trace of the default run; 45 us with 20 loads in flight per thread).
constexpr int kAdaptAccumWaves = 4;
__global__ __launch_bounds__(64 * kAdaptAccumWaves) void k_adapt_accum(const uint32_t* list, const ResRec* res, uint32_t k, int spp,
                                                                      int32_t* work) {
    __shared__ double buf[kAdaptAccumWaves][3 * 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t e = blockIdx.x * kAdaptAccumWaves + wv;
    if (e >= list[-1]) return;  // wave-uniform
    double* b = buf[wv];
    double acc = 0.0;  // lane c < 3: channel c
    const ResRec* r = res + static_cast<size_t>(e) * k;
    for (uint32_t j0 = 0; j0 < k; j0 += 64) {
        const uint32_t n = min(64u, k - j0);
        if (lane < n) {
            double x, y, z;
            load_res(r, j0 + lane, x, y, z);
            b[3 * lane] = x;
            b[3 * lane + 1] = y;
            b[3 * lane + 2] = z;
        }
        // one wave: its LDS writes complete before its reads (in-order LDS, the waitcnt), and the compiler keeps them apart
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane < 3)
            for (uint32_t i = 0; i < n; ++i) acc += b[3 * i + lane];
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next chunk's writes after these reads
    }
    if (lane >= 3) return;
    const double scale = 1.0 / spp;
    double x = sqrt(scale * acc);
    x = x < 0.0 ? 0.0 : (x > 0.999 ? 0.999 : x);
    work[3 * static_cast<size_t>(list[e]) + lane] = static_cast<int32_t>(256 * x);
}

// _compute_corners_heuristic (engine.h:96-136): any squared RGB distance between neighbouring corners > 100.
__device__ __forceinline__ bool adapt_subdivide(const int32_t* work, int W, int x, int y, int L) {
    const int32_t* c1 = work + 3 * (static_cast<size_t>(y) * W + x);
    const int32_t* c2 = work + 3 * (static_cast<size_t>(y) * W + x + L - 1);
    const int32_t* c3 = work + 3 * (static_cast<size_t>(y + L - 1) * W + x);
    const int32_t* c4 = work + 3 * (static_cast<size_t>(y + L - 1) * W + x + L - 1);
    auto d = [](const int32_t* a, const int32_t* b) {
        return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
    };
    return d(c1, c2) > 100 || d(c2, c4) > 100 || d(c4, c3) > 100 || d(c3, c1) > 100;
}

// Level-0 list: the four corners of every big square (ul, ur, bl, br: engine.h:223-233).
__global__ void k_adapt_corners(uint32_t* list, int W, int sqx, uint32_t nsq) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0) list[-1] = 4 * nsq;  // the entry count of a device-counted list (PassGeom::list_mode)
    if (s >= nsq) return;
    const uint32_t x = (s % sqx) * kBig, y = (s / sqx) * kBig;
    list[4 * s + 0] = y * W + x;
    list[4 * s + 1] = y * W + x + kBig - 1;
    list[4 * s + 2] = (y + kBig - 1) * W + x;
    list[4 * s + 3] = (y + kBig - 1) * W + x + kBig - 1;
}

// Heuristic of every level-`level` square (0: big, 1: mid, 2: small) whose parent was subdivided, and the list of
// the pixels the next level traces.  flags[level] holds one byte per square: index big, big*4+mid, (big*4+mid)*4+small.
__global__ void k_adapt_level(int level, int32_t* work, int W, int sqx, uint32_t nsq, uint8_t* f0, uint8_t* f1, uint8_t* f2, uint32_t* list,
                              uint32_t* count) {
    const uint32_t per = level == 0 ? 1u : (level == 1 ? 4u : 16u);
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nsq * per) return;
    const uint32_t big = id / per, sub = id % per;
    int x = static_cast<int>((big % sqx) * kBig), y = static_cast<int>((big / sqx) * kBig);
    int L = kBig;
    if (level >= 1) {
        if (!f0[big]) return;
        const uint32_t mid = level == 1 ? sub : sub / 4;
        x += static_cast<int>(mid & 1u) * kMid;
        y += static_cast<int>(mid >> 1) * kMid;
        L = kMid;
        if (level == 2) {
            if (!f1[big * 4 + mid]) return;
            x += static_cast<int>(sub & 1u) * kSmall;
            y += static_cast<int>((sub >> 1) & 1u) * kSmall;
            L = kSmall;
        }
    }
    const bool split = adapt_subdivide(work, W, x, y, L);
    (level == 0 ? f0 : (level == 1 ? f1 : f2))[id] = split ? 1 : 0;
    if (!split) return;
    if (level < 2) {  // the 16 corners of the 4 sub-squares minus this square's own 4 corners
        const int h = L / 2;
        const int xs[4] = {x, x + h - 1, x + h, x + L - 1}, ys[4] = {y, y + h - 1, y + h, y + L - 1};
        const uint32_t base = atomicAdd(count, 12u);
        uint32_t k = 0;
        for (int b = 0; b < 4; ++b)
            for (int a = 0; a < 4; ++a) {
                if ((a == 0 || a == 3) && (b == 0 || b == 3)) continue;
                list[base + k++] = static_cast<uint32_t>(ys[b]) * W + static_cast<uint32_t>(xs[a]);
            }
    } else {  // engine.h:268-278: the 5 non-corner pixels of the 3-px square
        const uint32_t base = atomicAdd(count, 5u);
        list[base + 0] = static_cast<uint32_t>(y) * W + x + 1;
        list[base + 1] = static_cast<uint32_t>(y + 1) * W + x;
        list[base + 2] = static_cast<uint32_t>(y + 1) * W + x + 1;
        list[base + 3] = static_cast<uint32_t>(y + 1) * W + x + 2;
        list[base + 4] = static_cast<uint32_t>(y + 2) * W + x + 1;
    }
}

// interpolate_square (engine.h:185-219) with _interpolate (engine.h:138-149, v/t == (1/t)*v), then the u8 frame.
__global__ void k_adapt_fill(int32_t* work, uint8_t* rgb, int W, int rows, int sqx, const uint8_t* f0, const uint8_t* f1, const uint8_t* f2) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= static_cast<uint32_t>(W) * static_cast<uint32_t>(rows)) return;
    const int x = static_cast<int>(p % W), y = static_cast<int>(p / W);
    int32_t* o = work + 3 * static_cast<size_t>(p);
    if (o[0] < 0) {
        const uint32_t big = static_cast<uint32_t>(y / kBig) * sqx + static_cast<uint32_t>(x / kBig);
        int x1 = (x / kBig) * kBig, y1 = (y / kBig) * kBig, L = kBig;
        if (f0[big]) {
            const uint32_t mid = static_cast<uint32_t>(((y % kBig) / kMid) * 2 + (x % kBig) / kMid);
            x1 += (x % kBig) / kMid * kMid;
            y1 += (y % kBig) / kMid * kMid;
            L = kMid;
            if (f1[big * 4 + mid]) {
                x1 += (x % kMid) / kSmall * kSmall;
                y1 += (y % kMid) / kSmall * kSmall;
                L = kSmall;
            }
        }
        const int x2 = x1 + L - 1, y2 = y1 + L - 1;
        const int32_t* q11 = work + 3 * (static_cast<size_t>(y1) * W + x1);
        const int32_t* q12 = work + 3 * (static_cast<size_t>(y2) * W + x1);
        const int32_t* q21 = work + 3 * (static_cast<size_t>(y1) * W + x2);
        const int32_t* q22 = work + 3 * (static_cast<size_t>(y2) * W + x2);
        const double ix = 1.0 / static_cast<double>(x2 - x1), iy = 1.0 / static_cast<double>(y2 - y1);
        const double ax = x2 - x, bx = x - x1, ay = y2 - y, by = y - y1;
        int32_t v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double r1 = ix * (ax * static_cast<double>(q11[c])) + ix * (bx * static_cast<double>(q21[c]));
            const double r2 = ix * (ax * static_cast<double>(q12[c])) + ix * (bx * static_cast<double>(q22[c]));
            v[c] = static_cast<int32_t>(iy * (ay * r1) + iy * (by * r2));
        }
        // written after all three reads: a neighbour never reads this pixel (only corners, which are traced)
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
    (void)f2;
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[3 * static_cast<size_t>(p) + c] = static_cast<uint8_t>(o[c]);
}

// The LDS-scene kernels address the scene image at LDS address 0 (device.h lds_f4): they must declare no static
// __shared__ variables, which would be placed first.
bool static_lds_is_zero(const void* kernel) {
    hipFuncAttributes a{};
    HIP_OK(hipFuncGetAttributes(&a, kernel));
    if (a.sharedSizeBytes != 0) throw std::runtime_error("LDS-scene kernel has static LDS: the scene image would not start at address 0");
    return true;
}
// Launch configuration per (kernel, device, dynamic LDS bytes): the > 64 KiB dynamic-LDS attribute, which
// hipFuncSetAttribute records per device, and the blocks per CU of a persistent grid (every block the CUs hold at
// once).  Scenes on different devices may render from different host threads, so the cache is
// mutex-guarded instead of living in function-local statics shared by all devices.
int blocks_per_cu(const void* kernel, int block, size_t lds) {
    static std::mutex mtx;
    static std::map<std::tuple<const void*, int, size_t>, int> cache;
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    const std::tuple<const void*, int, size_t> key{kernel, dev, lds};
    std::lock_guard<std::mutex> lock(mtx);
    const auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    if (lds > 64 * 1024) HIP_OK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    cache.emplace(key, per_cu);
    return per_cu;
}
template <uint32_t F, uint32_t M, uint32_t TF>
static int shade_blocks(int num_cu) {
    return blocks_per_cu(reinterpret_cast<const void*>(k_shade<F, M, TF>), kBlock, 0) * num_cu;
}
// Textured materials get the "solid + checker" instantiation unless the scene holds noise or image textures.
template <uint32_t F, uint32_t M>
static void launch_shade(uint32_t mat_types, bool tex_basic, int num_cu, hipStream_t st, const DevScene& S, const PassGeom& g,
                         const Work& w, int d) {
    if (!(mat_types & (1u << M))) return;
    constexpr bool textured = M == MAT_LAMBERTIAN || M == MAT_LIGHT || M == MAT_ISOTROPIC;
    if (!textured || tex_basic)
        hipLaunchKernelGGL((k_shade<F, M, kTexBasic>), dim3(shade_blocks<F, M, kTexBasic>(num_cu)), dim3(kBlock), 0, st, S, g, w, d);
    else
        hipLaunchKernelGGL((k_shade<F, M, TF_ALL>), dim3(shade_blocks<F, M, TF_ALL>(num_cu)), dim3(kBlock), 0, st, S, g, w, d);
}
// One bounce (extend + one shade launch per material type present) of the smallest kernel instantiation that
// covers the scene's features.
template <uint32_t F, bool L, bool FUSE>
static void launch_extend(int num_cu, hipStream_t st, const DevScene& S, const PassGeom& g, const CameraRec& cam, const Work& w, int d) {
    const size_t lds = extend_lds_bytes(L, g.stack);
    static const bool checked = !L || static_lds_is_zero(reinterpret_cast<const void*>(k_extend<F, L, FUSE>));
    (void)checked;
    // num_cu (256) is a multiple of 8: the wave count is a multiple of kShards
    const int blocks = blocks_per_cu(reinterpret_cast<const void*>(k_extend<F, L, FUSE>), L ? kBlockL : kBlock, lds) * num_cu;
    hipLaunchKernelGGL((k_extend<F, L, FUSE>), dim3(blocks), dim3(L ? kBlockL : kBlock), lds, st, S, g, cam, w, d);
}
// One bounce (extend + one shade launch per material type present, unless fused) of the smallest kernel
// instantiation that covers the scene's features.
template <uint32_t F>
static void launch_bounce(uint32_t mat_types, bool tex_basic, int variant, int num_cu, hipStream_t st, const DevScene& S, const PassGeom& g,
                          const CameraRec& cam, const Work& w, int d, const std::function<void()>& mark) {
    if (mark) mark();
    if constexpr (F == kFeatSpheres) {
        if (variant == EXT_FUSED) launch_extend<F, true, true>(num_cu, st, S, g, cam, w, d);
        else if (variant == EXT_LDS) launch_extend<F, true, false>(num_cu, st, S, g, cam, w, d);
        else launch_extend<F, false, false>(num_cu, st, S, g, cam, w, d);
    } else {
        launch_extend<F, false, false>(num_cu, st, S, g, cam, w, d);
    }
    if (mark) mark();
    if (variant != EXT_FUSED) {
        launch_shade<F, MAT_LAMBERTIAN>(mat_types, tex_basic, num_cu, st, S, g, w, d);
        launch_shade<F, MAT_METAL>(mat_types, tex_basic, num_cu, st, S, g, w, d);
        launch_shade<F, MAT_DIELECTRIC>(mat_types, tex_basic, num_cu, st, S, g, w, d);
        launch_shade<F, MAT_LIGHT>(mat_types, tex_basic, num_cu, st, S, g, w, d);
        launch_shade<F, MAT_ISOTROPIC>(mat_types, tex_basic, num_cu, st, S, g, w, d);
    }
    if (mark) mark();
}
int extend_variant(const DeviceScene& ds, int flags) {
    if (!ds.lds_scene || (flags & RT_GLOBAL_SCENE) || (ds.features & ~kFeatSpheres) != 0)
        return !(flags & RT_WAVEFRONT) ? EXT_MEGA_G : EXT_GLOBAL;
    // an LDS-image scene whose shading the LDS table cannot hold (noise / image textures: the two perlin spheres) runs
    // the persistent HBM-scene kernel, not the per-depth LDS wavefront one: r5 A/B (profiles/r5c_ab_scene3.txt) scene 3
    // 9 586 -> 23 864 Msamples/s; the wavefront variant stays reachable with RT_SPLIT_SHADE / RT_WAVEFRONT
    if (!ds.lds_shade)
        return !(flags & (RT_SPLIT_SHADE | RT_WAVEFRONT)) ? EXT_MEGA_G : EXT_LDS;
    if (flags & RT_SPLIT_SHADE) return EXT_LDS;
    return (flags & RT_WAVEFRONT) ? EXT_FUSED : EXT_MEGA;
}
// The persistent kernels' waves index the camera-ray rings (kPoolWavesPerCu per CU allocated)
static void check_ring_waves(int blocks, int block, int num_cu) {
    const size_t padded = (static_cast<size_t>(blocks) + kXcds - 1) / kXcds * kXcds;  // the XCD-major wave index (PathPool::init)
    if (padded * static_cast<size_t>(block / 64) > static_cast<size_t>(num_cu) * kPoolWavesPerCu)
        throw std::runtime_error("internal: persistent grid larger than the camera-ray rings");
}
template <uint32_t F, uint32_t TF>
static KernelId launch_paths_g_ft(int num_cu, hipStream_t st, const DevScene& S, const PassGeom& g, const CameraRec& cam,
                              const Work& w, uint32_t* next_slot) {
    // one persistent launch of the LM instantiation (a compile-time value) that was chosen
    auto go = [&](auto lm, int block, size_t lds, const DevScene& scene, const PassGeom& geom) -> KernelId {
        constexpr int LM = decltype(lm)::value;
        const int blocks = blocks_per_cu(reinterpret_cast<const void*>(k_paths_g<F, TF, LM>), block, lds) * num_cu;
        check_ring_waves(blocks, block, num_cu);
        hipLaunchKernelGGL((k_paths_g<F, TF, LM>), dim3(blocks), dim3(block), lds, st, scene, geom, cam, w, next_slot);
        return {F, TF, LM};
    };
    // g.stack = stack_rows: sentinel + entries + spare row
    const size_t lm_head = paths_g_head_bytes(g.stack, kBlockM, (F & F_CODE16) != 0) + paths_g_world_bytes(S.nworld, S.n_objs, lds_mats<TF>(S.n_mats));
    const size_t lds_m = align16(align128(lm_head) + paths_g_mesh_bytes(S.n_nodes, S.n_primrefs, (F & F_TRI) ? S.n_primrefs : 0u));
    // LM 1 also for a scene without BVH nodes (the earth scene: one sphere object): its world and objects in LDS and no
    // LM 0 suspend machinery (which spilled the earth's textured kernel)
    if (lds_m <= kPathsGLdsCap) {
        // no LM 1 instantiation of the F_LEAF2 kernels: leaves are pair-aligned only when some leaf starts past slot 8190
        // (build_device_scene: leaf16_ok fails), and 8191 primitive references of kLm1TriBytes each are 896 KiB
        if constexpr ((F & F_LEAF2) != 0) throw std::runtime_error("internal: pair-aligned leaves in a scene that fits the LDS");
        else {
        // the camera-ray rings (triangle-free kernels) when they fit too; otherwise the lanes generate their own rays
        const size_t lds_r = lds_m + paths_g_ring_bytes(kBlockM);
        PassGeom gr = g;
        // not for a world without a BVH node (the earth: one sphere): its traces are one primitive test and its paths end
        // after a segment or two, so most lanes start a path every round and the ring only adds LDS traffic (-1.4 %)
        gr.lds_ring = (paths_g_ring(F, 1) && S.n_nodes > 0 && lds_r <= kPathsGLdsCap) ? 1u : 0u;
        return go(std::integral_constant<int, 1>{}, kBlockM, gr.lds_ring ? lds_r : lds_m, S, gr);
        }
    }
    // too large for LM 1: as many of the first (top-level) nodes as fit beside the stacks
    const size_t head = align128(lm_head);
    const size_t node_bytes = sizeof(BvhNode);
    const uint32_t fit = head < kPathsGLdsCap ? static_cast<uint32_t>((kPathsGLdsCap - head) / node_bytes) : 0u;
    if (S.n_nodes > 0 && fit >= kLdsPartialMinNodes) {
        DevScene SP = S;
        // option render.lds_nodes_max (diagnostic): a cap on the LDS-resident nodes, to measure what each one is worth
        const uint32_t cap = static_cast<uint32_t>(opt(Opt::LdsNodesMax));
        SP.n_lds_nodes = std::min<uint32_t>(std::min<uint32_t>(fit, S.n_nodes), std::max<uint32_t>(cap, kLdsPartialMinNodes));
        return go(std::integral_constant<int, 2>{}, kBlockM, head + node_bytes * SP.n_lds_nodes, SP, g);
    }
    return go(std::integral_constant<int, 0>{}, kBlock, paths_g_head_bytes(g.stack, kBlock, (F & F_CODE16) != 0), S, g);
}
KernelId launch_paths_g(uint32_t feat, bool tex_basic, bool tex_bary, bool codes16, uint32_t leaf_shift, int num_cu, hipStream_t st,
                        const DevScene& S, const PassGeom& g, const CameraRec& cam, const Work& w, uint32_t* next_slot) {
    constexpr uint32_t C = F_CODE16;
    if (leaf_shift) {
        // pair-aligned leaves (build_device_scene: mesh feature sets with triangles only): the F_LEAF2 mesh kernels
        if (!codes16 || (feat & ~kFeatMesh) != 0 || !(feat & F_TRI)) throw std::runtime_error("internal: pair-aligned leaves outside the F_LEAF2 kernels");
        if (tex_basic) return launch_paths_g_ft<kMeshG | F_LEAF2, kTexBasic>(num_cu, st, S, g, cam, w, next_slot);
        if (tex_bary) return launch_paths_g_ft<kMeshG | F_LEAF2, kTexBary>(num_cu, st, S, g, cam, w, next_slot);
        return launch_paths_g_ft<kMeshG | F_LEAF2, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
    }
    if (!codes16 && (feat & F_MEDIA_G) == 0) {
        // 32-bit child codes (more than 32768 nodes or 8192 primitive references): the instantiations without F_CODE16.
        // A mesh scene (the capsule: 10 200 triangles, the reference's default scene) gets the mesh feature set, not
        // F_ALL (whose box, transform and boundary-traversal code spilled 45 VGPRs there); the triangle-free one when
        // the scene has no triangles (no triangle code in the kernel)
        if ((feat & ~kFeatMesh) == 0 && (feat & F_TRI)) {
            if (tex_basic) return launch_paths_g_ft<kFeatMesh, kTexBasic>(num_cu, st, S, g, cam, w, next_slot);
            return launch_paths_g_ft<kFeatMesh, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
        }
        if (feat & F_TRI) return launch_paths_g_ft<F_ALL, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
        if (tex_basic) return launch_paths_g_ft<F_ALL & ~F_TRI, kTexBasic>(num_cu, st, S, g, cam, w, next_slot);
        return launch_paths_g_ft<F_ALL & ~F_TRI, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
    } else if ((feat & ~kFeatSpheres) == 0) {
        if (tex_basic) return launch_paths_g_ft<kFeatSpheres | C, kTexBasic>(num_cu, st, S, g, cam, w, next_slot);
        else return launch_paths_g_ft<kFeatSpheres | C, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
    } else if ((feat & ~kFeatMesh) == 0) {
        // the F_TRI bit of an instantiation <=> the scene has triangles (leaf_tris exists)
        if (feat & F_TRI) {
            if (tex_basic) return launch_paths_g_ft<kFeatMesh | C, kTexBasic>(num_cu, st, S, g, cam, w, next_slot);
            if (tex_bary) return launch_paths_g_ft<kFeatMesh | C, kTexBary>(num_cu, st, S, g, cam, w, next_slot);
            else return launch_paths_g_ft<kFeatMesh | C, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
        } else {
            if (tex_basic) return launch_paths_g_ft<(kFeatMesh & ~F_TRI) | C, kTexBasic>(num_cu, st, S, g, cam, w, next_slot);
            else return launch_paths_g_ft<(kFeatMesh & ~F_TRI) | C, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
        }
    } else if ((feat & F_TRI) == 0) {  // e.g. the Next-Week final: no triangle code in the kernel
        // a non-sphere medium boundary (F_MEDIA_G: the Cornell smoke boxes) traverses from t = -inf: 32-bit codes
        if (feat & F_MEDIA_G) {
            if (tex_basic) return launch_paths_g_ft<F_ALL & ~F_TRI, kTexBasic>(num_cu, st, S, g, cam, w, next_slot);
            return launch_paths_g_ft<F_ALL & ~F_TRI, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
        }
        else return launch_paths_g_ft<(F_ALL & ~F_TRI & ~F_MEDIA_G) | C, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
    } else {
        return launch_paths_g_ft<F_ALL, TF_ALL>(num_cu, st, S, g, cam, w, next_slot);
    }
}
// The ray kernels (one thread per ray or pixel: k_trace_rays, k_guides, k_query_rays, k_occlude_rays) share their choice of
// instantiation and their launch (ray_launch.h).

void launch_trace_rays(const DeviceScene& ds, bool global_scene, hipStream_t st, const double* d_rays, uint32_t nn, double* d_t, double* d_n) {
    with_ray_features(ds, global_scene, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        constexpr bool L = decltype(l)::value;
        launch_ray_kernel<k_trace_rays<F, L>, L>(ds, st, nn, ds.view, d_rays, nn, stack_rows(ds.max_stack), d_t, d_n);
    });
}

void launch_guides(const DeviceScene& ds, int flags, hipStream_t st, const GuideGeom& g, const CameraRec& cam, double* guides,
                   double* rays) {
    const uint32_t npix = static_cast<uint32_t>(g.rows) * static_cast<uint32_t>(g.W);
    with_ray_features(ds, (flags & RT_GLOBAL_SCENE) != 0, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        constexpr bool L = decltype(l)::value;
        // the texture kinds the scene needs: solid + checker, those plus barycentric images on triangles, or all
        if (ds.tex_basic) return launch_ray_kernel<k_guides<F, L, kTexBasic>, L>(ds, st, npix, ds.view, g, cam, guides, rays);
        if constexpr ((F & F_TRI) != 0)
            if (ds.tex_bary) return launch_ray_kernel<k_guides<F, L, kTexBary>, L>(ds, st, npix, ds.view, g, cam, guides, rays);
        launch_ray_kernel<k_guides<F, L, TF_ALL>, L>(ds, st, npix, ds.view, g, cam, guides, rays);
    });
}

void bounce(const DeviceScene& ds, int variant, int num_cu, hipStream_t st, const PassGeom& g, const CameraRec& cam,
            const Work& w, int d, const std::function<void()>& mark) {
    const uint32_t feat = ds.features;
    if ((feat & ~kFeatSpheres) == 0)
        launch_bounce<kFeatSpheres>(ds.mat_types, ds.tex_basic, variant, num_cu, st, ds.view, g, cam, w, d, mark);
    else if ((feat & ~kFeatMesh) == 0)
        launch_bounce<kFeatMesh>(ds.mat_types, ds.tex_basic, EXT_GLOBAL, num_cu, st, ds.view, g, cam, w, d, mark);
    else
        launch_bounce<F_ALL>(ds.mat_types, ds.tex_basic, EXT_GLOBAL, num_cu, st, ds.view, g, cam, w, d, mark);
}

// The small kernels renderer.hip runs between the path launches, one thread per item unless noted.
static dim3 grid256(uint32_t n) { return dim3((n + 255) / 256); }
void launch_accum(hipStream_t st, const PassGeom& g, const Work& w, double* qsum, uint32_t m) {
    if (qsum) hipLaunchKernelGGL(k_accum_images, grid256(g.npix_pad), dim3(256), 0, st, g, w, qsum, m);
    else hipLaunchKernelGGL(k_accum, grid256(g.npix_pad), dim3(256), 0, st, g, w);
}
void launch_finalize(hipStream_t st, const double* acc, uint8_t* rgb, uint32_t n, int spp) {
    hipLaunchKernelGGL(k_finalize, grid256(n), dim3(256), 0, st, acc, rgb, n, spp);
}
void launch_adapt_corners(hipStream_t st, uint32_t* list, int W, int sqx, uint32_t nsq) {
    hipLaunchKernelGGL(k_adapt_corners, grid256(nsq), dim3(256), 0, st, list, W, sqx, nsq);
}
void launch_adapt_store(hipStream_t st, const uint32_t* list, uint32_t n, const double* acc, int spp, int32_t* work) {
    hipLaunchKernelGGL(k_adapt_store, grid256(n), dim3(256), 0, st, list, n, acc, spp, work);
}
// one wave per list entry, `cap` entries at the most (the count is on the device)
void launch_adapt_accum(hipStream_t st, const uint32_t* list, uint32_t cap, const ResRec* res, uint32_t k, int spp, int32_t* work) {
    hipLaunchKernelGGL(k_adapt_accum, dim3((cap + kAdaptAccumWaves - 1) / kAdaptAccumWaves), dim3(64 * kAdaptAccumWaves), 0, st, list, res, k, spp, work);
}
void launch_adapt_level(hipStream_t st, int level, int32_t* work, int W, int sqx, uint32_t nsq, uint8_t* f0, uint8_t* f1, uint8_t* f2, uint32_t* list,
                        uint32_t* count) {
    const uint32_t per = level == 0 ? 1u : (level == 1 ? 4u : 16u);
    hipLaunchKernelGGL(k_adapt_level, grid256(nsq * per), dim3(256), 0, st, level, work, W, sqx, nsq, f0, f1, f2, list, count);
}
void launch_adapt_fill(hipStream_t st, int32_t* work, uint8_t* rgb, int W, int rows, int sqx, const uint8_t* f0, const uint8_t* f1, const uint8_t* f2) {
    hipLaunchKernelGGL(k_adapt_fill, grid256(static_cast<uint32_t>(rows) * static_cast<uint32_t>(W)), dim3(256), 0, st, work, rgb, W, rows, sqx, f0, f1, f2);
}

// The rt_query_rays launchers close the file: they instantiate k_query_rays and k_occlude_rays, and the compiler emits
// device functions in instantiation order, so every earlier kernel and the out-of-line helpers it calls keep their
// relative places -- and with them their code bytes (DESIGN.md 4.7 compares them with the build before these kernels).
// rt_query_rays, closest mode
void launch_query_rays(const DeviceScene& ds, bool global_scene, hipStream_t st, const double* d_rays, const double* d_tmax, uint32_t nn,
                       bool no_media, double* d_hits) {
    with_ray_features(ds, global_scene, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        constexpr bool L = decltype(l)::value;
        launch_ray_kernel<k_query_rays<F, L>, L>(ds, st, nn, ds.view, d_rays, d_tmax, nn, no_media ? 1u : 0u, d_hits);
    });
}
// the any-hit kernels: the same choice with the media bits removed; the child order from option query.any_sorted
void launch_occlude_rays(const DeviceScene& ds, bool global_scene, hipStream_t st, const double* d_rays, const double* d_tmax, uint32_t nn,
                         uint8_t* d_occ) {
    with_ray_features<~(F_MEDIA | F_MEDIA_G)>(ds, global_scene, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        constexpr bool L = decltype(l)::value;
        if (opt(Opt::QueryAnySorted) != 0) launch_ray_kernel<k_occlude_rays<F, L, 1>, L>(ds, st, nn, ds.view, d_rays, d_tmax, nn, d_occ);
        else launch_ray_kernel<k_occlude_rays<F, L, 2>, L>(ds, st, nn, ds.view, d_rays, d_tmax, nn, d_occ);
    });
}

}  // namespace art

// path_work.h — what the path kernels share: the path, hit and result records, the pass geometry and the work
// queues, camera rays, the scatter / LDS shading code and the LDS layout constants (device side of kernels.hip,
// k_paths.hip and k_paths_g.h; the host files read the record sizes and fill PassGeom / Work).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "pass_plan.h"

namespace art {

// ------------------------------------------------------------------------------------------------ path records
// One path = one AoS record so that a lane touching a scattered slot reads whole cache lines:
//   128 B = line 0 {o.xyz, d.xyz, time, rng} (all extend reads) + line 1 {T.rgb, L.rgb}
struct PathRec {
    double2 a, b, c, e;  // line 0: (ox,oy) (oz,dx) (dy,dz) (tm,rng)
    double2 f, g, h, i;  // line 1: (Tr,Tg) (Tb,Lr) (Lg,Lb) (-,-)
};
static_assert(sizeof(PathRec) == 128, "PathRec is two 64-B lines");
struct PathState {
    Ray ray;
    V3 T, L;
    uint64_t rng;
};
__device__ __forceinline__ void load_path(const PathRec* P, uint32_t q, PathState& s, bool full) {
    const PathRec& p = P[q];
    const double2 a = p.a, b = p.b, c = p.c, e = p.e;
    s.ray.o = mk(a.x, a.y, b.x);
    s.ray.d = mk(b.y, c.x, c.y);
    s.ray.tm = e.x;
    s.rng = static_cast<uint64_t>(__double_as_longlong(e.y));
    if (full) {
        const double2 f = p.f, g = p.g, h = p.h;
        s.T = mk(f.x, f.y, g.x);
        s.L = mk(g.y, h.x, h.y);
    }
}
__device__ __forceinline__ void store_path(PathRec* P, uint32_t q, const PathState& s) {
    PathRec& p = P[q];
    p.a = make_double2(s.ray.o.x, s.ray.o.y);
    p.b = make_double2(s.ray.o.z, s.ray.d.x);
    p.c = make_double2(s.ray.d.y, s.ray.d.z);
    p.e = make_double2(s.ray.tm, __longlong_as_double(static_cast<long long>(s.rng)));
    p.f = make_double2(s.T.x, s.T.y);
    p.g = make_double2(s.T.z, s.L.x);
    p.h = make_double2(s.L.y, s.L.z);
}
__device__ __forceinline__ void store_rng(PathRec* P, uint32_t q, uint64_t rng) {
    P[q].e.y = __longlong_as_double(static_cast<long long>(rng));
}

struct HitRecD {  // extend -> shade hand-off, 16 B
    double t;
    uint32_t prim, obj;
};
static_assert(sizeof(HitRecD) == 16, "HitRecD is 16 B");

struct ResRec { double x, y, z; };  // final per-slot radiance; 24 B, unpadded: k_accum streams these at HBM rate
static_assert(sizeof(ResRec) == 24, "ResRec is 24 B");
// NT: non-temporal stores (read once, by k_accum after the pass), so the records do not evict k_paths' L2-resident
// camera-ray rings.  Measured (r5c, profiles/r5c_write_traffic.txt, HBM bytes per segment vs the 24-B records' own):
// each 8-B non-temporal store reaches HBM as its own partial write, 2.0x the record bytes (Next-Week final: 12.6 B
// against 6.3); temporal stores merge in L2 first, 1.18x (7.4 B), at equal speed -- so k_paths_g, which has no rings,
// stores temporally.  k_paths keeps NT: its writes are ring lines evicted between laps (27.8 B per segment with NT
// 24-B records, 27.2 with NT 32-B ones), and temporal records evict more of them (32.9 B written + 6.8 B re-read,
// -0.25 %).  32-B records cost k_accum a third more reads and lose 0.8-1.2 %.  r6i: the k_paths_g kernels whose BVH is
// not all in LDS (LM 0 / 2) store non-temporally after all: there the temporal records evict the L2-resident nodes
// and leaf triangles (capsule +1.7 %, cow +0.8 %, profiles/r6i_ab_res_nt.txt).
template <bool NT = true>
__device__ __forceinline__ void store_res(ResRec* res, uint32_t q, V3 L) {
    if constexpr (NT) {
        __builtin_nontemporal_store(L.x, &res[q].x);
        __builtin_nontemporal_store(L.y, &res[q].y);
        __builtin_nontemporal_store(L.z, &res[q].z);
    } else {
        res[q].x = L.x;
        res[q].y = L.y;
        res[q].z = L.z;
    }
}
__device__ __forceinline__ void load_res(const ResRec* res, uint32_t q, double& r, double& g, double& b) {
    r = res[q].x; g = res[q].y; b = res[q].z;
}

// ------------------------------------------------------------------------------------------------ work distribution
// Queues are split into kShards shards, each with its own counter on its own 128-B line.  Persistent waves take
// 64-item batches in a static grid-stride order (no claim atomic) and a wave appends only to shard
// (global wave id % kShards): one returning atomic per wave and queue, spread over kShards words instead of one
// (a single word saturates at ~88 atomics/us, MI355X_MICROARCH.md "dequeue").  Static assignment also bounds every
// shard: shard s only receives outputs of the batches b with b % kShards == s, so kShardCap(P) slots suffice.
constexpr int kShards = 32;
constexpr int kCounterStride = 32;                   // words between counters (128 B)
constexpr int kQueueKinds = 1 + kNumMatTypes;        // 0: active (extend input), 1..5: material queues
constexpr int kMatSegs = kNumMatTypes * kShards;     // shade input segments
// + 2 batches per material kernel: the kNumMatTypes shade launches of one depth all append to the same next-queue shards
__host__ __device__ inline uint32_t shard_cap(uint32_t P) { return 64u * ((((P + 63u) / 64u) + kShards - 1) / kShards + 2 * kNumMatTypes); }

// n / d for a divisor fixed per launch, as a multiply-high, an add and a shift (Granlund & Montgomery 1994,
// round-up variant): l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1, n / d = (mulhi(m, n) + n) >> l, exact for
// every n < 2^31 (the add cannot carry out) -- instead of the ~20-instruction integer division sequence.
struct FastDiv {
    uint32_t d, m, l;
    static FastDiv make(uint32_t d) {
        uint32_t l = 0;
        while (l < 32 && (1ull << l) < d) ++l;
        return FastDiv{d, static_cast<uint32_t>(((1ull << 32) * ((1ull << l) - d)) / d + 1), l};
    }
    __device__ __forceinline__ uint32_t div(uint32_t n) const { return (__umulhi(m, n) + n) >> l; }
};

struct PassGeom {
    int32_t W, H;               // full image
    int32_t rows;               // local rows
    int32_t band_rows, band_count, band_index;
    uint32_t tiles_x, npix_pad; // 8x8 tiles over (W x rows)
    uint32_t k;                 // samples in this pass
    uint32_t sample_base;       // first sample index of the pass
    uint32_t P;                 // k * npix_pad path slots
    uint32_t cap;               // shard capacity
    uint32_t live;              // k * rows * W: slots that are real pixels (depth-0 segments)
    uint32_t stack;             // LDS traversal stack rows per lane (stack_rows)
    int32_t max_depth;
    uint64_t seed;
    uint64_t seed_mix;          // splitmix64(seed): the per-frame half of pcg_seed, hoisted to the host
    FastDiv fd_npix, fd_tiles_x, fd_band_rows, fd_w;  // / npix_pad, / tiles_x, / band_rows, / W
    double inv_w1, inv_h1;      // RN(1 / (W - 1)), RN(1 / (H - 1)) for gen_ray's div_rcp (rt_render rejects W or H < 2)
    const uint32_t* list;       // pixel-list mode (engine_mode::adaptive levels): slot pixel = list[qi] (local ly*W+lx)
    uint32_t nlist;             //   for qi < nlist; nullptr = every local pixel in 8x8 tile order
    uint32_t chunk;             // persistent kernels: slots per claim (path_chunk: a power of two >= 64)
    uint32_t lds_ring;          // k_paths_g LM 1: the camera-ray rings are allocated in LDS (kRing, when they fit)
    // 1: pixel-list mode with the samples of a list entry on consecutive slots (slot = entry * k + sample: a wave's 64
    // lanes trace one pixel's samples, coherent rays, instead of 64 entries scattered over the image) and the entry
    // count on the device at list[-1] (the adaptive levels' lists, appended by k_adapt_level: no host round trip);
    // npix_pad = k then, and the persistent kernels take P = list[-1] * k and nlist = list[-1] at their start
    uint32_t list_mode;
};
struct Work {
    PathRec* paths;
    HitRecD* hits;
    ResRec* res;
    uint32_t* active[2];        // extend input of depth d: active[d & 1], kShards x cap
    uint32_t* mq;               // material queues: (m * kShards + s) * cap
    uint32_t* counters;         // [(depth * kQueueKinds + kind) * kShards + shard] * kCounterStride
    unsigned long long* segments;
    double* acc;                // local pixels * 3
    void* pool;                 // k_paths path pools: the paths a batch displaces, kPoolCap PoolRays per wave (path_pool.h)
    const void* tiles;          // k_paths: one TileRec per 8x8 tile of the pass geometry (tile_lists.h), or null: no lists
};
__host__ __device__ __forceinline__ uint32_t* counter(const Work& w, int d, int kind, int s) {
    return w.counters + (static_cast<size_t>((d * kQueueKinds + kind) * kShards + s)) * kCounterStride;
}

__device__ __forceinline__ int global_row(const PassGeom& g, int ly) {  // row-interleaved band partition
    const uint32_t b = g.fd_band_rows.div(static_cast<uint32_t>(ly));
    return static_cast<int>(b) * (g.band_rows * g.band_count) + g.band_index * g.band_rows + (ly - static_cast<int>(b) * g.band_rows);
}
// slot -> (qi: tile-order pixel or list entry, j: sample of the pass): sample-major slots (j * npix_pad + qi), or
// entry-major ones in list_mode 1 (qi * k + j, npix_pad == k)
__device__ __forceinline__ void slot_split(const PassGeom& g, uint32_t slot, uint32_t& qi, uint32_t& j) {
    const uint32_t a = g.fd_npix.div(slot), b = slot - a * g.npix_pad;
    qi = g.list_mode ? a : b;
    j = g.list_mode ? b : a;
}
__device__ __forceinline__ bool slot_pixel(const PassGeom& g, uint32_t qi, int& lx, int& ly) {
    if (g.list) {
        if (qi >= g.nlist) return false;
        const uint32_t p = g.list[qi];
        ly = static_cast<int>(g.fd_w.div(p));
        lx = static_cast<int>(p - static_cast<uint32_t>(ly) * static_cast<uint32_t>(g.W));
        return true;
    }
    const uint32_t tile = qi >> 6, within = qi & 63u;
    const uint32_t ty = g.fd_tiles_x.div(tile);
    lx = static_cast<int>((tile - ty * g.tiles_x) * 8 + (within & 7u));
    ly = static_cast<int>(ty * 8 + (within >> 3));
    return lx < g.W && ly < g.rows;
}

// Wave-aggregated append to one shard: one atomic per wave, lanes write in lane order.
__device__ __forceinline__ void wave_append(bool pred, uint32_t val, uint32_t* shard_buf, uint32_t* ctr) {
    const uint64_t mask = __ballot(pred);
    if (mask == 0) return;
    const int leader = __ffsll(static_cast<long long>(mask)) - 1;
    uint32_t base = 0;
    if (static_cast<int>(__lane_id()) == leader) base = atomicAdd(ctr, static_cast<uint32_t>(__popcll(mask)));
    base = __shfl(base, leader);
    if (pred) {
        const uint32_t off = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
        shard_buf[base + off] = val;
    }
}

// Appends every lane with mtype in [0, kNumMatTypes) to its material queue (this wave's shard) with ONE vector atomic:
// lane m reserves the slots of material m, so the wave pays one atomic round trip instead of one per material.
__device__ __forceinline__ void append_by_material(int mtype, uint32_t q, const Work& w, const PassGeom& g, int d, int shard) {
    uint64_t masks[kNumMatTypes];
    uint64_t any = 0;
#pragma unroll
    for (int m = 0; m < kNumMatTypes; ++m) {
        masks[m] = __ballot(mtype == m);
        any |= masks[m];
    }
    if (any == 0) return;
    const int lane = static_cast<int>(__lane_id());
    uint64_t my_mask = 0;
#pragma unroll
    for (int m = 0; m < kNumMatTypes; ++m)
        if (lane == m) my_mask = masks[m];
    uint32_t base = 0;
    if (lane < kNumMatTypes && my_mask != 0) base = atomicAdd(counter(w, d, 1 + lane, shard), static_cast<uint32_t>(__popcll(my_mask)));
    base = __shfl(base, mtype >= 0 ? mtype : 0);  // all lanes: lanes 0..4 own the reservations
    if (mtype >= 0) {
        uint64_t mine = masks[0];
#pragma unroll
        for (int m = 1; m < kNumMatTypes; ++m)
            if (mtype == m) mine = masks[m];
        const uint32_t off = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mine >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mine), 0u));
        w.mq[static_cast<size_t>(mtype * kShards + shard) * g.cap + base + off] = q;
    }
}

// Exclusive prefix of the n <= 64 shard counts v (held by threads 0..n-1) into pre[0..n] (pre[n] = total), by one wave
// scan; independent of the block size.
__device__ __forceinline__ void block_prefix(uint32_t* pre, int n, uint32_t v) {
    const int t = threadIdx.x;
    if (t < 64) {
        uint32_t x = t < n ? v : 0u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (t >= off) x += y;
        }
        if (t < n) pre[t + 1] = x;
        if (t == 0) pre[0] = 0u;
    }
    __syncthreads();
}
// Segment of item i: largest s with pre[s] <= i (pre strictly describes n segments).
__device__ __forceinline__ int find_segment(const uint32_t* pre, int n, uint32_t i) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ camera rays, shading
// engine.h:58-68 + camera.h:38-47 for sample j of the pass at local pixel (lx, ly) (slot_split).
// Runs inside the depth-0 extend: the camera ray never round-trips through HBM.
__device__ __forceinline__ void cam_ray(const PassGeom& g, const CameraRec& cam, uint32_t j, int lx, int ly, Ray& ray, uint64_t& rng_out) {
    const int gy = global_row(g, ly);
    const uint32_t pixel = static_cast<uint32_t>(gy) * static_cast<uint32_t>(g.W) + static_cast<uint32_t>(lx);
    uint64_t rng = splitmix64(((static_cast<uint64_t>(pixel) << 32) | (g.sample_base + j)) ^ g.seed_mix);  // == pcg_seed(g.seed, ...)
    const double ru = uniform(rng);
    const double rv = uniform(rng);
    const double s = div_rcp(static_cast<double>(lx) + ru, static_cast<double>(g.W - 1), g.inv_w1);  // == (lx + ru) / (W - 1), same bits
    const double t = div_rcp(static_cast<double>(g.H - 1 - gy) + rv, static_cast<double>(g.H - 1), g.inv_h1);
    V3 p;
    for (;;) {  // random_in_unit_disk (vec3.h:137-143): x, then y
        p.x = uniform_pm1(rng);
        p.y = uniform_pm1(rng);
        p.z = 0.0;
        if (len2(p) >= 1.0) continue;
        break;
    }
    const V3 rd = cam.lens_radius * p;
    const V3 offset = rd.x * ld3(cam.u) + rd.y * ld3(cam.v);
    ray.o = ld3(cam.origin) + offset;
    ray.d = ld3(cam.llc) + s * ld3(cam.horizontal) + t * ld3(cam.vertical) - ld3(cam.origin) - offset;
    ray.tm = uniform(rng, cam.time0, cam.time1);
    rng_out = rng;
}
__device__ __forceinline__ void gen_ray(const PassGeom& g, const CameraRec& cam, uint32_t j, int lx, int ly, PathState& st) {
    cam_ray(g, cam, j, lx, ly, st.ray, st.rng);
    st.T = mk(1.0, 1.0, 1.0);
    st.L = mk(0.0, 0.0, 0.0);
}

// material.h scatter() for one hit of material type M (compile time: one shade kernel per material type, so a wave
// never carries another material's code or registers); returns false when the path ends here.
// Shared steps already taken for the whole wave (k_paths_g), or null:
//   pre    the lane's random_in_unit_sphere() draw (coop_unit_sphere);
//   unitv  unit_vector of that draw (lambertian) or of the ray direction (metal, dielectric);
//   texc   the material's texture value at the hit (lambertian, isotropic).
template <uint32_t M, uint32_t TF>
__device__ __forceinline__ bool scatter(const DevScene& S, const MatRec& m, const Surf& s, PathState& st, V3& att, V3& dir,
                                        const V3* pre = nullptr, const V3* unitv = nullptr, const V3* texc = nullptr) {
    if (M == MAT_LAMBERTIAN) {  // material.h:20-43
        const V3 rv = unitv ? *unitv : unit(pre ? *pre : in_unit_sphere(st.rng));
        dir = s.n + rv;
        if (near_zero(dir)) dir = s.n;
        att = texc ? *texc : mat_tex_value<TF>(S, m, s.u, s.v, s.p);
        return true;
    } else if (M == MAT_METAL) {  // material.h:45-61
        const V3 reflected = reflect(unitv ? *unitv : unit(st.ray.d), s.n);
        dir = reflected + m.fuzz * (pre ? *pre : in_unit_sphere(st.rng));
        att = ld3(m.albedo);
        return dot(dir, s.n) > 0.0;
    } else if (M == MAT_DIELECTRIC) {  // material.h:63-99
        att = mk(1.0, 1.0, 1.0);
        const double ratio = s.ff ? (1.0 / m.ir) : m.ir;
        const V3 ud = unitv ? *unitv : unit(st.ray.d);
        const double cos_theta = fmin(dot(-ud, s.n), 1.0);
        const double sin_theta = sqrt_rn(1.0 - cos_theta * cos_theta);
        const bool cannot = ratio * sin_theta > 1.0;
        bool refl = cannot;
        if (!cannot) {
            double r0 = (1.0 - ratio) / (1.0 + ratio);
            r0 = r0 * r0;
            const double refl_p = r0 + (1.0 - r0) * pow5(1.0 - cos_theta);
            refl = refl_p > uniform(st.rng);
        }
        dir = refl ? reflect(ud, s.n) : refract(ud, s.n, ratio);
        return true;
    } else if (M == MAT_ISOTROPIC) {  // material.h:120-135
        dir = pre ? *pre : in_unit_sphere(st.rng);
        att = texc ? *texc : mat_tex_value<TF>(S, m, s.u, s.v, s.p);
        return true;
    }
    return false;  // diffuse_light (material.h:106-110)
}

// Emission + scatter of one hit of the fused extend variant, read entirely from the LDS scene image: the surface
// (sphere.h:57-63 via the slot's centre/radius/motion planes, which are the f64 values the hit test used) and the
// material (the image's shading table, layout.h) -- no dependent global loads after a hit.  The arithmetic and the
// draws are those of prim_surface + scatter<M, kTexBasic> (tex_value of a solid or solid/solid checker texture).
// Returns true when the path continues (st then holds the scattered ray and the updated throughput).
__device__ __forceinline__ V3 lds_mat_color(const uint8_t* lds, uint32_t e) {
    const double2* m = reinterpret_cast<const double2*>(lds + kLdsOffMat) + 2 * e;
    const double2 a = m[0], b = m[1];
    return mk(a.x, a.y, b.x);
}
// pre_ps: the lane's random_in_unit_sphere() draw, already taken by the wave (coop_unit_sphere) when non-null.
__device__ __forceinline__ bool shade_hit_lds(const uint8_t* lds, uint32_t slot, uint32_t mtype, double t, bool last, PathState& st,
                                              const V3* pre_ps = nullptr) {
    const double2* sp = reinterpret_cast<const double2*>(lds + kLdsOffSph) + slot;
    const double2 a = sp[0], b = sp[kLdsSlotCap];
    const uint32_t mi = reinterpret_cast<const uint16_t*>(lds + kLdsOffMatIdx)[slot];
    V3 center{a.x, a.y, b.x};
    center.y = center.y + st.ray.tm * reinterpret_cast<const double*>(lds + kLdsOffMov)[slot];  // dy = -0: static
    Surf s;
    s.p = st.ray.at(t);
    set_face_normal(s, st.ray, reinterpret_cast<const double*>(lds + kLdsOffInvR)[slot] * (s.p - center));  // (p - c) / r
    const uint32_t e = mi & ~kLdsMatChecker;
    const bool checker = (mi & kLdsMatChecker) != 0;
    if (mtype == MAT_LIGHT) {  // material.h:114-116; diffuse_light never scatters
        st.L = st.L + st.T * lds_mat_color(lds, (checker && checker_odd(s.p)) ? e + 1 : e);
        return false;
    }
    if (last) return false;
    // The three materials of a wave share their costly steps (each lane still draws exactly its own material's
    // sequence): lambertian and metal both start with random_in_unit_sphere() (material.h:33, :55 -- metal's
    // unit_vector(r_in.direction()) draws nothing), and all three need one unit_vector (of that sample for
    // lambertian, of the ray direction for metal and dielectric), so the wave runs one rejection loop and one
    // sqrt + divide sequence instead of one per material present.
    const bool lamb = mtype == MAT_LAMBERTIAN;
    V3 ps = mk(0.0, 0.0, 0.0);
    if (pre_ps) ps = *pre_ps;
    else if (mtype != MAT_DIELECTRIC) ps = in_unit_sphere(st.rng);
    const V3 u = unit(lamb ? ps : st.ray.d);
    V3 att, dir;
    if (lamb) {  // material.h:20-43
        dir = s.n + u;
        if (near_zero(dir)) dir = s.n;
        att = lds_mat_color(lds, (checker && checker_odd(s.p)) ? e + 1 : e);
    } else if (mtype == MAT_METAL) {  // material.h:45-61
        const double2* m = reinterpret_cast<const double2*>(lds + kLdsOffMat) + 2 * e;
        const double2 ma = m[0], mb = m[1];
        dir = reflect(u, s.n) + mb.y * ps;
        att = mk(ma.x, ma.y, mb.x);
        if (!(dot(dir, s.n) > 0.0)) return false;
    } else {  // dielectric, material.h:63-99
        // the table entry holds (1 / ir, r0 of the front face, r0 of the back face, ir), each computed on the host by
        // the same IEEE operations material.h:74 and :93-94 apply (lds_scene_image): no division per hit
        const double2* me = reinterpret_cast<const double2*>(lds + kLdsOffMat) + 2 * e;
        const double2 m0 = me[0], m1 = me[1];
        att = mk(1.0, 1.0, 1.0);
        const double ratio = s.ff ? m0.x : m1.y;  // front_face ? (1.0 / ir) : ir
        const double cos_theta = fmin(dot(-u, s.n), 1.0);
        const double sin_theta = sqrt_rn(1.0 - cos_theta * cos_theta);
        const bool cannot = ratio * sin_theta > 1.0;
        bool refl = cannot;
        if (!cannot) {
            const double r0 = s.ff ? m0.y : m1.x;  // ((1 - ratio) / (1 + ratio))^2
            const double refl_p = r0 + (1.0 - r0) * pow5(1.0 - cos_theta);
            refl = refl_p > uniform(st.rng);
        }
        dir = refl ? reflect(u, s.n) : refract(u, s.n, ratio);
    }
    st.T = st.T * att;
    st.ray.o = s.p;
    st.ray.d = dir;
    return true;
}

#ifndef ART_LDS_BLOCK
#define ART_LDS_BLOCK 1024
#endif
// Blocks of the LDS-scene variant: one block per CU holds the scene image once for 16 waves (4 per SIMD).
constexpr int kBlockL = ART_LDS_BLOCK;
// LDS bytes of one k_extend block: scene image (L) + per-lane stack + the shard prefix array.
__host__ __device__ constexpr size_t extend_pre_offset(bool L, uint32_t stack) {
    return ((L ? kLdsImageBytes + sizeof(int16_t) * stack * kBlockL : sizeof(int32_t) * stack * kBlock) + 15u) & ~size_t(15);
}

// Copies the LDS scene image (layout.h) into LDS in one round: every lane issues all of its 16-B loads before its
// first store, so the block pays one global-load latency instead of one per plane.
template <int B>
__device__ __forceinline__ void load_lds_image(const uint8_t* image, uint8_t* lds) {
    constexpr uint32_t n16 = kLdsImageBytes / 16;
    constexpr int per = static_cast<int>((n16 + B - 1) / B);
    const uint4* src = reinterpret_cast<const uint4*>(image);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    uint4 v[per];
#pragma unroll
    for (int j = 0; j < per; ++j) {
        const uint32_t i = threadIdx.x + static_cast<uint32_t>(j) * B;
        if (i < n16) v[j] = src[i];
    }
#pragma unroll
    for (int j = 0; j < per; ++j) {
        const uint32_t i = threadIdx.x + static_cast<uint32_t>(j) * B;
        if (i < n16) dst[i] = v[j];
    }
}

// ART_STATS builds: adds the cycles since the last tick to `acc` (a kernel that ticks declares tm_prev and its sums)
#ifdef ART_STATS
#define ART_TICK(acc)                                               \
    do {                                                            \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        acc += now_ - tm_prev;                                      \
        tm_prev = now_;                                             \
    } while (0)
#else
#define ART_TICK(acc)
#endif

// k_paths' path pools (k_paths.hip) and k_paths_g's camera-ray rings, sized per CU by the host.  XCD-contiguous: measured (r3m, 128-entry camera-ray rings in k_paths)
// HBM reads 11.3 -> 3.5 B per segment against the block-major layout, Msamples/s unchanged
constexpr uint32_t kXcds = 8;  // MI355X
constexpr uint32_t kPoolWavesPerCu = 32;  // pools / rings allocated per CU: the most waves a CU holds
__host__ __device__ constexpr size_t paths_stack_bytes(uint32_t stack) { return (sizeof(int16_t) * stack * kBlockL + 15u) & ~size_t(15); }
constexpr size_t kJumpBytes = sizeof(JumpEntry) * kJumpEntries;
// The world list and object records, copied into LDS by every k_paths block: each trace walks them, and from global
// memory they were three dependent vector loads (world slot -> object -> hoisted leaf) at the start of every trace
// (vector, not scalar, loads: the kernel stores, so the compiler cannot prove them unclobbered).  The LDS scene
// path requires a world of at most kPathsWorldCap objects (lds_scene_image; after world merging the benchmark scene
// has one).
constexpr uint32_t kPathsWorldCap = 16;
constexpr size_t kPathsWorldBytes = sizeof(int32_t) * kPathsWorldCap + sizeof(ObjRec) * kPathsWorldCap;
__host__ __device__ constexpr size_t paths_lds_head(uint32_t stack) {
    return ((kLdsImageBytes + paths_stack_bytes(stack) + kJumpBytes + sizeof(CameraRec) + sizeof(PassGeom)) + 15u) & ~size_t(15);
}
__host__ __device__ constexpr size_t paths_lds_bytes(uint32_t stack) { return paths_lds_head(stack) + kPathsWorldBytes; }

struct GuideGeom {  // k_guides' frame (kernels.hip)
    int32_t W, H, rows;
    int32_t band_rows, band_count, band_index;
};
constexpr int kBig = 12, kMid = kBig / 2, kSmall = kMid / 2;  // adaptive mode's squares (kernels.hip k_adapt_*)

#ifdef ART_TRACE
// Path tracing diagnostics (libart_trace.so builds only): ART_TRACE="pixel:sample" prints every segment of that one
// path from k_paths_g as bit patterns, in the format of the oracle's ORC_TRACE, so the two can be diffed.
__device__ long long g_trace_pixel = -1, g_trace_sample = -1;
#define ART_DBITS(x) static_cast<unsigned long long>(__double_as_longlong(x))
#endif

}  // namespace art

// k_paths_g.h — the k_paths_g kernel template and its LDS layout; instantiated by kernels.hip's launchers, except the
// two instantiations declared extern at the end (k_paths_g_mesh.hip).
#pragma once
#include "path_work.h"

namespace art {

// Persistent paths over the HBM scene (EXT_MEGA_G): the k_paths loop for every scene that does not fit the LDS
// image (triangles, rects, boxes, transforms, media, noise/image textures).  A lane owns one path from its camera
// ray to its end: trace_world over the global BVHs (the k_extend traversal, LDS stack) and, in place, world_surface +
// the material's scatter (the k_shade arithmetic, one switch over the material type instead of one launch per type),
// so the RNG draws and every f64 operation are those of the wavefront kernels and images are bit-identical to them.
// F / TF: the scene's primitive and texture features (smallest instantiation that covers them).
constexpr uint32_t kLdsPartialMinNodes = 64;
#ifndef ART_PATHS_G_WAVES
#define ART_PATHS_G_WAVES 3  // 3 waves per SIMD (<= 168 VGPRs): measured best over 2 and 4 (cow +22 %, final +18 %, dino +21 % over 2)
#endif
// LM (LDS BVH): a scene whose BVH nodes and primitive references -- and triangles, for a kernel with triangles --
// fit beside the stacks (small meshes: dino; the Next-Week final's 559 nodes) runs one 768-lane block per CU with
// those arrays copied into LDS: node and triangle fetches at LDS latency instead of L2's.  The other arrays stay in
// HBM.  The copies are plain LDS arrays reached through the DevScene pointers: the compiler infers their address
// space (ds_read, no flat loads).
constexpr int kBlockM = 256 * ART_PATHS_G_WAVES;  // one LM block per CU at the kernel's occupancy
constexpr size_t kPathsGLdsCap = 160 * 1024;
__host__ __device__ constexpr size_t align16(size_t x) { return (x + 15u) & ~size_t(15); }
__host__ __device__ constexpr size_t align128(size_t x) { return (x + 127u) & ~size_t(127); }
// s16: 16-bit stack entries (F_CODE16 instantiations, device.h StackF)
__host__ __device__ constexpr size_t paths_g_stack_bytes(uint32_t stack, int block, bool s16) { return (s16 ? 2u : 4u) * stack * block; }
__host__ __device__ constexpr size_t paths_g_head_bytes(uint32_t stack, int block, bool s16) {  // stack, camera, pass geometry, jumps, u,v
    return align16(paths_g_stack_bytes(stack, block, s16) + sizeof(CameraRec) + sizeof(PassGeom)) + kJumpBytes + kUvConstBytes;
}
// LM kernels also hold the world list and the object records (a few KiB): every segment walks them, and a prim
// object's test otherwise waits on three dependent L1 loads (world slot -> object -> primitive).  The textured ones
// (noise / image) also hold the material records when there are at most kMatsLdsCap of them (the Next-Week final: 12):
// every hit's shading reads its material (type, flags, the inlined solid colour) right after the surface, and from
// HBM that is one more dependent L2 round trip per bounce.
constexpr uint32_t kMatsLdsCap = 128;
template <uint32_t TF>
__host__ __device__ constexpr uint32_t lds_mats(uint32_t n_mats) {
    return ((TF & (TF_NOISE | TF_IMAGE)) != 0 && n_mats <= kMatsLdsCap) ? n_mats : 0u;
}
__host__ __device__ constexpr size_t paths_g_world_bytes(int32_t nworld, uint32_t n_objs, uint32_t n_lds_mats) {
    return align16(sizeof(int32_t) * static_cast<uint32_t>(nworld)) + (sizeof(ObjRec) + sizeof(PrimRec80)) * n_objs +
           sizeof(MatRec) * n_lds_mats;
}
// LM 1's LDS copy of the leaf triangle records: TriRec112 (plane precomputed, traverse's PL 2 path)
constexpr size_t kLm1TriBytes = sizeof(TriRec112);
__host__ __device__ constexpr size_t paths_g_mesh_bytes(uint32_t n_nodes, uint32_t n_primrefs, uint32_t n_tris) {  // n_tris: 0 unless F_TRI
    return sizeof(BvhNode) * n_nodes + align16(sizeof(uint32_t) * n_primrefs) + kLm1TriBytes * n_tris;
}
// Camera-ray ring in LDS (k_paths_g LM 1, ART_LDS_RING_G): the camera rays are generated 64 at a time by the whole wave,
// converged, into a per-wave ring of 64 entries in LDS, and the lanes that start a path read the next entries -- instead
// of every round's camera-ray code running diverged for the few lanes that start a path (about a third).  k_paths does
// the same through an L2-resident ring; in k_paths_g that ring's L2 round trip per take cost more than it saved (r3y:
// final -0.8 %), the LDS read does not.  An entry is 64 B: o, d, tm, rng; tm = NaN marks a padding slot of a partial
// tile (the taker idles a round), +inf a slot past the pass (the taker is drained).  Entry k holds slot b0 + k.
#ifndef ART_LDS_RING_G
#define ART_LDS_RING_G 1
#endif
constexpr uint32_t kRingG = 64;  // entries per wave
// Which kernels carry the ring: triangle-free LM 1 kernels (r5d, profiles/r5d_ab_lds_ring.txt: Cornell smoke +3.2 %,
// two perlin spheres +3.6 %, simple light +0.2 %; the mesh kernel, whose leaf triangles share the LDS, dino -1.1 %),
// except the Next-Week final's <189, 15, 1>: there the ring's registers push three loop-carried doubles into scratch
// (6 spilled VGPRs) for +0.5 %, so it keeps its spill-free ring-free form.
__host__ __device__ constexpr bool paths_g_ring(uint32_t F, int LM) {
    return ART_LDS_RING_G && LM == 1 && (F & F_TRI) == 0 && F != ((F_ALL & ~F_TRI & ~F_MEDIA_G) | F_CODE16);
}
__host__ __device__ constexpr size_t paths_g_ring_bytes(int block) { return static_cast<size_t>(block / 64) * kRingG * 64u; }
// A wave's ring is 64 entries of 8 fields (o.xyz, d.xyz, tm, rng) stored field-major (SoA: field f of entry k at
// f * 512 + k * 8 bytes), so a wave's reads and writes of one field are contiguous 8-B words (no bank conflicts; the
// AoS 64-B entries put 4 lanes on the same banks).
struct RingG {
    double* f;  // this wave's 8 x 64 doubles
    __device__ __forceinline__ double& at(uint32_t field, uint32_t k) const { return f[field * kRingG + k]; }
};
// 1 = a path starts (st, q), 0 = a padding slot (idle this round), 2 = the pass is drained
__device__ __forceinline__ int ring_take_g(const RingG& ring, uint32_t k, uint32_t b0, PathState& st, uint32_t& q) {
    const double tm = ring.at(6, k);
    if (tm != tm) return 0;
    if (tm == __builtin_inf()) return 2;
    st.ray.o = mk(ring.at(0, k), ring.at(1, k), ring.at(2, k));
    st.ray.d = mk(ring.at(3, k), ring.at(4, k), ring.at(5, k));
    st.ray.tm = tm;
    st.rng = static_cast<uint64_t>(__double_as_longlong(ring.at(7, k)));
    st.T = mk(1.0, 1.0, 1.0);
    st.L = mk(0.0, 0.0, 0.0);
    q = b0 + k;
    return 1;
}
__device__ __forceinline__ void ring_fill_g(const RingG& ring, uint32_t lane, uint32_t slot, const PassGeom& sg, const CameraRec& sc) {
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, __builtin_inf(), 0.0};
    if (slot < sg.P) {
        v[6] = __builtin_nan("");
        int lx, ly;
        uint32_t qi, j;
        slot_split(sg, slot, qi, j);
        if (slot_pixel(sg, qi, lx, ly)) {
            Ray r;
            uint64_t rng;
            cam_ray(sg, sc, j, lx, ly, r, rng);
            v[0] = r.o.x; v[1] = r.o.y; v[2] = r.o.z; v[3] = r.d.x;
            v[4] = r.d.y; v[5] = r.d.z; v[6] = r.tm; v[7] = __longlong_as_double(static_cast<long long>(rng));
        }
    }
#pragma unroll
    for (uint32_t f = 0; f < 8; ++f) ring.at(f, lane) = v[f];
}
template <uint32_t F, uint32_t TF, int LM>
__global__ __launch_bounds__(LM ? kBlockM : kBlock, LM ? 1 : ART_PATHS_G_WAVES) void k_paths_g(DevScene S0, PassGeom g, CameraRec cam, Work w,
                                                                                     uint32_t* next_slot) {
    // explicit-LDS node reads (traverse's PL path): LM 2 for its LDS part; LM 1 for every node (the XOR near/far
    // addressing needs the explicit LDS addresses; through the LDS-inferred pointer it costs more adds)
    constexpr int kLdsNodesPL = LM == 2 ? 1 : LM == 1 ? 2 : 0;
    constexpr int B = LM ? kBlockM : kBlock;
    // dynamic LDS: [traversal stack: g.stack entries x B lanes (+ sentinel row)][camera][pass geometry][LM: nodes,
    // primrefs, triangles] -- as in k_paths, the camera and pass geometry are read from LDS where a path starts (as
    // kernel arguments held in SGPRs for the whole loop they spilled ~100 SGPRs into VGPR lanes)
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr bool S16 = (F & F_CODE16) != 0;
    using ST = StackF<false, F>;
    ST* stk = reinterpret_cast<ST*>(smem) + B + stack_column<S16>(threadIdx.x);
    CameraRec& s_cam = *reinterpret_cast<CameraRec*>(smem + paths_g_stack_bytes(g.stack, B, S16));
    PassGeom& s_g = *reinterpret_cast<PassGeom*>(smem + paths_g_stack_bytes(g.stack, B, S16) + sizeof(CameraRec));
    stk[-B] = static_cast<ST>(kNodeEmpty);
    if (threadIdx.x == 0) {
        s_cam = cam;
        s_g = g;
        if (g.list_mode) {  // the list's entry count, on the device (PassGeom::list_mode)
            const uint32_t n = g.list[-1];
            s_g.nlist = n;
            s_g.P = n * g.k;
        }
    }
    [[maybe_unused]] JumpEntry* jt = reinterpret_cast<JumpEntry*>(smem + align16(paths_g_stack_bytes(g.stack, B, S16) + sizeof(CameraRec) + sizeof(PassGeom)));
    if (threadIdx.x < static_cast<uint32_t>(kJumpEntries)) jt[threadIdx.x] = pcg_jump(3u * threadIdx.x);
    DevScene S = S0;
    [[maybe_unused]] double* uvc = reinterpret_cast<double*>(jt + kJumpEntries);  // sphere u, v constants, LDS copy
    if constexpr ((TF & TF_IMAGE) != 0)
        if (threadIdx.x < static_cast<uint32_t>(kUvConsts)) uvc[threadIdx.x] = uv_table(S0)[threadIdx.x];
    size_t lm_off = paths_g_head_bytes(g.stack, B, S16);  // LM: world list and objects, then the BVH arrays
    if constexpr (LM != 0) {
        uint8_t* wb = smem + lm_off;
        for (int32_t i = static_cast<int32_t>(threadIdx.x); i < S0.nworld; i += B) reinterpret_cast<int32_t*>(wb)[i] = S0.world[i];
        uint8_t* ob = wb + align16(sizeof(int32_t) * static_cast<uint32_t>(S0.nworld));
        const uint4* os = reinterpret_cast<const uint4*>(S0.objs);
        for (uint32_t i = threadIdx.x; i < S0.n_objs * (sizeof(ObjRec) / 16); i += B) reinterpret_cast<uint4*>(ob)[i] = os[i];
        uint8_t* pb = ob + sizeof(ObjRec) * S0.n_objs;
        const uint4* ps = reinterpret_cast<const uint4*>(S0.obj_prims);
        for (uint32_t i = threadIdx.x; i < S0.n_objs * (sizeof(PrimRec80) / 16); i += B) reinterpret_cast<uint4*>(pb)[i] = ps[i];
        S.world = reinterpret_cast<const int32_t*>(wb);
        S.objs = reinterpret_cast<const ObjRec*>(ob);
        S.obj_prims = reinterpret_cast<const PrimRec80*>(pb);
        const uint32_t nm = lds_mats<TF>(S0.n_mats);
        if (nm) {
            uint8_t* mb = pb + sizeof(PrimRec80) * S0.n_objs;
            const uint2* ms = reinterpret_cast<const uint2*>(S0.mats);
            static_assert(sizeof(MatRec) % 8 == 0, "material records copied in 8-B pieces");
            for (uint32_t i = threadIdx.x; i < nm * (sizeof(MatRec) / 8); i += B) reinterpret_cast<uint2*>(mb)[i] = ms[i];
            S.mats = reinterpret_cast<const MatRec*>(mb);
        }
        lm_off += paths_g_world_bytes(S0.nworld, S0.n_objs, nm);
    }
    if constexpr (LM != 0) lm_off = align128(lm_off);  // node addresses multiples of 128 (device.h traverse: near/far planes by XOR)
    if constexpr (LM == 2) {  // the first n_lds_nodes nodes (the top levels of every BVH) into LDS
        BvhNode* m = reinterpret_cast<BvhNode*>(smem + lm_off);
        const uint4* s4 = reinterpret_cast<const uint4*>(S0.nodes);
        uint4* d4 = reinterpret_cast<uint4*>(m);
        for (uint32_t i = threadIdx.x; i < S0.n_lds_nodes * (sizeof(BvhNode) / 16); i += B) d4[i] = s4[i];
        S.nodes_lds = static_cast<uint32_t>(reinterpret_cast<size_t>((__attribute__((address_space(3))) BvhNode*)m));
    }
    if constexpr (LM == 1) {
        uint8_t* m = smem + lm_off;
        const size_t nb = sizeof(BvhNode) * S0.n_nodes, pb = align16(sizeof(uint32_t) * S0.n_primrefs);
        const size_t tb = (F & F_TRI) ? kLm1TriBytes * S0.n_primrefs : 0;
        auto copy = [&](uint8_t* dst, const void* src, size_t bytes) {
            const uint4* s4 = static_cast<const uint4*>(src);
            uint4* d4 = reinterpret_cast<uint4*>(dst);
            for (size_t i = threadIdx.x; i < bytes / 16; i += B) d4[i] = s4[i];
        };
        copy(m, S0.nodes, nb);
        // primrefs: 4-B entries, the tail of the last 16-B word comes from past the array's end -- copy word-wise
        for (uint32_t i = threadIdx.x; i < S0.n_primrefs; i += B) reinterpret_cast<uint32_t*>(m + nb)[i] = S0.primrefs[i];
        S.nodes = reinterpret_cast<const BvhNode*>(m);
        if constexpr (kLdsNodesPL) {  // every node read through the explicit-LDS path (device.h traverse, PL)
            S.nodes_lds = static_cast<uint32_t>(reinterpret_cast<size_t>((__attribute__((address_space(3))) uint8_t*)m));
            S.n_lds_nodes = S0.n_nodes;
        }
        S.primrefs = reinterpret_cast<const uint32_t*>(m + nb);
        if constexpr ((F & F_TRI) != 0) {
            copy(m + nb + pb, S0.leaf_tris112, tb);
            S.leaf_tris112 = reinterpret_cast<const TriRec112*>(m + nb + pb);
        }
        lm_off = align16(lm_off + nb + pb + tb);  // the camera-ray rings follow (kRing)
    }
    // radiance records: non-temporal where the scene's nodes and leaf records come from L2 (LM 0 / 2: the streaming
    // records would evict them; r6i: capsule +1.7 %, cow +0.8 %), temporal where they sit in LDS (LM 1: each 8-B NT
    // store reaches HBM as its own partial write, r5c; Cornell smoke -1.5 % with NT, the final and dino +-0)
    constexpr bool kResNT = LM != 1;
    constexpr bool kRing = paths_g_ring(F, LM);
    const bool use_ring = kRing && g.lds_ring != 0;  // the launch found room for the rings
    [[maybe_unused]] const RingG ring{reinterpret_cast<double*>(smem + lm_off) + (threadIdx.x / 64u) * (8u * kRingG)};
    [[maybe_unused]] uint32_t r_head = 0, r_avail = 0, r_b0 = 0;  // wave-uniform: next entry, entries left, batch slot
    [[maybe_unused]] bool r_exhausted = false;                   // every slot of the pass is in a batch
    const int max_depth = g.max_depth;
    __syncthreads();
    const uint32_t lane = __lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const V3 bg = mk(S.bg[0], S.bg[1], S.bg[2]);
    uint32_t cur = 0, end = 0;  // this wave's claimed slots [cur, end): wave-uniform
    bool busy = false, drained = false;
    uint32_t q = 0;
    int depth = 0;
    PathState st;
    unsigned long long segs = 0;
    // suspendable BVH traversals (ART_SUSPEND_LANES) where node fetches go to L2 (LM 0, 2); with the whole BVH in LDS
    // (LM 1) a traversal is short and suspending only adds rounds
    // (LM 1, the BVH in LDS: thresholds 4-40 measured -5 % to -22 % on dino and the final scene)
    constexpr int kSuspLanes = LM == 1 ? 0 : ART_SUSPEND_LANES;
    constexpr bool SUSP = kSuspLanes > 0;
    TraceState ts;  // the lane's segment trace, possibly suspended in a BVH
    bool in_trace = false;
#ifdef ART_TRACE
    bool tracing = false;
#endif
#ifdef ART_STATS
    unsigned long long tm_load = 0, tm_trace = 0, tm_shade = 0, tm_app = 0, tm_prev = __builtin_amdgcn_s_memtime();
    unsigned long long tm_surf = 0, tm_coop = 0, tm_tex = 0;  // the shading phase split (k_paths_g)
#endif
    for (;;) {
        const uint64_t idle = __ballot(!busy && !drained);
        if (use_ring && idle) {
            // the idle lanes of rank < first take the ring's remaining entries; when more lanes are idle than entries
            // are left (the ring is then empty) the wave refills it with the next 64 slots, converged, and the rest take
            // from the new batch (LDS operations of one wave complete in order: the refill's writes land after the
            // takes' reads of the old entries, and before the reads of the new ones)
            const uint32_t n = static_cast<uint32_t>(__popcll(idle));
            const uint32_t rank = static_cast<uint32_t>(__popcll(idle & below));
            const bool me = !busy && !drained;
            const uint32_t first = min(n, r_avail);
            int got = 0;
            if (me && rank < first) got = ring_take_g(ring, r_head + rank, r_b0, st, q);
            if (n > r_avail && !r_exhausted) {
                if (cur == end) {
                    const uint32_t chunk = s_g.chunk;
                    uint32_t nb = 0;
                    if (lane == 0) nb = atomicAdd(next_slot, chunk);
                    nb = __shfl(nb, 0);
                    cur = nb;
                    end = nb + chunk;
                }
                const uint32_t b = cur;
                cur += 64;
                __asm__ volatile("" ::: "memory");  // the LDS camera / pass geometry loads stay here (see k_paths)
                ring_fill_g(ring, lane, b + lane, s_g, s_cam);
                __asm__ volatile("" ::: "memory");
                r_b0 = b;
                r_exhausted = b + 64u >= s_g.P;  // g.P, or the device count's (list_mode): read where used
                if (me && rank >= first) got = ring_take_g(ring, rank - first, r_b0, st, q);
                r_head = n - first;
                r_avail = kRingG - r_head;
            } else {
                r_head += first;
                r_avail -= first;
                if (me && rank >= first) got = 2;  // no entries left and no slots: drained
            }
            if (me) {
                busy = got == 1;
                drained = got == 2;
                depth = 0;
#ifdef ART_TRACE
                if (busy) {  // as the ring-free path below: is this the traced (pixel, sample)?
                    int lx = 0, ly = 0;
                    uint32_t qi, j;
                    slot_split(s_g, q, qi, j);
                    slot_pixel(s_g, qi, lx, ly);
                    tracing = static_cast<long long>(global_row(s_g, ly)) * s_g.W + lx == g_trace_pixel &&
                              static_cast<long long>(s_g.sample_base + j) == g_trace_sample;
                }
#endif
            }
        } else if (idle) {
            const uint32_t n = static_cast<uint32_t>(__popcll(idle));
            const uint32_t rank = static_cast<uint32_t>(__popcll(idle & below));
            uint32_t slot;
            if (cur + n > end) {
                const uint32_t chunk = s_g.chunk;
                uint32_t nb = 0;
                if (lane == 0) nb = atomicAdd(next_slot, chunk);
                nb = __shfl(nb, 0);
                const uint32_t left = end - cur;
                slot = rank < left ? cur + rank : nb + (rank - left);
                cur = nb + (n - left);
                end = nb + chunk;
            } else {
                slot = cur + rank;
                cur += n;
            }
            if (!busy && !drained) {
                if (slot >= s_g.P) {
                    drained = true;
                } else {
                    int lx, ly;
                    q = slot;
                    __asm__ volatile("" ::: "memory");  // keep the LDS camera/geometry loads here (see k_paths)
                    uint32_t qi, j;
                    slot_split(s_g, slot, qi, j);
                    if (slot_pixel(s_g, qi, lx, ly)) {
                        gen_ray(s_g, s_cam, j, lx, ly, st);
                        busy = true;
                        depth = 0;
#ifdef ART_TRACE
                        tracing = static_cast<long long>(global_row(s_g, ly)) * s_g.W + lx == g_trace_pixel &&
                                  static_cast<long long>(s_g.sample_base + j) == g_trace_sample;
#endif
                    }
                }
            }
        }
        ART_TICK(tm_load);
        if (__ballot(busy) == 0) {
            if (__ballot(!drained) == 0) break;
            continue;
        }
        const bool allow = SUSP && __ballot(drained) == 0;  // suspend only while there are paths to start
        double t;
        HitOut h{0, 0, kMatUnknown};
        bool hitw = false, susp = false;
        Surf s;
        [[maybe_unused]] uint32_t mtype = MAT_LIGHT;
        if (busy) {
            const bool fresh = !in_trace;
            if (fresh) {
                ++segs;
                if constexpr (SUSP) ts.start();
            }
#ifdef ART_TRACE
            if (tracing && fresh)
                printf("TRACE d=%d o=%016llx,%016llx,%016llx dir=%016llx,%016llx,%016llx tm=%016llx rng=%016llx\n", depth, ART_DBITS(st.ray.o.x),
                       ART_DBITS(st.ray.o.y), ART_DBITS(st.ray.o.z), ART_DBITS(st.ray.d.x), ART_DBITS(st.ray.d.y), ART_DBITS(st.ray.d.z),
                       ART_DBITS(st.ray.tm), static_cast<unsigned long long>(st.rng));
#endif
            if constexpr (SUSP) {
                ts.tr.allow = allow;
                ts.tr.lanes = kSuspLanes;
                in_trace = !trace_world_res<F, B, kLdsNodesPL>(S, st.ray, stk, st.rng, ts);
                hitw = ts.any;
                t = ts.closest;
                h = ts.h;
            } else {
                hitw = trace_world<F, B, false, kLdsNodesPL>(S, nullptr, st.ray, stk, st.rng, t, h);
            }
            susp = in_trace;  // suspended: nothing to shade this round
            ART_TICK(tm_trace);
            if (!susp && hitw) {
                world_surface<F, (TF & TF_IMAGE) != 0, (TF & (TF_IMAGE | TF_BARY)) != 0>(S, h, st.ray, t, s, uvc);
                mtype = S.mats[s.mat].type;
            }
        }
        ART_TICK(tm_surf);
        // the whole wave draws random_in_unit_sphere for its lambertian, metal and isotropic hits (material.h:33, :55,
        // :129: each scatters with it first; metal's unit_vector draws nothing), as k_paths does
        const bool need = busy && !susp && hitw && (mtype == MAT_LAMBERTIAN || mtype == MAT_METAL || mtype == MAT_ISOTROPIC) &&
                          depth + 1 < max_depth;
        const V3 ps = coop_unit_sphere(need, st.rng, jt);
        const V3* pre = &ps;
        ART_TICK(tm_coop);
        if (busy) {
            bool cont = false;
            if (susp) {
            } else if (hitw) {
#ifdef ART_TRACE
                if (tracing)
                    printf("TRACE hit t=%016llx p=%016llx,%016llx,%016llx n=%016llx,%016llx,%016llx ff=%d mat=%d prim=%08x obj=%08x\n", ART_DBITS(t),
                           ART_DBITS(s.p.x), ART_DBITS(s.p.y), ART_DBITS(s.p.z), ART_DBITS(s.n.x), ART_DBITS(s.n.y), ART_DBITS(s.n.z), s.ff ? 1 : 0,
                           static_cast<int>(s.mat), h.prim, h.obj);
#endif
                const MatRec& mat = S.mats[s.mat];
                // In kernels with noise or image textures (where a texture value is costly): the
                // steps several materials take, once for the wave instead of once per material branch present -- the
                // texture value (diffuse_light, lambertian, isotropic: no draws) and one unit_vector (of the sphere
                // draw for lambertian, of the ray direction for metal and dielectric).  Measured +1.3 % on the
                // Next-Week final; with solid / checker textures only (cow, dino) the longer live ranges cost 1.5-2 %.
                constexpr bool kShared = (TF & (TF_NOISE | TF_IMAGE)) != 0;
                V3 texc = mk(0.0, 0.0, 0.0), uv = mk(0.0, 0.0, 0.0);
                if constexpr (kShared) {
                    const bool scat = depth + 1 < max_depth;
                    if (mat.type == MAT_LIGHT || (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_ISOTROPIC)))
                        texc = mat_tex_value<TF>(S, mat, s.u, s.v, s.p);
                    if (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_METAL || mat.type == MAT_DIELECTRIC))
                        uv = unit(mat.type == MAT_LAMBERTIAN ? *pre : st.ray.d);
                }
                const V3* texp = kShared ? &texc : nullptr;
                const V3* uvp = kShared ? &uv : nullptr;
                ART_TICK(tm_tex);
                if (mat.type == MAT_LIGHT) {  // material.h:114-116; diffuse_light never scatters
                    st.L = st.L + st.T * (texp ? *texp : mat_tex_value<TF>(S, mat, s.u, s.v, s.p));
                } else if (depth + 1 < max_depth) {
                    V3 att, dir;
                    bool sc = false;
                    switch (mat.type) {
                        case MAT_LAMBERTIAN: sc = scatter<MAT_LAMBERTIAN, TF>(S, mat, s, st, att, dir, pre, uvp, texp); break;
                        case MAT_METAL: sc = scatter<MAT_METAL, TF>(S, mat, s, st, att, dir, pre, uvp); break;
                        case MAT_DIELECTRIC: sc = scatter<MAT_DIELECTRIC, TF>(S, mat, s, st, att, dir, nullptr, uvp); break;
                        case MAT_ISOTROPIC: sc = scatter<MAT_ISOTROPIC, TF>(S, mat, s, st, att, dir, pre, nullptr, texp); break;
                        default: break;
                    }
                    if (sc) {
                        st.T = st.T * att;
                        st.ray.o = s.p;
                        st.ray.d = dir;
                        cont = true;
                    }
                }
            } else {  // engine.h:455-456: miss -> background
#ifdef ART_TRACE
                if (tracing) printf("TRACE miss\n");
#endif
                st.L = st.L + st.T * bg;
            }
            ART_TICK(tm_shade);
            if (susp) {
            } else if (cont) {
                ++depth;
            } else {
                store_res<kResNT>(w.res, q, st.L);
                busy = false;
            }
        }
        ART_TICK(tm_app);
    }
    for (int off = 32; off > 0; off >>= 1) segs += __shfl_xor(segs, off);
    if (lane == 0) atomicAdd(w.segments, segs);
#ifdef ART_STATS
    if (lane == 0) {
        atomicAdd(&g_art_stats[8], tm_load);
        atomicAdd(&g_art_stats[9], tm_trace);
        atomicAdd(&g_art_stats[10], tm_shade);
        atomicAdd(&g_art_stats[11], tm_app);
        atomicAdd(&g_art_stats[24], tm_surf);
        atomicAdd(&g_art_stats[25], tm_coop);
        atomicAdd(&g_art_stats[26], tm_tex);
    }
#endif
}

// k_paths_g instantiations without F_MEDIA_G sort packed keys over 16-bit child codes (F_CODE16); a scene
// whose codes do not fit them (more than 32768 nodes or 8192 primitive references) takes the F_ALL kernel instead
// The instantiations for meshes with solid/checker textures whose BVH is not all in LDS (LM 0 / 2: cow) live in
// k_paths_g_mesh.hip, compiled with LLVM's iterative-maxocc scheduler (Makefile MESH_SCHED): cow +1.3 % to +1.8 % over
// the default scheduler; dino's LM 1 kernel loses 0.9 % under it and the Next-Week final's 4.6 % (its spills double), so
// they stay in kernels.hip's object (r3z2)
constexpr uint32_t kMeshG = kFeatMesh | F_CODE16;
extern template __global__ void k_paths_g<kMeshG, kTexBasic, 0>(DevScene, PassGeom, CameraRec, Work, uint32_t*);
extern template __global__ void k_paths_g<kMeshG, kTexBasic, 2>(DevScene, PassGeom, CameraRec, Work, uint32_t*);

}  // namespace art

// k_paths.hip — k_paths, the persistent-path kernel of the LDS scene (the benchmark kernel), and its launcher, in
// their own object: the Makefile compiles it under PATHS_SCHED with ART_LDS_LEAF_NOREF=$(PATHS_NOREF).
#include "launch.h"
#include "path_work.h"

namespace art {

// Persistent-path variant of the fused LDS scene (EXT_MEGA): one launch traces a whole pass.  Every lane owns one
// path at a time and keeps it in registers from its camera ray to its end (engine.h:447-466 flattened: trace,
// shade_hit_lds, repeat until a miss, an absorption, a light or max_depth), then writes the slot's radiance and takes
// the next slot -- no path records, queues or per-depth launches, and the deep bounces of old paths share the waves
// with the first bounces of new ones instead of running as a tail of nearly empty launches.  Slots are claimed in
// increasing order in wave chunks of PassGeom::chunk from one counter (one atomic per chunk).  The bounce arithmetic
// and the RNG draws are those of the fused k_extend, so images are bit-identical to the wavefront variants.
// The slots a wave claims per atomic on the pass counter: PassGeom::chunk = path_chunk (pass_plan.h).
// First-bounce pool: a path start is run by the whole wave for however few lanes start a path (~a third of them per
// round), so paths are started 64 at a time -- one per lane, converged -- in a round of their own: the wave claims 64
// consecutive slots, generates their camera rays and traces and shades their first segment with the loop's own trace
// and shading code while the 64 rays are still together (sample-major slots: one 8x8-pixel patch; entry-major: one
// pixel -- nearly identical traversals, instead of one lane each in waves of unrelated secondary rays).  A path that
// ends there (miss, light, absorbed, max_depth 1) writes its radiance; one that continues is appended, compacted, to
// a per-wave ring in global memory as it stands after the bounce (scattered ray, throughput, RNG state, slot), and a
// lane that falls idle loads the next ring entry and goes on at depth 1.  The paths the lanes hold meanwhile are
// parked in a per-lane area behind the wave's ring for the round (plain vector stores and loads; their registers are
// the batch's), so the kernel keeps one trace and one shading site and its register count.
// ART_POOL_RING: ring entries per wave.  A batch runs whenever 64 entries are free (a batch may append fewer, a sky
// tile none); a round with more takers than entries leaves the rest idle for that round.  Measured for the camera-ray
// ring this one replaces (r3m, scene 1, PMC per segment; XCD-contiguous rings): HBM reads 3.50 B (128 entries) ->
// 0.10 B (96), writes 33.5 -> 27.9 B, Msamples/s +0.4 % (within the run-to-run spread).
#ifndef ART_POOL_RING
#define ART_POOL_RING 96
#endif
constexpr uint32_t kPoolRing = ART_POOL_RING;
static_assert(kPoolRing >= 96 && kPoolRing <= 128, "a ring holds the unread part of one batch and a whole new one");
struct __align__(16) PoolRay {  // a path after its first bounce: six 16-B pieces
    double2 a, b, c;  // (ox,oy) (oz,dx) (dy,dz)
    double2 d, e;     // (tm,Tr) (Tg,Tb)
    uint64_t rng;
    uint32_t slot, pad;
};
static_assert(sizeof(PoolRay) == 96, "ring entries and parked lanes are six 16-B pieces");
constexpr uint32_t kPoolPark = 64;  // PoolRay-sized records behind a wave's ring: the parked path of each lane
// A wave's ring.  Fields other than the pointer are wave-uniform.  batch(), append(), park() and unpark() are called
// by the whole wave in a first-bounce round; take() by the idle lanes of an ordinary round.  An entry is read at least
// one round after its stores: a first-bounce round ends with s_waitcnt vmcnt(0).
struct RayRing {
    PoolRay* ring;
    uint32_t head, tail;    // positions consumed / produced
    uint32_t cur, end;      // the wave's claimed slot chunk [cur, end)
    bool exhausted;         // every slot of the pass is in a batch
    // wave w of block b: the rings of one XCD's blocks are contiguous (blocks go to the 8 XCDs round
    // robin, block b to XCD b % 8), so each XCD's rings spread over all of its L2's sets instead of every block's
    // chunk landing on the same sets (block-major rings of one XCD lie 8 chunks apart: a power-of-two stride)
    __device__ __forceinline__ void init(void* pool, uint32_t block, uint32_t nblocks, uint32_t waves_per_block, uint32_t w) {
        const uint32_t per_xcd = (nblocks + kXcds - 1) / kXcds;
        const uint32_t wave = ((block % kXcds) * per_xcd + block / kXcds) * waves_per_block + w;
        ring = static_cast<PoolRay*>(pool) + static_cast<size_t>(wave) * (kPoolRing + kPoolPark);
        head = tail = cur = end = 0;
        exhausted = false;
    }
    // a first-bounce round is due: the ring has room for a whole batch's paths
    __device__ __forceinline__ bool room() const { return !exhausted && tail - head <= kPoolRing - 64u; }
    // Claims the next 64 slots and generates their camera rays: true for a lane whose slot is a pixel of the pass
    // (st: the new path, q: its slot); a padding slot of a partial tile or a slot >= P does nothing.
    __device__ __forceinline__ bool batch(const PassGeom& sg, const CameraRec<double>& sc, uint32_t* next_slot, uint32_t lane, PathState<double>& st,
                                          uint32_t& q) {
        if (cur == end) {
            const uint32_t chunk = sg.chunk;
            uint32_t nb = 0;
            if (lane == 0) nb = atomicAdd(next_slot, chunk);
            nb = __builtin_amdgcn_readfirstlane(nb);  // the whole wave is here: lane 0's
            cur = nb;
            end = nb + chunk;
        }
        const uint32_t b = cur;
        cur += 64;
        q = b + lane;
        __asm__ volatile("" ::: "memory");  // the LDS camera loads stay here
        if (b + 64u >= sg.P) exhausted = true;
        int lx, ly;
        uint32_t qi, j;
        slot_split(sg, q, qi, j);
        if (!(q < sg.P && slot_pixel(sg, qi, lx, ly))) return false;
        cam_ray(sg, sc, j, lx, ly, st.ray, st.rng);
        st.T = mk(1.0, 1.0, 1.0);
        return true;
    }
    // The batch's continuing paths, compacted: position = tail + the lane's rank among them.
    __device__ __forceinline__ void append(bool cont, uint64_t below, const PathState<double>& st, uint32_t q) {
        const uint64_t m = __ballot(cont);
        if (cont) {
            PoolRay& e = ring[(tail + static_cast<uint32_t>(__popcll(m & below))) % kPoolRing];
            e.a = make_double2(st.ray.o.x, st.ray.o.y);
            e.b = make_double2(st.ray.o.z, st.ray.d.x);
            e.c = make_double2(st.ray.d.y, st.ray.d.z);
            e.d = make_double2(st.ray.tm, st.T.x);
            e.e = make_double2(st.T.y, st.T.z);
            e.rng = st.rng;
            e.slot = q;
        }
        tail += static_cast<uint32_t>(__popcll(m));
    }
    // The idle lane of rank `rank`: 1 = a path goes on after its first bounce (st, q), 0 = the ring ran dry this round
    // (the lane idles a round), 2 = the pass is drained.
    __device__ __forceinline__ int take(uint32_t rank, PathState<double>& st, uint32_t& q) const {
        const uint32_t pos = head + rank;
        if (pos >= tail) return exhausted ? 2 : 0;
        const PoolRay& e = ring[pos % kPoolRing];
        const double2 a = e.a, b = e.b, c = e.c, d = e.d, f = e.e;
        st.ray.o = mk(a.x, a.y, b.x);
        st.ray.d = mk(b.y, c.x, c.y);
        st.ray.tm = d.x;
        st.T = mk(d.y, f.x, f.y);
        st.rng = e.rng;
        q = e.slot;
        return 1;
    }
    // after the round's take(): n entries consumed
    __device__ __forceinline__ void advance(uint32_t n) { head = min(head + n, tail); }
    // The lane's path for the length of a first-bounce round, piece-major behind the ring (each piece of the wave is
    // 1 KiB contiguous).  The compiler barriers keep the values dead between the stores and the loads.
    __device__ __forceinline__ void park(uint32_t lane, const PathState<double>& st, uint32_t q, int depth) const {
        double2* p = reinterpret_cast<double2*>(ring + kPoolRing) + lane;
        p[0 * 64] = make_double2(st.ray.o.x, st.ray.o.y);
        p[1 * 64] = make_double2(st.ray.o.z, st.ray.d.x);
        p[2 * 64] = make_double2(st.ray.d.y, st.ray.d.z);
        p[3 * 64] = make_double2(st.ray.tm, st.T.x);
        p[4 * 64] = make_double2(st.T.y, st.T.z);
        p[5 * 64] = make_double2(__longlong_as_double(static_cast<long long>(st.rng)),
                                 __hiloint2double(depth, static_cast<int>(q)));
        __asm__ volatile("" ::: "memory");
    }
    __device__ __forceinline__ void unpark(uint32_t lane, PathState<double>& st, uint32_t& q, int& depth) const {
        __asm__ volatile("" ::: "memory");
        const double2* p = reinterpret_cast<const double2*>(ring + kPoolRing) + lane;
        const double2 a = p[0 * 64], b = p[1 * 64], c = p[2 * 64], d = p[3 * 64], e = p[4 * 64], f = p[5 * 64];
        st.ray.o = mk(a.x, a.y, b.x);
        st.ray.d = mk(b.y, c.x, c.y);
        st.ray.tm = d.x;
        st.T = mk(d.y, e.x, e.y);
        st.rng = static_cast<uint64_t>(__double_as_longlong(f.x));
        q = static_cast<uint32_t>(__double2loint(f.y));
        depth = __double2hiint(f.y);
    }
};
__global__ __launch_bounds__(kBlockL, 1) void k_paths(DevScene<double> S0, PassGeom g, CameraRec<double> cam, Work<double> w, uint32_t* next_slot) {
    using R = double;
    constexpr int B = kBlockL;
    // dynamic LDS only (no static __shared__, so the image starts at LDS address 0 and every image offset is an
    // immediate): [scene image][traversal stack][camera][pass geometry] -- the camera and pass geometry are read
    // from LDS where a new path starts instead of being held in registers for the whole kernel (as kernel arguments
    // they pin ~60 SGPRs, which spill)
    extern __shared__ __align__(16) uint8_t smem[];
    const uint8_t* lds = smem;
    StackT<true>* stk = reinterpret_cast<StackT<true>*>(smem + kLdsImageBytes) + B + stack_column<true>(threadIdx.x);
    JumpEntry* jt = reinterpret_cast<JumpEntry*>(smem + kLdsImageBytes + paths_stack_bytes(g.stack));
    CameraRec<double>& s_cam = *reinterpret_cast<CameraRec<double>*>(smem + kLdsImageBytes + paths_stack_bytes(g.stack) + kJumpBytes);
    PassGeom& s_g = *reinterpret_cast<PassGeom*>(smem + kLdsImageBytes + paths_stack_bytes(g.stack) + kJumpBytes + sizeof(CameraRec<double>));
    stk[-B] = static_cast<StackT<true>>(kNodeEmpty);
    load_lds_image<B>(S0.lds_image, smem);
    if (threadIdx.x < static_cast<uint32_t>(kJumpEntries)) jt[threadIdx.x] = pcg_jump(3u * threadIdx.x);
    if (threadIdx.x == 0) {
        s_cam = cam;
        s_g = g;
        if (g.list_mode) {  // the list's entry count, on the device (PassGeom::list_mode)
            const uint32_t n = g.list[-1];
            s_g.nlist = n;
            s_g.P = n * g.k;
        }
    }
    DevScene<double> S = S0;
    {
        uint8_t* wb = smem + paths_lds_head(g.stack);
        uint8_t* ob = wb + sizeof(int32_t) * kPathsWorldCap;
        if (threadIdx.x < static_cast<uint32_t>(S0.nworld)) reinterpret_cast<int32_t*>(wb)[threadIdx.x] = S0.world[threadIdx.x];
        if (threadIdx.x < S0.n_objs * (sizeof(ObjRec<double>) / 16))
            reinterpret_cast<uint4*>(ob)[threadIdx.x] = reinterpret_cast<const uint4*>(S0.objs)[threadIdx.x];
        S.world = reinterpret_cast<const int32_t*>(wb);
        S.objs = reinterpret_cast<const ObjRec<double>*>(ob);
    }
    __syncthreads();
    const uint32_t lane = __lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const V3<R> bg = mk(S.bg[0], S.bg[1], S.bg[2]);
    bool busy = false, drained = false;
    uint32_t q = 0;
    int depth = 0;
    PathState<R> st;
    unsigned long long segs = 0;
#ifdef ART_STATS
    unsigned long long tm_load = 0, tm_trace = 0, tm_shade = 0, tm_app = 0, tm_fb = 0, tm_prev = __builtin_amdgcn_s_memtime();
#endif
    RayRing rr;
    rr.init(w.pool, blockIdx.x, gridDim.x, B / 64, threadIdx.x / 64);
    for (;;) {
        // A round is either a first-bounce round (the ring has room for a batch: all 64 lanes start a path, the paths
        // they hold are parked) or an ordinary one (idle lanes take ring entries, busy lanes trace their segment).
        // `act`: the lane traces and shades this round.  The ring and the area are private to the wave and no lane or
        // wave waits on another; every first-bounce round consumes 64 slots, so their number is bounded by the pass.
        const bool fb = rr.room();
        const bool held = __ballot(busy) != 0;
        bool act;
        if (fb) {
            if (held) rr.park(lane, st, q, depth);
            act = rr.batch(s_g, s_cam, next_slot, lane, st, q);
            depth = 0;
        } else {
            // every idle lane takes the next ring entry (more takers than entries: the rest idle a round)
            const uint64_t idle = __ballot(!busy && !drained);
            if (idle) {
                const uint32_t n = static_cast<uint32_t>(__popcll(idle));
                const uint32_t rank = static_cast<uint32_t>(__popcll(idle & below));
                if (!busy && !drained) {
                    const int got = rr.take(rank, st, q);
                    drained = got == 2;
                    busy = got == 1;
                    depth = 1;
                }
                rr.advance(n);
            }
            if (__ballot(busy) == 0) {
                ART_TICK(tm_load);
                if (__ballot(!drained) == 0) break;
                continue;
            }
            act = busy;
        }
        ART_TICK((fb ? tm_fb : tm_load));
        R t = R(0);
        HitOut h{0, 0, kMatUnknown};
        bool hitw = false;
        if (act) {
            ++segs;
            hitw = trace_world<R, kFeatSpheres, B, true>(S, lds, st.ray, stk, st.rng, t, h);
#if ART_LDS_LEAF_NOREF
            if (hitw) h.mt = reinterpret_cast<const uint32_t*>(lds + kLdsOffRef)[h.obj >> 16] >> kLdsRefMatShift;
#endif
        }
        // an ordinary round's ring loads are complete
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ART_TICK((fb ? tm_fb : tm_trace));
        // the whole wave draws random_in_unit_sphere for its lambertian and metal hits (material.h:33, :55), which
        // scatter with it first; lights and the max_depth bounce draw nothing
        const bool need = act && hitw && (h.mt == MAT_LAMBERTIAN || h.mt == MAT_METAL) && depth + 1 < g.max_depth;
        const V3<R> ps = coop_unit_sphere<R>(need, st.rng, jt);
        bool cont = false;
        if (act) {
            // a live path's radiance is zero: only a miss (engine.h:455-456) or a light adds to it, and both end the path
            st.L = mk(R(0), R(0), R(0));
            if (hitw) {
                cont = shade_hit_lds(lds, h.obj >> 16, h.mt, t, depth + 1 >= g.max_depth, st, &ps);
            } else {  // engine.h:455-456: miss -> background
                st.L = st.L + st.T * bg;
            }
            if (!cont) store_res(w.res, q, st.L);
        }
        ART_TICK((fb ? tm_fb : tm_shade));
        if (fb) {
#ifdef ART_STATS
            const uint64_t m_act = __ballot(act), m_cont = __ballot(cont);
            if (lane == 0) {
                atomicAdd(&g_art_stats[49], 1ull);
                atomicAdd(&g_art_stats[50], static_cast<unsigned long long>(__popcll(m_act)));
                atomicAdd(&g_art_stats[51], static_cast<unsigned long long>(__popcll(m_cont)));
            }
#endif
            rr.append(cont, below, st, q);
            if (held) rr.unpark(lane, st, q, depth);
            // the ring entries are stored before a later round loads them, and the parked paths are back
            __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (act) {
            if (cont) ++depth;
            else busy = false;
        }
        ART_TICK((fb ? tm_fb : tm_app));
    }
    for (int off = 32; off > 0; off >>= 1) segs += __shfl_xor(segs, off);
    if (lane == 0) atomicAdd(w.segments, segs);
#ifdef ART_STATS
    if (lane == 0) {
        atomicAdd(&g_art_stats[8], tm_load);
        atomicAdd(&g_art_stats[9], tm_trace);
        atomicAdd(&g_art_stats[10], tm_shade);
        atomicAdd(&g_art_stats[11], tm_app);
        atomicAdd(&g_art_stats[48], tm_fb);
    }
#endif
}

void launch_paths(int num_cu, hipStream_t st, const DevScene<double>& S, const PassGeom& g, const CameraRec<double>& cam, const Work<double>& w,
                  uint32_t* next_slot) {
    const size_t lds = paths_lds_bytes(g.stack);
    static const bool checked = static_lds_is_zero(reinterpret_cast<const void*>(k_paths));
    (void)checked;
    (void)blocks_per_cu(reinterpret_cast<const void*>(k_paths), kBlockL, lds);  // the LDS attribute; the grid is one block per CU
    hipLaunchKernelGGL(k_paths, dim3(num_cu), dim3(kBlockL), lds, st, S, g, cam, w, next_slot);
}
size_t pool_bytes(int variant, int num_cu) {
    return variant == EXT_MEGA ? sizeof(PoolRay) * (kPoolRing + kPoolPark) * kPoolWavesPerCu * static_cast<size_t>(num_cu) : 0;
}

}  // namespace art

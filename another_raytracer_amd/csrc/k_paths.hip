// k_paths.hip — k_paths, the persistent-path kernel of the LDS scene (the benchmark kernel), and its launcher, in
// their own object: the Makefile compiles it under PATHS_SCHED with ART_LDS_LEAF_NOREF=$(PATHS_NOREF).
#include "launch.h"
#include "path_pool.h"
#include "path_work.h"
#include "tile_lists.h"

namespace art {

// Persistent-path variant of the fused LDS scene (EXT_MEGA): one launch traces a whole pass.  Every lane owns one
// path at a time and keeps it in registers to its end (engine.h:447-466 flattened: trace, shade_hit_lds, repeat until
// a miss, an absorption, a light or max_depth; a path that a batch displaces waits in the wave's pool, below), then
// writes the slot's radiance -- no path records, queues or per-depth launches, and the deep bounces of old paths share the waves
// with the first bounces of new ones instead of running as a tail of nearly empty launches.  Slots are claimed in
// increasing order in wave chunks of PassGeom::chunk from one counter (one atomic per chunk).  The bounce arithmetic
// and the RNG draws are those of the fused k_extend, so images are bit-identical to the wavefront variants.
// The slots a wave claims per atomic on the pass counter: PassGeom::chunk = path_chunk (pass_plan.h).
// Path start: a path start is run by the whole wave for however few lanes start a path (~a third of them per round),
// so paths are started 64 at a time -- one per lane, converged -- in a round of their own, a batch: the wave claims 64
// consecutive slots, generates their camera rays and traces and shades their first segment with the loop's own trace
// and shading code while the 64 rays are still together (sample-major slots: one 8x8-pixel patch; entry-major: one
// pixel -- nearly identical traversals, instead of one lane each in waves of unrelated secondary rays).  A path that
// ends there (miss, light, absorbed, max_depth 1) writes its radiance; one that continues stays in its lane, in
// registers, and goes on at depth 1 in the next round.  The paths the lanes held before the batch are pushed,
// compacted, onto a per-wave LIFO pool in global memory (ray, throughput, RNG state, slot, depth), and a lane that falls
// idle in an ordinary round pops one.  A batch is due when kBatchIdle idle lanes would find the pool empty
// (path_pool.h), so the pool holds at most kPoolBound entries and its hot part is the few on top.  One trace and one
// shading site, and the register count of the loop without batches.
struct __align__(16) PoolRay {  // a displaced path: six 16-B pieces
    double2 a, b, c;  // (ox,oy) (oz,dx) (dy,dz)
    double2 d, e;     // (tm,Tr) (Tg,Tb)
    uint64_t rng;
    uint32_t slot, depth;
};
static_assert(sizeof(PoolRay) == 96, "pool entries are six 16-B pieces");
// A wave's pool.  Fields other than the pointer are wave-uniform.  batch() and push() are called by the whole wave in
// a batch round, pop() by the idle lanes of an ordinary round.  Memory ordering rests on the s_waitcnt vmcnt(0) that
// follows the trace of every round: a round's pushes and pops are issued before its trace, so (1) an entry is loaded
// at least one round after its stores completed, and (2) a slot is overwritten only in a round after the one whose
// load read it, when that load has completed.  Nothing after the trace touches the pool, so a round needs no wait
// at its end.
struct PathPool {
    PoolRay* base;
    uint32_t count;         // entries held
    uint32_t cur, end;      // the wave's claimed slot chunk [cur, end)
    bool exhausted;         // every slot of the pass is in a batch
    // wave w of block b: the pools of one XCD's blocks are contiguous (blocks go to the 8 XCDs round
    // robin, block b to XCD b % 8), so each XCD's pools spread over all of its L2's sets instead of every block's
    // chunk landing on the same sets (block-major pools of one XCD lie 8 chunks apart: a power-of-two stride)
    __device__ __forceinline__ void init(void* pool, uint32_t block, uint32_t nblocks, uint32_t waves_per_block, uint32_t w) {
        const uint32_t per_xcd = (nblocks + kXcds - 1) / kXcds;
        const uint32_t wave = ((block % kXcds) * per_xcd + block / kXcds) * waves_per_block + w;
        base = static_cast<PoolRay*>(pool) + static_cast<size_t>(wave) * kPoolCap;
        count = cur = end = 0;
        exhausted = false;
    }
    // Claims the next 64 slots and generates their camera rays: true for a lane whose slot is a pixel of the pass
    // (st: the new path, q: its slot); a padding slot of a partial tile or a slot >= P does nothing.
    // tile: the batch's 8x8 tile in sample-major passes (wave-uniform: its 64 slots are one tile's pixels).
    __device__ __forceinline__ bool batch(const PassGeom& sg, const CameraRec& sc, uint32_t* next_slot, uint32_t lane, PathState& st,
                                          uint32_t& q, uint32_t& tile) {
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
        tile = __builtin_amdgcn_readfirstlane(qi >> 6);  // the whole wave is here
        if (!(q < sg.P && slot_pixel(sg, qi, lx, ly))) return false;
        cam_ray(sg, sc, j, lx, ly, st.ray, st.rng);
        st.T = mk(1.0, 1.0, 1.0);
        return true;
    }
    // The paths a batch displaces, compacted: the busy lane of rank r among `m` stores at pool_push_pos(count, r).
    __device__ __forceinline__ void push(uint64_t m, uint32_t rank, bool busy, const PathState& st, uint32_t q, int depth) {
        if (busy) {
            PoolRay& e = base[pool_push_pos(count, rank)];
            e.a = make_double2(st.ray.o.x, st.ray.o.y);
            e.b = make_double2(st.ray.o.z, st.ray.d.x);
            e.c = make_double2(st.ray.d.y, st.ray.d.z);
            e.d = make_double2(st.ray.tm, st.T.x);
            e.e = make_double2(st.T.y, st.T.z);
            e.rng = st.rng;
            e.slot = q;
            e.depth = static_cast<uint32_t>(depth);
        }
        count += static_cast<uint32_t>(__popcll(m));
        __asm__ volatile("" ::: "memory");  // the stores are issued before the batch's camera rays and trace
    }
    // The idle lane of rank `rank` < npop takes the entry pool_pop_pos(count, rank); the caller lowers count by npop.
    __device__ __forceinline__ void pop(uint32_t rank, PathState& st, uint32_t& q, int& depth) const {
        const PoolRay& e = base[pool_pop_pos(count, rank)];
        const double2 a = e.a, b = e.b, c = e.c, d = e.d, f = e.e;
        st.ray.o = mk(a.x, a.y, b.x);
        st.ray.d = mk(b.y, c.x, c.y);
        st.ray.tm = d.x;
        st.T = mk(d.y, f.x, f.y);
        st.rng = e.rng;
        q = e.slot;
        depth = static_cast<int>(e.depth);
    }
};
// A batch's trace over its tile's record (tile_lists.h TileRec, as eight wave-uniform dwords: the count, then up to
// kTileK leaf slots, nearest first) instead of the tree: every active lane tests the record's slots in order on
// [0.001, closest], the interval and the leaf test of the world walk.  The record holds every sphere a camera ray of
// the tile can reach, and sphere_root's candidate root (the near root if >= tmin, else the far one) is accepted iff
// it is <= the current tmax, so the nearest accepted root over this superset is the one the traversal finds, whatever
// the order; all slots of a sphere hold the same bytes (device_scene.hip), so shading by the representative gives the
// same bits.  No stack, no node planes.
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bool trace_tile_list(const uint8_t* lds, const Ray& r, u32x8 rec, double& t, HitOut& h) {
    const double d_a = len2(r.d), d_inv_a = 1.0 / d_a;  // traverse()'s
    uint64_t q0 = rec[0] | (static_cast<uint64_t>(rec[1]) << 32), q1 = rec[2] | (static_cast<uint64_t>(rec[3]) << 32);
    uint64_t q2 = rec[4] | (static_cast<uint64_t>(rec[5]) << 32), q3 = rec[6] | (static_cast<uint64_t>(rec[7]) << 32);
    const uint32_t n = static_cast<uint32_t>(q0) & 0xFFFFu;
    double closest = __builtin_inf();
    bool any = false;
    for (uint32_t k = 0; k < n; ++k) {
        q0 = (q0 >> 16) | (q1 << 48), q1 = (q1 >> 16) | (q2 << 48), q2 = (q2 >> 16) | (q3 << 48), q3 >>= 16;
        const uint32_t slot = static_cast<uint32_t>(q0) & 0xFFFFu;
        double tt;
        uint32_t prim, mt;
        if (hit_lds_slot(lds, slot, r, d_a, d_inv_a, 0.001, closest, tt, prim, mt)) {
            closest = tt;
            any = true;
            h.prim = prim;
            h.obj = slot << 16;
            h.mt = mt;
        }
    }
    t = closest;
    return any;
}

__global__ __launch_bounds__(kBlockL, 1) void k_paths(DevScene S0, PassGeom g, CameraRec cam, Work w, uint32_t* next_slot) {
    constexpr int B = kBlockL;
    // dynamic LDS only (no static __shared__, so the image starts at LDS address 0 and every image offset is an
    // immediate): [scene image][traversal stack][camera][pass geometry] -- the camera and pass geometry are read
    // from LDS where a new path starts instead of being held in registers for the whole kernel (as kernel arguments
    // they pin ~60 SGPRs, which spill)
    extern __shared__ __align__(16) uint8_t smem[];
    const uint8_t* lds = smem;
    StackT<true>* stk = reinterpret_cast<StackT<true>*>(smem + kLdsImageBytes) + B + stack_column<true>(threadIdx.x);
    JumpEntry* jt = reinterpret_cast<JumpEntry*>(smem + kLdsImageBytes + paths_stack_bytes(g.stack));
    CameraRec& s_cam = *reinterpret_cast<CameraRec*>(smem + kLdsImageBytes + paths_stack_bytes(g.stack) + kJumpBytes);
    PassGeom& s_g = *reinterpret_cast<PassGeom*>(smem + kLdsImageBytes + paths_stack_bytes(g.stack) + kJumpBytes + sizeof(CameraRec));
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
    DevScene S = S0;
    {
        uint8_t* wb = smem + paths_lds_head(g.stack);
        uint8_t* ob = wb + sizeof(int32_t) * kPathsWorldCap;
        if (threadIdx.x < static_cast<uint32_t>(S0.nworld)) reinterpret_cast<int32_t*>(wb)[threadIdx.x] = S0.world[threadIdx.x];
        if (threadIdx.x < S0.n_objs * (sizeof(ObjRec) / 16))
            reinterpret_cast<uint4*>(ob)[threadIdx.x] = reinterpret_cast<const uint4*>(S0.objs)[threadIdx.x];
        S.world = reinterpret_cast<const int32_t*>(wb);
        S.objs = reinterpret_cast<const ObjRec*>(ob);
    }
    __syncthreads();
    const uint32_t lane = __lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const V3 bg = mk(S.bg[0], S.bg[1], S.bg[2]);
    bool busy = false;
    uint32_t q = 0;
    int depth = 0;
    PathState st;
    unsigned long long segs = 0;
#ifdef ART_STATS
    unsigned long long tm_load = 0, tm_trace = 0, tm_shade = 0, tm_app = 0, tm_fb = 0, tm_prev = __builtin_amdgcn_s_memtime();
#endif
    const bool lists = w.tiles != nullptr && g.list == nullptr;  // tile-order slots only (pixel lists keep the tree)
    uint32_t tile = 0;
    PathPool pp;
    pp.init(w.pool, blockIdx.x, gridDim.x, B / 64, threadIdx.x / 64);
    for (;;) {
        // A round is either a batch (enough idle lanes would find the pool empty: the busy lanes push their paths and
        // all 64 lanes start a new one) or an ordinary one (idle lanes pop entries, busy lanes trace their segment).
        // The entries a batch leaves in the pool stay there: popping them would only push them again.
        // `act`: the lane traces and shades this round.  The pool is private to the wave and no lane or wave waits on
        // another; every batch consumes 64 slots, so their number is bounded by the pass.
        const uint64_t m_busy = __ballot(busy);
        const uint32_t n_idle = 64u - static_cast<uint32_t>(__popcll(m_busy));
        const bool fb = pool_batch_due(pp.exhausted, pp.count, n_idle);
        bool act;
        if (fb) {
#ifdef ART_STATS
            if (lane == 0) atomicAdd(&g_art_stats[51], static_cast<unsigned long long>(__popcll(m_busy)));
#endif
            if (m_busy) pp.push(m_busy, static_cast<uint32_t>(__popcll(m_busy & below)), busy, st, q, depth);
            act = pp.batch(s_g, s_cam, next_slot, lane, st, q, tile);
            depth = 0;
        } else {
            const uint32_t npop = pool_pop_count(pp.count, n_idle);
            if (npop) {
                const uint32_t rank = static_cast<uint32_t>(__popcll(~m_busy & below));
                if (!busy && rank < npop) {
                    pp.pop(rank, st, q, depth);
                    busy = true;
                }
                pp.count -= npop;
            } else if (m_busy == 0) {  // the pass is exhausted, the pool is empty and no lane holds a path
                ART_TICK(tm_load);
                break;
            }
            act = busy;
        }
        ART_TICK((fb ? tm_fb : tm_load));
        double t = 0.0;
        HitOut h{0, 0, kMatUnknown};
        bool hitw = false;
        if (act) {
            ++segs;
            // a batch of a pass with tile lists (whole-image sample-major passes: Work::tiles) reads its tile's record
            // with one scalar load (constant address space: written by k_tile_lists before the launch); an overflow
            // tile, and every ordinary round, walks the tree
            u32x8 rec = {kTileOverflow, 0, 0, 0, 0, 0, 0, 0};
            if (fb && lists)
                rec = *(reinterpret_cast<const __attribute__((address_space(4))) u32x8*>(reinterpret_cast<uintptr_t>(w.tiles)) +
                        __builtin_amdgcn_readfirstlane(tile));
            if ((rec[0] & 0xFFFFu) != kTileOverflow) hitw = trace_tile_list(lds, st.ray, rec, t, h);
            else hitw = trace_world<kFeatSpheres, B, true>(S, lds, st.ray, stk, st.rng, t, h);
#if ART_LDS_LEAF_NOREF
            if (hitw) h.mt = reinterpret_cast<const uint32_t*>(lds + kLdsOffRef)[h.obj >> 16] >> kLdsRefMatShift;
#endif
        }
        // the round's pool stores and loads are complete (PathPool: both ordering rules rest on this wait)
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ART_TICK((fb ? tm_fb : tm_trace));
        // the whole wave draws random_in_unit_sphere for its lambertian and metal hits (material.h:33, :55), which
        // scatter with it first; lights and the max_depth bounce draw nothing
        const bool need = act && hitw && (h.mt == MAT_LAMBERTIAN || h.mt == MAT_METAL) && depth + 1 < g.max_depth;
        const V3 ps = coop_unit_sphere(need, st.rng, jt);
        bool cont = false;
        if (act) {
            // a live path's radiance is zero: only a miss (engine.h:455-456) or a light adds to it, and both end the path
            st.L = mk(0.0, 0.0, 0.0);
            if (hitw) {
                cont = shade_hit_lds(lds, h.obj >> 16, h.mt, t, depth + 1 >= g.max_depth, st, &ps);
            } else {  // engine.h:455-456: miss -> background
                st.L = st.L + st.T * bg;
            }
            if (!cont) store_res(w.res, q, st.L);
        }
        ART_TICK((fb ? tm_fb : tm_shade));
#ifdef ART_STATS
        if (fb) {
            const uint64_t m_act = __ballot(act);
            if (lane == 0) {
                atomicAdd(&g_art_stats[49], 1ull);
                atomicAdd(&g_art_stats[50], static_cast<unsigned long long>(__popcll(m_act)));
            }
        }
#endif
        // a batch's lanes all hold a new path or none; an ordinary round's idle lanes stay idle
        if (fb || act) {
            busy = cont;
            ++depth;
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

void launch_paths(int num_cu, hipStream_t st, const DevScene& S, const PassGeom& g, const CameraRec& cam, const Work& w,
                  uint32_t* next_slot) {
    const size_t lds = paths_lds_bytes(g.stack);
    static const bool checked = static_lds_is_zero(reinterpret_cast<const void*>(k_paths));
    (void)checked;
    (void)blocks_per_cu(reinterpret_cast<const void*>(k_paths), kBlockL, lds);  // the LDS attribute; the grid is one block per CU
    hipLaunchKernelGGL(k_paths, dim3(num_cu), dim3(kBlockL), lds, st, S, g, cam, w, next_slot);
}
size_t pool_bytes(int variant, int num_cu) {
    return variant == EXT_MEGA ? sizeof(PoolRay) * kPoolCap * kPoolWavesPerCu * static_cast<size_t>(num_cu) : 0;
}

}  // namespace art

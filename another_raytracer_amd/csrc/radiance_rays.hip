// radiance_rays.hip — rt_radiance_rays and rt_camera_rays: path-traced radiance along caller-given rays, and the
// renderer's own camera rays as data.  The kernels and their launchers (launch.h) in an object of their own, so that no
// kernel of kernels.hip, k_paths.hip or k_paths_g_mesh.hip moves.
#include <algorithm>

#include "art.h"
#include "path_work.h"
#include "ray_launch.h"

namespace art {

// Waves per SIMD of the HBM-scene forms, as k_paths_g's: 3 caps them at 168 VGPRs.  The three F_ALL forms then spill 2-3
// VGPRs (173-177 VGPRs and no spill at 2); the others fit either way (129-157).  Measured at 1920x1080x16 on the
// Next-Week final: 4.94 against 3.90 Gsegments/s at 2; cow, whose form fits either way, +-0.
constexpr int kRadianceWaves = 3;

// Dynamic LDS of a k_radiance_rays block: [scene image (L)][traversal stacks: `stack` rows x B lanes][jump table][job]
__host__ __device__ constexpr size_t radiance_jump_offset(bool L, uint32_t stack) {
    return L ? kLdsImageBytes + paths_stack_bytes(stack) : sizeof(int32_t) * stack * kBlock;
}
__host__ __device__ constexpr size_t radiance_lds_bytes(bool L, uint32_t stack) { return radiance_jump_offset(L, stack) + kJumpBytes + sizeof(RadianceJob); }

// Persistent paths from caller-given rays (rt_radiance_rays): path p = i * spp + s starts at ray i with throughput 1 and
// the RNG state job.rng[p], or pcg_seed(seed, id_base + i, sample_base + s), and runs _ray_color (engine.h:447-466) as
// k_paths_g's loop runs it -- the same trace_world, world_surface, wave-cooperative sphere draw and scatter calls in the
// same order, so a path started from cam_ray's ray and state ends with rt_render's bits.  Waves claim job.chunk path
// indices per atomic from one counter, and a lane whose path ended takes the wave's next index by ballot rank
// (k_paths_g's ring-free path start with the ray read from memory instead of generated); the path stays in registers.
// F / L as the other ray kernels (ray_launch.h), TF as k_guides.  L: the scene image at LDS address 0, no static LDS.
template <uint32_t F, bool L, uint32_t TF>
__global__ __launch_bounds__(L ? kBlockL : kBlock, L ? 1 : kRadianceWaves) void k_radiance_rays(DevScene S, RadianceJob job0) {
    constexpr int B = L ? kBlockL : kBlock;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem + (L ? kLdsImageBytes : 0u)) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    JumpEntry* jt = reinterpret_cast<JumpEntry*>(smem + radiance_jump_offset(L, job0.stack));
    if (threadIdx.x < static_cast<uint32_t>(kJumpEntries)) jt[threadIdx.x] = pcg_jump(3u * threadIdx.x);
    // the job is read from LDS where a path starts or ends, as k_paths_g reads its pass geometry: held in SGPRs for the
    // whole loop beside the scene view, the kernel arguments spill into VGPR lanes
    const RadianceJob& job = *reinterpret_cast<const RadianceJob*>(jt + kJumpEntries);
    if (threadIdx.x == 0) *reinterpret_cast<RadianceJob*>(jt + kJumpEntries) = job0;
    if constexpr (L) load_lds_image<B>(S.lds_image, smem);
    __syncthreads();
    const uint8_t* lds = L ? smem : nullptr;
    const uint32_t lane = __lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const V3 bg = mk(S.bg[0], S.bg[1], S.bg[2]);
    const int max_depth = job0.max_depth;
    uint32_t cur = 0, end = 0;  // this wave's claimed path indices [cur, end): wave-uniform
    bool busy = false, drained = false;
    uint32_t q = 0;
    int depth = 0;
    PathState st;
    uint32_t segs = 0;  // this lane's segments (32 bits: a register less in the loop; summed in 64)
    for (;;) {
        const uint64_t idle = __ballot(!busy && !drained);
        if (idle) {
            const uint32_t n = static_cast<uint32_t>(__popcll(idle));
            const uint32_t rank = static_cast<uint32_t>(__popcll(idle & below));
            uint32_t p;
            if (cur + n > end) {
                uint32_t nb = 0;
                if (lane == 0) nb = atomicAdd(job.next, job.chunk);
                nb = __shfl(nb, 0);
                const uint32_t left = end - cur;
                p = rank < left ? cur + rank : nb + (rank - left);
                cur = nb + (n - left);
                end = nb + job.chunk;
            } else {
                p = cur + rank;
                cur += n;
            }
            if (!busy && !drained) {
                __asm__ volatile("" ::: "memory");  // keep the LDS job loads here
                if (p >= job.P) {
                    drained = true;
                } else {
                    const uint32_t i = job.fd_spp.div(p), s = p - i * job.spp;
                    const double* r = job.rays + 7 * static_cast<size_t>(i);
                    st.ray.o = mk(r[0], r[1], r[2]);
                    st.ray.d = mk(r[3], r[4], r[5]);
                    st.ray.tm = r[6];
                    st.rng = job.rng ? job.rng[p]
                                     : splitmix64(((static_cast<uint64_t>(job.id_base + i) << 32) | (job.sample_base + s)) ^ job.seed_mix);
                    st.T = mk(1.0, 1.0, 1.0);
                    q = p;
                    busy = true;
                    depth = 0;
                }
            }
        }
        if (__ballot(busy) == 0) {
            if (__ballot(!drained) == 0) break;
            continue;
        }
        double t;
        HitOut h{0, 0, kMatUnknown};
        bool hitw = false;
        Surf s;
        uint32_t mtype = MAT_LIGHT;
        if (busy) {
            ++segs;
            hitw = trace_world<F, B, L>(S, lds, st.ray, stk, st.rng, t, h);
            if (hitw) {
                world_surface<F, (TF & TF_IMAGE) != 0, (TF & (TF_IMAGE | TF_BARY)) != 0>(S, h, st.ray, t, s, uv_table(S));
                mtype = S.mats[s.mat].type;
            }
        }
        // the whole wave draws random_in_unit_sphere for its lambertian, metal and isotropic hits, as k_paths_g does
        const bool need = busy && hitw && (mtype == MAT_LAMBERTIAN || mtype == MAT_METAL || mtype == MAT_ISOTROPIC) && depth + 1 < max_depth;
        const V3 ps = coop_unit_sphere(need, st.rng, jt);
        const V3* pre = &ps;
        if (busy) {
            bool cont = false;
            // a live path's radiance is zero: only a miss or a light adds to it, and both end the path
            st.L = mk(0.0, 0.0, 0.0);
            if (hitw) {
                const MatRec& mat = S.mats[s.mat];
                // the steps several materials share, once for the wave (k_paths_g.h: kernels with noise or image textures)
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
                st.L = st.L + st.T * bg;
            }
            if (cont) {
                ++depth;
            } else {
                if (job.res) {
                    store_res<false>(job.res, q, st.L);
                } else {  // spp == 1: path q is ray q; the sum of one sample from +0.0
                    double* o = job.radiance + 3 * static_cast<size_t>(q);
                    o[0] = 0.0 + st.L.x;
                    o[1] = 0.0 + st.L.y;
                    o[2] = 0.0 + st.L.z;
                }
                busy = false;
            }
        }
    }
    unsigned long long wsegs = segs;
    for (int off = 32; off > 0; off >>= 1) wsegs += __shfl_xor(wsegs, off);
    if (lane == 0) atomicAdd(job0.segments, wsegs);
}

// radiance[i] = +0.0 + L(i, 0) + L(i, 1) + ...: ray i's spp records in sample order (k_accum's order from a zeroed sum)
__global__ __launch_bounds__(256) void k_radiance_sum(const ResRec* res, uint32_t n, uint32_t spp, double* radiance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ResRec* r = res + static_cast<size_t>(i) * spp;
    double x = 0.0, y = 0.0, z = 0.0;
    for (uint32_t s = 0; s < spp; ++s) {
        double a, b, c;
        load_res(r, s, a, b, c);
        x += a;
        y += b;
        z += c;
    }
    double* o = radiance + 3 * static_cast<size_t>(i);
    o[0] = x;
    o[1] = y;
    o[2] = z;
}

// rt_camera_rays: cam_ray of every (local pixel, sample) slot of g, one thread per slot in the renderer's slot order
__global__ __launch_bounds__(256) void k_camera_rays(PassGeom g, CameraRec cam, double* rays, uint64_t* rng) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= g.P) return;
    uint32_t qi, j;
    slot_split(g, slot, qi, j);
    int lx, ly;
    if (!slot_pixel(g, qi, lx, ly)) return;
    Ray r;
    uint64_t state;
    cam_ray(g, cam, j, lx, ly, r, state);
    const size_t e = (static_cast<size_t>(ly) * static_cast<size_t>(g.W) + static_cast<size_t>(lx)) * g.k + j;
    double* o = rays + 7 * e;
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z;
    o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
    o[6] = r.tm;
    if (rng) rng[e] = state;
}

template <uint32_t F, bool L, uint32_t TF>
static void launch_radiance_ft(const DeviceScene& ds, int num_cu, hipStream_t st, const DevScene& S, const RadianceJob& job) {
    const void* kernel = reinterpret_cast<const void*>(k_radiance_rays<F, L, TF>);
    constexpr int B = L ? kBlockL : kBlock;
    const size_t lds = radiance_lds_bytes(L, job.stack);
    if constexpr (L) {
        static const bool checked = static_lds_is_zero(kernel);
        (void)checked;
    }
    // a persistent grid: every block the CUs hold at once, or fewer when the job has fewer paths than their lanes
    const uint64_t full = static_cast<uint64_t>(blocks_per_cu(kernel, B, lds)) * static_cast<uint64_t>(num_cu);
    const uint64_t need = (static_cast<uint64_t>(job.P) + B - 1) / B;
    hipLaunchKernelGGL((k_radiance_rays<F, L, TF>), dim3(static_cast<uint32_t>(std::min(full, need))), dim3(B), lds, st, S, job);
    (void)ds;
}

void launch_radiance_rays(const DeviceScene& ds, int flags, int num_cu, hipStream_t st, const RadianceJob& job, uint32_t n, const double background[3]) {
    DevScene S = ds.view;
    for (int a = 0; a < 3; ++a) S.bg[a] = background[a];
    // The LDS scene image only with solid / checker textures: with noise or image textures the 1024-lane block's 128
    // VGPRs do not hold the loop (19 spilled), so such a scene (the two perlin spheres, the earth) takes the HBM form --
    // as rt_render takes k_paths_g for it (extend_variant).
    with_ray_features(ds, (flags & RT_GLOBAL_SCENE) != 0 || !ds.tex_basic, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        constexpr bool L = decltype(l)::value;
        // the texture kinds the scene needs, as launch_guides chooses them
        if (ds.tex_basic) return launch_radiance_ft<F, L, kTexBasic>(ds, num_cu, st, S, job);
        if constexpr (!L) {
            if constexpr ((F & F_TRI) != 0)
                if (ds.tex_bary) return launch_radiance_ft<F, L, kTexBary>(ds, num_cu, st, S, job);
            launch_radiance_ft<F, L, TF_ALL>(ds, num_cu, st, S, job);
        }
    });
    if (job.res) hipLaunchKernelGGL(k_radiance_sum, dim3((n + 255) / 256), dim3(256), 0, st, job.res, n, job.spp, job.radiance);
}

void launch_camera_rays(hipStream_t st, const PassGeom& g, const CameraRec& cam, double* rays, uint64_t* rng) {
    hipLaunchKernelGGL(k_camera_rays, dim3((g.P + 255) / 256), dim3(256), 0, st, g, cam, rays, rng);
}

}  // namespace art

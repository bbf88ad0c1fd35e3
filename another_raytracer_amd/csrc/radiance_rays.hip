// radiance_rays.hip — rt_radiance_rays, rt_render_views and rt_camera_rays: path-traced radiance along caller-given rays
// or from a table of cameras, and the renderer's own camera rays as data.  The kernels and their launchers (launch.h) in
// an object of their own, so that no kernel of kernels.hip, k_paths.hip or k_paths_g_mesh.hip moves.
#include <algorithm>
#include <type_traits>

#include "art.h"
#include "path_work.h"
#include "ray_launch.h"

namespace art {

// Waves per SIMD of the HBM-scene forms, as k_paths_g's: 3 caps them at 168 VGPRs.  The three F_ALL forms then spill 2-3
// VGPRs (173-177 VGPRs and no spill at 2); the others fit either way (129-157).  Measured at 1920x1080x16 on the
// Next-Week final: 4.94 against 3.90 Gsegments/s at 2; cow, whose form fits either way, +-0.
constexpr int kRadianceWaves = 3;

// Dynamic LDS of a k_radiance_rays / k_radiance_views block: [scene image (L)][traversal stacks: `stack` rows x B lanes]
// [jump table][job]
__host__ __device__ constexpr size_t radiance_jump_offset(bool L, uint32_t stack) {
    return L ? kLdsImageBytes + paths_stack_bytes(stack) : sizeof(int32_t) * stack * kBlock;
}
template <class Job>
__host__ __device__ constexpr size_t radiance_lds_bytes(bool L, uint32_t stack) { return radiance_jump_offset(L, stack) + kJumpBytes + sizeof(Job); }

// cam_ray (path_work.h) for sample s at pixel (lx, ly) of a whole W x H frame -- band fields (H, 1, 0): the global row is
// the local one -- with the view's own camera and seed: the same operations in the same order.  Restated, not shared:
// a cam_ray that forwards to a core taking the seed apart moved k_paths and k_paths_g (other code for equal results).
__device__ __forceinline__ void view_cam_ray(const ViewsJob& job, const ViewRec& view, uint32_t s, int lx, int ly, Ray& ray, uint64_t& rng_out) {
    const CameraRec& cam = view.cam;
    const uint32_t pixel = static_cast<uint32_t>(ly) * static_cast<uint32_t>(job.W) + static_cast<uint32_t>(lx);
    uint64_t rng = splitmix64(((static_cast<uint64_t>(pixel) << 32) | s) ^ view.seed_mix);  // == pcg_seed(seed of the view, pixel, s)
    const double ru = uniform(rng);
    const double rv = uniform(rng);
    const double su = div_rcp(static_cast<double>(lx) + ru, static_cast<double>(job.W - 1), job.inv_w1);
    const double tv = div_rcp(static_cast<double>(job.H - 1 - ly) + rv, static_cast<double>(job.H - 1), job.inv_h1);
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
    Ray r;
    r.o = ld3(cam.origin) + offset;
    r.d = ld3(cam.llc) + su * ld3(cam.horizontal) + tv * ld3(cam.vertical) - ld3(cam.origin) - offset;
    r.tm = uniform(rng, cam.time0, cam.time1);
    // The ray and the state enter the path's registers as eight opaque values, as the memory source's enter as loads.
    // Without this the register coalescer joins the arithmetic above with the path state (whose origin is also the hit
    // point that scatter writes), and k_radiance_views<127, false, 3 / 19> park a 16-byte value of world_surface at 12
    // places (.vgpr_spill_count 48 against their siblings' 2 / 3); with it every form has its sibling's VGPRs (the first
    // of the two one more) and spills what its sibling does, or less.
    __asm__ volatile("" : "+v"(r.o.x), "+v"(r.o.y), "+v"(r.o.z), "+v"(r.d.x), "+v"(r.d.y), "+v"(r.d.z), "+v"(r.tm), "+v"(rng));
    ray = r;
    rng_out = rng;
}

// The persistent path kernel (radiance_loop.inc), built once per path source: k_radiance_rays and k_radiance_views.
// RadianceJob, paths from caller-given rays (rt_radiance_rays): path p = i * spp + s starts at ray i with throughput 1 and
// the RNG state job.rng[p], or pcg_seed(seed, id_base + i, sample_base + s), and runs _ray_color (engine.h:447-466) as
// k_paths_g's loop runs it -- the same trace_world, world_surface, wave-cooperative sphere draw and scatter calls in the
// same order, so a path started from cam_ray's ray and state ends with rt_render's bits.  Waves claim job.chunk path
// indices per atomic from one counter, and a lane whose path ended takes the wave's next index by ballot rank
// (k_paths_g's ring-free path start with the ray read from memory instead of generated); the path stays in registers.
// ViewsJob, paths from a table of cameras (rt_render_views): p = (v * npix + ly * W + lx) * spp + s starts at cam_ray's
// ray and post-camera state of view v's camera and seed (job.views[v], read at the path's start) for pixel (lx, ly),
// sample s of the whole W x H frame -- cam_ray's arithmetic (view_cam_ray) with the ray in registers -- so the path ends
// with the bits rt_render gives that view.  Row-major pixels: with a pixel's samples on consecutive indices a wave's 64
// claimed indices are 64 / spp neighbouring pixels of a row in tile order as well (from 8 samples up), and p is at once
// the index of the path's record and, over spp, of the pixel's sums: no padded slots, nothing to carry to the path's end.
// F / L as the other ray kernels (ray_launch.h), TF as k_guides.  L: the scene image at LDS address 0, no static LDS.
// rt_render_views' kernel has the same nine (F, L, TF) forms, the LDS-image one with one 1024-lane block per CU.
#define RADIANCE_KERNEL k_radiance_rays
#define RADIANCE_JOB RadianceJob
#define RADIANCE_CAMERAS 0
#include "radiance_loop.inc"
#undef RADIANCE_KERNEL
#undef RADIANCE_JOB
#undef RADIANCE_CAMERAS
#define RADIANCE_KERNEL k_radiance_views
#define RADIANCE_JOB ViewsJob
#define RADIANCE_CAMERAS 1
#include "radiance_loop.inc"
#undef RADIANCE_KERNEL
#undef RADIANCE_JOB
#undef RADIANCE_CAMERAS

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

template <uint32_t F, bool L, uint32_t TF, class Job>
static void launch_radiance_ft(const DeviceScene& ds, int num_cu, hipStream_t st, const DevScene& S, const Job& job) {
    const auto kfn = [] {
        if constexpr (std::is_same<Job, ViewsJob>::value) return &k_radiance_views<F, L, TF>;
        else return &k_radiance_rays<F, L, TF>;
    }();
    const void* kernel = reinterpret_cast<const void*>(kfn);
    constexpr int B = L ? kBlockL : kBlock;
    const size_t lds = radiance_lds_bytes<Job>(L, job.stack);
    if constexpr (L) {
        static const bool checked = static_lds_is_zero(kernel);
        (void)checked;
    }
    // a persistent grid: every block the CUs hold at once, or fewer when the job has fewer paths than their lanes
    const uint64_t full = static_cast<uint64_t>(blocks_per_cu(kernel, B, lds)) * static_cast<uint64_t>(num_cu);
    const uint64_t need = (static_cast<uint64_t>(job.P) + B - 1) / B;
    hipLaunchKernelGGL(kfn, dim3(static_cast<uint32_t>(std::min(full, need))), dim3(B), lds, st, S, job);
    (void)ds;
}

// The path kernel of either job type, then the sums of its n rays / pixels when job.res is set
template <class Job>
static void launch_radiance_job(const DeviceScene& ds, int flags, int num_cu, hipStream_t st, const Job& job, uint32_t n, const double background[3]) {
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

void launch_radiance_rays(const DeviceScene& ds, int flags, int num_cu, hipStream_t st, const RadianceJob& job, uint32_t n, const double background[3]) {
    launch_radiance_job(ds, flags, num_cu, st, job, n, background);
}
void launch_radiance_sum(hipStream_t st, const ResRec* res, uint32_t n, uint32_t spp, double* radiance) {
    hipLaunchKernelGGL(k_radiance_sum, dim3((n + 255) / 256), dim3(256), 0, st, res, n, spp, radiance);
}
void launch_radiance_views(const DeviceScene& ds, int flags, int num_cu, hipStream_t st, const ViewsJob& job, uint32_t npixels, const double background[3]) {
    launch_radiance_job(ds, flags, num_cu, st, job, npixels, background);
}

void launch_camera_rays(hipStream_t st, const PassGeom& g, const CameraRec& cam, double* rays, uint64_t* rng) {
    hipLaunchKernelGGL(k_camera_rays, dim3((g.P + 255) / 256), dim3(256), 0, st, g, cam, rays, rng);
}

}  // namespace art

// radiance_grad.hip — rt_radiance_grad: the gradient of path-traced radiance with respect to the solid texture colours,
// the metal albedos and the background, along caller-given rays.  The kernels and their launcher (launch.h) in an object
// of their own, so that no kernel of another object moves.
//
// With a fixed seed no scatter direction depends on a colour and _ray_color has no Russian roulette, so a path's
// radiance is a product: the attenuations a_0 .. a_{k-1} of its k scatter vertices times what ended it (a light's
// emission or the background, E).  k_radiance_grad walks rt_radiance_rays' path (radiance_loop.inc's loop: the same
// trace_world, world_surface, cooperative sphere draw and scatter calls in the same order, the same claim by ballot
// rank), records a GradVertex per scatter, and at a path's end walks the records back (art.h states the products op for
// op).  Contributions are summed exactly: each f64 as a 192-bit integer (grad_fixed.h) with integer atomics, carries by
// hand, rounded once by k_grad_finish -- the gradient's bits depend on neither the grid nor the order of the rays.
// Every path adds to the background's row or a lamp's, and most paths to a few large surfaces' rows.  Two remedies, both
// exact because integer sums commute: the lanes of a wave whose paths end in the same loop iteration walk back together,
// and at each step the lanes that add to the same row sum their integers in LDS first (wave_add), one lane then adding
// the sum; and the accumulator table exists in up to kGradMaxCopies copies, a block adding to copy blockIdx.x % copies,
// which k_grad_finish sums.
// The kernel's text is radiance_grad_loop.inc and its helpers grad_kernel.h: texel_grad.hip's k_texel_grad shares both.
#include <algorithm>

#include "grad_kernel.h"

namespace art {

#define GRAD_TEXELS 0
#include "radiance_grad_loop.inc"
#undef GRAD_TEXELS

// One thread per (row, column) of the three outputs: a colour column is the row's accumulator summed over the copies
// and rounded once (NaN when any copy's flag is set), every other column +0.0.
__global__ __launch_bounds__(256) void k_grad_finish(const unsigned long long* acc, uint32_t copies, uint32_t rows, uint32_t n_texs, uint32_t n_mats,
                                                     double* gt, double* gm, double* gb) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nt = n_texs * RT_TEXTURE_DOUBLES, nm = n_mats * RT_MATERIAL_DOUBLES;
    if (e >= nt + nm + 3) return;
    uint32_t row, col;
    double* out;
    if (e < nt) row = e / RT_TEXTURE_DOUBLES, col = e % RT_TEXTURE_DOUBLES, out = gt ? gt + e : nullptr;
    else if (e < nt + nm) row = n_texs + (e - nt) / RT_MATERIAL_DOUBLES, col = (e - nt) % RT_MATERIAL_DOUBLES, out = gm ? gm + (e - nt) : nullptr;
    else row = rows - 1, col = e - nt - nm, out = gb ? gb + col : nullptr;
    if (!out) return;
    if (col >= 3) {
        *out = 0.0;
        return;
    }
    Fix192 sum{{0, 0, 0}};
    unsigned long long bad = 0;
    for (uint32_t c = 0; c < copies; ++c) {
        const unsigned long long* r = acc + (static_cast<size_t>(c) * rows + row) * kGradRowLimbs;
        const Fix192 part{{r[3 * col], r[3 * col + 1], r[3 * col + 2]}};
        fix_add(sum, part);
        bad |= r[9];
    }
    *out = bad ? fix_double(0x7ff8000000000000ull) : fix_to_double(sum);
}

// The kernel for this scene: every scene takes an HBM-scene form (with_ray_features' global_scene), the texture kinds
// as launch_radiance_job chooses them.  fn(kernel)
template <class Fn>
static void with_grad_kernel(const DeviceScene& ds, Fn&& fn) {
    with_ray_features(ds, true, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        if constexpr (!decltype(l)::value) {
            if (ds.tex_basic) return fn(&k_radiance_grad<F, kTexBasic>);
            if constexpr ((F & F_TRI) != 0)
                if (ds.tex_bary) return fn(&k_radiance_grad<F, kTexBary>);
            fn(&k_radiance_grad<F, TF_ALL>);
        }
    });
}

uint32_t radiance_grad_grid(const DeviceScene& ds, int num_cu, uint32_t P, uint32_t stack) {
    uint64_t full = 0;
    with_grad_kernel(ds, [&](auto kfn) {
        full = static_cast<uint64_t>(blocks_per_cu(reinterpret_cast<const void*>(kfn), kBlock, grad_lds_bytes(stack))) * static_cast<uint64_t>(num_cu);
    });
    const uint64_t need = (static_cast<uint64_t>(P) + kBlock - 1) / kBlock;
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min(full, need)));
}

void launch_radiance_grad(const DeviceScene& ds, hipStream_t st, const GradJob& job, uint32_t grid, uint32_t n, const double background[3],
                          uint32_t n_mats, double* grad_textures, double* grad_materials, double* grad_background) {
    DevScene S = ds.view;
    for (int a = 0; a < 3; ++a) S.bg[a] = background[a];
    with_grad_kernel(ds, [&](auto kfn) { hipLaunchKernelGGL(kfn, dim3(grid), dim3(kBlock), grad_lds_bytes(job.path.stack), st, S, job); });
    if (job.path.res) launch_radiance_sum(st, job.path.res, n, job.path.spp, job.path.radiance);
    launch_grad_finish(st, job, n_mats, grad_textures, grad_materials, grad_background);
}

void launch_grad_finish(hipStream_t st, const GradJob& job, uint32_t n_mats, double* grad_textures, double* grad_materials, double* grad_background) {
    const uint32_t cells = job.n_texs * RT_TEXTURE_DOUBLES + n_mats * RT_MATERIAL_DOUBLES + 3;
    if (grad_textures || grad_materials || grad_background)
        hipLaunchKernelGGL(k_grad_finish, dim3((cells + 255) / 256), dim3(256), 0, st, job.acc, job.copies, job.rows, job.n_texs, n_mats, grad_textures,
                           grad_materials, grad_background);
}

}  // namespace art

// texel_grad.hip — rt_radiance_grad_texels with a texel output: rt_radiance_grad (radiance_grad.hip) with a row per
// image texel as well.  The kernels and their launcher (launch.h) in an object of their own, so that no kernel of
// another object moves.
//
// image_value (device.h) is a nearest-texel lookup whose result enters scatter as texc, exactly where a solid colour
// does, and no scatter direction depends on it: with a fixed seed the radiance is the same kind of product in the texel
// values (byte / 255 per channel) as in the solid colours.  k_texel_grad is k_radiance_grad's text
// (radiance_grad_loop.inc) with the value's row taken where the value is (grad_kernel.h image_value_row): the global
// texel first_k + j * w + i behind the T + M + 1 rows of the textures, the materials and the background.
// What differs is size: a scene has a few hundred of those rows and may have millions of texels, so the texel rows
// live in a second table whose copy count the host chooses within a byte budget (down to one: most texels are cold, and
// a small, magnified image -- the hot case -- is the one where copies are cheap).  Integer sums commute, so no bit
// depends on either count; wave_add's pre-sum in LDS serves texel rows as it serves the others (the lanes of a wave
// often land in one texel).  k_texel_finish sums a texel's copies and rounds once per channel, as k_grad_finish does.
#include <algorithm>

#include "grad_kernel.h"

namespace art {

#define GRAD_TEXELS 1
#include "radiance_grad_loop.inc"
#undef GRAD_TEXELS

// One thread per (texel, channel) of grad_texels: the row's accumulator summed over the copies and rounded once (NaN
// when any copy's flag is set).  A texel nothing was added to -- every texel of an image with bpp < 3 among them --
// comes out +0.0.
__global__ __launch_bounds__(256) void k_texel_finish(const unsigned long long* acc, uint32_t copies, uint32_t n_texels, double* out) {
    const uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= 3ull * n_texels) return;
    const uint32_t row = static_cast<uint32_t>(e / 3u), col = static_cast<uint32_t>(e - 3ull * row);
    Fix192 sum{{0, 0, 0}};
    unsigned long long bad = 0;
    for (uint32_t c = 0; c < copies; ++c) {
        const unsigned long long* r = acc + (static_cast<size_t>(c) * n_texels + row) * kGradRowLimbs;
        const Fix192 part{{r[3 * col], r[3 * col + 1], r[3 * col + 2]}};
        fix_add(sum, part);
        bad |= r[9];
    }
    out[e] = bad ? fix_double(0x7ff8000000000000ull) : fix_to_double(sum);
}

// The texel kernel for this scene, as with_grad_kernel chooses k_radiance_grad's: only the forms whose textures include
// an image.  fn(kernel); false (fn not called) for a scene of solid and checker textures.
template <class Fn>
static bool with_texel_kernel(const DeviceScene& ds, Fn&& fn) {
    if (ds.tex_basic) return false;
    with_ray_features(ds, true, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        if constexpr (!decltype(l)::value) {
            if constexpr ((F & F_TRI) != 0)
                if (ds.tex_bary) return fn(&k_texel_grad<F, kTexBary>);
            fn(&k_texel_grad<F, TF_ALL>);
        }
    });
    return true;
}

bool texel_grad_kernel(const DeviceScene& ds) { return !ds.tex_basic; }

uint32_t texel_grad_grid(const DeviceScene& ds, int num_cu, uint32_t P, uint32_t stack) {
    uint64_t full = 0;
    with_texel_kernel(ds, [&](auto kfn) {
        full = static_cast<uint64_t>(blocks_per_cu(reinterpret_cast<const void*>(kfn), kBlock, grad_lds_bytes(stack, sizeof(TexelJob)))) *
               static_cast<uint64_t>(num_cu);
    });
    const uint64_t need = (static_cast<uint64_t>(P) + kBlock - 1) / kBlock;
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min(full, need)));
}

void launch_texel_grad(const DeviceScene& ds, hipStream_t st, const TexelJob& job, uint32_t grid, uint32_t n, const double background[3],
                       uint32_t n_mats, double* grad_textures, double* grad_materials, double* grad_background, double* grad_texels) {
    DevScene S = ds.view;
    for (int a = 0; a < 3; ++a) S.bg[a] = background[a];
    with_texel_kernel(ds, [&](auto kfn) {
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(kBlock), grad_lds_bytes(job.g.path.stack, sizeof(TexelJob)), st, S, job);
    });
    if (job.g.path.res) launch_radiance_sum(st, job.g.path.res, n, job.g.path.spp, job.g.path.radiance);
    launch_grad_finish(st, job.g, n_mats, grad_textures, grad_materials, grad_background);
    const uint64_t cells = 3ull * job.n_texels;
    if (grad_texels && cells)
        hipLaunchKernelGGL(k_texel_finish, dim3(static_cast<uint32_t>((cells + 255) / 256)), dim3(256), 0, st, job.texel_acc, job.texel_copies,
                           job.n_texels, grad_texels);
}

}  // namespace art

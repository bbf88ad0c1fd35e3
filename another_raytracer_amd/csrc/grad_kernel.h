// grad_kernel.h — what the gradient path kernels share beside their loop (radiance_grad_loop.inc): the LDS layout of a
// block, the texture value with the accumulator row it came from, and the exact adds (grad_fixed.h) into a table of
// rows.  Included by radiance_grad.hip (k_radiance_grad) and texel_grad.hip (k_texel_grad).
#pragma once
#include "art.h"
#include "path_work.h"
#include "ray_launch.h"
#include "grad_fixed.h"

namespace art {

// Waves per SIMD, as k_radiance_rays' HBM-scene forms: 168 VGPRs
constexpr int kGradWaves = 3;

// Dynamic LDS of a gradient block: [traversal stacks: `stack` rows x kBlock lanes][jump table][job: `job_bytes`][a row
// of accumulator limbs per wave: wave_add's]
__host__ __device__ constexpr size_t grad_jump_offset(uint32_t stack) { return sizeof(int32_t) * stack * kBlock; }
__host__ __device__ constexpr size_t grad_scratch_offset(uint32_t stack, size_t job_bytes = sizeof(GradJob)) {
    return (grad_jump_offset(stack) + kJumpBytes + job_bytes + 7u) & ~size_t(7);
}
__host__ __device__ constexpr size_t grad_lds_bytes(uint32_t stack, size_t job_bytes = sizeof(GradJob)) {
    return grad_scratch_offset(stack, job_bytes) + sizeof(unsigned long long) * kGradRowLimbs * (kBlock / 64);
}

// tex_value (device.h) with the solid texture the value resolved to: `solid` is its index, or -1 for a noise or image
// value (and for the error colour).  The same doubles as tex_value.
template <uint32_t TF>
__device__ __forceinline__ V3 tex_value_id(const DevScene& S, int32_t ti, double u, double v, V3 p, int32_t& solid) {
    solid = -1;
    for (int level = 0; level < 4; ++level) {
        const TexRec& t = S.texs[ti];
        if (TF == TF_SOLID || t.type == TEX_SOLID) {
            solid = ti;
            return ld3(t.c);
        }
        if ((TF & TF_CHECKER) && t.type == TEX_CHECKER) {
            ti = checker_odd(p) ? t.odd : t.even;
            continue;
        }
        if ((TF & TF_NOISE) && t.type == TEX_NOISE) {
            const V3 q = t.scale * p;
            const double n = perlin_call(&S.perlins[t.perlin], q.x, q.y, q.z);
            const double h = (1.0 + n) * 0.5;
            return mk(h, h, h);
        }
        if ((TF & TF_IMAGE) && t.type == TEX_IMAGE) return image_value(S, t.image, u, v);
        if ((TF & (TF_IMAGE | TF_BARY)) && t.type == TEX_BARY_IMAGE) {
            const double w = 1.0 - u - v;
            return image_value(S, t.image, u * t.uv[0] + v * t.uv[2] + w * t.uv[4], u * t.uv[1] + v * t.uv[3] + w * t.uv[5]);
        }
        break;
    }
    return mk(0.0, 1.0, 1.0);
}
// mat_tex_value (device.h) likewise: the inlined copy of a MATF_SOLID record is its texture m.tex
template <uint32_t TF>
__device__ __forceinline__ V3 mat_tex_value_id(const DevScene& S, const MatRec& m, double u, double v, V3 p, int32_t& solid) {
    if (m.flags & MATF_SOLID) {
        solid = m.tex;
        return ld3(m.albedo);
    }
    return tex_value_id<TF>(S, m.tex, u, v, p, solid);
}

// image_value (device.h) with the accumulator row of the texel it read: image_row[im] is the row of the image's texel
// (0, 0) -- or kGradNoRow for an image with fewer than three bytes per texel, where the colour spans neighbouring
// texels' bytes and no texel owns it -- and texel (i, j) follows at j * w + i.  The same doubles as image_value.
__device__ __forceinline__ V3 image_value_row(const DevScene& S, const uint32_t* image_row, int32_t im, double u, double v, uint32_t& row) {
    const ImageRec& I = S.images[im];
    u = fmin(fmax(u, 0.0), 1.0);
    v = 1.0 - fmin(fmax(v, 0.0), 1.0);
    int i = static_cast<int>(u * static_cast<double>(I.w));
    int j = static_cast<int>(v * static_cast<double>(I.h));
    if (i >= I.w) i = I.w - 1;
    if (j >= I.h) j = I.h - 1;
    const double cs = 1.0 / 255.0;
    const uint8_t* px = S.texels + I.offset + static_cast<uint64_t>(j) * static_cast<uint64_t>(I.bpp * I.w) + static_cast<uint64_t>(i) * I.bpp;
    const uint32_t first = image_row[im];
    row = first == kGradNoRow ? kGradNoRow : first + static_cast<uint32_t>(j) * static_cast<uint32_t>(I.w) + static_cast<uint32_t>(i);
    return mk(cs * static_cast<double>(px[0]), cs * static_cast<double>(px[1]), cs * static_cast<double>(px[2]));
}
// tex_value_id with the row of an image value as well: `row` is the solid texture's index, the texel's row, or
// kGradNoRow (a noise value, a texel without a row, the error colour)
template <uint32_t TF>
__device__ __forceinline__ V3 tex_value_row(const DevScene& S, const uint32_t* image_row, int32_t ti, double u, double v, V3 p, uint32_t& row) {
    row = kGradNoRow;
    for (int level = 0; level < 4; ++level) {
        const TexRec& t = S.texs[ti];
        if (t.type == TEX_SOLID) {
            row = static_cast<uint32_t>(ti);
            return ld3(t.c);
        }
        if ((TF & TF_CHECKER) && t.type == TEX_CHECKER) {
            ti = checker_odd(p) ? t.odd : t.even;
            continue;
        }
        if ((TF & TF_NOISE) && t.type == TEX_NOISE) {
            const V3 q = t.scale * p;
            const double n = perlin_call(&S.perlins[t.perlin], q.x, q.y, q.z);
            const double h = (1.0 + n) * 0.5;
            return mk(h, h, h);
        }
        if ((TF & TF_IMAGE) && t.type == TEX_IMAGE) return image_value_row(S, image_row, t.image, u, v, row);
        if ((TF & (TF_IMAGE | TF_BARY)) && t.type == TEX_BARY_IMAGE) {
            const double w = 1.0 - u - v;
            return image_value_row(S, image_row, t.image, u * t.uv[0] + v * t.uv[2] + w * t.uv[4], u * t.uv[1] + v * t.uv[3] + w * t.uv[5], row);
        }
        break;
    }
    return mk(0.0, 1.0, 1.0);
}
template <uint32_t TF>
__device__ __forceinline__ V3 mat_tex_value_row(const DevScene& S, const uint32_t* image_row, const MatRec& m, double u, double v, V3 p, uint32_t& row) {
    if (m.flags & MATF_SOLID) {
        row = static_cast<uint32_t>(m.tex);
        return ld3(m.albedo);
    }
    return tex_value_row<TF>(S, image_row, m.tex, u, v, p, row);
}

// limb[0..2] += f, exactly, with integer atomics (global memory or LDS): limb by limb, a limb's carry (read from the
// atomic's return) added to the next; a zero limb with no carry adds nothing.
__device__ __forceinline__ void grad_add_fix(unsigned long long* limb, const Fix192& f) {
    uint64_t carry = 0;
    if (f.w[0]) {
        const uint64_t old = atomicAdd(limb, static_cast<unsigned long long>(f.w[0]));
        carry = old + f.w[0] < old ? 1u : 0u;
    }
    const uint64_t a1 = f.w[1] + carry;
    carry = a1 < carry ? 1u : 0u;  // (then a1 is 0)
    if (a1) {
        const uint64_t old = atomicAdd(limb + 1, static_cast<unsigned long long>(a1));
        carry += old + a1 < old ? 1u : 0u;
    }
    const uint64_t a2 = f.w[2] + carry;
    if (a2) atomicAdd(limb + 2, static_cast<unsigned long long>(a2));
}
// row += c, exactly: each colour as a Fix192.  A contribution grad_fixed.h refuses sets the row's NaN flag.
__device__ __forceinline__ void grad_add(unsigned long long* row, V3 c) {
    const double v[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Fix192 f;
        if (fix_from_double(v[a], f)) grad_add_fix(row + 3 * a, f);
        else atomicOr(row + 9, 1ull);
    }
}
// Where the rows of a block's accumulators are.  MainRows: one table (a block's copy of the textures + materials +
// background table).  TexelRows: that table for rows below `rows`, and the block's copy of the texel table behind it.
struct MainRows {
    unsigned long long* acc;
    __device__ __forceinline__ unsigned long long* operator()(uint32_t r) const { return acc + static_cast<size_t>(r) * kGradRowLimbs; }
};
struct TexelRows {
    unsigned long long *acc, *texels;
    uint32_t rows;
    __device__ __forceinline__ unsigned long long* operator()(uint32_t r) const {
        return r < rows ? acc + static_cast<size_t>(r) * kGradRowLimbs : texels + static_cast<size_t>(r - rows) * kGradRowLimbs;
    }
};
// Every lane with `has` adds c to row `row` of the table(s) `at`.  The lanes of a row that several lanes add to sum in
// the wave's LDS row `scratch` (zero on entry and on return) with the same limb arithmetic, and the first of them adds
// that sum to the table: one set of global atomics per distinct row instead of one per lane.  A lane alone on its row
// adds by itself, after the loop and together with the other such lanes.  Called by the whole wave.
template <class Rows>
__device__ __forceinline__ void wave_add_rows(const Rows& at, unsigned long long* scratch, uint32_t lane, bool has, uint32_t row, V3 c) {
    uint64_t todo = __ballot(has);
    bool alone = false;
    while (todo) {
        const int leader = __ffsll(static_cast<unsigned long long>(todo)) - 1;
        const uint32_t r = static_cast<uint32_t>(__shfl(static_cast<int>(row), leader));
        const bool mine = has && row == r;
        const uint64_t members = __ballot(mine);
        if (__popcll(members) == 1) {
            alone = alone || mine;
        } else {
            if (mine) grad_add(scratch, c);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup", "local");  // the wave's LDS atomics above, before the reads below
            if (lane == static_cast<uint32_t>(leader)) {
                unsigned long long* dst = at(r);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    Fix192 f;
                    f.w[0] = atomicExch(scratch + 3 * a, 0ull);
                    f.w[1] = atomicExch(scratch + 3 * a + 1, 0ull);
                    f.w[2] = atomicExch(scratch + 3 * a + 2, 0ull);
                    grad_add_fix(dst + 3 * a, f);
                }
                if (atomicExch(scratch + 9, 0ull)) atomicOr(dst + 9, 1ull);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup", "local");
        }
        todo &= ~members;
    }
    if (alone) grad_add(at(row), c);
}
__device__ __forceinline__ void wave_add(unsigned long long* acc, unsigned long long* scratch, uint32_t lane, bool has, uint32_t row, V3 c) {
    wave_add_rows(MainRows{acc}, scratch, lane, has, row, c);
}
__device__ __forceinline__ void wave_add(const TexelRows& at, unsigned long long* scratch, uint32_t lane, bool has, uint32_t row, V3 c) {
    wave_add_rows(at, scratch, lane, has, row, c);
}

}  // namespace art

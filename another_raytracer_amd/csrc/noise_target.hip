// noise_target.hip — the bookkeeping kernels of noise-target rendering (rt_render_noise_target): every
// pixel is traced until the standard error of its mean luminance is below a relative tolerance, up to a cap.  The paths
// themselves are traced by the persistent kernels k_paths / k_paths_g (whole-image passes, then pixel-list passes with
// entry-major slots); the kernels here add the radiance records onto the per-pixel sums, evaluate the test, build the
// next round's pixel list and write the frame.
//
// Exactness: a pixel that received n samples holds the sums and the RGB8 of rt_render with spp = n.  Every accumulator
// (acc[3], S1, S2) is continued from its stored value one sample at a time in sample order, as k_accum adds them; the
// test uses + - * / and comparisons only, compiled without contraction, and tests/nt_reference.py restates it.
#include "hip_check.h"
#include "noise_target.h"

namespace art {

// luminance of a radiance record (Rec. 709 weights), in this order
__device__ __forceinline__ double nt_luminance(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }

// true when the mean of n samples with sums S1, S2 is NOT yet within the tolerance: the standard error squared,
// var / n, against (rel_tol * (mean + lum_floor))^2.  NaN sums count as unconverged.
__device__ __forceinline__ bool nt_unconverged(double s1, double s2, int n, double rel_tol, double lum_floor) {
    const double dn = static_cast<double>(n);
    const double mean = s1 / dn;
    double var = (s2 - s1 * mean) / (dn - 1.0);
    if (var < 0.0) var = 0.0;
    const double se2 = var / dn;
    const double thr = rel_tol * (mean + lum_floor);
    return !(se2 <= thr * thr);
}

// One thread per tile-order pixel qi (k_accum's mapping: 8x8 tiles over W x rows), its k records at j * npix_pad + qi.
__global__ __launch_bounds__(256) void k_nt_accum_base(const double* __restrict__ res, uint32_t k, uint32_t npix_pad, uint32_t tiles_x, int W, int rows,
                                                       double* __restrict__ acc, double* __restrict__ mom) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= npix_pad) return;
    const uint32_t tile = qi >> 6, within = qi & 63u;
    const uint32_t ty = tile / tiles_x;
    const int lx = static_cast<int>((tile - ty * tiles_x) * 8 + (within & 7u));
    const int ly = static_cast<int>(ty * 8 + (within >> 3));
    if (lx >= W || ly >= rows) return;
    const size_t pix = static_cast<size_t>(ly) * W + lx;
    double* a = acc + 3 * pix;
    double* m = mom + 2 * pix;
    double r = a[0], g = a[1], b = a[2], s1 = m[0], s2 = m[1];
    for (uint32_t j = 0; j < k; ++j) {
        const double* rec = res + 3 * (static_cast<size_t>(j) * npix_pad + qi);
        const double x = rec[0], y = rec[1], z = rec[2];
        r += x;
        g += y;
        b += z;
        const double lum = nt_luminance(x, y, z);
        s1 += lum;
        s2 += lum * lum;
    }
    a[0] = r;
    a[1] = g;
    a[2] = b;
    m[0] = s1;
    m[1] = s2;
}

// One wave per list entry (as k_adapt_accum): the entry's k records are consecutive, the wave stages 64 of them per
// coalesced load in LDS and lanes 0..4 (r, g, b, S1, S2) each continue one running sum in sample order.
constexpr int kNtAccumWaves = 4;
__global__ __launch_bounds__(64 * kNtAccumWaves) void k_nt_accum_list(const uint32_t* __restrict__ list, const double* __restrict__ res, uint32_t k,
                                                                     double* __restrict__ acc, double* __restrict__ mom) {
    __shared__ double buf[kNtAccumWaves][3 * 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t e = blockIdx.x * kNtAccumWaves + wv;
    if (e >= list[-1]) return;  // wave-uniform
    const size_t pix = list[e];
    double* b = buf[wv];
    double* slot = lane < 3 ? acc + 3 * pix + lane : mom + 2 * pix + (lane - 3);  // lanes 0..4 only
    double sum = lane < 5 ? *slot : 0.0;
    const double* r = res + 3 * static_cast<size_t>(e) * k;
    for (uint32_t j0 = 0; j0 < k; j0 += 64) {
        const uint32_t n = min(64u, k - j0);
        if (lane < n) {
            const double* rec = r + 3 * static_cast<size_t>(j0 + lane);
            b[3 * lane] = rec[0];
            b[3 * lane + 1] = rec[1];
            b[3 * lane + 2] = rec[2];
        }
        // one wave: its LDS writes complete before its reads (in-order LDS, the waitcnt), and the compiler keeps them apart
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane < 5) {
            for (uint32_t i = 0; i < n; ++i) {
                const double x = b[3 * i], y = b[3 * i + 1], z = b[3 * i + 2];
                const double lum = nt_luminance(x, y, z);
                sum += lane == 0 ? x : lane == 1 ? y : lane == 2 ? z : lane == 3 ? lum : lum * lum;
            }
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next chunk's writes after these reads
    }
    if (lane < 5) *slot = sum;
}

// dilate only: the test's result of every active pixel into the flag plane (retired pixels keep their 0)
__global__ __launch_bounds__(256) void k_nt_flag(const uint32_t* __restrict__ cur, uint32_t n, const double* __restrict__ mom, int n_done, double rel_tol,
                                                 double lum_floor, uint8_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t p = cur ? cur[i] : i;
    flag[p] = nt_unconverged(mom[2 * p], mom[2 * p + 1], n_done, rel_tol, lum_floor) ? 1 : 0;
}

// Wave-aggregated append (path_work.h wave_append): one atomic per wave on the list's count word.  List order across
// waves varies from run to run; nothing downstream depends on it (every per-pixel sum is addressed by pixel).
template <bool DILATE>
__global__ __launch_bounds__(256) void k_nt_select(const uint32_t* __restrict__ cur, uint32_t n, const double* __restrict__ mom,
                                                   const uint8_t* __restrict__ flag, int W, int rows, int n_done, int k_next, double rel_tol,
                                                   double lum_floor, uint32_t* __restrict__ next, int32_t* __restrict__ count,
                                                   uint32_t* __restrict__ converged) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    uint32_t p = 0;
    bool want = false;  // the test keeps the pixel active
    if (valid) {
        p = cur ? cur[i] : i;
        if constexpr (DILATE) {
            const int y = static_cast<int>(p / static_cast<uint32_t>(W)), x = static_cast<int>(p - static_cast<uint32_t>(y) * static_cast<uint32_t>(W));
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx, yy = y + dy;
                    if (xx >= 0 && xx < W && yy >= 0 && yy < rows) want = want || flag[static_cast<size_t>(yy) * W + xx] != 0;
                }
        } else {
            want = nt_unconverged(mom[2 * static_cast<size_t>(p)], mom[2 * static_cast<size_t>(p) + 1], n_done, rel_tol, lum_floor);
        }
    }
    const bool keep = valid && want && k_next > 0;
    if (valid) count[p] = n_done + (keep ? k_next : 0);
    const uint32_t lane = __lane_id();
    const uint64_t mask = __ballot(keep);
    if (mask != 0) {
        const int leader = __ffsll(static_cast<long long>(mask)) - 1;
        uint32_t base = 0;
        if (static_cast<int>(lane) == leader) base = atomicAdd(next - 1, static_cast<uint32_t>(__popcll(mask)));
        base = __shfl(base, leader);
        if (keep) {
            const uint32_t off = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
            next[base + off] = p;
        }
    }
    const uint64_t done = __ballot(valid && !want);
    if (done != 0 && lane == static_cast<uint32_t>(__ffsll(static_cast<long long>(done)) - 1)) atomicAdd(converged, static_cast<uint32_t>(__popcll(done)));
}

__global__ __launch_bounds__(256) void k_nt_finalize(const double* __restrict__ acc, const int32_t* __restrict__ count, uint8_t* __restrict__ rgb,
                                                     uint32_t n) {  // k_finalize with the pixel's own count
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double scale = 1.0 / count[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double x = sqrt(scale * acc[3 * static_cast<size_t>(i) + c]);
        x = x < 0.0 ? 0.0 : (x > 0.999 ? 0.999 : x);
        rgb[3 * static_cast<size_t>(i) + c] = static_cast<uint8_t>(256 * x);
    }
}

void nt_accum_base(void* stream, const double* res, uint32_t k, uint32_t npix_pad, uint32_t tiles_x, int W, int rows, double* acc, double* mom) {
    hipLaunchKernelGGL(k_nt_accum_base, dim3((npix_pad + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), res, k, npix_pad, tiles_x, W, rows,
                       acc, mom);
    HIP_OK(hipGetLastError());
}
void nt_accum_list(void* stream, const uint32_t* list, uint32_t n, const double* res, uint32_t k, double* acc, double* mom) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_nt_accum_list, dim3((n + kNtAccumWaves - 1) / kNtAccumWaves), dim3(64 * kNtAccumWaves), 0, static_cast<hipStream_t>(stream), list,
                       res, k, acc, mom);
    HIP_OK(hipGetLastError());
}
void nt_select(void* stream, const uint32_t* cur, uint32_t n, const double* mom, uint8_t* flag, int W, int rows, int n_done, int k_next, bool dilate,
               double rel_tol, double lum_floor, uint32_t* next, int32_t* count, uint32_t* converged) {
    if (n == 0) return;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((n + 255) / 256), block(256);
    if (dilate) {
        hipLaunchKernelGGL(k_nt_flag, grid, block, 0, st, cur, n, mom, n_done, rel_tol, lum_floor, flag);
        hipLaunchKernelGGL(k_nt_select<true>, grid, block, 0, st, cur, n, mom, flag, W, rows, n_done, k_next, rel_tol, lum_floor, next, count, converged);
    } else {
        hipLaunchKernelGGL(k_nt_select<false>, grid, block, 0, st, cur, n, mom, flag, W, rows, n_done, k_next, rel_tol, lum_floor, next, count, converged);
    }
    HIP_OK(hipGetLastError());
}
void nt_finalize(void* stream, const double* acc, const int32_t* count, uint8_t* rgb, uint32_t npix) {
    hipLaunchKernelGGL(k_nt_finalize, dim3((npix + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), acc, count, rgb, npix);
    HIP_OK(hipGetLastError());
}

}  // namespace art

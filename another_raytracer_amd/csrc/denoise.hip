// denoise.hip — variance-guided edge-avoiding a-trous wavelet filter over the renderer's f64 radiance sums and the
// first-hit guide buffers (kernels.hip k_guides).
//
// Two half-renders of the same frame (independent seeds) give a per-pixel mean and an estimate of the mean's variance;
// the mean is divided by the first hit's albedo (demodulation, so texture detail is not filtered), then `iterations`
// 5x5 a-trous passes (tap spacing 1, 2, 4, ...) average it with weights from the guides (normal, plane distance, miss)
// and from the colour difference measured against the 3x3-blurred variance, which is filtered along (weights squared).
// The arithmetic is IEEE f64 + - * / and comparisons in one fixed order (the build's -ffp-contract=off keeps it
// unfused), with no exp / pow / sqrt before the final write_color: tests/dn_reference.py restates it in numpy and the
// GPU result equals it bit for bit.
#include <map>
#include <memory>
#include <mutex>
#include <utility>

#include "denoise.h"
#include "hip_check.h"
#include "options.h"
#include "workspace.h"

namespace art {
namespace {

constexpr int kGuide = 10;        // RT_GUIDE_DOUBLES: albedo[3], normal[3], position[3], t
constexpr int kDnBlockX = 64, kDnBlockY = 4;

// np.maximum(a, b) for a b that is not NaN: a NaN a stays NaN (fmax would drop it)
__device__ __forceinline__ double dn_max(double a, double b) { return (a > b || a != a) ? a : b; }

// The filter's working set is planar (one plane of npix doubles per quantity, so a wave's 64 pixels read 512 contiguous
// bytes per plane): L[3] and V ping-pong between iterations; the guide planes normal[3], position[3], t are written once
// by k_dn_prepare from the 10-double guide records.
enum DnPlane : int { PL_L0 = 0, PL_L1, PL_L2, PL_V, PL_NX, PL_NY, PL_NZ, PL_PX, PL_PY, PL_PZ, PL_T, kDnPlanes };

// Per pixel and channel: a = accum_a / spp, b = accum_b / spp, c = (a + b) / 2, var = ((a - b) / 2)^2,
// A = max(albedo, floor) (1 without demodulation), L = c / A, V = (var0 / A0^2 + var1 / A1^2) + var2 / A2^2.
__global__ void k_dn_prepare(uint32_t n, const double* __restrict__ acc_a, const double* __restrict__ acc_b, double spp_each,
                             const double* __restrict__ guides, double floor_a, int demod, double* __restrict__ L, double* __restrict__ V,
                             double* __restrict__ G) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* g = guides + kGuide * static_cast<size_t>(i);
    double q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = acc_a[3 * static_cast<size_t>(i) + c] / spp_each;
        const double b = acc_b[3 * static_cast<size_t>(i) + c] / spp_each;
        const double mean = (a + b) / 2.0;
        const double half = (a - b) / 2.0;
        const double var = half * half;
        const double A = demod ? dn_max(g[c], floor_a) : 1.0;
        L[static_cast<size_t>(c) * n + i] = mean / A;
        q[c] = var / (A * A);
    }
    V[i] = (q[0] + q[1]) + q[2];
#pragma unroll
    for (int k = 0; k < 7; ++k) G[static_cast<size_t>(k) * n + i] = g[3 + k];
}

// Where an a-trous iteration reads its taps: the planes in global memory, or a block's tile of them in LDS.
struct DnGlobalSrc {
    const double* L;
    const double* V;
    const double* G;
    size_t n;
    int W;
    template <int P>
    __device__ __forceinline__ double at(int x, int y) const {
        const size_t q = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
        if (P < PL_V) return L[static_cast<size_t>(P) * n + q];
        if (P == PL_V) return V[q];
        return G[static_cast<size_t>(P - PL_NX) * n + q];
    }
};
template <int TW, int TH>
struct DnLdsSrc {
    const double* tile;  // kDnPlanes planes of TW x TH doubles
    int x0, y0;          // image coordinates of the tile's first entry
    template <int P>
    __device__ __forceinline__ double at(int x, int y) const {
        return tile[P * (TW * TH) + (y - y0) * TW + (x - x0)];
    }
};

// One pixel of one a-trous iteration with tap spacing STEP.  The 3x3 variance blur of the centre pixel is computed
// here.  Tap order (dy = -2..2, then dx = -2..2, out-of-image taps skipped) and every sum's order are the contract.
template <int STEP, class Src>
__device__ __forceinline__ void dn_atrous_pixel(const Src& src, int x, int y, int W, int H, double sc2, double sp2, int squarings, double out[4]) {
    const double G3[3] = {1.0 / 4, 1.0 / 2, 1.0 / 4};
    const double K[5] = {1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16};
    double bs = 0.0, bw = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const double g = G3[dy + 1] * G3[dx + 1];
            bs += g * src.template at<PL_V>(qx, qy);
            bw += g;
        }
    }
    const double vf = bs / bw;
    const double cden = sc2 * vf + 1e-12;
    const double npx = src.template at<PL_NX>(x, y), npy = src.template at<PL_NY>(x, y), npz = src.template at<PL_NZ>(x, y);
    const double ppx = src.template at<PL_PX>(x, y), ppy = src.template at<PL_PY>(x, y), ppz = src.template at<PL_PZ>(x, y);
    const bool miss_p = !(src.template at<PL_T>(x, y) < __builtin_inf());
    const double lp0 = src.template at<PL_L0>(x, y), lp1 = src.template at<PL_L1>(x, y), lp2 = src.template at<PL_L2>(x, y);
    double sw = 0.0, sl0 = 0.0, sl1 = 0.0, sl2 = 0.0, sv = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * STEP;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * STEP;
            if (qx < 0 || qx >= W) continue;
            const double h = K[dy + 2] * K[dx + 2];
            const double lq0 = src.template at<PL_L0>(qx, qy), lq1 = src.template at<PL_L1>(qx, qy), lq2 = src.template at<PL_L2>(qx, qy);
            const double vq = src.template at<PL_V>(qx, qy);
            double w = h;
            if (dx != 0 || dy != 0) {
                const bool miss_q = !(src.template at<PL_T>(qx, qy) < __builtin_inf());
                double wg;
                if (miss_p || miss_q) {
                    wg = (miss_p && miss_q) ? 1.0 : 0.0;
                } else {
                    const double nqx = src.template at<PL_NX>(qx, qy), nqy = src.template at<PL_NY>(qx, qy), nqz = src.template at<PL_NZ>(qx, qy);
                    double dn = dn_max((npx * nqx + npy * nqy) + npz * nqz, 0.0);
                    for (int k = 0; k < squarings; ++k) dn = dn * dn;
                    const double ddx = src.template at<PL_PX>(qx, qy) - ppx, ddy = src.template at<PL_PY>(qx, qy) - ppy,
                                 ddz = src.template at<PL_PZ>(qx, qy) - ppz;
                    const double dp = (npx * ddx + npy * ddy) + npz * ddz;
                    const double dd = (ddx * ddx + ddy * ddy) + ddz * ddz;
                    const double wp = dd > 0.0 ? dn_max(1.0 - (dp * dp) / (sp2 * dd), 0.0) : 1.0;
                    wg = dn * wp;
                }
                const double e0 = lq0 - lp0, e1 = lq1 - lp1, e2 = lq2 - lp2;
                const double dc = (e0 * e0 + e1 * e1) + e2 * e2;
                const double wc = 1.0 / (1.0 + dc / cden);
                w = (h * wg) * wc;
            }
            sw += w;
            sl0 += w * lq0;
            sl1 += w * lq1;
            sl2 += w * lq2;
            sv += (w * w) * vq;
        }
    }
    out[0] = sl0 / sw;
    out[1] = sl1 / sw;
    out[2] = sl2 / sw;
    out[3] = sv / (sw * sw);
}

// Direct form: one pixel per thread, every tap a global load (served by L1 / L2; from tap spacing 4 on, a block's taps
// hardly overlap and a tile's halo would outgrow it).
template <int STEP>
__global__ __launch_bounds__(kDnBlockX* kDnBlockY) void k_dn_atrous(int W, int H, const double* __restrict__ Lin, const double* __restrict__ Vin,
                                                                    const double* __restrict__ G, double* __restrict__ Lout,
                                                                    double* __restrict__ Vout, double sc2, double sp2, int squarings) {
    const int x = static_cast<int>(blockIdx.x) * kDnBlockX + static_cast<int>(threadIdx.x);
    const int y = static_cast<int>(blockIdx.y) * kDnBlockY + static_cast<int>(threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t n = static_cast<size_t>(W) * static_cast<size_t>(H);
    const DnGlobalSrc src{Lin, Vin, G, n, W};
    double o[4];
    dn_atrous_pixel<STEP>(src, x, y, W, H, sc2, sp2, squarings, o);
    const size_t p = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
    Lout[p] = o[0];
    Lout[n + p] = o[1];
    Lout[2 * n + p] = o[2];
    Vout[p] = o[3];
}

// LDS-tile form for tap spacings 1 and 2, where the 25 taps of neighbouring pixels overlap: a block of kDnTileX x
// kDnTileY pixels first copies the 11 planes of its tile plus a 2 * STEP halo into LDS (in-image entries only; the taps
// never leave the image), then every thread reads its taps from there.  Same arithmetic, same order.
constexpr int kDnTileX = 32, kDnTileY = 16;
template <int STEP>
constexpr size_t dn_tile_bytes() {
    return sizeof(double) * kDnPlanes * (kDnTileX + 4 * STEP) * (kDnTileY + 4 * STEP);
}
template <int STEP>
__global__ __launch_bounds__(kDnTileX* kDnTileY) void k_dn_atrous_lds(int W, int H, const double* __restrict__ Lin, const double* __restrict__ Vin,
                                                                      const double* __restrict__ G, double* __restrict__ Lout,
                                                                      double* __restrict__ Vout, double sc2, double sp2, int squarings) {
    constexpr int R = 2 * STEP, TW = kDnTileX + 2 * R, TH = kDnTileY + 2 * R;
    extern __shared__ __align__(16) double dn_tile[];
    const int x0 = static_cast<int>(blockIdx.x) * kDnTileX - R, y0 = static_cast<int>(blockIdx.y) * kDnTileY - R;
    const size_t n = static_cast<size_t>(W) * static_cast<size_t>(H);
    const int tid = static_cast<int>(threadIdx.y) * kDnTileX + static_cast<int>(threadIdx.x);
    for (int e = tid; e < TW * TH; e += kDnTileX * kDnTileY) {
        const int ty = e / TW, tx = e - ty * TW;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx < 0 || gx >= W || gy < 0 || gy >= H) continue;
        const size_t q = static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx);
#pragma unroll
        for (int c = 0; c < 3; ++c) dn_tile[c * (TW * TH) + e] = Lin[static_cast<size_t>(c) * n + q];
        dn_tile[PL_V * (TW * TH) + e] = Vin[q];
#pragma unroll
        for (int k = 0; k < 7; ++k) dn_tile[(PL_NX + k) * (TW * TH) + e] = G[static_cast<size_t>(k) * n + q];
    }
    __syncthreads();
    const int x = static_cast<int>(blockIdx.x) * kDnTileX + static_cast<int>(threadIdx.x);
    const int y = static_cast<int>(blockIdx.y) * kDnTileY + static_cast<int>(threadIdx.y);
    if (x >= W || y >= H) return;
    const DnLdsSrc<TW, TH> src{dn_tile, x0, y0};
    double o[4];
    dn_atrous_pixel<STEP>(src, x, y, W, H, sc2, sp2, squarings, o);
    const size_t p = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
    Lout[p] = o[0];
    Lout[n + p] = o[1];
    Lout[2 * n + p] = o[2];
    Vout[p] = o[3];
}

// out = L * A (remodulation) and, when rgb is non-NULL, write_color of it: k_finalize's arithmetic with spp = 1
// (color.h:6-22: sqrt, clamp to [0, 0.999], 256 * x truncated).
__global__ void k_dn_finish(uint32_t n, const double* __restrict__ L, const double* __restrict__ guides, double floor_a, int demod,
                            double* __restrict__ out, uint8_t* __restrict__ rgb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double scale = 1.0 / 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double A = demod ? dn_max(guides[kGuide * static_cast<size_t>(i) + c], floor_a) : 1.0;
        const double v = L[static_cast<size_t>(c) * n + i] * A;
        out[3 * static_cast<size_t>(i) + c] = v;
        if (rgb) {
            double x = sqrt(scale * v);
            x = x < 0.0 ? 0.0 : (x > 0.999 ? 0.999 : x);
            rgb[3 * static_cast<size_t>(i) + c] = static_cast<uint8_t>(256 * x);
        }
    }
}

using AtrousFn = void (*)(int, int, const double*, const double*, const double*, double*, double*, double, double, int);
AtrousFn atrous_kernel(int s) {  // iteration s: tap spacing 2^s (rt_denoise refuses more than 8 iterations)
    switch (s) {
        case 0: return k_dn_atrous<1>;
        case 1: return k_dn_atrous<2>;
        case 2: return k_dn_atrous<4>;
        case 3: return k_dn_atrous<8>;
        case 4: return k_dn_atrous<16>;
        case 5: return k_dn_atrous<32>;
        case 6: return k_dn_atrous<64>;
        case 7: return k_dn_atrous<128>;
    }
    throw std::runtime_error("internal: a-trous iteration out of range");
}

// A kernel's dynamic LDS above 64 KiB needs the attribute, recorded per device (set once per kernel and device).
void dn_allow_lds(const void* kernel, size_t lds) {
    if (lds <= 64 * 1024) return;
    static std::mutex mtx;
    static std::map<std::pair<const void*, int>, bool> done;
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mtx);
    bool& d = done[{kernel, dev}];
    if (d) return;
    HIP_OK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    d = true;
}

// Per-device state: the grow-only workspace (workspace.h, with the test.fault_workspace_bytes fault point), a stream and
// two events.  It lives until the process ends.
struct DnDevice {
    std::mutex mtx;  // one denoise call at a time per device
    DeviceBuffer ws{true};
    hipStream_t own_stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
};
DnDevice& dn_device(int device) {
    static std::mutex mtx;
    static std::map<int, std::unique_ptr<DnDevice>>* devs = new std::map<int, std::unique_ptr<DnDevice>>();  // never destroyed
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) throw std::runtime_error("no such HIP device: " + std::to_string(device));
    std::lock_guard<std::mutex> lock(mtx);
    auto& d = (*devs)[device];
    if (!d) d = std::make_unique<DnDevice>();
    return *d;
}

// Workspace layout of a W x H frame over `base`.  The frame part (inputs, result) is used when the caller's buffers are
// host memory and by rt_render_denoised; it comes first, so a reserved frame stays where it is.
struct DnLayout {
    double *a, *b, *g, *out;
    uint8_t* rgb;
    double *L[2], *V[2], *G;  // G: normal, position, t planes
    size_t total;
};
DnLayout dn_layout(void* base, size_t npix, bool frame) {
    Carver c(base);
    DnLayout l{};
    l.a = c.take<double>(3 * npix, frame);
    l.b = c.take<double>(3 * npix, frame);
    l.g = c.take<double>(kGuide * npix, frame);
    l.out = c.take<double>(3 * npix, frame);
    l.rgb = c.take<uint8_t>(3 * npix, frame);
    for (auto& p : l.L) p = c.take<double>(3 * npix);
    for (auto& p : l.V) p = c.take<double>(npix);
    l.G = c.take<double>(7 * npix);
    l.total = c.total();
    return l;
}
// The layout in D's workspace, grown to hold it.
DnLayout dn_workspace(DnDevice& D, size_t npix, bool frame) {
    return dn_layout(D.ws.reserve(dn_layout(nullptr, npix, frame).total), npix, frame);
}

// prepare -> iterations x a-trous (L / V ping-pong) -> finish, on `st`; all pointers are device memory.
void run_filter(DnDevice& D, hipStream_t st, const DenoiseParams& p, const DnLayout& l, const double* d_a, const double* d_b, int spp_each,
                const double* d_g, double* d_out, uint8_t* d_rgb) {
    const uint32_t n = static_cast<uint32_t>(static_cast<size_t>(p.width) * p.height);
    double *const *L = l.L, *const *V = l.V, *G = l.G;
    const int demod = p.demodulate ? 1 : 0;
    for (auto& e : D.ev)
        if (!e) HIP_OK(hipEventCreate(&e));
    HIP_OK(hipEventRecord(D.ev[0], st));
    hipLaunchKernelGGL(k_dn_prepare, dim3((n + 255) / 256), dim3(256), 0, st, n, d_a, d_b, static_cast<double>(spp_each), d_g, p.albedo_floor, demod,
                       L[0], V[0], G);
    const double sc2 = p.sigma_color * p.sigma_color, sp2 = p.sigma_plane * p.sigma_plane;
    // iterations below denoise.lds_iterations (tap spacings 1, 2) run the LDS-tile kernel, the others the direct one
    const int lds_iters = static_cast<int>(opt(Opt::DenoiseLdsIterations));
    const dim3 block(kDnBlockX, kDnBlockY);
    const dim3 grid((p.width + kDnBlockX - 1) / kDnBlockX, (p.height + kDnBlockY - 1) / kDnBlockY);
    const dim3 tblock(kDnTileX, kDnTileY);
    const dim3 tgrid((p.width + kDnTileX - 1) / kDnTileX, (p.height + kDnTileY - 1) / kDnTileY);
    int cur = 0;
    for (int s = 0; s < p.iterations; ++s) {
        if (s < lds_iters && s < 2) {
            const size_t lds = s == 0 ? dn_tile_bytes<1>() : dn_tile_bytes<2>();
            const AtrousFn k = s == 0 ? k_dn_atrous_lds<1> : k_dn_atrous_lds<2>;
            dn_allow_lds(reinterpret_cast<const void*>(k), lds);
            hipLaunchKernelGGL(k, tgrid, tblock, lds, st, p.width, p.height, L[cur], V[cur], G, L[cur ^ 1], V[cur ^ 1], sc2, sp2, p.normal_squarings);
        } else {
            hipLaunchKernelGGL(atrous_kernel(s), grid, block, 0, st, p.width, p.height, L[cur], V[cur], G, L[cur ^ 1], V[cur ^ 1], sc2, sp2,
                               p.normal_squarings);
        }
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_dn_finish, dim3((n + 255) / 256), dim3(256), 0, st, n, L[cur], d_g, p.albedo_floor, demod, d_out, d_rgb);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(D.ev[1], st));
}

hipStream_t dn_stream(DnDevice& D, const DenoiseParams& p) {
    if (p.stream) return static_cast<hipStream_t>(p.stream);
    if (!D.own_stream) HIP_OK(hipStreamCreateWithFlags(&D.own_stream, hipStreamNonBlocking));
    return D.own_stream;
}
void elapsed(DnDevice& D, double* ms) {
    if (!ms) return;
    float f = 0;
    HIP_OK(hipEventElapsedTime(&f, D.ev[0], D.ev[1]));
    *ms = f;
}

}  // namespace

void denoise(int device, const DenoiseParams& p, const double* accum_a, const double* accum_b, int spp_each, const double* guides, double* out_color,
             uint8_t* out_rgb8, bool device_ptrs, double* ms) {
    DnDevice& D = dn_device(device);
    std::lock_guard<std::mutex> lock(D.mtx);
    HIP_OK(hipSetDevice(device));
    hipStream_t st = dn_stream(D, p);
    const size_t npix = static_cast<size_t>(p.width) * p.height;
    const DnLayout l = dn_workspace(D, npix, !device_ptrs);
    if (device_ptrs) {
        run_filter(D, st, p, l, accum_a, accum_b, spp_each, guides, out_color, out_rgb8);
    } else {
        HIP_OK(hipMemcpyAsync(l.a, accum_a, sizeof(double) * 3 * npix, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(l.b, accum_b, sizeof(double) * 3 * npix, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(l.g, guides, sizeof(double) * kGuide * npix, hipMemcpyHostToDevice, st));
        run_filter(D, st, p, l, l.a, l.b, spp_each, l.g, l.out, out_rgb8 ? l.rgb : nullptr);
        HIP_OK(hipMemcpyAsync(out_color, l.out, sizeof(double) * 3 * npix, hipMemcpyDeviceToHost, st));
        if (out_rgb8) HIP_OK(hipMemcpyAsync(out_rgb8, l.rgb, 3 * npix, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    elapsed(D, ms);
}

DenoiseFrame denoise_reserve(int device, int width, int height) {
    DnDevice& D = dn_device(device);
    std::lock_guard<std::mutex> lock(D.mtx);
    HIP_OK(hipSetDevice(device));
    const DnLayout l = dn_workspace(D, static_cast<size_t>(width) * height, true);
    return DenoiseFrame{l.a, l.b, l.g};
}

void denoise_reserved(int device, const DenoiseParams& p, int spp_each, double* out_color, uint8_t* out_rgb8, bool device_ptrs, double* ms) {
    DnDevice& D = dn_device(device);
    std::lock_guard<std::mutex> lock(D.mtx);
    HIP_OK(hipSetDevice(device));
    hipStream_t st = dn_stream(D, p);
    const size_t npix = static_cast<size_t>(p.width) * p.height;
    const DnLayout l = dn_layout(D.ws.data(), npix, true);
    if (D.ws.size() < l.total) throw std::runtime_error("internal: denoise_reserved without denoise_reserve");
    run_filter(D, st, p, l, l.a, l.b, spp_each, l.g, l.out, out_rgb8 ? l.rgb : nullptr);
    const hipMemcpyKind kind = device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (out_color) HIP_OK(hipMemcpyAsync(out_color, l.out, sizeof(double) * 3 * npix, kind, st));
    if (out_rgb8) HIP_OK(hipMemcpyAsync(out_rgb8, l.rgb, 3 * npix, kind, st));
    HIP_OK(hipStreamSynchronize(st));
    elapsed(D, ms);
}

}  // namespace art

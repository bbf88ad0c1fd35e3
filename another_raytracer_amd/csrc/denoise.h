// denoise.h — variance-guided a-trous denoiser (implemented in denoise.hip; no HIP types in this header).
#pragma once
#include <cstddef>
#include <cstdint>

namespace art {

struct DenoiseParams {  // rt_denoise_params with the defaults filled in
    int width = 0, height = 0;
    int iterations = 5;
    int normal_squarings = 6;
    double sigma_color = 1.0, sigma_plane = 0.1, albedo_floor = 0.5;
    bool demodulate = true;
    void* stream = nullptr;  // hipStream_t, or NULL for the device's own denoise stream
};

// rt_denoise: accum_a / accum_b (W*H*3 radiance sums of spp_each samples each) and guides (W*H*10, k_guides' record)
// -> out_color (W*H*3) and, when non-NULL, out_rgb8 (W*H*3, write_color with spp 1).  Host buffers, or device buffers
// on `device` with device_ptrs.  ms (may be NULL): device time of the filter kernels (HIP events).  Blocking.
void denoise(int device, const DenoiseParams& p, const double* accum_a, const double* accum_b, int spp_each, const double* guides,
             double* out_color, uint8_t* out_rgb8, bool device_ptrs, double* ms);

// rt_render_denoised keeps the frame on the device: denoise_reserve grows the device's denoise workspace for a W x H
// frame and returns the input buffers inside it (valid until the next denoise call of another size on that device);
// denoise_reserved filters what the caller rendered into them and copies the result out.
struct DenoiseFrame {
    double* accum_a;
    double* accum_b;
    double* guides;
};
DenoiseFrame denoise_reserve(int device, int width, int height);
void denoise_reserved(int device, const DenoiseParams& p, int spp_each, double* out_color, uint8_t* out_rgb8, bool device_ptrs, double* ms);

}  // namespace art

// noise_target.h — noise-target rendering (rt_render_noise_target): the per-pixel bookkeeping kernels of
// noise_target.hip, launched by Renderer::render_noise_target (renderer.hip).  No HIP types in this header.
#pragma once
#include <cstddef>
#include <cstdint>

namespace art {

struct NoiseParams {  // rt_noise_params with the defaults filled in
    int min_spp = 32, step_spp = 32;  // measured: DESIGN.md §4.6
    bool dilate = false;
    double rel_tol = 0.05, lum_floor = 0.01;
};
struct NoiseResult {
    int rounds = 0;
    int64_t converged_pixels = 0;
    uint64_t samples = 0;
};

// The two ping-pong pixel lists: each is its count word (list[-1], on a 64-word line of its own) and round64(local_pix)
// entries.  One expression for the allocation, the memset and the list pointers.
inline size_t nt_list_stride(size_t local_pix) { return 64 + ((local_pix + 63) & ~static_cast<size_t>(63)); }
inline size_t nt_list_words(size_t local_pix) { return 2 * nt_list_stride(local_pix); }

// `stream` is a hipStream_t; `res` the pass's radiance records (3 f64 per slot), acc / mom / count per local pixel
// (3 f64, {S1, S2}, int32).
// Base pass: the k samples of every local pixel (tile-order slots, sample-major: slot j * npix_pad + qi), added in
// sample order onto acc, S1 and S2.
void nt_accum_base(void* stream, const double* res, uint32_t k, uint32_t npix_pad, uint32_t tiles_x, int W, int rows, double* acc, double* mom);
// Refinement pass: the k samples of every entry of `list` (n entries, entry-major slots: entry * k + j), added in
// sample order onto the listed pixel's acc, S1 and S2.
void nt_accum_list(void* stream, const uint32_t* list, uint32_t n, const double* res, uint32_t k, double* acc, double* mom);
// After a round that left every active pixel at n_done samples: the convergence test of the active pixels (`cur` with n
// entries, or every local pixel when cur is NULL), count[p] = n_done (+ k_next when p stays active), the pixels that
// stay active appended to next (count at next[-1], zeroed by the caller) and the ones the test retired added to
// *converged.  With dilate the test's result goes through the flag plane (1 = active and unconverged) and a pixel
// stays active when any pixel of its 3x3 neighbourhood is flagged.  k_next = 0 (the cap is reached) keeps nothing.
void nt_select(void* stream, const uint32_t* cur, uint32_t n, const double* mom, uint8_t* flag, int W, int rows, int n_done, int k_next, bool dilate,
               double rel_tol, double lum_floor, uint32_t* next, int32_t* count, uint32_t* converged);
// write_color (color.h:6-22) of every pixel's sums with its own sample count.
void nt_finalize(void* stream, const double* acc, const int32_t* count, uint8_t* rgb, uint32_t npix);

}  // namespace art

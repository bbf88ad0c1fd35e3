// pass_plan.h -- the pass arithmetic of the renderer as pure functions (g++ and hipcc; tests/native/pass_plan_check.cpp):
// how many samples a pass holds and how many passes a frame takes, the samples per pass of a pixel list and of a
// noise-target round, and how a pass's path slots are handed out to the persistent kernels' waves.
#pragma once
#include <algorithm>
#include <cstdint>

namespace art {

// Slot ids, FastDiv operands and shard capacities are u32 and exact below 2^31: a pass never holds more slots.
constexpr uint64_t kMaxPassSlots = 1ull << 31;

// Samples per whole-image pass and the passes `spp` samples take.  k is the caller's samples_per_pass, or (0) as many
// as slot_target path slots hold, in both cases at most kMaxPassSlots / npix_pad and at most spp.  Every pass pays
// max_depth bounces of fixed launch / tail cost whatever its size, so on a 288 GB part the 1080p x 1024 spp frame runs
// in 3 passes instead of ~40 (5.6 -> 6.9 Gsamples/s measured).  spread (rt_render): k becomes ceil(spp / npasses), the
// same passes of even size; the noise-target base pass keeps k (npasses is then the passes of its sample cap).
// npix_pad in [1, kMaxPassSlots].
struct PassPlan {
    uint32_t k;
    int npasses;
};
constexpr PassPlan plan_passes(uint64_t slot_target, int samples_per_pass, uint32_t npix_pad, int spp, bool spread) {
    const uint64_t n = static_cast<uint64_t>(std::max(1, spp));
    const uint64_t target = std::min<uint64_t>(slot_target, kMaxPassSlots);
    const uint64_t k_cap = std::max<uint64_t>(1, kMaxPassSlots / npix_pad);
    const uint64_t k64 = samples_per_pass > 0 ? static_cast<uint64_t>(samples_per_pass) : std::max<uint64_t>(1, target / npix_pad);
    uint64_t k = std::min<uint64_t>(std::min<uint64_t>(k64, k_cap), n);
    const uint64_t npasses = (n + k - 1) / k;
    if (spread) k = (n + npasses - 1) / npasses;
    return PassPlan{static_cast<uint32_t>(k), static_cast<int>(npasses)};
}
// A pixel list's slots per sample (the list padded to whole waves) and its samples per pass in a workspace of Pmax slots.
constexpr uint32_t list_pad(uint32_t nlist) { return (nlist + 63u) & ~63u; }
// Words of adaptive mode's four level lists over nsq big squares (at most 4 / 12 / 48 / 80 entries of every square's 144
// pixels), each padded to whole 64-entry batches behind the 64-word line of its count.  More than the frame's pixels
// while a level's padding shows: 2 squares (24 x 12) need 704 words, not 288 + 256.
constexpr uint32_t adaptive_list_words(uint32_t nsq) {
    return 4u * 64u + list_pad(4u * nsq) + list_pad(12u * nsq) + list_pad(48u * nsq) + list_pad(80u * nsq);
}
constexpr uint32_t list_pass_samples(uint32_t spp, uint32_t Pmax, uint32_t nlist) {
    return std::max<uint32_t>(1, std::min<uint32_t>(spp, Pmax / std::max<uint32_t>(list_pad(nlist), 64u)));
}
// Samples per sub-pass of a noise-target round of k_next samples over n_active pixels (1 <= n_active <= Pmax).
constexpr uint32_t round_pass_samples(uint32_t k_next, uint32_t Pmax, uint32_t n_active) { return std::min<uint32_t>(k_next, Pmax / n_active); }

// The split of one planned whole-image pass of k samples into two k_paths launches, head [0, k - tail) and tail
// [k - tail, k), so that the head's radiance records are summed on a second stream while the tail traces (renderer.hip
// trace_samples): k_paths is bound by VALU issue and k_accum by HBM, and run back to back each leaves idle what the
// other needs.  tail == 0: no split.  Both launches write the pass's one record buffer, the tail behind the head's
// head * npix_pad records, so head + tail == k keeps them within the planned k * npix_pad slots.
//   mode      option render.accum_overlap: 0 never, 1 auto, 2 whenever k >= 2 (tests, A/B)
//   eligible  the pass is k_paths' (EXT_MEGA), whole-image and sample-major (no pixel list), with no progressive callback
//             between passes and no parallel_images quarter sums; auto also wants the pass size planned by the library
//             (samples_per_pass 0): a caller who sets it gets exactly the launches asked for
// Measured on the benchmark frame (1920x1080x1024, profiles/accum_overlap_kernel_trace.txt, accum_overlap_ab_bench.txt):
// beside a resident k_paths block a SIMD holds one k_accum wave (18 VGPRs next to 4 x 120), and with one record in
// flight per wave the head's 45 GB are summed in 21 to 24.5 ms (about 2 TB/s) instead of 7.3 ms alone.  The tail has to
// last that long to hide them: 96 samples (22 ms at the frame's 0.23 ms per sample) cover it in some runs and not in
// others (one round of five 1 % slower), 128 always did; 64 gains half as much, 32 nothing, 16 is slower than no split.
// The tail's own sums stay exposed (1.1 ms there).  A split costs the tail's trace about 2.7 ms on that frame: one more
// launch boundary of the persistent kernel (0.55 ms, profiles/r6j_ab_fused_accum.txt) and about 0.28 ms per ms of sums
// hidden.  So a head whose sums take T ms alone gains about 0.72 T - 0.55 ms; auto splits from kAccumOverlapMinBytes =
// 8 GiB of head records on (T = 1.4 ms, twice the break-even), which at 1920x1080 is a pass of 301 samples or more
// (measured with a tail of 96: +0.9 % at 320 spp, +0.6 % at 272).
constexpr uint32_t kAccumOverlapTail = 128;
constexpr uint64_t kAccumOverlapMinBytes = 8ull << 30;
constexpr uint64_t kResRecBytes = 24;  // sizeof(ResRec), path_work.h
struct PassSplit {
    uint32_t head, tail;
};
constexpr PassSplit split_pass(uint32_t k, uint32_t npix_pad, int mode, bool eligible) {
    if (!eligible || mode <= 0 || k < 2) return PassSplit{k, 0};
    const uint32_t tail = std::max<uint32_t>(1, std::min<uint32_t>(kAccumOverlapTail, k / 2));
    const uint32_t head = k - tail;
    if (mode == 1 && static_cast<uint64_t>(head) * npix_pad * kResRecBytes < kAccumOverlapMinBytes) return PassSplit{k, 0};
    return PassSplit{head, tail};
}
// The head's sums run as launches of at most this many samples each, one after the other on the second stream: many
// short workgroups instead of one thread per pixel that lives for the whole head.  A k_paths block needs a whole CU's
// LDS and 480 of a SIMD's 512 registers, so a CU that holds two k_accum waves on one SIMD is shut to the tail's blocks
// until they drain.  Every launch re-reads and re-writes the pixel sums, 48 B per pixel against 24 B per sample and
// pixel.  One launch for the whole head was 0.8 ms slower on the benchmark frame; 32, 64 and 128 were equal.
constexpr uint32_t kAccumLaunchSamples = 128;

// The chunk (PassGeom::chunk, path_chunk on the host) is a power of two in [64, 2048], at most the pass's slots / 64
// claims per wave of a full CU.  The counter is one word every wave of the chip claims from: at 256 slots per claim
// k_paths took ~67 M claims/s, and each claim stalls its wave for the device-scope atomic's round trip.  Against 256
// (r4r_ab_path_chunk.txt): C2 +2.9 %, cow +3.2 %, the final +1.2 %, dino +1.2 %.  Larger chunks leave longer tails at
// the end of a pass: at 0.27-0.54 G slots per pass k_paths_g was fastest at 1024 (2048: -1 to -2.6 %, 4096: -3 to
// -8 %), at the configs' 1.1-1.7 G at 2048 (cow +0.9 % over 1024, the final +-0); k_paths (C2, 2.1 G) +-0 from 2048
// to 4096.  Claiming the next chunk one chunk ahead lost 1.5-2 % (its return is waited for at the loop's next vmcnt
// wait).  Small passes (pixel lists, small frames) keep at least 64 claims per wave.
constexpr uint32_t path_chunk(uint32_t P, int num_cu) {
    const uint64_t per = static_cast<uint64_t>(P) / (static_cast<uint64_t>(num_cu > 0 ? num_cu : 1) * 16u * 64u);
    uint32_t c = 64;
    while (c < 2048u && 2ull * c <= per) c *= 2;
    return c;
}

}  // namespace art

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
constexpr uint32_t list_pass_samples(uint32_t spp, uint32_t Pmax, uint32_t nlist) {
    return std::max<uint32_t>(1, std::min<uint32_t>(spp, Pmax / std::max<uint32_t>(list_pad(nlist), 64u)));
}
// Samples per sub-pass of a noise-target round of k_next samples over n_active pixels (1 <= n_active <= Pmax).
constexpr uint32_t round_pass_samples(uint32_t k_next, uint32_t Pmax, uint32_t n_active) { return std::min<uint32_t>(k_next, Pmax / n_active); }

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

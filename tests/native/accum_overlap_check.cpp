// pass_plan.h's split_pass (option render.accum_overlap): the split of one planned whole-image k_paths pass of k samples
// into a head and a tail launch.  Checks head + tail == k and tail >= 1 wherever it splits, "no split" for k = 1, for
// mode 0, for passes that are not eligible (pixel lists, callbacks, quarter sums, other kernels) and below the auto
// threshold, the threshold at its boundary, mode 2 at k = 2, and that the tail's records end within the planned pass.
// Prints "ok" or the first failure.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "pass_plan.h"

using art::PassSplit;
using art::split_pass;

static int fail(const char* what, uint32_t k, uint32_t npix_pad, int mode, bool eligible, PassSplit s) {
    std::printf("FAIL %s k=%u npix_pad=%u mode=%d eligible=%d -> head=%u tail=%u\n", what, k, npix_pad, mode, eligible ? 1 : 0, s.head, s.tail);
    return 1;
}
static bool unsplit(PassSplit s, uint32_t k) { return s.tail == 0 && s.head == k; }

int main() {
    static_assert(art::kResRecBytes == 24, "a radiance record is three doubles");
    static_assert(art::kAccumOverlapTail >= 1 && art::kAccumLaunchSamples >= 1, "tail and launch sizes");
    static_assert(split_pass(2, 64, 2, true).head == 1 && split_pass(2, 64, 2, true).tail == 1, "usable in constant expressions");
    const uint32_t hd = 240u * 135u * 64u;  // 1920x1080 in 8x8 tiles
    const uint32_t tail = art::kAccumOverlapTail;

    // mode 2 splits at k = 2 and nothing splits k = 1
    for (uint32_t npix_pad : {64u, 3072u, hd, 1u << 30}) {
        const PassSplit s2 = split_pass(2, npix_pad, 2, true);
        if (s2.head != 1 || s2.tail != 1) return fail("mode 2 at k = 2", 2, npix_pad, 2, true, s2);
        for (int mode : {0, 1, 2})
            if (!unsplit(split_pass(1, npix_pad, mode, true), 1)) return fail("k = 1 splits", 1, npix_pad, mode, true, split_pass(1, npix_pad, mode, true));
    }
    // the frame of the new GPU tests and the existing small-frame tests: auto leaves them alone, mode 2 splits them
    if (!unsplit(split_pass(24, 9u * 5u * 64u, 1, true), 24)) return fail("auto splits a small frame", 24, 2880, 1, true, split_pass(24, 2880, 1, true));
    {
        const PassSplit s = split_pass(24, 9u * 5u * 64u, 2, true);
        if (s.head + s.tail != 24 || s.tail != (tail < 12 ? tail : 12)) return fail("mode 2 on 72x40x24", 24, 2880, 2, true, s);
    }
    // the benchmark frame: 1024 samples of 1920x1080 are 51 GB of records, auto splits the configured tail off
    {
        const PassSplit s = split_pass(1024, hd, 1, true);
        if (s.tail != (tail < 512 ? tail : 512) || s.head + s.tail != 1024) return fail("auto on the benchmark frame", 1024, hd, 1, true, s);
    }
    // the auto threshold at its boundary: the smallest k whose head holds kAccumOverlapMinBytes splits, k - 1 does not
    for (uint32_t npix_pad : {hd, 4096u * 4096u, 1u << 22}) {
        const uint64_t per_sample = static_cast<uint64_t>(npix_pad) * art::kResRecBytes;
        const uint64_t head_min = (art::kAccumOverlapMinBytes + per_sample - 1) / per_sample;  // samples of the smallest head that splits
        // head = k - min(tail, k / 2): the smallest k with head >= head_min
        uint32_t k = 2;
        while (k - (tail < k / 2 ? tail : k / 2) < head_min) ++k;
        if (static_cast<uint64_t>(k) * npix_pad > art::kMaxPassSlots) continue;  // such a pass does not exist
        const PassSplit at = split_pass(k, npix_pad, 1, true), below = split_pass(k - 1, npix_pad, 1, true);
        if (at.tail == 0 || static_cast<uint64_t>(at.head) * per_sample < art::kAccumOverlapMinBytes) return fail("threshold: at", k, npix_pad, 1, true, at);
        if (!unsplit(below, k - 1)) return fail("threshold: below", k - 1, npix_pad, 1, true, below);
    }
    // the invariants over a sweep
    for (uint32_t npix_pad : {64u, 2880u, 3072u, hd, 4096u * 4096u, 1u << 30, uint32_t(art::kMaxPassSlots)})
        for (uint32_t k : {1u, 2u, 3u, 4u, 5u, 10u, 24u, 63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 700u, 1024u, 1035u, 8192u}) {
            if (static_cast<uint64_t>(k) * npix_pad > art::kMaxPassSlots) continue;  // plan_passes never plans it
            const uint64_t Pmax = static_cast<uint64_t>(k) * npix_pad;
            for (int mode : {0, 1, 2})
                for (bool eligible : {false, true}) {
                    const PassSplit s = split_pass(k, npix_pad, mode, eligible);
                    if (s.head + s.tail != k) return fail("head + tail != k", k, npix_pad, mode, eligible, s);
                    if ((mode == 0 || !eligible || k == 1) && !unsplit(s, k)) return fail("split where none may be", k, npix_pad, mode, eligible, s);
                    if (mode == 2 && eligible && k >= 2 && s.tail == 0) return fail("mode 2 did not split", k, npix_pad, mode, eligible, s);
                    if (s.tail == 0) continue;
                    if (s.head < 1 || s.tail > s.head) return fail("tail larger than head", k, npix_pad, mode, eligible, s);
                    if (mode == 1 && static_cast<uint64_t>(s.head) * npix_pad * art::kResRecBytes < art::kAccumOverlapMinBytes)
                        return fail("auto split below the threshold", k, npix_pad, mode, eligible, s);
                    // the tail's records start at head * npix_pad and hold tail * npix_pad slots
                    if (static_cast<uint64_t>(s.head) * npix_pad + static_cast<uint64_t>(s.tail) * npix_pad > Pmax)
                        return fail("tail beyond the planned pass", k, npix_pad, mode, eligible, s);
                }
        }
    std::printf("ok\n");
    return 0;
}

// pass_plan.h's path_chunk (the slots a persistent kernel's wave claims per atomic): the values at the BASELINE
// configs' pass sizes, and its invariants over a sweep of pass sizes and CU counts.  Then (alone with the argument
// "plan") the pass arithmetic: plan_passes, list_pass_samples and round_pass_samples at the cases worked out from the
// renderer's rules, and plan_passes' invariants over a sweep.  Prints "ok" or the first failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "pass_plan.h"

static int fail(const char* what, uint64_t P, int cu, uint32_t c) {
    std::printf("FAIL %s P=%llu cu=%d chunk=%u\n", what, static_cast<unsigned long long>(P), cu, c);
    return 1;
}

static int fail_plan(const char* what, uint64_t target, int spass, uint32_t npix_pad, int spp, bool spread, art::PassPlan got) {
    std::printf("FAIL %s target=%llu samples_per_pass=%d npix_pad=%u spp=%d spread=%d -> k=%u npasses=%d\n", what,
                static_cast<unsigned long long>(target), spass, npix_pad, spp, spread ? 1 : 0, got.k, got.npasses);
    return 1;
}

static int check_plan() {
    const uint32_t hd = 240u * 135u * 64u;  // 1920x1080 in 8x8 tiles: 2 073 600 padded pixels
    const uint64_t big = 1ull << 40;        // a slot target no clamp but kMaxPassSlots stops
    struct Case { uint64_t target; int spass; uint32_t npix_pad; int spp; bool spread; uint32_t k; int npasses; } cases[] = {
        {big, 2100, hd, 2100, true, 700, 3},      // clamp to 2^31 / 2 073 600 = 1035, 3 passes, spread evenly
        {big, 2100, hd, 2100, false, 1035, 3},    // the noise-target base plan: the same clamp, no spread
        {big, 0, hd, 2100, true, 700, 3},         // the slot target is clamped to 2^31 as well
        {hd - 1, 0, hd, 16, true, 1, 16},         // a slot target below one sample of the frame
        {0, 0, hd, 16, true, 1, 16},
        {big, 0, hd, 0, true, 1, 1}, {big, 0, hd, 1, true, 1, 1}, {big, 5, hd, 0, true, 1, 1}, {big, 5, hd, 1, false, 1, 1},
        {big, 64, 3072, 16, true, 16, 1},         // samples_per_pass above spp: one pass of spp
        {big, 64, 3072, 16, false, 16, 1},
        {10ull * 3072, 0, 3072, 25, true, 9, 3},  // 10 per pass from memory: 3 passes, spread to 9 + 9 + 7
        {10ull * 3072, 0, 3072, 25, false, 10, 3},
        {big, 2, 3072, 4, true, 2, 2},
        {big, 1, uint32_t(art::kMaxPassSlots), 3, true, 1, 3},  // the largest frame: one sample per pass
    };
    for (const Case& c : cases) {
        const art::PassPlan got = art::plan_passes(c.target, c.spass, c.npix_pad, c.spp, c.spread);
        if (got.k != c.k || got.npasses != c.npasses) return fail_plan("plan value", c.target, c.spass, c.npix_pad, c.spp, c.spread, got);
    }
    for (uint64_t target : {0ull, 1ull, 1000ull, 1ull << 20, 1ull << 31, 1ull << 40})
        for (int spass : {0, 1, 2, 3, 7, 64, 1035, 1036, 2100, 1 << 30})
            for (uint32_t npix_pad : {64u, 3072u, hd, 1u << 30, uint32_t(art::kMaxPassSlots)})
                for (int spp : {0, 1, 2, 3, 4, 5, 16, 25, 1024, 2100, 100000})
                    for (bool spread : {false, true}) {
                        const art::PassPlan got = art::plan_passes(target, spass, npix_pad, spp, spread);
                        const uint64_t n = spp < 1 ? 1 : spp, k = got.k, np = got.npasses;
                        const bool ok = k >= 1 && k * npix_pad <= art::kMaxPassSlots && np >= 1 && np * k >= n && (np - 1) * k < n &&
                                        (spass <= 0 || k <= static_cast<uint64_t>(spass)) && k <= n;
                        if (!ok) return fail_plan("plan invariant", target, spass, npix_pad, spp, spread, got);
                    }
    // pixel lists (sample-major, padded to whole waves)
    struct ListCase { uint32_t spp, Pmax, nlist, want; } lists[] = {
        {16, 4096, 1, 16},      // nlist 1: 64 padded entries, Pmax / 64 = 64 >= spp
        {100, 4096, 1, 64},     //   ... and below spp
        {16, 4096, 64, 16}, {16, 4096, 65, 16}, {100, 4096, 65, 32},
        {16, 4096, 0, 16},      // an empty list still divides by 64
        {16, 4096, 4097, 1},    // padded size 4160 > Pmax
        {16, 4096, 4096, 1}, {16, 8192, 4096, 2},
    };
    for (const ListCase& c : lists) {
        const uint32_t kk = art::list_pass_samples(c.spp, c.Pmax, c.nlist);
        if (kk != c.want) {
            std::printf("FAIL list_pass_samples spp=%u Pmax=%u nlist=%u -> %u (want %u)\n", c.spp, c.Pmax, c.nlist, kk, c.want);
            return 1;
        }
    }
    if (art::list_pad(1) != 64 || art::list_pad(64) != 64 || art::list_pad(65) != 128 || art::list_pad(0) != 0) {
        std::printf("FAIL list_pad\n");
        return 1;
    }
    // adaptive mode's four level lists lie one after another, each behind its count line and padded to whole batches:
    // the words reserved hold that layout for every frame size (2 squares: 704 words, more than 288 pixels + 256)
    for (uint32_t nsq = 1; nsq <= 4096; nsq += (nsq < 64 ? 1 : 61)) {
        uint32_t end = 0;
        for (uint32_t cap : {4u, 12u, 48u, 80u}) end += 64 + art::list_pad(cap * nsq);
        if (art::adaptive_list_words(nsq) != end || end < 144 * nsq + 256) {
            std::printf("FAIL adaptive_list_words nsq=%u -> %u (layout ends at %u)\n", nsq, art::adaptive_list_words(nsq), end);
            return 1;
        }
    }
    if (art::adaptive_list_words(2) != 704 || art::adaptive_list_words(32) != 32 * 144 + 256) {
        std::printf("FAIL adaptive_list_words small frames\n");
        return 1;
    }
    // noise-target rounds (entry-major: no padding)
    struct RoundCase { uint32_t k_next, Pmax, n_active, want; } rounds[] = {
        {32, 4096, 4096, 1},   // n_active = Pmax
        {32, 4096, 128, 32},   // n_active * k_next = Pmax
        {32, 4096, 100, 32},   // ... below it
        {32, 4096, 129, 31}, {32, 4096, 2049, 1}, {4, 3840, 1728, 2}, {1, 4096, 1, 1},
    };
    for (const RoundCase& c : rounds) {
        const uint32_t kk = art::round_pass_samples(c.k_next, c.Pmax, c.n_active);
        if (kk != c.want || kk < 1 || static_cast<uint64_t>(kk) * c.n_active > c.Pmax) {
            std::printf("FAIL round_pass_samples k_next=%u Pmax=%u n_active=%u -> %u (want %u)\n", c.k_next, c.Pmax, c.n_active, kk, c.want);
            return 1;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "plan") == 0) {
        if (check_plan()) return 1;
        std::printf("ok\n");
        return 0;
    }
    // configs at 256 CUs: C2 1920x1080 (2 073 600 padded pixels) x 1024 spp in one pass, C3 x 512, C4/C5 passes of
    // ~1-2 G slots, and the 0.54 G pass of a 256-spp frame (1024: smaller chunks won at that size)
    struct Case { uint64_t P; uint32_t want; } cases[] = {
        {2073600ull * 1024, 2048}, {2073600ull * 512, 2048}, {2073600ull * 256, 1024}, {16777216ull * 128, 2048},
        {320ull * 192 * 4, 64}, {0, 64}, {1, 64}};
    for (const Case& k : cases) {
        const uint32_t c = art::path_chunk(static_cast<uint32_t>(k.P), 256);
        if (c != k.want) return fail("config value", k.P, 256, c);
    }
    for (int cu : {1, 8, 64, 256, 304}) {
        uint32_t prev = 0;
        for (uint64_t P = 1; P < (1ull << 31); P = P * 3 / 2 + 1) {
            const uint32_t c = art::path_chunk(static_cast<uint32_t>(P), cu);
            if (c < 64 || c > 2048 || (c & (c - 1)) != 0) return fail("power of two in [64, 2048]", P, cu, c);
            if (c < prev) return fail("monotone in P", P, cu, c);
            if (c > 64 && static_cast<uint64_t>(c) * cu * 16u * 64u > P) return fail("at least 64 claims per wave", P, cu, c);
            prev = c;
        }
    }
    std::printf("ok\n");
    return 0;
}

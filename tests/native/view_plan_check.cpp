// view_plan.h's plan_views (how rt_render_views cuts its views into launches): the cases worked out from its rules, then
// its invariants over a sweep -- groups are whole views, in order, and cover every view once; a group's paths stay within
// kMaxPassSlots, the workspace budget and views.max_paths wherever those hold one view; a single view above
// kMaxPassSlots is refused.  Prints "ok" or the first failure.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "view_plan.h"

using art::kMaxPassSlots;
using art::ViewPlan;

static int fail(const char* what, uint64_t nviews, uint64_t view_paths, uint64_t budget, uint64_t max_paths, bool ok, ViewPlan got) {
    std::printf("FAIL %s nviews=%llu view_paths=%llu budget=%llu max_paths=%llu -> ok=%d per_group=%u ngroups=%u\n", what,
                static_cast<unsigned long long>(nviews), static_cast<unsigned long long>(view_paths), static_cast<unsigned long long>(budget),
                static_cast<unsigned long long>(max_paths), ok ? 1 : 0, got.per_group, got.ngroups);
    return 1;
}

int main() {
    using u64 = unsigned long long;     // the literals' type, so that the sweeps' lists hold one type
    const u64 big = 1ull << 40;         // a budget no cap but kMaxPassSlots stops
    const u64 small = 40ull * 24 * 4;   // 3840 paths: the GPU tests' view
    const u64 tile = 128ull * 128 * 16;  // 262 144 paths: one full persistent grid
    const u64 hd = 1920ull * 1080 * 16;  // 33 177 600 paths
    struct Case { uint64_t nviews, view_paths, budget, max_paths; bool ok; uint32_t per_group, ngroups; } cases[] = {
        {5, small, big, 0, true, 5, 1},                 // everything in one launch
        {5, small, big, 2 * small, true, 2, 3},         // two views a launch: 2 + 2 + 1
        {5, small, big, 2 * small + small - 1, true, 2, 3},  // a cap between two and three views
        {5, small, big, 4 * small, true, 3, 2},         // 4 would fit: 2 launches, evened out to 3 + 2
        {5, small, big, small, true, 1, 5},             // a cap of exactly one view
        {5, small, big, small - 1, true, 1, 5},         // a cap below one view: still one view a launch
        {5, small, big, 1, true, 1, 5},
        {5, small, 0, 0, true, 1, 5},                   // no memory at all: one view a launch (the allocation then decides)
        {5, small, 3 * small, 0, true, 3, 2},           // the budget cuts as the option does
        {5, small, 3 * small, 2 * small, true, 2, 3},   // the smaller cap wins
        {1, small, big, 0, true, 1, 1},                 // V = 1
        {1, small, big, 1, true, 1, 1},
        {1, kMaxPassSlots, big, 0, true, 1, 1},         // the largest view
        {3, kMaxPassSlots, big, 0, true, 1, 3},
        {1, kMaxPassSlots + 1, big, 0, false, 0, 0},    // a single view above kMaxPassSlots
        {64, kMaxPassSlots + 1, big, 0, false, 0, 0},
        {64, tile, big, 0, true, 64, 1},                // the measured small shape: 16.8 M paths
        {4, hd, big, 0, true, 4, 1},                    // the measured large shape: 132.7 M paths
        {100, hd, big, 0, true, 50, 2},                 // 64 views of 1080p x 16 fit 2^31: 100 run as 50 + 50
        {8192, tile, big, 0, true, 8192, 1},            // 2^31 / 2^18 = 8192 views fit exactly ...
        {8193, tile, big, 0, true, 4097, 2},            // ... one more makes two launches
        {3, (1ull << 31) - 7, big, 0, true, 1, 3},      // npix * spp just below 2^31
        {2, 1ull << 30, big, 0, true, 2, 1},            // two views of 2^30 are exactly 2^31
        {3, 1ull << 30, big, 0, true, 2, 2},
        {0, small, big, 0, false, 0, 0},                // no view, no path: nothing to plan
        {5, 0, big, 0, false, 0, 0},
    };
    for (const Case& c : cases) {
        ViewPlan got{0, 0};
        const bool ok = art::plan_views(c.nviews, c.view_paths, c.budget, c.max_paths, got);
        if (ok != c.ok || got.per_group != c.per_group || got.ngroups != c.ngroups) return fail("plan value", c.nviews, c.view_paths, c.budget, c.max_paths, ok, got);
    }
    for (u64 nviews : {1ull, 2ull, 3ull, 5ull, 6ull, 7ull, 64ull, 100ull, 8191ull, 8192ull, 8193ull, 1ull << 20, (1ull << 31) - 1})
        for (u64 view_paths : {1ull, 63ull, 64ull, small, tile, hd, (1ull << 30) - 1, 1ull << 30, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 1, 1ull << 33})
            for (u64 budget : {0ull, 1ull, small, 3 * small, tile, 1ull << 31, big})
                for (u64 max_paths : {0ull, 1ull, small - 1, small, 2 * small, 5 * small, 1ull << 31}) {
                    ViewPlan got{0, 0};
                    const bool ok = art::plan_views(nviews, view_paths, budget, max_paths, got);
                    if (ok != (view_paths <= kMaxPassSlots)) return fail("refuses exactly a view above kMaxPassSlots", nviews, view_paths, budget, max_paths, ok, got);
                    if (!ok) {
                        if (got.per_group != 0 || got.ngroups != 0) return fail("a refusal leaves the plan untouched", nviews, view_paths, budget, max_paths, ok, got);
                        continue;
                    }
                    const uint64_t per = got.per_group, ng = got.ngroups;
                    // whole views, in order, every view once: full groups and a last one of 1..per views
                    if (per < 1 || ng < 1 || per * ng < nviews || per * (ng - 1) >= nviews) return fail("covers every view once", nviews, view_paths, budget, max_paths, ok, got);
                    const uint64_t paths = per * view_paths;
                    if (paths > kMaxPassSlots) return fail("within kMaxPassSlots", nviews, view_paths, budget, max_paths, ok, got);
                    if (per > 1 && paths > budget) return fail("within the budget", nviews, view_paths, budget, max_paths, ok, got);
                    if (per > 1 && max_paths > 0 && paths > max_paths) return fail("within views.max_paths", nviews, view_paths, budget, max_paths, ok, got);
                    // the fewest launches the caps allow
                    uint64_t cap = budget < kMaxPassSlots ? budget : kMaxPassSlots;
                    if (max_paths > 0 && max_paths < cap) cap = max_paths;
                    uint64_t fit = cap / view_paths;
                    if (fit < 1) fit = 1;
                    if (fit > nviews) fit = nviews;
                    if (ng != (nviews + fit - 1) / fit) return fail("the fewest launches", nviews, view_paths, budget, max_paths, ok, got);
                }
    std::printf("ok\n");
    return 0;
}

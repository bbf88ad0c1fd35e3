// view_plan.h -- how rt_render_views cuts its views into launches, as a pure function (g++ and hipcc;
// tests/native/view_plan_check.cpp).  A launch of the persistent path kernel traces a group of whole, consecutive views:
// path p = (view * npix + pixel) * spp + sample, one ResRec per path in the workspace.
#pragma once
#include <algorithm>
#include <cstdint>

#include "pass_plan.h"

namespace art {

// Group g holds the views [g * per_group, min(nviews, (g + 1) * per_group)): every group but the last is full.
struct ViewPlan {
    uint32_t per_group;  // views per launch
    uint32_t ngroups;    // launches
};

// The groups of nviews >= 1 views of view_paths = W * H * spp paths each.  A group's paths stay within three caps:
// kMaxPassSlots (path indices and FastDiv operands are exact below 2^31), budget_paths (the records the workspace may
// hold) and max_paths (option views.max_paths; 0 = off).  A group is never less than one view: a budget or an option
// below view_paths gives groups of one view, and only kMaxPassSlots refuses -- false when one view alone exceeds it (or
// has no path), and out is untouched.  The fewest groups the caps allow, then evened out (5 views under a cap of 2 run
// as 2 + 2 + 1, 5 under a cap of 4 as 3 + 2), so that no launch is a short tail of its own.
constexpr bool plan_views(uint64_t nviews, uint64_t view_paths, uint64_t budget_paths, uint64_t max_paths, ViewPlan& out) {
    if (nviews == 0 || nviews > 0xFFFFFFFFull || view_paths == 0 || view_paths > kMaxPassSlots) return false;
    uint64_t cap = std::min<uint64_t>(kMaxPassSlots, budget_paths);
    if (max_paths > 0) cap = std::min<uint64_t>(cap, max_paths);
    const uint64_t fit = std::min<uint64_t>(std::max<uint64_t>(1, cap / view_paths), nviews);
    const uint64_t ngroups = (nviews + fit - 1) / fit;
    const uint64_t per = (nviews + ngroups - 1) / ngroups;  // <= fit
    out = ViewPlan{static_cast<uint32_t>(per), static_cast<uint32_t>((nviews + per - 1) / per)};
    return true;
}

}  // namespace art

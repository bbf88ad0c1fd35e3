// call_plan.h: which stream a call on the caller's buffers runs on and whether it waits before it returns -- the full
// truth table of (device buffers, caller's stream non-null, timed) for the two rules, every row's answer stated -- and
// the workspace's slot target.  Prints "ok" or the first failure.
#include <cstdint>
#include <cstdio>

#include "call_plan.h"

using art::CallPlan;

struct Row {
    bool device, stream, timed;
    bool callers_stream, wait;
};

static int check(const char* rule, CallPlan (*plan)(bool, bool, bool), const Row (&rows)[8]) {
    bool seen[8] = {};
    for (const Row& r : rows) {
        const CallPlan got = plan(r.device, r.stream, r.timed);
        if (got.callers_stream != r.callers_stream || got.wait != r.wait) {
            std::printf("FAIL %s device=%d stream=%d timed=%d -> callers_stream=%d wait=%d, expected %d %d\n", rule, r.device, r.stream, r.timed,
                        got.callers_stream, got.wait, r.callers_stream, r.wait);
            return 1;
        }
        // a timed call reads its events, a call on the renderer's own stream cannot be waited for by anybody else
        if ((r.timed || !got.callers_stream) && !got.wait) {
            std::printf("FAIL %s device=%d stream=%d timed=%d returns enqueued\n", rule, r.device, r.stream, r.timed);
            return 1;
        }
        seen[r.device * 4 + r.stream * 2 + r.timed] = true;
    }
    for (bool s : seen)
        if (!s) {
            std::printf("FAIL %s: the table misses a row\n", rule);
            return 1;
        }
    return 0;
}

int main() {
    // rt_query_rays, rt_radiance_rays, rt_render_views, rt_scene_update_triangles, rt_camera_rays, rt_trace_rays
    const Row call[8] = {
        // device stream timed   caller's stream, waits
        {false, false, false, false, true},  // host buffers: staged on the own stream, copied back, waited for
        {false, false, true, false, true},
        {false, true, false, false, true},   // (the ABI passes a handle through with host buffers: it is not used)
        {false, true, true, false, true},
        {true, false, false, false, true},   // the null handle: the own stream, on which nobody else can wait
        {true, false, true, false, true},
        {true, true, false, true, false},    // the one row that returns enqueued
        {true, true, true, true, true},      // stats or the elapsed time: on the caller's stream, and waits
    };
    if (check("plan_call", art::plan_call, call)) return 1;
    // rt_render, rt_render_noise_target, rt_render_guides: the caller's stream whenever given, and always waits
    const Row frame[8] = {
        {false, false, false, false, true},
        {false, false, true, false, true},
        {false, true, false, true, true},    // host buffers on the caller's stream
        {false, true, true, true, true},
        {true, false, false, false, true},
        {true, false, true, false, true},
        {true, true, false, true, true},     // rt_render_guides on a side stream still waits
        {true, true, true, true, true},
    };
    if (check("plan_frame_call", art::plan_frame_call, frame)) return 1;

    // the slot target: half of (free + owned), in whole slots
    struct Slots { uint64_t free, owned, slot_bytes, expect; } slots[] = {
        {0, 0, 24, 0},
        {47, 0, 24, 0},                      // half of 47 bytes holds no 24-byte slot ...
        {48, 0, 24, 1},                      // ... half of 48 holds one
        {24, 24, 24, 1},                     // the owned workspace counts as free: a fixed point
        {1000, 0, 24, 20},
        {0, 1000, 24, 20},
        {600, 400, 24, 20},
        {288ull << 30, 0, 24, (288ull << 30) / 48},                 // an empty 288 GB part, a persistent kernel's ResRec
        {(288ull << 30) - (64ull << 30), 64ull << 30, 24, (288ull << 30) / 48},  // the same after it owns 64 GB
        {~0ull / 2, ~0ull / 2, 1, ~0ull / 2},                       // no overflow below 2^64 bytes in all
    };
    for (const Slots& s : slots)
        if (art::slot_target(s.free, s.owned, s.slot_bytes) != s.expect) {
            std::printf("FAIL slot_target free=%llu owned=%llu slot_bytes=%llu -> %llu, expected %llu\n", static_cast<unsigned long long>(s.free),
                        static_cast<unsigned long long>(s.owned), static_cast<unsigned long long>(s.slot_bytes),
                        static_cast<unsigned long long>(art::slot_target(s.free, s.owned, s.slot_bytes)), static_cast<unsigned long long>(s.expect));
            return 1;
        }
    std::printf("ok\n");
    return 0;
}

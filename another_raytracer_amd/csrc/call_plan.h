// call_plan.h -- the decisions of a call on the caller's own buffers as pure functions (g++ and hipcc;
// tests/native/call_plan_check.cpp): which stream the call runs on, whether it waits before it returns, and how many
// slots the workspace is planned for.  renderer.hip's Call is the only reader.
#pragma once
#include <cstdint>

namespace art {

// The caller's stream or the renderer's own, and whether the call returns only after the stream has drained.  A call
// that does not wait returns enqueued: its workspace parts are still in use, so the next call on the scene has to be
// ordered after it on the same stream.
struct CallPlan {
    bool callers_stream;
    bool wait;
};

// rt_query_rays, rt_radiance_rays, rt_render_views, rt_scene_update_triangles, rt_camera_rays (and rt_trace_rays, which
// is always the host row).  device: the buffers are device pointers (RT_OUT_DEVICE); stream: the caller's handle is
// non-null; timed: the stats or the elapsed time are asked for (never, for rt_query_rays and rt_camera_rays).  Host
// buffers go through the workspace on the renderer's own stream, whatever handle was passed.  A device call on the
// caller's stream without timing returns enqueued; every other waits: the host copies must have landed, nobody else
// can wait on the renderer's own stream, and the elapsed time is read from the events.
constexpr CallPlan plan_call(bool device, bool stream, bool timed) { return CallPlan{device && stream, !device || !stream || timed}; }

// rt_render, rt_render_noise_target, rt_render_guides: the caller's stream whenever one is given, host buffers included,
// and the call always waits (the frame calls always fill their stats; rt_render_guides has none and waits all the same).
constexpr CallPlan plan_frame_call(bool /*device*/, bool stream, bool /*timed*/) { return CallPlan{stream, true}; }

// The slot target of a workspace: what half of the free HBM holds, counting the workspace the renderer already owns as
// free -- a fixed point: a second call of the same size plans the same slots and regrows nothing.
constexpr uint64_t slot_target(uint64_t free, uint64_t owned, uint64_t slot_bytes) { return (free + owned) / 2 / slot_bytes; }

}  // namespace art

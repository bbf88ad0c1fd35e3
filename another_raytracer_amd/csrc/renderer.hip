// renderer.hip — Renderer (renderer.h): the workspace, the pass loops of rt_render and rt_render_noise_target, ray
// queries, radiance along caller-given rays, many views of a scene in one launch, camera rays and guide buffers.  Host
// code only: every kernel is launched through launch.h / noise_target.h.
//
// The workspace is one grow-only DeviceBuffer that every entry point carves (workspace.h); a Call is the protocol of one
// entry point on the caller's buffers: stream, staging, timing and the wait (call_plan.h).  rt_render and
// rt_render_noise_target share a Frame: begin_frame sets it up (geometry, variant, the samples per pass of pass_plan.h,
// workspace, events) and opens the timed region, run_pass runs one pass and keeps the pass, launch and RT_PROFILE
// accounts, end_frame closes the region, copies the frame out and fills the stats.  rt_render's three modes and the
// noise-target rounds are loops of run_pass.
#include "renderer.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "call_plan.h"
#include "launch.h"
#include "lds_image.h"
#include "options.h"
#include "pass_plan.h"
#include "refit.h"
#include "tile_lists.h"
#include "view_plan.h"
#include "workspace.h"

namespace art {

struct Renderer::Impl {
    int device = 0;
    int num_cu = 256;
    hipStream_t own_stream = nullptr;
    FlatScene flat;
    DeviceScene s64;
    bool up64 = false;
    DeviceBuffer ws{true};  // the workspace, with the test.fault_workspace_bytes fault point
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<ViewRec> view_table;  // rt_render_views: the camera table of the last call, as uploaded
    uint64_t gen = 0, fetched_gen = 0;  // rt_scene_update_* calls so far / the one `flat` was last fetched after
    uint64_t texel_gen = 0, fetched_texel_gen = 0;  // rt_scene_update_texels calls likewise (the texel pool is fetched only after one)
    const uint32_t* image_row = nullptr;  // rt_radiance_grad_texels: TexelJob::image_row on the device, made by the first such call
    // The second stream of a split pass (pass_plan.h split_pass) and its events: fork[0] the head's k_paths launch has
    // ended, fork[1] the head's sums are in.  Created by the first split.  The stream has the lowest priority, so that
    // of two dispatches that become ready together -- the tail's k_paths and the head's k_accum -- the path kernel's
    // blocks are placed first.
    hipStream_t accum_stream = nullptr;
    hipEvent_t fork[2] = {nullptr, nullptr};

    void need_accum_stream() {
        if (!accum_stream) {
            int least = 0, greatest = 0;
            HIP_OK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIP_OK(hipStreamCreateWithPriority(&accum_stream, hipStreamNonBlocking, least));
        }
        for (auto& e : fork)
            if (!e) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    ~Impl() {
        s64.release();
        ws.release();
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        for (auto& e : fork) if (e) (void)hipEventDestroy(e);
        if (accum_stream) (void)hipStreamDestroy(accum_stream);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

// A split pass between its fork and its join.  join() orders the frame's stream after the second stream's work; an exit
// that never reaches it (a thrown HIP_OK) waits on the host instead, so the workspace is never handed to the next call
// while the second stream still reads it.
struct AccumFork {
    Renderer::Impl& I;
    bool open = false;
    explicit AccumFork(Renderer::Impl& I) : I(I) {}
    AccumFork(const AccumFork&) = delete;
    AccumFork& operator=(const AccumFork&) = delete;
    ~AccumFork() {
        if (open) (void)hipStreamSynchronize(I.accum_stream);
    }
    // after `from`'s work so far, the second stream may run
    void fork(hipStream_t from) {
        I.need_accum_stream();
        HIP_OK(hipEventRecord(I.fork[0], from));
        open = true;  // (before the wait: from here on the second stream may hold work)
        HIP_OK(hipStreamWaitEvent(I.accum_stream, I.fork[0], 0));
    }
    void join(hipStream_t into) {
        HIP_OK(hipEventRecord(I.fork[1], I.accum_stream));
        HIP_OK(hipStreamWaitEvent(into, I.fork[1], 0));
        open = false;
    }
};

Renderer::Renderer(FlatScene flat, int device) : impl_(new Impl) {
    impl_->device = device;
    HIP_OK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    impl_->num_cu = prop.multiProcessorCount;
    impl_->flat = std::move(flat);
    HIP_OK(hipStreamCreateWithFlags(&impl_->own_stream, hipStreamNonBlocking));
}
Renderer::~Renderer() {
    if (impl_) {
        (void)hipSetDevice(impl_->device);
        delete impl_;
    }
}

// One call's host protocol, in the order every entry point enqueues it: the stream (call_plan.h), the workspace layout
// with the copies in, [the caller's memsets,] begin(), [the launches,] end() with the copies out, finish() with the wait.
// `rule` is plan_call or plan_frame_call; own / ev are the renderer's stream and Impl::ev (rt_camera_rays, which has no
// renderer: the null stream and no events).
struct Call {
    bool device = false, timed = false, wait = true, sizing = false;
    hipStream_t st = nullptr;
    hipEvent_t* ev = nullptr;
    struct Copy { void* dst; const void* src; size_t bytes; } outs[6];
    int nouts = 0;

    Call() = default;
    Call(hipStream_t own, hipEvent_t* ev, bool device, void* stream, bool timed, CallPlan (*rule)(bool, bool, bool) = plan_call)
        : device(device), timed(timed), ev(ev) {
        const CallPlan plan = rule(device, stream != nullptr, timed);
        st = plan.callers_stream ? static_cast<hipStream_t>(stream) : own;
        wait = plan.wait;
    }
    // Lays `buf` out: layout(Carver&) runs twice, over a null base for the size and over the allocation for the pointers.
    template <class Layout>
    void carve(DeviceBuffer& buf, Layout&& layout, size_t align = 256) {
        Carver size(nullptr, align);
        sizing = true, layout(size);
        Carver parts(buf.reserve(size.total()), align);
        sizing = false, nouts = 0, layout(parts);
    }
    // Within a layout, the device pointer of a caller's input / of a result: the caller's as it is (null stays null), or a
    // part of the workspace -- an input is copied there now, a result is copied out by end().
    template <class T>
    const T* in(Carver& c, const T* src, size_t count) {
        T* staged = c.take<T>(count, !device && src);
        if (device || !src) return src;
        if (!sizing) HIP_OK(hipMemcpyAsync(staged, src, sizeof(T) * count, hipMemcpyHostToDevice, st));
        return staged;
    }
    template <class T>
    T* out(Carver& c, T* dst, size_t count) {
        T* staged = c.take<T>(count, !device && dst);
        if (device || !dst) return dst;
        outs[nouts++] = Copy{dst, staged, sizeof(T) * count};
        return staged;
    }
    // A result that always leaves the workspace: to the caller's device or host buffer (null: not asked for).
    void copy_out(void* dst, const void* src, size_t bytes) {
        if (dst) HIP_OK(hipMemcpyAsync(dst, src, bytes, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    }
    // The timed region (Impl::ev, created on the first timed call).
    void begin() {
        for (int i = 0; timed && i < 2; ++i)
            if (!ev[i]) HIP_OK(hipEventCreate(&ev[i]));
        if (timed) HIP_OK(hipEventRecord(ev[0], st));
    }
    void end() {
        HIP_OK(hipGetLastError());
        if (timed) HIP_OK(hipEventRecord(ev[1], st));
        for (int i = 0; i < nouts; ++i) HIP_OK(hipMemcpyAsync(outs[i].dst, outs[i].src, outs[i].bytes, hipMemcpyDeviceToHost, st));
    }
    // The wait rule; a timed call (which always waits) gets the elapsed time and the segment count at d_segments.
    struct Done {
        float ms = 0;
        unsigned long long segments = 0;
        void fill(RenderStats* s, uint64_t primary, int passes, int samples_per_pass) const {
            if (s) *s = RenderStats{}, s->segments = segments, s->primary = primary, s->ms = ms, s->passes = passes, s->samples_per_pass = samples_per_pass;
        }
    };
    Done finish(const unsigned long long* d_segments = nullptr) {
        Done d;
        if (timed && d_segments) HIP_OK(hipMemcpyAsync(&d.segments, d_segments, sizeof d.segments, hipMemcpyDeviceToHost, st));
        if (wait) HIP_OK(hipStreamSynchronize(st));
        if (timed) HIP_OK(hipEventElapsedTime(&d.ms, ev[0], ev[1]));
        return d;
    }
};
// What half of the free HBM holds in slots of slot_bytes (call_plan.h's slot_target).
static uint64_t slot_target(const Renderer::Impl& I, size_t slot_bytes) {
    size_t free_b = 0, total_b = 0;
    HIP_OK(hipMemGetInfo(&free_b, &total_b));
    return slot_target(free_b, I.ws.size(), slot_bytes);
}

size_t Renderer::scene_bytes() const { return impl_->s64.bytes; }
int Renderer::device() const { return impl_->device; }
const FlatScene& Renderer::flat() const { return impl_->flat; }

// ------------------------------------------------------------------------------------------------ pass setup
// What rt_render (render_impl) and rt_render_noise_target share.
// The geometry of the nrows local rows (band_local_rows) in 8x8-tile order; the per-pass fields (k, sample_base, P,
// live, cap, chunk, the pixel list) are the caller's.
static PassGeom make_pass_geom(const RenderParams& p, int nrows, uint32_t stack) {
    PassGeom g{};
    g.W = p.width;
    g.H = p.height;
    g.rows = nrows;
    g.band_rows = p.band_rows;
    g.band_count = p.band_count;
    g.band_index = p.band_index;
    g.tiles_x = static_cast<uint32_t>((p.width + 7) / 8);
    const uint32_t tiles_y = static_cast<uint32_t>((nrows + 7) / 8);
    g.npix_pad = g.tiles_x * tiles_y * 64u;
    g.max_depth = p.max_depth;
    g.seed = p.seed;
    g.seed_mix = splitmix64(p.seed);
    g.fd_tiles_x = FastDiv::make(g.tiles_x);
    g.fd_band_rows = FastDiv::make(static_cast<uint32_t>(p.band_rows));
    g.fd_w = FastDiv::make(static_cast<uint32_t>(p.width));
    g.fd_npix = FastDiv::make(g.npix_pad);
    g.inv_w1 = 1.0 / static_cast<double>(p.width - 1);
    g.inv_h1 = 1.0 / static_cast<double>(p.height - 1);
    g.stack = stack;
    return g;
}
// Does a whole-image render of k samples per pass build k_paths' tile lists (option render.tile_lists)?  Only the LDS
// scene's persistent kernel reads them, and only a scene whose image carries representative slots gets them.  Auto:
// when the table's one launch stays below 1 % of a pass.  Both scale with the tile count, so the rule is a sample count:
// k_tile_lists takes 168 microseconds per 1920x1080 frame and scene 1 traces 0.26 ms per sample there: 0.9 % at 72
// (DESIGN 4.1).
constexpr uint32_t kTileListsAutoSpp = 72;
static bool tile_lists_wanted(const DeviceScene& ds, int variant, uint32_t k) {
    const int mode = static_cast<int>(opt(Opt::TileLists));
    return variant == EXT_MEGA && ds.tile_reps > 0 && (mode == 2 || (mode == 1 && k >= kTileListsAutoSpp));
}
// The wavefront variants' queue counters: a line per depth (at least 4: the device-counted adaptive levels take one each)
static size_t counter_words(int max_depth) { return static_cast<size_t>(std::max(max_depth + 1, 4)) * kQueueKinds * kShards * kCounterStride; }

// RT_PROFILE's events, destroyed on every exit path.  rt_render reserves them before the timed region; a mark beyond
// the reserve creates its event (noise-target rendering: the number of rounds is not known beforehand).
struct ProfileMarks {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    ~ProfileMarks() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
    void reserve(size_t n) {
        while (ev.size() < n) {
            ev.push_back(nullptr);
            HIP_OK(hipEventCreate(&ev.back()));
        }
    }
    void mark(hipStream_t stream) {
        reserve(used + 1);  // (creates nothing within the reserve)
        HIP_OK(hipEventRecord(ev[used++], stream));
    }
    // The marks come in groups of `per`: a persistent launch's {start, end}, a wavefront bounce's {start, extend end, shade end}.
    void sum(size_t per, double& ext_ms, double& sh_ms) const {
        ext_ms = sh_ms = 0;
        for (size_t e = 0; e + per <= used; e += per) {
            float a = 0, b = 0;
            HIP_OK(hipEventElapsedTime(&a, ev[e], ev[e + 1]));
            if (per > 2) HIP_OK(hipEventElapsedTime(&b, ev[e + 1], ev[e + 2]));
            ext_ms += a, sh_ms += b;
        }
    }
};

// One render (rt_render or rt_render_noise_target) from begin_frame to end_frame.
struct Frame {
    Renderer::Impl& I;
    DeviceScene& ds;
    const CameraRec& cam;
    const RenderParams& p;
    Call call;                 // timed, on `stream`
    hipStream_t stream = nullptr;
    int variant = 0, nrows = 0;
    bool mega = false;         // a persistent-path kernel: one launch per pass, a slot is its radiance record only
    PassGeom g{};              // the local rows in 8x8-tile order; every pass fills the per-pass fields of its own copy
    Work w{};
    uint8_t* drgb = nullptr;
    uint32_t k = 0, Pmax = 0;  // samples per whole-image pass, and its slots: what the workspace holds
    size_t local_pix = 0, counter_bytes = 0;  // a pass clears counter_bytes: one line (persistent) or the wavefront queues' 1.25 MB
    int npasses = 0, passes = 0;  // planned for `spp` samples / run so far
    uint64_t launches = 0;
    KernelId kid;              // the persistent kernel the passes ran (stays {0, 0, -1} for the wavefront variants)
    ProfileMarks marks;
    std::function<void()> mark;  // records the next of `marks` (empty without RT_PROFILE)
};

#ifdef ART_TRACE
static void trace_setup() {
    long long tp = -1, ts = -1;
    if (const char* t = std::getenv("ART_TRACE")) std::sscanf(t, "%lld:%lld", &tp, &ts);
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_pixel), &tp, sizeof tp));
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_sample), &ts, sizeof ts));
}
#endif
#ifdef ART_STATS
static void dump_art_stats(hipStream_t stream) {
    unsigned long long st[kArtStats] = {0};
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_art_stats), sizeof st));
    std::fprintf(stderr, "ART_STATS node_w %llu node_l %llu (util %.3f) leaf_w %llu leaf_l %llu (util %.3f) outer_w %llu outer_l %llu (util %.3f) "
                 "traversals %llu nodes/trav %.2f leaftests/trav %.2f\n",
                 st[0], st[1], st[1] / (64.0 * st[0]), st[2], st[3], st[3] / (64.0 * st[2]), st[4], st[5], st[5] / (64.0 * st[4]), st[6],
                 double(st[1]) / st[6], double(st[3]) / st[6]);
    std::fprintf(stderr, "ART_STATS dead node visits (LDS scene) %llu (%.3f of visits), stale visits (box entered beyond tmax) %llu (%.3f), "
                 "leaf tests that shorten tmax %llu (%.3f of tests)\n",
                 st[12], double(st[12]) / st[1], st[14], double(st[14]) / st[1], st[13], double(st[13]) / st[3]);
    if (st[15] + st[17] + st[19] + st[21] > 0)
        std::fprintf(stderr, "ART_STATS leaf tests by type (lane tests, wave iterations running it): box %llu %llu sphere %llu %llu triangle %llu %llu rect %llu %llu\n",
                     st[15], st[16], st[17], st[18], st[19], st[20], st[21], st[22]);
    const double tt = double(st[8] + st[9] + st[10] + st[11] + st[24] + st[25] + st[26] + st[48]);
    if (tt > 0)
        std::fprintf(stderr, "ART_STATS cycles: load/claim %.3f trace %.3f shade %.3f append/store %.3f (k_paths_g shading split: surface %.3f "
                     "coop-sphere %.3f texture+unit %.3f scatter %.3f)\n",
                     st[8] / tt, st[9] / tt, (st[10] + st[24] + st[25] + st[26]) / tt, st[11] / tt, st[24] / tt, st[25] / tt, st[26] / tt, st[10] / tt);
    if (st[49] > 0)
        std::fprintf(stderr, "ART_STATS batches: cycles %.3f batches %llu camera rays %llu (util %.3f) entries pushed %llu (%.2f per batch)\n",
                     st[48] / tt, st[49], st[50], st[50] / (64.0 * st[49]), st[51], double(st[51]) / st[49]);
    if (st[28] + st[30] > 0)
        std::fprintf(stderr, "ART_STATS texture evaluations (wave iterations, lanes): noise %llu %llu image %llu %llu\n", st[28], st[29], st[30], st[31]);
    if (st[46] > 0)
        std::fprintf(stderr, "ART_STATS leaf phases %llu: leaf-loop wave iterations %llu, a wave-cooperative leaf test's %llu (%.3f)\n", st[46], st[2],
                     st[47], double(st[47]) / double(st[2]));
    if (st[44] > 0)
        std::fprintf(stderr, "ART_STATS surface branches (wave iterations, lanes): world_surface %llu %llu sphere %llu %llu sphere-uv %llu %llu "
                     "unwind %llu %llu medium %llu %llu box/rect-record %llu %llu box/rect-carried %llu %llu\n",
                     st[44], st[45], st[40], st[41], st[32], st[33], st[34], st[35], st[36], st[37], st[38], st[39], st[42], st[43]);
    std::memset(st, 0, sizeof st);
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_art_stats), st, sizeof st));
}
#endif

// Sets the frame up and opens the timed region (Impl::ev[0]); false: this band has no rows, nothing to render.  spp and
// spread go to plan_passes; carve(Carver&) lays the workspace out (run twice, for the size and for the pointers: it fills
// f.w, f.drgb and the caller's own, and may read what is set before); RT_PROFILE's marks are created here for
// profile_levels x the planned passes (0: on demand).
template <class Carve>
static bool begin_frame(Frame& f, RenderStats& stats, int spp, bool spread, int profile_levels, Carve&& carve) {
    Renderer::Impl& I = f.I;
    const RenderParams& p = f.p;
    f.call = Call(I.own_stream, I.ev, (p.flags & RT_OUT_DEVICE) != 0, p.stream, true, plan_frame_call);
    f.stream = f.call.st;
    for (int a = 0; a < 3; ++a) f.ds.view.bg[a] = p.background[a];  // engine::set_scene's background
    f.nrows = band_local_rows(p.height, p.band_rows, p.band_count, p.band_index);
    stats.local_rows = f.nrows;
    if (f.nrows == 0) return false;
    f.g = make_pass_geom(p, f.nrows, stack_rows(f.ds.max_stack));
    f.variant = extend_variant(f.ds, p.flags);
    f.mega = f.variant == EXT_MEGA || f.variant == EXT_MEGA_G;
    const size_t slot_bytes = f.mega ? sizeof(ResRec) : sizeof(PathRec) + sizeof(HitRecD) + sizeof(ResRec) + 4u * (2u + kNumMatTypes) + 8u;
    const uint64_t target = slot_target(I, slot_bytes);
    if (f.g.npix_pad > kMaxPassSlots) throw std::runtime_error("image too large for one pass (more than 2^31 padded pixels)");
    const PassPlan plan = plan_passes(target, p.samples_per_pass, f.g.npix_pad, spp, spread);
    f.k = plan.k, f.npasses = plan.npasses;
    f.Pmax = f.k * f.g.npix_pad;  // <= kMaxPassSlots (plan_passes)
    f.g.cap = shard_cap(f.Pmax);
    f.local_pix = static_cast<size_t>(f.nrows) * p.width;
    f.counter_bytes = f.mega ? 4u * kCounterStride : 4ull * counter_words(p.max_depth);
    f.call.carve(I.ws, carve);
    if (p.flags & RT_PROFILE) {  // (a pixel-list level never needs more passes than k gives)
        // (a k_paths pass may run as two launches: split_pass)
        f.marks.reserve(static_cast<size_t>(profile_levels) * f.npasses * (f.variant == EXT_MEGA ? 4 : f.mega ? 2 : 3 * p.max_depth));
        f.mark = [&f]() { f.marks.mark(f.stream); };
    }
    f.call.begin();
    HIP_OK(hipMemsetAsync(f.w.segments, 0, sizeof(unsigned long long), f.stream));
    if (p.max_depth == 0) HIP_OK(hipMemsetAsync(f.w.res, 0, sizeof(ResRec) * f.Pmax, f.stream));  // engine.h:451-452
    return true;
}

// One pass of g through the variant's kernels: the counters' clear (unless the caller cleared them), then max_depth
// wavefront bounces, or one persistent launch claiming from counter line `line`.  A pass at max_depth 0 launches
// nothing and still counts.  RT_PROFILE's marks enclose the persistent launch alone.  res_first: the pass's records
// begin at that record of the workspace's (the tail of a split pass; persistent kernels only).
static void run_pass(Frame& f, PassGeom g, int line = 0, bool clear = true, size_t res_first = 0) {
    Work w = f.w;
    w.res += res_first;
    if (clear) HIP_OK(hipMemsetAsync(f.w.counters, 0, f.counter_bytes, f.stream));
    if (!f.mega) {
        for (int d = 0; d < f.p.max_depth; ++d) bounce(f.ds, f.variant, f.I.num_cu, f.stream, g, f.cam, w, d, f.mark);
        f.launches += static_cast<uint64_t>(f.p.max_depth);
    } else if (f.p.max_depth > 0) {
        g.chunk = path_chunk(g.P, f.I.num_cu);
        if (f.mark) f.mark();
        if (f.variant == EXT_MEGA) {
            launch_paths(f.I.num_cu, f.stream, f.ds.view, g, f.cam, w, counter(w, line, 0, 0));
            f.kid = KernelId{kFeatSpheres, 0, 3};
        } else {
            f.kid = launch_paths_g(f.ds.features, f.ds.tex_basic, f.ds.tex_bary, f.ds.codes16, f.ds.leaf_shift, f.I.num_cu, f.stream, f.ds.view, g,
                                   f.cam, w, counter(w, line, 0, 0));
        }
        if (f.mark) f.mark();
        ++f.launches;
    }
    ++f.passes;
}

// g in entry-major pixel-list mode (PassGeom::list_mode 1): k samples from sample_base of every entry of `list`, the
// samples of an entry on consecutive slots.  nlist and P are the entry count and its slots, or upper bounds of them
// when the count stays on the device (list[-1]).
static PassGeom list_geom(PassGeom g, const uint32_t* list, uint32_t nlist, uint32_t k, uint32_t sample_base, uint32_t P) {
    g.list_mode = 1, g.list = list, g.nlist = nlist;
    g.k = g.npix_pad = k, g.fd_npix = FastDiv::make(k), g.sample_base = sample_base;
    g.P = g.live = P;
    return g;
}

// Closes the timed region and hands the frame over: Impl::ev[1], the copies of the RGB8 frame and (out_acc non-null)
// the sums, the caller's further copies, the segment count; after the stream has drained, every field of the stats but
// `primary`, which is the caller's.
static void end_frame(Frame& f, RenderStats& stats, uint8_t* out_rgb, double* out_acc, const std::function<void()>& more_copies = {}) {
#ifdef ART_STATS
    HIP_OK(hipGetLastError());
    dump_art_stats(f.stream);
#endif
    f.call.end();
    f.call.copy_out(out_rgb, f.drgb, 3 * f.local_pix);
    f.call.copy_out(out_acc, f.w.acc, sizeof(double) * 3 * f.local_pix);
    if (more_copies) more_copies();
    const Call::Done done = f.call.finish(f.w.segments);
    stats.ms = done.ms, stats.segments = done.segments, stats.passes = f.passes, stats.samples_per_pass = static_cast<int>(f.k);
    stats.extend_variant = f.variant, stats.kernel_features = f.kid.f, stats.kernel_textures = f.kid.tf, stats.kernel_lds_mode = f.kid.lm;
    if (f.p.flags & RT_PROFILE) {
        f.marks.sum(f.mega ? 2 : 3, stats.extend_ms, stats.shade_ms);
        stats.extend_launches = f.launches;
        stats.shade_launches = f.variant == EXT_GLOBAL || f.variant == EXT_LDS ? f.launches : 0;
    }
}

// ------------------------------------------------------------------------------------------------ rt_render
// What rt_render's modes need beside the Frame.
struct RenderBufs {
    int spp_t;          // samples traced per pixel: spp, or parallel_images' 4 * (spp / 4) (engine.h:411-414)
    uint8_t* out_rgb;   // the caller's buffers (progressive snapshots)
    double *out_acc, *qsum;  // qsum: parallel_images' quarter sums (null in every other mode)
    // adaptive mode: the int work frame, the pixel lists (four, one per level, at most 4 / 12 / 48 / 80 of every 144
    // pixels, each after the 64-word line of its count), the three levels' square flags, the host-counted list's counter
    int32_t* ad_work;
    uint32_t *ad_lists, *ad_count;
    uint8_t *ad_f0, *ad_f1, *ad_f2;
    int sqx;            // big squares per row, and in the local rows
    uint32_t nsq;
};

// Traces spp_t samples of every local pixel (list == nullptr) or of every entry of a device pixel list into w.acc (per
// local pixel, or per list entry), in passes of sample-major slots.  Returns the samples traced: spp_t, or fewer when
// the progressive callback (whole-image traces only) ended the render.
static int trace_samples(Frame& f, const RenderBufs& b, const uint32_t* list, uint32_t nlist) {
    const RenderParams& p = f.p;
    PassGeom g = f.g;
    uint32_t kk = f.k, npix = static_cast<uint32_t>(f.local_pix);
    if (list) {
        g.list = list, g.nlist = npix = nlist;
        g.npix_pad = list_pad(nlist), g.fd_npix = FastDiv::make(g.npix_pad);
        kk = list_pass_samples(static_cast<uint32_t>(p.spp), f.Pmax, nlist);
    }
    HIP_OK(hipMemsetAsync(f.w.acc, 0, sizeof(double) * 3 * npix, f.stream));
    if (b.qsum) HIP_OK(hipMemsetAsync(b.qsum, 0, sizeof(double) * 3 * npix, f.stream));
    const uint32_t spp_t = static_cast<uint32_t>(b.spp_t);
    int done = 0;
    // a split pass (pass_plan.h split_pass): the head's sums run on the second stream while the tail traces
    const bool can_split = f.variant == EXT_MEGA && !list && !p.on_pass && !b.qsum;
    int split_mode = static_cast<int>(opt(Opt::AccumOverlap));
    if (split_mode == 1 && p.samples_per_pass > 0) split_mode = 0;  // auto keeps a caller's own passes at one launch each
    AccumFork fork(f.I);
    const auto sized = [&](PassGeom s, uint32_t first, uint32_t k) {  // samples [first, first + k) of g's pass
        s.sample_base = g.sample_base + first, s.k = k;
        s.P = k * s.npix_pad, s.live = k * npix;
        return s;
    };
    for (uint32_t sb = 0; sb < spp_t; sb += kk) {
        g.sample_base = sb, g.k = std::min<uint32_t>(kk, spp_t - sb);
        g.P = g.k * g.npix_pad, g.live = g.k * npix;
        const PassSplit split = split_pass(g.k, g.npix_pad, split_mode, can_split);
        if (split.tail == 0) {
            run_pass(f, g);
            launch_accum(f.stream, g, f.w, b.qsum, spp_t / 4);
        } else {
            run_pass(f, sized(g, 0, split.head));
            fork.fork(f.stream);
            // sums continue from the stored value in sample order, launch after launch, as they do pass after pass
            for (uint32_t s0 = 0; s0 < split.head; s0 += kAccumLaunchSamples) {
                Work w = f.w;
                w.res += static_cast<size_t>(s0) * g.npix_pad;
                launch_accum(f.I.accum_stream, sized(g, s0, std::min(kAccumLaunchSamples, split.head - s0)), w, nullptr, 0);
            }
            const size_t tail_first = static_cast<size_t>(split.head) * g.npix_pad;
            run_pass(f, sized(g, split.head, split.tail), 0, true, tail_first);
            fork.join(f.stream);
            Work w = f.w;
            w.res += tail_first;
            launch_accum(f.stream, sized(g, split.head, split.tail), w, nullptr, 0);
        }
        done = static_cast<int>(sb + g.k);
        // progressive snapshot: write_color of the sums so far, with the samples so far
        if (!list && p.on_pass) {
            launch_finalize(f.stream, f.w.acc, f.drgb, npix, done);
            f.call.copy_out(b.out_rgb, f.drgb, 3ull * npix);
            f.call.copy_out(b.out_acc, f.w.acc, sizeof(double) * 3 * npix);
            HIP_OK(hipStreamSynchronize(f.stream));
            if (!p.on_pass(done)) break;
        }
    }
    return done;
}

// The three modes: each leaves the RGB8 frame in f.drgb and returns the primary samples (the device-counted levels'
// come back with the frame).
static uint64_t render_whole(Frame& f, const RenderBufs& b) {
    const int done = trace_samples(f, b, nullptr, 0);
    launch_finalize(f.stream, f.w.acc, f.drgb, static_cast<uint32_t>(f.local_pix), done < b.spp_t ? done : f.p.spp);
    return f.local_pix * static_cast<uint64_t>(done);
}
// engine.h:151-333: levels 0..3 (k_adapt_*), one pass each, with no host round trip: each level's list count stays on
// the device (list[-1], PassGeom::list_mode 1), the persistent kernel reads it at its start and the level's samples
// are entry-major (a wave traces one pixel's samples: coherent rays).  counts[] receive the four entry counts once the
// stream has drained: their sum x spp are the primary samples.
static void adaptive_device_counted(Frame& f, const RenderBufs& b, uint32_t counts[4]) {
    const RenderParams& p = f.p;
    const uint32_t caps[4] = {4 * b.nsq, 12 * b.nsq, 48 * b.nsq, 80 * b.nsq};
    uint32_t* lists[4];
    uint32_t* at = b.ad_lists;
    for (int L = 0; L < 4; ++L) {
        lists[L] = at + 64;  // the count word at lists[L][-1]
        at = lists[L] + list_pad(caps[L]);
    }
    HIP_OK(hipMemsetAsync(b.ad_lists, 0, 4ull * adaptive_list_words(b.nsq), f.stream));  // every count 0
    HIP_OK(hipMemsetAsync(b.ad_work, 0xFF, sizeof(int32_t) * 3 * f.local_pix, f.stream));  // the reference's -1 frame
    launch_adapt_corners(f.stream, lists[0], p.width, b.sqx, b.nsq);
    // one slot counter line per level (counter(w, level, 0, 0): the wavefront variants' depth lines, unused here),
    // cleared together before level 0 instead of one fill launch per level
    HIP_OK(hipMemsetAsync(f.w.counters, 0, 4ull * kQueueKinds * kShards * kCounterStride * 4, f.stream));
    for (int level = 0; level < 4; ++level) {
        const uint64_t slots = static_cast<uint64_t>(caps[level]) * f.k;  // upper bounds: the kernels read the count
        if (slots > f.Pmax) throw std::runtime_error("internal: adaptive level larger than the pass workspace");
        run_pass(f, list_geom(f.g, lists[level], caps[level], f.k, 0, static_cast<uint32_t>(slots)), level, false);
        launch_adapt_accum(f.stream, lists[level], caps[level], f.w.res, f.k, p.spp, b.ad_work);
        if (level == 3) break;
        launch_adapt_level(f.stream, level, b.ad_work, p.width, b.sqx, b.nsq, b.ad_f0, b.ad_f1, b.ad_f2, lists[level + 1], lists[level + 1] - 1);
    }
    launch_adapt_fill(f.stream, b.ad_work, f.drgb, p.width, f.nrows, b.sqx, b.ad_f0, b.ad_f1, b.ad_f2);
    for (int L = 0; L < 4; ++L) HIP_OK(hipMemcpyAsync(&counts[L], lists[L] - 1, 4, hipMemcpyDeviceToHost, f.stream));
}
// engine.h:151-333: levels 0..3 (k_adapt_*); the list sizes come back to the host between levels (multi-pass levels,
// the wavefront variants), one list at a time
static uint64_t adaptive_host_counted(Frame& f, const RenderBufs& b) {
    const RenderParams& p = f.p;
    uint32_t* list = b.ad_lists + 64;
    HIP_OK(hipMemsetAsync(b.ad_work, 0xFF, sizeof(int32_t) * 3 * f.local_pix, f.stream));  // the reference's -1 frame
    launch_adapt_corners(f.stream, list, p.width, b.sqx, b.nsq);
    uint32_t n = 4 * b.nsq;
    uint64_t traced = 0;
    for (int level = 0;; ++level) {
        trace_samples(f, b, list, n);
        launch_adapt_store(f.stream, list, n, f.w.acc, p.spp, b.ad_work);
        traced += n;
        if (level == 3) break;
        HIP_OK(hipMemsetAsync(b.ad_count, 0, 4, f.stream));
        launch_adapt_level(f.stream, level, b.ad_work, p.width, b.sqx, b.nsq, b.ad_f0, b.ad_f1, b.ad_f2, list, b.ad_count);
        HIP_OK(hipMemcpyAsync(&n, b.ad_count, 4, hipMemcpyDeviceToHost, f.stream));
        HIP_OK(hipStreamSynchronize(f.stream));
        if (n == 0) break;
    }
    launch_adapt_fill(f.stream, b.ad_work, f.drgb, p.width, f.nrows, b.sqx, b.ad_f0, b.ad_f1, b.ad_f2);
    return traced * static_cast<uint64_t>(b.spp_t);
}

void Renderer::render(const CameraRec& cam, const RenderParams& p, uint8_t* out_rgb, double* out_acc, RenderStats& stats) {
    if (p.fp_mode != RT_FP64) throw std::runtime_error("fp_mode must be RT_FP64");
    upload();
    Impl& I = *impl_;
    Frame f{I, I.s64, cam, p};
    const bool images = (p.flags & RT_PARALLEL_IMAGES) != 0, adaptive = (p.flags & RT_ADAPTIVE) != 0;
    RenderBufs b{};
    b.spp_t = images ? 4 * (p.spp / 4) : p.spp, b.out_rgb = out_rgb, b.out_acc = out_acc;
#ifdef ART_TRACE
    trace_setup();
#endif
    TileRec* tile_tab = nullptr;
    if (!begin_frame(f, stats, b.spp_t, true, adaptive ? 4 : 1, [&](Carver& c) {
        const bool wf = !f.mega;  // wavefront-only buffers
        f.w.paths = c.take<PathRec>(f.Pmax, wf);
        f.w.hits = c.take<HitRecD>(f.Pmax, wf);
        f.w.res = c.take<ResRec>(f.Pmax);
        f.w.active[0] = c.take<uint32_t>(static_cast<size_t>(kShards) * f.g.cap, wf);
        f.w.active[1] = c.take<uint32_t>(static_cast<size_t>(kShards) * f.g.cap, wf);
        f.w.mq = c.take<uint32_t>(static_cast<size_t>(kMatSegs) * f.g.cap, wf);
        f.w.counters = c.take<uint32_t>(counter_words(p.max_depth));
        f.w.segments = c.take<unsigned long long>(1);
        f.w.acc = c.take<double>(3 * f.local_pix);
        f.drgb = c.take<uint8_t>(3 * f.local_pix);
        double* qsum = c.take<double>(3 * f.local_pix, images);
        b.qsum = images ? qsum : nullptr;
        f.w.pool = c.take<char>(pool_bytes(f.variant, I.num_cu));
        tile_tab = c.take<TileRec>(f.g.npix_pad / 64u, !adaptive && tile_lists_wanted(f.ds, f.variant, f.k));
        b.ad_work = c.take<int32_t>(3 * f.local_pix, adaptive);
        b.ad_lists = c.take<uint32_t>(adaptive_list_words(static_cast<uint32_t>(f.local_pix / (kBig * kBig))), adaptive);
        b.ad_f0 = c.take<uint8_t>(21 * (f.local_pix / (kBig * kBig)), adaptive);  // 1 + 4 + 16 flags per big square
        b.ad_count = c.take<uint32_t>(1, adaptive);
    })) return;
    b.ad_f1 = b.ad_f0 + f.local_pix / (kBig * kBig), b.ad_f2 = b.ad_f1 + 4 * (f.local_pix / (kBig * kBig));
    b.sqx = p.width / kBig, b.nsq = static_cast<uint32_t>(b.sqx) * static_cast<uint32_t>(f.nrows / kBig);
    uint32_t ad_counts[4] = {0, 0, 0, 0};  // the device-counted levels' entry counts (read back with the frame)
    uint64_t primary = 0;
    // the tile lists of this call's camera and geometry (nothing is kept across calls), before the first pass; the
    // adaptive levels' passes are pixel lists and keep the tree
    if (!adaptive && p.max_depth > 0 && tile_lists_wanted(f.ds, f.variant, f.k)) {
        launch_tile_lists(f.stream, f.ds.view, f.g, cam, tile_tab);
        f.w.tiles = tile_tab;
    }
    if (!adaptive) primary = render_whole(f, b);
    else if (f.mega && f.k == static_cast<uint32_t>(b.spp_t) && !images && !p.on_pass) adaptive_device_counted(f, b, ad_counts);
    else primary = adaptive_host_counted(f, b);
    end_frame(f, stats, out_rgb, adaptive ? nullptr : out_acc);
    stats.primary = primary + (static_cast<uint64_t>(ad_counts[0]) + ad_counts[1] + ad_counts[2] + ad_counts[3]) * static_cast<uint64_t>(b.spp_t);
}

int Renderer::tile_candidates(const CameraRec& cam, const RenderParams& p, uint16_t* counts, size_t cap) {
    upload();
    Impl& I = *impl_;
    DeviceScene& ds = I.s64;
    const int nrows = band_local_rows(p.height, p.band_rows, p.band_count, p.band_index);
    if (nrows == 0 || p.max_depth <= 0 || (p.flags & RT_ADAPTIVE)) return 0;
    const PassGeom g = make_pass_geom(p, nrows, stack_rows(ds.max_stack));
    if (g.npix_pad > kMaxPassSlots) throw std::runtime_error("image too large for one pass (more than 2^31 padded pixels)");
    const int variant = extend_variant(ds, p.flags);
    // the samples per pass begin_frame would plan for a persistent kernel
    const int spp_t = (p.flags & RT_PARALLEL_IMAGES) ? 4 * (p.spp / 4) : p.spp;
    const PassPlan plan = plan_passes(slot_target(I, sizeof(ResRec)), p.samples_per_pass, g.npix_pad, spp_t, true);
    if (!tile_lists_wanted(ds, variant, plan.k)) return 0;
    const size_t ntiles = g.npix_pad / 64u;
    if (!counts) return static_cast<int>(ntiles);
    if (cap < ntiles) throw std::runtime_error("rt_tile_candidates: counts holds fewer entries than the frame has tiles");
    Carver c(I.ws.reserve(sizeof(TileRec) * ntiles));
    TileRec* tab = c.take<TileRec>(ntiles);
    launch_tile_lists(I.own_stream, ds.view, g, cam, tab);
    HIP_OK(hipGetLastError());
    std::vector<TileRec> host(ntiles);
    HIP_OK(hipMemcpyAsync(host.data(), tab, sizeof(TileRec) * ntiles, hipMemcpyDeviceToHost, I.own_stream));
    HIP_OK(hipStreamSynchronize(I.own_stream));
    for (size_t i = 0; i < ntiles; ++i) counts[i] = host[i].n;
    return static_cast<int>(ntiles);
}

void Renderer::upload() {
    HIP_OK(hipSetDevice(impl_->device));
    if (!impl_->up64) {
        build_device_scene(impl_->flat, impl_->s64);
        impl_->up64 = true;
    }
}

void Renderer::trace_rays(const double* rays, size_t n, bool global_scene, double* t_out, double* n_out) {
    upload();
    const DeviceScene& ds = impl_->s64;
    if (n == 0) return;
    if (n > (1u << 30)) throw std::runtime_error("too many rays");
    Call call(impl_->own_stream, impl_->ev, false, nullptr, false);
    const double* d_rays = nullptr;
    double *d_t = nullptr, *d_n = nullptr;
    call.carve(impl_->ws, [&](Carver& c) { d_rays = call.in(c, rays, 7 * n), d_t = call.out(c, t_out, n), d_n = call.out(c, n_out, 3 * n); }, 1);  // packed
    launch_trace_rays(ds, global_scene, call.st, d_rays, static_cast<uint32_t>(n), d_t, d_n);
    call.end();
    call.finish();
}

void Renderer::query_rays(const double* rays, const double* t_max, size_t n, bool device, bool global_scene, bool any_hit, bool no_media,
                          void* stream, double* hits, uint8_t* occluded) {
    upload();
    Impl& I = *impl_;
    const DeviceScene& ds = I.s64;
    if (n == 0) return;
    if (n > (1u << 30)) throw std::runtime_error("too many rays");
    // never timed: a device call waits exactly on the scene's own stream (the null handle), on which nobody else can
    Call call(I.own_stream, I.ev, device, stream, false);
    // device buffers: the caller's as they are, no workspace, no copy; host buffers: [rays][t_max][hits or occluded]
    // packed in the workspace (each part 8-byte aligned)
    const double *d_rays = nullptr, *d_tm = nullptr;
    double* d_hits = nullptr;
    uint8_t* d_occ = nullptr;
    call.carve(I.ws, [&](Carver& c) {
        d_rays = call.in(c, rays, 7 * n), d_tm = call.in(c, t_max, n);
        if (any_hit) d_occ = call.out(c, occluded, n);
        else d_hits = call.out(c, hits, RT_HIT_DOUBLES * n);
    }, 1);
    if (any_hit) launch_occlude_rays(ds, global_scene, call.st, d_rays, d_tm, static_cast<uint32_t>(n), d_occ);
    else launch_query_rays(ds, global_scene, call.st, d_rays, d_tm, static_cast<uint32_t>(n), no_media, d_hits);
    call.end();
    call.finish();
}

void Renderer::render_guides(const CameraRec& cam, const RenderParams& p, double* guides, double* rays_out) {
    upload();
    Impl& I = *impl_;
    const DeviceScene& ds = I.s64;
    GuideGeom g{p.width, p.height, band_local_rows(p.height, p.band_rows, p.band_count, p.band_index), p.band_rows, p.band_count, p.band_index};
    if (g.rows == 0) return;
    const size_t npix = static_cast<size_t>(g.rows) * p.width;
    const bool device = (p.flags & RT_OUT_DEVICE) != 0;
    Call call(I.own_stream, I.ev, device, p.stream, false, plan_frame_call);
    // host buffers: the kernel writes the (packed) workspace, copied out by end()
    double *d_g = nullptr, *d_r = nullptr;
    call.carve(I.ws, [&](Carver& c) { d_g = call.out(c, guides, 10 * npix), d_r = call.out(c, rays_out, 7 * npix); }, 1);
    launch_guides(ds, p.flags, call.st, g, cam, d_g, d_r);
    call.end();
    call.finish();
}

void Renderer::radiance_rays(const RadianceParams& p, const double* rays, const uint64_t* rng, size_t n, double* radiance, RenderStats* stats) {
    upload();
    Impl& I = *impl_;
    const DeviceScene& ds = I.s64;
    if (n == 0) return;
    const uint32_t spp = static_cast<uint32_t>(std::max(1, p.spp));
    const uint64_t P = static_cast<uint64_t>(n) * spp;
    if (n > (1u << 30) || P > kMaxPassSlots) throw std::runtime_error("too many rays or paths");
    Call call(I.own_stream, I.ev, p.device, p.stream, stats != nullptr);
    hipStream_t st = call.st;
    // workspace: the claim counter's line, the segment count, the per-path records (spp > 1) and, for host buffers,
    // the device copies of the caller's
    RadianceJob job{};
    call.carve(I.ws, [&](Carver& c) {
        job.next = c.take<uint32_t>(kCounterStride);
        job.segments = c.take<unsigned long long>(1);
        job.res = c.take<ResRec>(P, spp > 1);
        job.rays = call.in(c, rays, 7 * n);
        job.rng = call.in(c, rng, P);
        job.radiance = call.out(c, radiance, 3 * n);
    });
    if (spp == 1) job.res = nullptr;
    job.P = static_cast<uint32_t>(P), job.spp = spp, job.chunk = path_chunk(job.P, I.num_cu);
    job.sample_base = p.sample_base, job.id_base = static_cast<uint32_t>(p.id_base);
    job.stack = stack_rows(ds.max_stack);
    job.max_depth = p.max_depth;
    job.seed_mix = splitmix64(p.seed);
    job.fd_spp = FastDiv::make(spp);
    HIP_OK(hipMemsetAsync(job.next, 0, sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(job.segments, 0, sizeof(unsigned long long), st));
    call.begin();
    launch_radiance_rays(ds, p.global_scene ? RT_GLOBAL_SCENE : 0, I.num_cu, st, job, static_cast<uint32_t>(n), p.background);
    call.end();
    call.finish(job.segments).fill(stats, P, 1, static_cast<int>(spp));  // (a device call on the caller's stream without stats returns enqueued)
}

void Renderer::radiance_grad(const RadianceParams& p, const double* rays, const uint64_t* rng, const double* weights, size_t n, double* radiance,
                             double* grad_textures, double* grad_materials, double* grad_background, double* grad_texels, RenderStats* stats) {
    upload();
    Impl& I = *impl_;
    DeviceScene& ds = I.s64;
    if (n == 0) return;
    const uint32_t spp = static_cast<uint32_t>(std::max(1, p.spp));
    const uint64_t P = static_cast<uint64_t>(n) * spp;
    if (n > (1u << 30) || P > kMaxPassSlots) throw std::runtime_error("too many rays or paths");
    const size_t T = I.flat.texs.size(), M = I.flat.mats.size();
    // the texel rows: global texel t is row T + M + 1 + t of a vertex record (32 bits; abi.cpp refuses a scene beyond)
    size_t N = 0;
    for (const ImageRec& im : I.flat.images) N += static_cast<size_t>(im.w) * static_cast<size_t>(im.h);
    if (grad_texels && T + M + 1 + N > 0xFFFFFFFFull) throw std::runtime_error("too many texels for a 32-bit row");
    // with a texel output the scene's kernel is k_texel_grad -- unless the scene has no image texture (then no texel has
    // a row: k_radiance_grad, and zeros)
    const bool texels = grad_texels && N > 0 && texel_grad_kernel(ds);
    if (texels && !I.image_row) {
        std::vector<uint32_t> rows;
        uint64_t first = T + M + 1;
        for (const ImageRec& im : I.flat.images) {
            rows.push_back(im.bpp >= 3 ? static_cast<uint32_t>(first) : kGradNoRow);
            first += static_cast<uint64_t>(im.w) * static_cast<uint64_t>(im.h);
        }
        I.image_row = ds.upload(rows);
    }
    Call call(I.own_stream, I.ev, p.device, p.stream, stats != nullptr);
    hipStream_t st = call.st;
    TexelJob tjob{};
    GradJob& job = tjob.g;
    RadianceJob& path = job.path;
    path.stack = stack_rows(ds.max_stack);
    const uint32_t grid = texels ? texel_grad_grid(ds, I.num_cu, static_cast<uint32_t>(P), path.stack)
                                 : radiance_grad_grid(ds, I.num_cu, static_cast<uint32_t>(P), path.stack);
    job.lanes = grid * static_cast<uint32_t>(kBlock);
    job.rows = static_cast<uint32_t>(T + M + 1), job.n_texs = static_cast<uint32_t>(T);
    job.copies = std::min(grid, kGradMaxCopies);
    // workspace: rt_radiance_rays' parts, then the accumulator table's copies (copies x rows x 80 B) and the vertex
    // records (lanes x max(max_depth - 1, 1) x 64 B)
    const size_t acc_limbs = static_cast<size_t>(job.copies) * job.rows * kGradRowLimbs;
    const size_t nverts = static_cast<size_t>(job.lanes) * static_cast<size_t>(std::max(p.max_depth - 1, 1));
    // and with a texel output the texel table's copies (texel_copies x N x 80 B): as many as kTexelTableBudget holds, at
    // least one, at most the other table's count; option grad.texel_copies > 0 sets the count instead (A/B, tests)
    tjob.n_texels = static_cast<uint32_t>(N);
    tjob.image_row = I.image_row;
    if (texels) {
        const size_t one = N * kGradRowLimbs * sizeof(unsigned long long);
        const uint32_t forced = static_cast<uint32_t>(opt(Opt::GradTexelCopies));
        const uint32_t want = forced ? forced : static_cast<uint32_t>(std::max<size_t>(1, kTexelTableBudget / one));
        tjob.texel_copies = std::min(want, job.copies);
    }
    const size_t texel_limbs = texels ? static_cast<size_t>(tjob.texel_copies) * N * kGradRowLimbs : 0;
    double *d_gt = nullptr, *d_gm = nullptr, *d_gb = nullptr, *d_gx = nullptr;
    // none: the kernel records and adds nothing
    const bool grads = grad_textures || grad_materials || grad_background || texels;
    call.carve(I.ws, [&](Carver& c) {
        path.next = c.take<uint32_t>(kCounterStride);
        path.segments = c.take<unsigned long long>(1);
        path.res = c.take<ResRec>(P, spp > 1 && radiance);
        job.acc = c.take<unsigned long long>(acc_limbs, grads);
        job.verts = c.take<GradVertex>(nverts, grads);
        tjob.texel_acc = c.take<unsigned long long>(texel_limbs, texels);
        path.rays = call.in(c, rays, 7 * n);
        path.rng = call.in(c, rng, P);
        job.weights = call.in(c, weights, 3 * n);
        path.radiance = call.out(c, radiance, 3 * n);
        d_gt = call.out(c, grad_textures, RT_TEXTURE_DOUBLES * T);
        d_gm = call.out(c, grad_materials, RT_MATERIAL_DOUBLES * M);
        d_gb = call.out(c, grad_background, 3);
        d_gx = call.out(c, N ? grad_texels : nullptr, 3 * N);
    });
    if (spp == 1 || !radiance) path.res = nullptr;
    path.P = static_cast<uint32_t>(P), path.spp = spp, path.chunk = path_chunk(path.P, I.num_cu);
    path.sample_base = p.sample_base, path.id_base = static_cast<uint32_t>(p.id_base);
    path.max_depth = p.max_depth;
    path.seed_mix = splitmix64(p.seed);
    path.fd_spp = FastDiv::make(spp);
    HIP_OK(hipMemsetAsync(path.next, 0, sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(path.segments, 0, sizeof(unsigned long long), st));
    if (!grads) job.acc = nullptr, job.verts = nullptr;
    else HIP_OK(hipMemsetAsync(job.acc, 0, sizeof(unsigned long long) * acc_limbs, st));
    call.begin();  // (the texel table's zeroing is inside the timed region: it is what a texel output costs)
    if (texels) {
        HIP_OK(hipMemsetAsync(tjob.texel_acc, 0, sizeof(unsigned long long) * texel_limbs, st));
        launch_texel_grad(ds, st, tjob, grid, static_cast<uint32_t>(n), p.background, static_cast<uint32_t>(M), d_gt, d_gm, d_gb, d_gx);
    } else {
        launch_radiance_grad(ds, st, job, grid, static_cast<uint32_t>(n), p.background, static_cast<uint32_t>(M), d_gt, d_gm, d_gb);
        if (d_gx && N) HIP_OK(hipMemsetAsync(d_gx, 0, sizeof(double) * 3 * N, st));
    }
    call.end();
    call.finish(path.segments).fill(stats, P, 1, static_cast<int>(spp));
}

void Renderer::render_views(const CameraRec* cams, const uint64_t* seeds, size_t nviews, const RenderParams& p, uint8_t* out_rgb, double* out_acc,
                            RenderStats* stats) {
    upload();
    Impl& I = *impl_;
    const DeviceScene& ds = I.s64;
    if (nviews == 0) return;
    const bool device = (p.flags & RT_OUT_DEVICE) != 0;
    Call call(I.own_stream, I.ev, device, p.stream, stats != nullptr);
    hipStream_t st = call.st;
    const uint32_t spp = static_cast<uint32_t>(p.spp);
    const uint64_t npix = static_cast<uint64_t>(p.width) * static_cast<uint64_t>(p.height);
    const uint64_t view_paths = npix * spp;
    // the groups (view_plan.h): a launch's records within begin_frame's slot target, within kMaxPassSlots and within
    // views.max_paths
    ViewPlan plan{};
    if (!plan_views(nviews, view_paths, slot_target(I, sizeof(ResRec)), static_cast<uint64_t>(opt(Opt::ViewsMaxPaths)), plan))
        throw std::runtime_error("a view has more paths than one launch holds (kMaxPassSlots)");
    const uint64_t group_paths = static_cast<uint64_t>(plan.per_group) * view_paths;
    const size_t pixels = static_cast<size_t>(nviews) * static_cast<size_t>(npix);
    // workspace: a claim counter's line per group, the segment count, the camera table, the largest group's per-path
    // records (spp > 1) and the frames' sums and bytes unless the caller's device buffers take them
    uint32_t* next = nullptr;
    unsigned long long* segments = nullptr;
    ViewRec* table = nullptr;
    ResRec* res = nullptr;
    double* acc = nullptr;
    uint8_t* rgb = nullptr;
    call.carve(I.ws, [&](Carver& c) {
        next = c.take<uint32_t>(static_cast<size_t>(plan.ngroups) * kCounterStride);
        segments = c.take<unsigned long long>(1);
        table = c.take<ViewRec>(nviews);
        res = c.take<ResRec>(group_paths, spp > 1);
        rgb = call.out(c, out_rgb, 3 * pixels);
        acc = out_acc ? call.out(c, out_acc, 3 * pixels) : c.take<double>(3 * pixels);  // the sums are traced even when nobody asks for them
    });
    // the table's host copy lives in the renderer until the next call: the upload may still read it when a call on the
    // caller's stream returns
    I.view_table.resize(nviews);
    for (size_t v = 0; v < nviews; ++v) I.view_table[v] = ViewRec{cams[v], splitmix64(seeds ? seeds[v] : p.seed)};
    HIP_OK(hipMemcpyAsync(table, I.view_table.data(), sizeof(ViewRec) * nviews, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(next, 0, sizeof(uint32_t) * plan.ngroups * kCounterStride, st));
    HIP_OK(hipMemsetAsync(segments, 0, sizeof(unsigned long long), st));
    call.begin();
    ViewsJob job{};
    job.segments = segments;
    job.spp = spp, job.npix = static_cast<uint32_t>(npix);
    job.stack = stack_rows(ds.max_stack);
    job.max_depth = p.max_depth;
    job.W = p.width, job.H = p.height;
    job.inv_w1 = 1.0 / static_cast<double>(p.width - 1), job.inv_h1 = 1.0 / static_cast<double>(p.height - 1);  // make_pass_geom's
    job.fd_spp = FastDiv::make(spp), job.fd_npix = FastDiv::make(job.npix), job.fd_w = FastDiv::make(static_cast<uint32_t>(p.width));
    for (uint32_t g = 0; g < plan.ngroups; ++g) {
        const size_t v0 = static_cast<size_t>(g) * plan.per_group, nv = std::min<size_t>(plan.per_group, nviews - v0);
        const uint32_t gpix = static_cast<uint32_t>(nv * npix);  // <= group_paths <= kMaxPassSlots
        job.views = table + v0;
        job.radiance = acc + 3 * v0 * npix;
        job.res = spp > 1 ? res : nullptr;
        job.next = next + static_cast<size_t>(g) * kCounterStride;
        job.P = static_cast<uint32_t>(nv * view_paths), job.chunk = path_chunk(job.P, I.num_cu);
        launch_radiance_views(ds, p.flags, I.num_cu, st, job, gpix, p.background);
        launch_finalize(st, job.radiance, rgb + 3 * v0 * npix, gpix, p.spp);
    }
    call.end();
    // (a device call on the caller's stream without stats returns enqueued)
    call.finish(segments).fill(stats, static_cast<uint64_t>(nviews) * view_paths, static_cast<int>(plan.ngroups), p.spp);
}

void Renderer::camera_rays(int device, const CameraRec& cam, const RenderParams& p, uint32_t sample_base, double* rays_out, uint64_t* rng_out) {
    HIP_OK(hipSetDevice(device));
    const int nrows = band_local_rows(p.height, p.band_rows, p.band_count, p.band_index);
    if (nrows == 0) return;
    PassGeom g = make_pass_geom(p, nrows, 0);  // rt_render's geometry; no traversal, no stack
    const uint32_t k = static_cast<uint32_t>(p.spp);
    if (static_cast<uint64_t>(k) * g.npix_pad > kMaxPassSlots) throw std::runtime_error("too many camera rays for one call");
    g.k = k, g.sample_base = sample_base, g.P = k * g.npix_pad;
    const size_t ne = static_cast<size_t>(nrows) * static_cast<size_t>(p.width) * k;
    g.live = static_cast<uint32_t>(ne);
    // no scene, so no renderer: the null stream stands in for its own (a call there waits), and host buffers are staged
    // in a buffer of the call's, freed on return
    Call call(nullptr, nullptr, (p.flags & RT_OUT_DEVICE) != 0, p.stream, false);
    DeviceBuffer tmp;
    double* d_rays = nullptr;
    uint64_t* d_rng = nullptr;
    call.carve(tmp, [&](Carver& c) { d_rays = call.out(c, rays_out, 7 * ne), d_rng = call.out(c, rng_out, ne); }, 1);
    launch_camera_rays(call.st, g, cam, d_rays, d_rng);
    call.end();
    call.finish();
}

// Noise-target rendering (rt_render_noise_target; the kernels in noise_target.hip).  The base pass traces samples
// [0, min_spp) of every local pixel through the whole-image path; every refinement round then traces the next step_spp
// samples of the pixels the test left active, through the persistent kernel in pixel-list mode with entry-major slots
// (list_geom) and one sample_base: retirement is sticky, so every active pixel has the same count.  Every sum is
// continued in sample order, so a pixel with n samples equals rt_render's at spp = n.  The host reads the 4-byte entry
// count back once per round: it ends the loop, and sizes g.P, path_chunk, the grids and the split of a round that
// exceeds the pass workspace into sub-passes by sample range.
void Renderer::render_noise_target(const CameraRec& cam, const RenderParams& p, const NoiseParams& np, uint8_t* out_rgb, double* out_acc,
                                   int32_t* out_count, double* out_moments, RenderStats& stats, NoiseResult& result) {
    if (p.fp_mode != RT_FP64) throw std::runtime_error("fp_mode must be RT_FP64");
    upload();
    Impl& I = *impl_;
    Frame f{I, I.s64, cam, p};
    result = NoiseResult{};
    double* mom = nullptr;
    int32_t* count = nullptr;
    uint8_t* flag = nullptr;
    uint32_t *list_base = nullptr, *conv = nullptr;
    // samples per whole-image pass for the cap (a slot is its radiance record), not spread evenly: the base pass traces
    // min_spp; RT_PROFILE's marks are created as the rounds come
    if (!begin_frame(f, stats, p.spp, false, 0, [&](Carver& c) {
        f.w.res = c.take<ResRec>(f.Pmax);
        f.w.counters = c.take<uint32_t>(kCounterStride);
        f.w.segments = c.take<unsigned long long>(1);
        f.w.acc = c.take<double>(3 * f.local_pix);
        mom = c.take<double>(2 * f.local_pix);
        count = c.take<int32_t>(f.local_pix);
        flag = c.take<uint8_t>(f.local_pix);
        f.drgb = c.take<uint8_t>(3 * f.local_pix);
        list_base = c.take<uint32_t>(nt_list_words(f.local_pix));  // both lists with their count lines: allocation == memset
        conv = c.take<uint32_t>(1);
        f.w.pool = c.take<char>(pool_bytes(f.variant, I.num_cu));
    })) return;
    if (!f.mega) throw std::runtime_error("internal: noise-target rendering needs a persistent-path kernel");
    hipStream_t stream = f.stream;
    const Work& w = f.w;
    const size_t local_pix = f.local_pix;
    const uint32_t npix = static_cast<uint32_t>(local_pix), tile_pad = f.g.npix_pad;
    const double* res = reinterpret_cast<const double*>(w.res);
    uint32_t* lists[2] = {list_base + 64, list_base + nt_list_stride(local_pix) + 64};
    HIP_OK(hipMemsetAsync(w.acc, 0, sizeof(double) * 3 * local_pix, stream));
    HIP_OK(hipMemsetAsync(mom, 0, sizeof(double) * 2 * local_pix, stream));
    HIP_OK(hipMemsetAsync(flag, 0, local_pix, stream));
    HIP_OK(hipMemsetAsync(list_base, 0, 4 * nt_list_words(local_pix), stream));
    HIP_OK(hipMemsetAsync(conv, 0, 4, stream));
    // base pass: samples [0, min_spp) of every local pixel, tile-order slots
    const uint32_t min_spp = static_cast<uint32_t>(np.min_spp), cap_spp = static_cast<uint32_t>(p.spp), step = static_cast<uint32_t>(np.step_spp);
    PassGeom g = f.g;
    for (uint32_t sb = 0; sb < min_spp; sb += f.k) {
        g.sample_base = sb;
        g.k = std::min<uint32_t>(f.k, min_spp - sb);
        g.P = g.k * tile_pad;
        g.live = g.k * npix;
        run_pass(f, g);
        nt_accum_base(stream, res, g.k, tile_pad, g.tiles_x, p.width, f.nrows, w.acc, mom);
    }
    // refinement rounds
    uint64_t samples = static_cast<uint64_t>(local_pix) * min_spp;
    uint32_t n_done = min_spp, n_active = npix;
    const uint32_t* cur = nullptr;  // A_0: every local pixel
    int rounds = 0;
    for (int side = 0;; side ^= 1) {
        const uint32_t k_next = std::min<uint32_t>(step, cap_spp - n_done);
        uint32_t* next = lists[side];
        HIP_OK(hipMemsetAsync(next - 1, 0, 4, stream));
        nt_select(stream, cur, n_active, mom, flag, p.width, f.nrows, static_cast<int>(n_done), static_cast<int>(k_next), np.dilate, np.rel_tol,
                  np.lum_floor, next, count, conv);
        if (k_next == 0) break;  // every active pixel is at the cap
        HIP_OK(hipMemcpyAsync(&n_active, next - 1, 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (n_active == 0) break;
        if (n_active > npix) throw std::runtime_error("internal: noise-target list longer than the image");
        // sub-passes by sample range when the round's slots exceed the pass workspace (Pmax >= tile_pad >= n_active)
        const uint32_t kk = round_pass_samples(k_next, f.Pmax, n_active);
        for (uint32_t sb = 0; sb < k_next; sb += kk) {
            const uint32_t ks = std::min<uint32_t>(kk, k_next - sb);
            run_pass(f, list_geom(f.g, next, n_active, ks, n_done + sb, n_active * ks));
            nt_accum_list(stream, next, n_active, res, ks, w.acc, mom);
        }
        samples += static_cast<uint64_t>(n_active) * k_next;
        n_done += k_next;
        cur = next;
        ++rounds;
    }
    nt_finalize(stream, w.acc, count, f.drgb, npix);
    uint32_t nconv = 0;
    end_frame(f, stats, out_rgb, out_acc, [&]() {
        f.call.copy_out(out_count, count, sizeof(int32_t) * local_pix);
        f.call.copy_out(out_moments, mom, sizeof(double) * 2 * local_pix);
        HIP_OK(hipMemcpyAsync(&nconv, conv, 4, hipMemcpyDeviceToHost, stream));
    });
    stats.primary = result.samples = samples;
    result.rounds = rounds, result.converged_pixels = nconv;
}

// ------------------------------------------------------------------------------------------------ rt_scene_update_*
// What a scene's first update makes: the f64 box of every leaf slot's primitive from the host records (refit.h; a
// pad slot of the pair-aligned copy gets the empty box), uploaded once -- after that only the update kernels of the
// Refit kinds write it -- and the level ranges of the node array.
static void prepare_refit(const FlatScene& f, DeviceScene& ds) {
    if (ds.slot_box || ds.slot_refs.empty()) return;
    ds.level_begin = refit_levels(f.nodes, f.objs);
    std::vector<double> box(6 * ds.slot_refs.size());
    for (size_t i = 0; i < ds.slot_refs.size(); ++i) {
        double* b = box.data() + 6 * i;
        const uint32_t ref = ds.slot_refs[i], idx = primref_index(ref);
        if (ds.slot_pad[i]) {
            empty_box6(b);
            continue;
        }
        switch (primref_type(ref)) {
            case PRIM_SPHERE: sphere_box(f.spheres.at(idx), b); break;
            case PRIM_TRIANGLE: tri_box(f.tris.at(idx).p, b); break;
            case PRIM_RECT: rect_box(f.rects.at(idx), b); break;
            default: box_box(f.boxes.at(idx), b); break;
        }
    }
    ds.slot_box = const_cast<double*>(ds.upload(box));
    ds.slot_pad_dev = ds.upload(ds.slot_pad);
}

// What a scene's first material or texture update makes: with an image, the entry code of every material on the
// device.  (No slot boxes: nothing moves.)
static void prepare_appearance(const FlatScene& f, DeviceScene& ds) {
    if (!ds.lds_scene || ds.mat_entry_dev) return;
    std::vector<int32_t> entry(f.mats.size(), -1);
    bool complete = false;
    // f.primrefs: what build_lds_image walked (an image scene is never pair-aligned, so these are the device's slots)
    image_material_entries(f.primrefs.data(), f.primrefs.size(), f.spheres.data(), f.mats.data(), f.mats.size(), f.texs.data(), f.texs.size(),
                           entry.data(), complete);
    ds.mat_entry_dev = ds.upload(entry);
}

// The kind's job struct from the device scene and its launches: the kind's kernel, then for geometry the refit of every
// box (once a first update made the slot boxes) and, for spheres, the image's box planes from the refitted nodes; an
// appearance kind and the objects kind move no box and return after their kernels.  The
// arrays build_device_scene uploaded are const in the kernels' view only: the DeviceScene owns them.
static void enqueue_update(UpdateKind kind, hipStream_t st, const DeviceScene& ds, const double* v, uint32_t first, uint32_t n) {
    const auto& w = ds.view;
    uint8_t* image = ds.lds_scene ? const_cast<uint8_t*>(w.lds_image) : nullptr;
    switch (kind) {
        case UpdateKind::Triangles: {
            UpdateJob job{};
            job.p = v, job.first = first, job.n = n;
            job.primrefs = w.primrefs, job.objs = w.objs;
            job.n_slots = w.n_primrefs, job.n_objs = w.n_objs;
            job.tris = const_cast<TriRec*>(w.tris);
            job.leaf_tris = const_cast<TriRec*>(w.leaf_tris);
            job.leaf_tris112 = const_cast<TriRec112*>(w.leaf_tris112);
            job.leaf_prims = const_cast<PrimRec80*>(w.leaf_prims);
            job.obj_prims = const_cast<PrimRec80*>(w.obj_prims);
            job.slot_box = ds.slot_box;
            launch_update_tris(st, job);
            break;
        }
        case UpdateKind::Spheres: {
            SphereJob job{};
            job.s = v, job.first = first, job.n = n;
            job.primrefs = w.primrefs, job.slot_pad = ds.slot_pad_dev, job.objs = w.objs;
            job.n_slots = ds.slot_box ? w.n_primrefs : 0u, job.n_objs = w.n_objs;
            job.spheres = const_cast<SphereRec*>(w.spheres);
            job.leaf_prims = const_cast<PrimRec80*>(w.leaf_prims);
            job.obj_prims = const_cast<PrimRec80*>(w.obj_prims);
            job.slot_box = ds.slot_box;
            job.image = image;
            launch_update_spheres(st, job);
            break;
        }
        case UpdateKind::Rects:
        case UpdateKind::Boxes: {
            RigidJob job{};
            job.v = v, job.first = first, job.n = n;
            job.primrefs = w.primrefs, job.slot_pad = ds.slot_pad_dev, job.objs = w.objs;
            job.n_slots = ds.slot_box ? w.n_primrefs : 0u, job.n_objs = w.n_objs;  // (a scene without a BVH has no slots)
            job.rects = const_cast<RectRec*>(w.rects);
            job.boxes = const_cast<BoxRec*>(w.boxes);
            job.leaf_prims = const_cast<PrimRec80*>(w.leaf_prims);
            job.obj_prims = const_cast<PrimRec80*>(w.obj_prims);
            job.slot_box = ds.slot_box;
            (kind == UpdateKind::Rects ? launch_update_rects : launch_update_boxes)(st, job);
            break;
        }
        case UpdateKind::Objects: {
            ObjectJob job{};
            job.v = v, job.first = first, job.n = n;
            job.objs = const_cast<ObjRec*>(w.objs);
            launch_update_objects(st, job);
            return;  // no box depends on an object's parameters
        }
        default: {
            AppearanceJob job{};
            job.v = v, job.first = first, job.n = n;
            job.mats = const_cast<MatRec*>(w.mats);
            job.texs = const_cast<TexRec*>(w.texs);
            job.n_mats = w.n_mats;
            job.entry = ds.mat_entry_dev;
            job.image = image;
            (kind == UpdateKind::Materials ? launch_update_materials : launch_update_textures)(st, job);
            return;  // nothing moved
        }
    }
    if (ds.slot_box) launch_refit_levels(st, const_cast<BvhNode*>(w.nodes), w.n_nodes, ds.slot_box, w.n_primrefs, ds.level_begin);
    if (kind == UpdateKind::Spheres) launch_image_nodes(st, image, w.nodes, w.n_nodes);
}

// The update runner, what every rt_scene_update_* call shares: the call protocol over `count` values v of the caller's
// (a host v goes through the workspace), enqueue(stream, the values on the device) between the timing events, one more
// generation, and the wait rule.
template <class T, class Enqueue>
static void run_update(Renderer::Impl& I, const T* v, size_t count, bool device, void* stream, double* ms, Enqueue&& enqueue) {
    Call call(I.own_stream, I.ev, device, stream, ms != nullptr);
    const T* in = nullptr;
    call.carve(I.ws, [&](Carver& c) { in = call.in(c, v, count); }, 1);  // host values: through the workspace
    call.begin();
    enqueue(call.st, in);
    call.end();
    ++I.gen;
    const Call::Done done = call.finish();  // (a device call on the caller's stream without ms returns enqueued)
    if (ms) *ms = done.ms;
}

void Renderer::update(UpdateKind kind, const double* v, size_t first, size_t n, bool device, void* stream, double* ms) {
    const UpdateRow& row = update_row(kind);
    upload();
    Impl& I = *impl_;
    DeviceScene& ds = I.s64;
    if (n == 0) return;
    if (first + n > update_count(I.flat, kind)) throw std::runtime_error(std::string("update_") + row.nouns + ": range beyond the scene's " + row.nouns);
    if (row.cls == UpdateClass::Refit) prepare_refit(I.flat, ds);
    if (row.cls == UpdateClass::Appearance) prepare_appearance(I.flat, ds);
    run_update(I, v, row.width * n, device, stream, ms, [&](hipStream_t st, const double* in) {
        enqueue_update(kind, st, ds, in, static_cast<uint32_t>(first), static_cast<uint32_t>(n));
    });
}

// The texel pool is the only device copy of an image's bytes (device_scene.hip uploads it once; the LDS scene image holds
// materials' shading entries, no texel), so the update is one copy on the call's stream: rows [first_row, first_row +
// n_rows) of the image are contiguous in the pool.
void Renderer::update_texels(size_t image, const uint8_t* bytes, size_t first_row, size_t n_rows, bool device, void* stream, double* ms) {
    upload();
    Impl& I = *impl_;
    if (n_rows == 0) return;
    if (image >= I.flat.images.size()) throw std::runtime_error("update_texels: image beyond the scene's images");
    const ImageRec& im = I.flat.images[image];
    if (first_row + n_rows > static_cast<size_t>(im.h)) throw std::runtime_error("update_texels: rows beyond the image");
    const size_t pitch = static_cast<size_t>(im.w) * static_cast<size_t>(im.bpp);
    uint8_t* dst = const_cast<uint8_t*>(I.s64.view.texels) + im.offset + first_row * pitch;
    run_update(I, bytes, n_rows * pitch, device, stream, ms, [&](hipStream_t st, const uint8_t* in) {
        HIP_OK(hipMemcpyAsync(dst, in, n_rows * pitch, hipMemcpyDeviceToDevice, st));
    });
    ++I.texel_gen;
}

size_t Renderer::lds_image_get(bool rebuilt, uint8_t* out) {
    upload();
    Impl& I = *impl_;
    const DeviceScene& ds = I.s64;
    if (!ds.lds_scene) return 0;
    const size_t bytes = kLdsImageBytes + sizeof(TileReps);
    if (!out) return bytes;
    if (rebuilt) {
        uint32_t nmov = 0, tile_reps = 0;
        bool shade_ok = false;
        const std::vector<uint8_t> img = build_lds_image(current_flat(), nmov, shade_ok, tile_reps);
        if (img.size() != bytes) throw std::runtime_error("lds_image_get: the scene as the device holds it no longer qualifies for an image");
        std::memcpy(out, img.data(), bytes);
        return bytes;
    }
    HIP_OK(hipSetDevice(I.device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, ds.view.lds_image, bytes, hipMemcpyDeviceToHost));
    return bytes;
}

uint64_t Renderer::generation() const { return impl_->gen; }
uint64_t Renderer::texel_generation() const { return impl_->texel_gen; }

const FlatScene& Renderer::current_flat() {
    Impl& I = *impl_;
    if (I.fetched_gen == I.gen) return I.flat;
    HIP_OK(hipSetDevice(I.device));
    HIP_OK(hipDeviceSynchronize());  // an update enqueued on a caller's stream included
    const DeviceScene& ds = I.s64;
    std::vector<TriRec> tris(I.flat.tris.size());
    if (!tris.empty()) HIP_OK(hipMemcpy(tris.data(), ds.view.tris, sizeof(TriRec) * tris.size(), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < tris.size(); ++t) std::memcpy(I.flat.tris[t].p, tris[t].p, sizeof tris[t].p);
    std::vector<SphereRec> spheres(I.flat.spheres.size());
    if (!spheres.empty()) HIP_OK(hipMemcpy(spheres.data(), ds.view.spheres, sizeof(SphereRec) * spheres.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < spheres.size(); ++k) {
        std::memcpy(I.flat.spheres[k].c, spheres[k].c, sizeof spheres[k].c);
        I.flat.spheres[k].r = spheres[k].r;
    }
    // of a material and a texture, the fields an update writes -- not the solid colour the upload inlined into a
    // lambertian's, a light's or an isotropic's device record (MATF_SOLID)
    std::vector<MatRec> mats(I.flat.mats.size());
    if (!mats.empty()) HIP_OK(hipMemcpy(mats.data(), ds.view.mats, sizeof(MatRec) * mats.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < mats.size(); ++k) {
        MatRec& m = I.flat.mats[k];
        if (m.type == MAT_METAL) std::memcpy(m.albedo, mats[k].albedo, sizeof m.albedo), m.fuzz = mats[k].fuzz;
        if (m.type == MAT_DIELECTRIC) m.ir = mats[k].ir;
    }
    std::vector<TexRec> texs(I.flat.texs.size());
    if (!texs.empty()) HIP_OK(hipMemcpy(texs.data(), ds.view.texs, sizeof(TexRec) * texs.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < texs.size(); ++k) {
        TexRec& t = I.flat.texs[k];
        if (t.type == TEX_SOLID) std::memcpy(t.c, texs[k].c, sizeof t.c);
        if (t.type == TEX_NOISE) t.scale = texs[k].scale;
    }
    std::vector<RectRec> rects(I.flat.rects.size());
    if (!rects.empty()) HIP_OK(hipMemcpy(rects.data(), ds.view.rects, sizeof(RectRec) * rects.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < rects.size(); ++k) {
        RectRec& r = I.flat.rects[k];
        r.a0 = rects[k].a0, r.a1 = rects[k].a1, r.b0 = rects[k].b0, r.b1 = rects[k].b1, r.k = rects[k].k;
    }
    std::vector<BoxRec> boxes(I.flat.boxes.size());
    if (!boxes.empty()) HIP_OK(hipMemcpy(boxes.data(), ds.view.boxes, sizeof(BoxRec) * boxes.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < boxes.size(); ++k) {
        std::memcpy(I.flat.boxes[k].mn, boxes[k].mn, sizeof boxes[k].mn);
        std::memcpy(I.flat.boxes[k].mx, boxes[k].mx, sizeof boxes[k].mx);
    }
    // of an object, p only: the device's b may be a pair-aligned leaf code, the host's addresses the compiled slots
    std::vector<ObjRec> objs(I.flat.objs.size());
    if (!objs.empty()) HIP_OK(hipMemcpy(objs.data(), ds.view.objs, sizeof(ObjRec) * objs.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < objs.size(); ++k) std::memcpy(I.flat.objs[k].p, objs[k].p, sizeof objs[k].p);
    std::vector<BvhNode> nodes(I.flat.nodes.size());
    if (!nodes.empty()) HIP_OK(hipMemcpy(nodes.data(), ds.view.nodes, sizeof(BvhNode) * nodes.size(), hipMemcpyDeviceToHost));
    // the 24 box floats only: the device's leaf codes address the pair-aligned slots, the host's the compiled ones
    for (size_t k = 0; k < nodes.size(); ++k) std::memcpy(&I.flat.nodes[k], &nodes[k], 24 * sizeof(float));
    // the texel pool, when an rt_scene_update_texels call wrote it since the last fetch
    if (I.fetched_texel_gen != I.texel_gen && !I.flat.texels.empty())
        HIP_OK(hipMemcpy(I.flat.texels.data(), ds.view.texels, I.flat.texels.size(), hipMemcpyDeviceToHost));
    I.fetched_texel_gen = I.texel_gen;
    I.fetched_gen = I.gen;
    return I.flat;
}

void Renderer::bvh_get(void* nodes_out, uint32_t* primrefs_out, size_t& n_nodes, size_t& n_primrefs) {
    upload();
    const DeviceScene& ds = impl_->s64;
    n_nodes = ds.view.n_nodes, n_primrefs = ds.view.n_primrefs;
    if (!nodes_out && !primrefs_out) return;
    HIP_OK(hipDeviceSynchronize());
    if (nodes_out && n_nodes) HIP_OK(hipMemcpy(nodes_out, ds.view.nodes, sizeof(BvhNode) * n_nodes, hipMemcpyDeviceToHost));
    if (primrefs_out && n_primrefs) HIP_OK(hipMemcpy(primrefs_out, ds.view.primrefs, sizeof(uint32_t) * n_primrefs, hipMemcpyDeviceToHost));
}

int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
}  // namespace art

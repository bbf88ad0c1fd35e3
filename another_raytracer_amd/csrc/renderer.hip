// renderer.hip — Renderer (renderer.h): the workspace, the pass loops of rt_render and rt_render_noise_target, ray
// queries and guide buffers.  Host code only: every kernel is launched through launch.h / noise_target.h.
#include "renderer.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "launch.h"
#include "options.h"
#include "pass_plan.h"

namespace art {

struct Renderer::Impl {
    int device = 0;
    int num_cu = 256;
    hipStream_t own_stream = nullptr;
    FlatScene flat;
    DeviceScene s64;
    bool up64 = false;
    // workspace (grow-only)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};

    ~Impl() {
        s64.release();
        if (ws) (void)hipFree(ws);
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
    // Grow-only workspace.  The old buffer is released before the larger one is allocated (both need not fit), and
    // ws / ws_bytes describe a live allocation at every point: a failed hipMalloc leaves them at {nullptr, 0}, so the
    // next render allocates again instead of handing out offsets from a null base.
    void* workspace(size_t bytes) {
        // fault point (tests): option test.fault_workspace_bytes = N > 0 makes every workspace growth beyond N bytes
        // fail as a refused hipMalloc would, after the old buffer is released
        const double lim = opt(Opt::FaultWorkspaceBytes);
        if (bytes > ws_bytes) {
            if (lim > 0 && static_cast<double>(bytes) > lim) {
                if (ws) (void)hipFree(ws);
                ws = nullptr;
                ws_bytes = 0;
                throw std::runtime_error("workspace allocation of " + std::to_string(bytes) + " bytes refused (test.fault_workspace_bytes)");
            }
            if (ws) {
                void* old = ws;
                ws = nullptr;
                ws_bytes = 0;
                HIP_OK(hipFree(old));
            }
            void* p = nullptr;
            HIP_OK(hipMalloc(&p, bytes));
            ws = p;
            ws_bytes = bytes;
        }
        return ws;
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
size_t Renderer::scene_bytes() const { return impl_->s64.bytes; }
int Renderer::device() const { return impl_->device; }
const FlatScene& Renderer::flat() const { return impl_->flat; }

// ------------------------------------------------------------------------------------------------ pass setup
// What rt_render (render_impl) and rt_render_noise_target share.
// The geometry of the nrows local rows (band_local_rows) in 8x8-tile order; the per-pass fields (k, sample_base, P,
// live, cap, chunk, the pixel list) are the caller's.
static PassGeom make_pass_geom(const RenderParams& p, int nrows, const DeviceScene& ds) {
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
    g.stack = stack_rows(ds.max_stack);
    return g;
}
// Samples per whole-image pass, at most `spp`: the caller's samples_per_pass, or as many path slots of slot_bytes as
// half of the free HBM holds (plus the workspace this renderer already owns: a fixed point, no regrowth).  Every pass
// pays max_depth bounces of fixed launch/tail cost whatever its size, so on a 288 GB part the 1080p x 1024 spp frame
// runs in 3 passes instead of ~40 (5.6 -> 6.9 Gsamples/s measured).
// Slot ids, FastDiv operands and shard capacities are u32 and exact below 2^31: a pass never holds more than
// kMaxPassSlots slots, whether k comes from free memory or from the caller.
static uint32_t samples_per_pass(const Renderer::Impl& I, const RenderParams& p, const PassGeom& g, size_t slot_bytes, int spp) {
    size_t free_b = 0, total_b = 0;
    HIP_OK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t target = std::min<uint64_t>((free_b + I.ws_bytes) / 2 / slot_bytes, kMaxPassSlots);
    if (g.npix_pad > kMaxPassSlots) throw std::runtime_error("image too large for one pass (more than 2^31 padded pixels)");
    const uint64_t k_cap = std::max<uint64_t>(1, kMaxPassSlots / g.npix_pad);
    const uint64_t k64 = p.samples_per_pass > 0 ? static_cast<uint64_t>(p.samples_per_pass) : std::max<uint64_t>(1, target / g.npix_pad);
    return static_cast<uint32_t>(std::min<uint64_t>(std::min<uint64_t>(k64, k_cap), static_cast<uint64_t>(spp)));
}
static size_t al(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }  // workspace offsets: 256-B aligned
// One pass of g through the scene's persistent kernel; `counter` is the pass's slot counter.
static KernelId launch_persistent(int variant, const DeviceScene& ds, const Renderer::Impl& I, hipStream_t stream, PassGeom g,
                                  const CameraRec& cam, const Work& w, uint32_t* counter) {
    g.chunk = path_chunk(g.P, I.num_cu);
    if (variant == EXT_MEGA) {
        launch_paths(I.num_cu, stream, ds.view, g, cam, w, counter);
        return KernelId{kFeatSpheres, 0, 3};
    }
    return launch_paths_g(ds.features, ds.tex_basic, ds.tex_bary, ds.codes16, ds.leaf_shift, I.num_cu, stream, ds.view, g, cam, w, counter);
}
// After the frame's stream is synchronized: the fields every render reports.
static void fill_stats(RenderStats& stats, const Renderer::Impl& I, int passes, uint32_t k, uint64_t segments, int variant, const KernelId& kid,
                       uint64_t primary) {
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, I.ev[0], I.ev[1]));
    stats.ms = ms;
    stats.passes = passes;
    stats.samples_per_pass = static_cast<int>(k);
    stats.segments = segments;
    stats.extend_variant = variant;
    stats.kernel_features = kid.f;
    stats.kernel_textures = kid.tf;
    stats.kernel_lds_mode = kid.lm;
    stats.primary = primary;
}

static void render_impl(Renderer::Impl& I, DeviceScene& ds, const CameraRec& cam, const RenderParams& p, uint8_t* out_rgb,
                        double* out_acc, RenderStats& stats) {
    hipStream_t stream = p.stream ? static_cast<hipStream_t>(p.stream) : I.own_stream;
    for (int a = 0; a < 3; ++a) ds.view.bg[a] = p.background[a];  // engine::set_scene's background
    const int nrows = band_local_rows(p.height, p.band_rows, p.band_count, p.band_index);
    stats.local_rows = nrows;
    if (nrows == 0) return;
    PassGeom g = make_pass_geom(p, nrows, ds);
    const int variant = extend_variant(ds, p.flags);
    KernelId kid;  // the persistent kernel the passes ran (stays {0, 0, -1} for the wavefront variants)
    const bool mega = variant == EXT_MEGA || variant == EXT_MEGA_G;
    // (persistent paths keep the path state in registers: a slot is its radiance record only)
    const size_t slot_bytes = mega ? sizeof(ResRec) : sizeof(PathRec) + sizeof(HitRecD) + sizeof(ResRec) + 4u * (2u + kNumMatTypes) + 8u;
    // samples traced per pixel: spp, or parallel_images' 4 * (spp / 4) (engine.h:411-414)
    const bool images = (p.flags & RT_PARALLEL_IMAGES) != 0;
    const int spp_t = images ? 4 * (p.spp / 4) : p.spp;
    uint32_t k = samples_per_pass(I, p, g, slot_bytes, std::max(1, spp_t));
    const int npasses = static_cast<int>((std::max(1, spp_t) + k - 1) / k);
    k = static_cast<uint32_t>((std::max(1, spp_t) + npasses - 1) / npasses);  // spread evenly over the passes
    const uint64_t Pmax64 = static_cast<uint64_t>(k) * g.npix_pad;
    if (Pmax64 > kMaxPassSlots) throw std::runtime_error("internal: pass larger than 2^31 slots");
    const uint32_t Pmax = static_cast<uint32_t>(Pmax64);
    g.cap = shard_cap(Pmax);
    const size_t local_pix = static_cast<size_t>(nrows) * p.width;

    size_t off = 0;
    const size_t wf = mega ? 0u : 1u;  // wavefront-only buffers
    const size_t o_paths = off; off += wf * al(sizeof(PathRec) * Pmax);
    const size_t o_hits = off; off += wf * al(sizeof(HitRecD) * Pmax);
    const size_t o_res = off; off += al(sizeof(ResRec) * Pmax);
    const size_t o_a0 = off; off += wf * al(4ull * kShards * g.cap);
    const size_t o_a1 = off; off += wf * al(4ull * kShards * g.cap);
    const size_t o_mq = off; off += wf * al(4ull * kMatSegs * g.cap);
    // (at least 4 depth lines: the device-counted adaptive levels take one each)
    const size_t cnt_words = static_cast<size_t>(std::max(p.max_depth + 1, 4)) * kQueueKinds * kShards * kCounterStride;
    const size_t o_cnt = off; off += al(4ull * cnt_words);
    const size_t o_seg = off; off += al(sizeof(unsigned long long));
    const size_t o_acc = off; off += al(sizeof(double) * 3 * local_pix);
    const size_t o_rgb = off; off += al(3 * local_pix);
    const size_t o_qsum = off; off += images ? al(sizeof(double) * 3 * local_pix) : 0;  // parallel_images quarter sums
    const size_t o_pool = off; off += al(pool_bytes(variant, I.num_cu));
    // adaptive mode: int work frame, pixel list (<= 80 of every 144 pixels per level), square flags, list counter
    const bool adaptive = (p.flags & RT_ADAPTIVE) != 0;
    const size_t nsq_ws = adaptive ? local_pix / (kBig * kBig) : 0;
    const size_t o_adw = off; off += adaptive ? al(sizeof(int32_t) * 3 * local_pix) : 0;
    // four lists (one per level, at most 4 / 12 / 48 / 80 of every 144 pixels), each after its count word
    const size_t o_adl = off; off += adaptive ? al(4 * local_pix + 4 * 4 * 64) : 0;
    const size_t o_adf = off; off += adaptive ? al(21 * nsq_ws) : 0;
    const size_t o_adc = off; off += adaptive ? al(4) : 0;
    char* base = static_cast<char*>(I.workspace(off));
    int32_t* ad_work = reinterpret_cast<int32_t*>(base + o_adw);
    uint32_t* ad_list = reinterpret_cast<uint32_t*>(base + o_adl) + 64;  // host-counted levels: one list at a time
    uint8_t* ad_f0 = reinterpret_cast<uint8_t*>(base + o_adf);
    uint8_t* ad_f1 = ad_f0 + nsq_ws;
    uint8_t* ad_f2 = ad_f1 + 4 * nsq_ws;
    uint32_t* ad_count = reinterpret_cast<uint32_t*>(base + o_adc);

    Work w{};
    w.paths = reinterpret_cast<PathRec*>(base + o_paths);
    w.hits = reinterpret_cast<HitRecD*>(base + o_hits);
    w.res = reinterpret_cast<ResRec*>(base + o_res);
    w.active[0] = reinterpret_cast<uint32_t*>(base + o_a0);
    w.active[1] = reinterpret_cast<uint32_t*>(base + o_a1);
    w.mq = reinterpret_cast<uint32_t*>(base + o_mq);
    w.counters = reinterpret_cast<uint32_t*>(base + o_cnt);
    w.segments = reinterpret_cast<unsigned long long*>(base + o_seg);
    w.acc = reinterpret_cast<double*>(base + o_acc);
    w.pool = base + o_pool;
    uint8_t* drgb = reinterpret_cast<uint8_t*>(base + o_rgb);
    double* qsum = reinterpret_cast<double*>(base + o_qsum);

    const bool prof = (p.flags & RT_PROFILE) != 0;
    const int levels = adaptive ? 4 : 1;
    std::vector<hipEvent_t> evs;
    for (auto& e : I.ev)
        if (!e) HIP_OK(hipEventCreate(&e));
    if (prof) {  // event pool created before the timed region (a pixel-list level never needs more passes than k gives)
        evs.resize(static_cast<size_t>(levels) * npasses * p.max_depth * 3);
        for (auto& e : evs) HIP_OK(hipEventCreate(&e));
    }
    size_t ev_next = 0;
    auto mark = [&]() { HIP_OK(hipEventRecord(evs[ev_next++], stream)); };
    int passes_run = 0;
    uint64_t ext_launches = 0;
    int spp_done = 0;      // samples traced so far (progressive snapshots)
    bool stopped = false;  // the progressive callback ended the render early
    // Traces spp samples of every local pixel (list == nullptr) or of every entry of a device pixel list, into
    // w.acc (per local pixel, or per list entry).
    auto trace = [&](const uint32_t* list, uint32_t nlist) {
        g.list = list;
        g.nlist = nlist;
        uint32_t kk = k, npix = static_cast<uint32_t>(local_pix);
        if (list) {
            npix = nlist;
            g.npix_pad = (nlist + 63u) & ~63u;
            g.fd_npix = FastDiv::make(g.npix_pad);
            kk = std::max<uint32_t>(1, std::min<uint32_t>(static_cast<uint32_t>(p.spp), Pmax / std::max<uint32_t>(g.npix_pad, 64u)));
        }
        HIP_OK(hipMemsetAsync(w.acc, 0, sizeof(double) * 3 * npix, stream));
        if (images) HIP_OK(hipMemsetAsync(qsum, 0, sizeof(double) * 3 * npix, stream));
        for (uint32_t sb = 0; sb < static_cast<uint32_t>(spp_t); sb += kk) {
            g.sample_base = sb;
            g.k = std::min<uint32_t>(kk, static_cast<uint32_t>(spp_t) - sb);
            g.P = g.k * g.npix_pad;
            g.live = g.k * npix;
            // the persistent kernels use one counter (counter(w, 0, 0, 0)): clear its line, not the wavefront queues' 1.25 MB
            HIP_OK(hipMemsetAsync(w.counters, 0, mega ? 4u * kCounterStride : 4ull * cnt_words, stream));
            if (!mega) {
                for (int d = 0; d < p.max_depth; ++d)
                    bounce(ds, variant, I.num_cu, stream, g, cam, w, d, prof ? std::function<void()>(mark) : std::function<void()>());
                ext_launches += static_cast<uint64_t>(p.max_depth);
            } else if (p.max_depth > 0) {
                if (prof) mark();
                kid = launch_persistent(variant, ds, I, stream, g, cam, w, counter(w, 0, 0, 0));
                if (prof) { mark(); mark(); }
                ++ext_launches;
            }
            launch_accum(stream, g, w, images ? qsum : nullptr, static_cast<uint32_t>(spp_t / 4));
            ++passes_run;
            spp_done = static_cast<int>(sb + g.k);
            // progressive snapshot (whole-image traces only): write_color of the sums so far, with the samples so far
            if (!list && p.on_pass) {
                launch_finalize(stream, w.acc, drgb, npix, spp_done);
                const hipMemcpyKind kind = (p.flags & RT_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
                if (out_rgb) HIP_OK(hipMemcpyAsync(out_rgb, drgb, 3ull * npix, kind, stream));
                if (out_acc) HIP_OK(hipMemcpyAsync(out_acc, w.acc, sizeof(double) * 3 * npix, kind, stream));
                HIP_OK(hipStreamSynchronize(stream));
                if (!p.on_pass(spp_done)) {
                    stopped = true;
                    break;
                }
            }
        }
    };
#ifdef ART_TRACE
    {
        long long tp = -1, ts = -1;
        if (const char* t = std::getenv("ART_TRACE")) std::sscanf(t, "%lld:%lld", &tp, &ts);
        HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_pixel), &tp, sizeof tp));
        HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_sample), &ts, sizeof ts));
    }
#endif
    HIP_OK(hipEventRecord(I.ev[0], stream));
    HIP_OK(hipMemsetAsync(w.segments, 0, sizeof(unsigned long long), stream));
    if (p.max_depth == 0) HIP_OK(hipMemsetAsync(w.res, 0, sizeof(ResRec) * Pmax, stream));  // engine.h:451-452
    uint64_t traced = local_pix;
    uint32_t ad_counts[4] = {0, 0, 0, 0};  // the device-counted levels' entry counts (read back with the frame)
    bool dev_counted = false;
    const int sqx = p.width / kBig;  // adaptive mode: big squares per row, and in the local rows
    const uint32_t nsq = static_cast<uint32_t>(sqx) * static_cast<uint32_t>(nrows / kBig);
    if (!adaptive) {
        trace(nullptr, 0);
        const uint32_t npix = static_cast<uint32_t>(local_pix);
        launch_finalize(stream, w.acc, drgb, npix, stopped ? spp_done : p.spp);
    } else if (mega && k == static_cast<uint32_t>(spp_t) && !images && !p.on_pass) {
        // engine.h:151-333: levels 0..3 (k_adapt_* above), one pass each, with no host round trip: each level's list
        // count stays on the device (list[-1], PassGeom::list_mode 1), the persistent kernel reads it at its start and
        // the level's samples are entry-major (a wave traces one pixel's samples: coherent rays)
        const uint32_t caps[4] = {4 * nsq, 12 * nsq, 48 * nsq, 80 * nsq};
        uint32_t* lists[4];
        {
            uint32_t* at = reinterpret_cast<uint32_t*>(base + o_adl);
            for (int L = 0; L < 4; ++L) {
                lists[L] = at + 64;  // the count word at lists[L][-1]
                at = lists[L] + ((caps[L] + 63u) & ~63u);
            }
        }
        HIP_OK(hipMemsetAsync(base + o_adl, 0, 4 * local_pix + 4 * 4 * 64, stream));  // every count 0
        HIP_OK(hipMemsetAsync(ad_work, 0xFF, sizeof(int32_t) * 3 * local_pix, stream));  // the reference's -1 frame
        launch_adapt_corners(stream, lists[0], p.width, sqx, nsq);
        g.list_mode = 1;
        g.k = k;
        g.npix_pad = k;
        g.fd_npix = FastDiv::make(k);
        g.sample_base = 0;
        // one slot counter line per level (counter(w, level, 0, 0): the wavefront variants' depth lines, unused here),
        // cleared together before level 0 instead of one fill launch per level
        HIP_OK(hipMemsetAsync(w.counters, 0, 4ull * kQueueKinds * kShards * kCounterStride * 4, stream));
        for (int level = 0; level < 4; ++level) {
            g.list = lists[level];
            g.nlist = caps[level];                      // upper bounds: the kernels read the count
            g.P = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(caps[level]) * k, kMaxPassSlots));
            g.live = g.P;
            if (static_cast<uint64_t>(caps[level]) * k > Pmax) throw std::runtime_error("internal: adaptive level larger than the pass workspace");
            if (p.max_depth > 0) {
                if (prof) mark();
                kid = launch_persistent(variant, ds, I, stream, g, cam, w, counter(w, level, 0, 0));
                if (prof) { mark(); mark(); }
                ++ext_launches;
            }
            ++passes_run;
            launch_adapt_accum(stream, lists[level], caps[level], w.res, k, p.spp, ad_work);
            if (level == 3) break;
            launch_adapt_level(stream, level, ad_work, p.width, sqx, nsq, ad_f0, ad_f1, ad_f2, lists[level + 1], lists[level + 1] - 1);
        }
        launch_adapt_fill(stream, ad_work, drgb, p.width, nrows, sqx, ad_f0, ad_f1, ad_f2);
        for (int L = 0; L < 4; ++L) HIP_OK(hipMemcpyAsync(&ad_counts[L], lists[L] - 1, 4, hipMemcpyDeviceToHost, stream));
        dev_counted = true;
    } else {
        // engine.h:151-333: levels 0..3 (k_adapt_* above); the list sizes come back to the host between levels
        // (multi-pass levels, the wavefront variants)
        HIP_OK(hipMemsetAsync(ad_work, 0xFF, sizeof(int32_t) * 3 * local_pix, stream));  // the reference's -1 frame
        launch_adapt_corners(stream, ad_list, p.width, sqx, nsq);
        uint32_t n = 4 * nsq;
        traced = 0;
        for (int level = 0;; ++level) {
            trace(ad_list, n);
            launch_adapt_store(stream, ad_list, n, w.acc, p.spp, ad_work);
            traced += n;
            if (level == 3) break;
            HIP_OK(hipMemsetAsync(ad_count, 0, 4, stream));
            launch_adapt_level(stream, level, ad_work, p.width, sqx, nsq, ad_f0, ad_f1, ad_f2, ad_list, ad_count);
            HIP_OK(hipMemcpyAsync(&n, ad_count, 4, hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (n == 0) break;
        }
        launch_adapt_fill(stream, ad_work, drgb, p.width, nrows, sqx, ad_f0, ad_f1, ad_f2);
    }
    HIP_OK(hipGetLastError());
#ifdef ART_STATS
    {
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
    HIP_OK(hipEventRecord(I.ev[1], stream));
    const hipMemcpyKind kind_rgb = (p.flags & RT_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (out_rgb) HIP_OK(hipMemcpyAsync(out_rgb, drgb, 3 * local_pix, kind_rgb, stream));
    if (out_acc && !adaptive) HIP_OK(hipMemcpyAsync(out_acc, w.acc, sizeof(double) * 3 * local_pix, kind_rgb, stream));
    unsigned long long segs = 0;
    HIP_OK(hipMemcpyAsync(&segs, w.segments, sizeof segs, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (dev_counted) traced = static_cast<uint64_t>(ad_counts[0]) + ad_counts[1] + ad_counts[2] + ad_counts[3];
    fill_stats(stats, I, passes_run, k, segs, variant, kid, traced * static_cast<uint64_t>(stopped ? spp_done : spp_t));
    if (prof) {
        double ext_ms = 0, sh_ms = 0;
        for (size_t e = 0; e + 2 < ev_next; e += 3) {
            float a = 0, b = 0;
            HIP_OK(hipEventElapsedTime(&a, evs[e], evs[e + 1]));
            HIP_OK(hipEventElapsedTime(&b, evs[e + 1], evs[e + 2]));
            ext_ms += a;
            sh_ms += b;
        }
        stats.extend_ms = ext_ms;
        stats.shade_ms = sh_ms;
        stats.extend_launches = ext_launches;
        stats.shade_launches = variant == EXT_GLOBAL || variant == EXT_LDS ? ext_launches : 0;
        for (auto e : evs) (void)hipEventDestroy(e);
    }
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
    hipStream_t st = impl_->own_stream;
    const size_t in_b = sizeof(double) * 7 * n, t_b = sizeof(double) * n, n_b = sizeof(double) * 3 * n;
    char* base = static_cast<char*>(impl_->workspace(in_b + t_b + n_b));
    double* d_rays = reinterpret_cast<double*>(base);
    double* d_t = reinterpret_cast<double*>(base + in_b);
    double* d_n = reinterpret_cast<double*>(base + in_b + t_b);
    HIP_OK(hipMemcpyAsync(d_rays, rays, in_b, hipMemcpyHostToDevice, st));
    launch_trace_rays(ds, global_scene, st, d_rays, static_cast<uint32_t>(n), d_t, d_n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(t_out, d_t, t_b, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(n_out, d_n, n_b, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
}

void Renderer::query_rays(const double* rays, const double* t_max, size_t n, bool device, bool global_scene, bool any_hit, bool no_media,
                          void* stream, double* hits, uint8_t* occluded) {
    upload();
    Impl& I = *impl_;
    const DeviceScene& ds = I.s64;
    if (n == 0) return;
    if (n > (1u << 30)) throw std::runtime_error("too many rays");
    hipStream_t st = (device && stream) ? static_cast<hipStream_t>(stream) : I.own_stream;
    const uint32_t nn = static_cast<uint32_t>(n);
    if (device) {  // the caller's buffers as they are: no workspace, no copy
        if (any_hit) launch_occlude_rays(ds, global_scene, st, rays, t_max, nn, occluded);
        else launch_query_rays(ds, global_scene, st, rays, t_max, nn, no_media, hits);
        HIP_OK(hipGetLastError());
        if (!stream) HIP_OK(hipStreamSynchronize(st));  // the scene's own stream: nobody else can wait on it
        return;
    }
    // host buffers: [rays][t_max][hits or occluded] in the workspace (each part 8-byte aligned)
    const size_t in_b = sizeof(double) * 7 * n, tm_b = t_max ? sizeof(double) * n : 0;
    const size_t out_b = any_hit ? n : sizeof(double) * RT_HIT_DOUBLES * n;
    char* base = static_cast<char*>(I.workspace(in_b + tm_b + out_b));
    double* d_rays = reinterpret_cast<double*>(base);
    double* d_tm = t_max ? reinterpret_cast<double*>(base + in_b) : nullptr;
    char* d_out = base + in_b + tm_b;
    HIP_OK(hipMemcpyAsync(d_rays, rays, in_b, hipMemcpyHostToDevice, st));
    if (t_max) HIP_OK(hipMemcpyAsync(d_tm, t_max, tm_b, hipMemcpyHostToDevice, st));
    if (any_hit) launch_occlude_rays(ds, global_scene, st, d_rays, d_tm, nn, reinterpret_cast<uint8_t*>(d_out));
    else launch_query_rays(ds, global_scene, st, d_rays, d_tm, nn, no_media, reinterpret_cast<double*>(d_out));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(any_hit ? static_cast<void*>(occluded) : static_cast<void*>(hits), d_out, out_b, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
}

void Renderer::render_guides(const CameraRec& cam, const RenderParams& p, double* guides, double* rays_out) {
    upload();
    Impl& I = *impl_;
    const DeviceScene& ds = I.s64;
    hipStream_t st = p.stream ? static_cast<hipStream_t>(p.stream) : I.own_stream;
    GuideGeom g{p.width, p.height, band_local_rows(p.height, p.band_rows, p.band_count, p.band_index), p.band_rows, p.band_count, p.band_index};
    if (g.rows == 0) return;
    const size_t npix = static_cast<size_t>(g.rows) * p.width;
    const size_t g_b = sizeof(double) * 10 * npix, r_b = sizeof(double) * 7 * npix;
    const bool dev_out = (p.flags & RT_OUT_DEVICE) != 0;
    double* d_g = guides;
    double* d_r = rays_out;
    if (!dev_out) {  // host buffers: the kernel writes the workspace, copied out below
        char* base = static_cast<char*>(I.workspace(g_b + (rays_out ? r_b : 0)));
        d_g = reinterpret_cast<double*>(base);
        d_r = rays_out ? reinterpret_cast<double*>(base + g_b) : nullptr;
    }
    launch_guides(ds, p.flags, st, g, cam, d_g, d_r);
    HIP_OK(hipGetLastError());
    if (!dev_out) {
        HIP_OK(hipMemcpyAsync(guides, d_g, g_b, hipMemcpyDeviceToHost, st));
        if (rays_out) HIP_OK(hipMemcpyAsync(rays_out, d_r, r_b, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
}

void Renderer::render(const CameraRec& cam, const RenderParams& p, uint8_t* out_rgb, double* out_acc, RenderStats& stats) {
    if (p.fp_mode != RT_FP64) throw std::runtime_error("fp_mode must be RT_FP64");
    upload();
    render_impl(*impl_, impl_->s64, cam, p, out_rgb, out_acc, stats);
}

// Noise-target rendering (rt_render_noise_target; render_impl's sibling, the kernels in noise_target.hip).  The base
// pass traces samples [0, min_spp) of every local pixel through the whole-image path; every refinement round then
// traces the next step_spp samples of the pixels the test left active, through the persistent kernel in pixel-list
// mode with entry-major slots (PassGeom::list_mode 1) and one sample_base: retirement is sticky, so every active pixel
// has the same count.  Every sum is continued in sample order, so a pixel with n samples equals rt_render's at spp = n.
// The host reads the 4-byte entry count back once per round: it ends the loop, and sizes g.P, path_chunk, the grids and
// the split of a round that exceeds the pass workspace into sub-passes by sample range.
void Renderer::render_noise_target(const CameraRec& cam, const RenderParams& p, const NoiseParams& np, uint8_t* out_rgb, double* out_acc,
                                   int32_t* out_count, double* out_moments, RenderStats& stats, NoiseResult& result) {
    if (p.fp_mode != RT_FP64) throw std::runtime_error("fp_mode must be RT_FP64");
    upload();
    Impl& I = *impl_;
    DeviceScene& ds = I.s64;
    hipStream_t stream = p.stream ? static_cast<hipStream_t>(p.stream) : I.own_stream;
    for (int a = 0; a < 3; ++a) ds.view.bg[a] = p.background[a];
    const int nrows = band_local_rows(p.height, p.band_rows, p.band_count, p.band_index);
    stats.local_rows = nrows;
    result = NoiseResult{};
    if (nrows == 0) return;
    PassGeom g = make_pass_geom(p, nrows, ds);
    const uint32_t tile_pad = g.npix_pad;
    const int variant = extend_variant(ds, p.flags);
    if (variant != EXT_MEGA && variant != EXT_MEGA_G) throw std::runtime_error("internal: noise-target rendering needs a persistent-path kernel");
    KernelId kid;
    // samples per whole-image pass (a slot is its radiance record); not spread evenly: the base pass traces min_spp
    const uint32_t k = samples_per_pass(I, p, g, sizeof(ResRec), p.spp);
    const uint32_t Pmax = k * tile_pad;  // <= kMaxPassSlots
    g.cap = shard_cap(Pmax);
    const size_t local_pix = static_cast<size_t>(nrows) * p.width;
    const uint32_t npix = static_cast<uint32_t>(local_pix);

    size_t off = 0;
    const size_t o_res = off; off += al(sizeof(ResRec) * Pmax);
    const size_t o_cnt = off; off += al(4ull * kCounterStride);
    const size_t o_seg = off; off += al(sizeof(unsigned long long));
    const size_t o_acc = off; off += al(sizeof(double) * 3 * local_pix);
    const size_t o_mom = off; off += al(sizeof(double) * 2 * local_pix);
    const size_t o_count = off; off += al(sizeof(int32_t) * local_pix);
    const size_t o_flag = off; off += al(local_pix);
    const size_t o_rgb = off; off += al(3 * local_pix);
    const size_t list_bytes = 4 * nt_list_words(local_pix);  // both lists with their count lines: allocation == memset
    const size_t o_list = off; off += al(list_bytes);
    const size_t o_conv = off; off += al(4);
    const size_t o_pool = off; off += al(pool_bytes(variant, I.num_cu));
    char* base = static_cast<char*>(I.workspace(off));

    Work w{};
    w.res = reinterpret_cast<ResRec*>(base + o_res);
    w.counters = reinterpret_cast<uint32_t*>(base + o_cnt);
    w.segments = reinterpret_cast<unsigned long long*>(base + o_seg);
    w.acc = reinterpret_cast<double*>(base + o_acc);
    w.pool = base + o_pool;
    const double* res = reinterpret_cast<const double*>(w.res);
    double* mom = reinterpret_cast<double*>(base + o_mom);
    int32_t* count = reinterpret_cast<int32_t*>(base + o_count);
    uint8_t* flag = reinterpret_cast<uint8_t*>(base + o_flag);
    uint8_t* drgb = reinterpret_cast<uint8_t*>(base + o_rgb);
    uint32_t* lists[2] = {reinterpret_cast<uint32_t*>(base + o_list) + 64, reinterpret_cast<uint32_t*>(base + o_list) + nt_list_stride(local_pix) + 64};
    uint32_t* conv = reinterpret_cast<uint32_t*>(base + o_conv);

    const bool prof = (p.flags & RT_PROFILE) != 0;
    for (auto& e : I.ev)
        if (!e) HIP_OK(hipEventCreate(&e));
    std::vector<hipEvent_t> evs;  // RT_PROFILE: two per path launch (the number of rounds is not known beforehand)
    struct EvGuard {
        std::vector<hipEvent_t>& v;
        ~EvGuard() { for (auto e : v) (void)hipEventDestroy(e); }
    } ev_guard{evs};
    auto mark = [&]() {
        hipEvent_t e = nullptr;
        HIP_OK(hipEventCreate(&e));
        evs.push_back(e);
        HIP_OK(hipEventRecord(e, stream));
    };
    int passes_run = 0;
    uint64_t launches = 0;
    // one pass of g (whole image or list) through the persistent kernel
    auto paths = [&]() {
        HIP_OK(hipMemsetAsync(w.counters, 0, 4u * kCounterStride, stream));
        ++passes_run;
        if (p.max_depth == 0) return;  // the records stay 0 (engine.h:451-452)
        if (prof) mark();
        kid = launch_persistent(variant, ds, I, stream, g, cam, w, counter(w, 0, 0, 0));
        if (prof) mark();
        ++launches;
    };

    HIP_OK(hipEventRecord(I.ev[0], stream));
    HIP_OK(hipMemsetAsync(w.segments, 0, sizeof(unsigned long long), stream));
    if (p.max_depth == 0) HIP_OK(hipMemsetAsync(w.res, 0, sizeof(ResRec) * Pmax, stream));
    HIP_OK(hipMemsetAsync(w.acc, 0, sizeof(double) * 3 * local_pix, stream));
    HIP_OK(hipMemsetAsync(mom, 0, sizeof(double) * 2 * local_pix, stream));
    HIP_OK(hipMemsetAsync(flag, 0, local_pix, stream));
    HIP_OK(hipMemsetAsync(base + o_list, 0, list_bytes, stream));
    HIP_OK(hipMemsetAsync(conv, 0, 4, stream));
    // base pass: samples [0, min_spp) of every local pixel, tile-order slots
    const uint32_t min_spp = static_cast<uint32_t>(np.min_spp), cap_spp = static_cast<uint32_t>(p.spp), step = static_cast<uint32_t>(np.step_spp);
    for (uint32_t sb = 0; sb < min_spp; sb += k) {
        g.sample_base = sb;
        g.k = std::min<uint32_t>(k, min_spp - sb);
        g.P = g.k * tile_pad;
        g.live = g.k * npix;
        paths();
        nt_accum_base(stream, res, g.k, tile_pad, g.tiles_x, p.width, nrows, w.acc, mom);
    }
    // refinement rounds
    uint64_t samples = static_cast<uint64_t>(local_pix) * min_spp;
    uint32_t n_done = min_spp, n_active = npix;
    const uint32_t* cur = nullptr;  // A_0: every local pixel
    int rounds = 0;
    g.list_mode = 1;
    for (int side = 0;; side ^= 1) {
        const uint32_t k_next = std::min<uint32_t>(step, cap_spp - n_done);
        uint32_t* next = lists[side];
        HIP_OK(hipMemsetAsync(next - 1, 0, 4, stream));
        nt_select(stream, cur, n_active, mom, flag, p.width, nrows, static_cast<int>(n_done), static_cast<int>(k_next), np.dilate, np.rel_tol, np.lum_floor,
                  next, count, conv);
        if (k_next == 0) break;  // every active pixel is at the cap
        HIP_OK(hipMemcpyAsync(&n_active, next - 1, 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (n_active == 0) break;
        if (n_active > npix) throw std::runtime_error("internal: noise-target list longer than the image");
        g.list = next;
        g.nlist = n_active;
        // sub-passes by sample range when the round's slots exceed the pass workspace (Pmax >= tile_pad >= n_active)
        const uint32_t kk = std::min<uint32_t>(k_next, Pmax / n_active);
        for (uint32_t sb = 0; sb < k_next; sb += kk) {
            g.sample_base = n_done + sb;
            g.k = std::min<uint32_t>(kk, k_next - sb);
            g.npix_pad = g.k;
            g.fd_npix = FastDiv::make(g.k);
            g.P = n_active * g.k;
            g.live = g.P;
            paths();
            nt_accum_list(stream, next, n_active, res, g.k, w.acc, mom);
        }
        samples += static_cast<uint64_t>(n_active) * k_next;
        n_done += k_next;
        cur = next;
        ++rounds;
    }
    nt_finalize(stream, w.acc, count, drgb, npix);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(I.ev[1], stream));
    const hipMemcpyKind kind = (p.flags & RT_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (out_rgb) HIP_OK(hipMemcpyAsync(out_rgb, drgb, 3 * local_pix, kind, stream));
    if (out_acc) HIP_OK(hipMemcpyAsync(out_acc, w.acc, sizeof(double) * 3 * local_pix, kind, stream));
    if (out_count) HIP_OK(hipMemcpyAsync(out_count, count, sizeof(int32_t) * local_pix, kind, stream));
    if (out_moments) HIP_OK(hipMemcpyAsync(out_moments, mom, sizeof(double) * 2 * local_pix, kind, stream));
    unsigned long long segs = 0;
    uint32_t nconv = 0;
    HIP_OK(hipMemcpyAsync(&segs, w.segments, sizeof segs, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(&nconv, conv, 4, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    fill_stats(stats, I, passes_run, k, segs, variant, kid, samples);
    if (prof) {
        double ext_ms = 0;
        for (size_t e = 0; e + 1 < evs.size(); e += 2) {
            float a = 0;
            HIP_OK(hipEventElapsedTime(&a, evs[e], evs[e + 1]));
            ext_ms += a;
        }
        stats.extend_ms = ext_ms;
        stats.extend_launches = launches;
    }
    result.rounds = rounds;
    result.converged_pixels = nconv;
    result.samples = samples;
}

int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
}  // namespace art

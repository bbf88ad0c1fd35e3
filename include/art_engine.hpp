// include/art_engine.hpp — C++ host surface of the reference's engine path over the C ABI (include/art.h).
//
// The reference's src/main.cpp (main.cpp:25-60) drives three classes: scene_manager::build (scene_manager.cpp:260),
// camera (camera.h:8-36) and engine<W,H,C> (engine.h:19-54).  This header restates that surface for C++ callers on
// top of libart.so, so a reference-style main() changes its includes and nothing else:
//
//     art::scene_manager sm("assets");                           // asset_dir: earthmap.jpg, models/...
//     art::scene world = sm.build("1");                          // scene_alias::random
//     art::camera cam(world.lookfrom, world.lookat, {0, 1, 0}, world.vfov, double(W) / H, world.aperture, 10.0, 0, 1);
//     art::engine<W, H, 3> eng(cam, art::engine_mode::parallel_stripes);
//     eng.set_scene(world, world.background);
//     std::vector<uint8_t> image(W * H * 3);
//     int ms = eng.run(image.data());                            // -1 on an empty world, like engine.h:32-36
//     art::imageio::save_image("output.png", W, H, 3, image.data());
//
// Header-only; no HIP, torch or ROCm header is needed by the caller (link with -lart).  Errors surface as the
// reference's exceptions: std::logic_error for an adaptive size off the 12-px grid (engine.h:178-179) and for an
// unknown scene (scene_manager.cpp:351), std::runtime_error for everything else (message from rt_last_error()).
#ifndef ART_ENGINE_HPP
#define ART_ENGINE_HPP

#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <exception>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "art.h"

namespace art {

struct vec3 {  // core/vec3.h (storage only: the arithmetic runs inside libart)
    double e[3] = {0, 0, 0};
    double x() const { return e[0]; }
    double y() const { return e[1]; }
    double z() const { return e[2]; }
};
using point3 = vec3;
using color = vec3;

inline void check(int rc, const char* where) {
    if (rc < 0) throw std::runtime_error(std::string(where) + ": " + rt_last_error());
}

enum class engine_mode { single, adaptive, parallel_stripes, parallel_images };  // engine.h:10-16

class camera {  // camera.h:8-36 (the basis is built inside libart from the same nine arguments, in f64)
public:
    camera(point3 lookfrom, point3 lookat, vec3 vup, double vfov, double aspect_ratio, double aperture, double focus_dist,
           double time0 = 0, double time1 = 0) {
        for (int k = 0; k < 3; ++k) {
            c_.lookfrom[k] = lookfrom.e[k];
            c_.lookat[k] = lookat.e[k];
            c_.vup[k] = vup.e[k];
        }
        c_.vfov = vfov;
        c_.aspect = aspect_ratio;
        c_.aperture = aperture;
        c_.focus_dist = focus_dist;
        c_.time0 = time0;
        c_.time1 = time1;
    }
    const rt_camera& raw() const { return c_; }

private:
    rt_camera c_{};
};

struct scene {  // scene_manager.h:6-14; `objects` is the compiled world on one device
    std::shared_ptr<rt_scene> objects;
    color background;
    point3 lookfrom, lookat;
    double vfov = 40.0, aperture = 0.0;
    rt_scene_info info{};
};

class scene_manager {  // scene_manager.h:29-42
public:
    explicit scene_manager(std::string asset_dir, int device = 0) : assets_(std::move(asset_dir)), device_(device) {}
    // aliases "1".."9" or the scene_alias names, plus "c1", "cow", "dino" 
    scene build(const std::string& alias) const {
        rt_scene* raw = nullptr;
        const int rc = rt_scene_build(alias.c_str(), assets_.c_str(), device_, &raw);
        if (rc < 0) {
            const std::string msg = rt_last_error();
            if (msg.find("unkwnown scene requested") != std::string::npos) throw std::logic_error(msg);
            throw std::runtime_error("scene_manager::build(" + alias + "): " + msg);
        }
        return wrap(raw);
    }
    // A scene written by save_scene (rt_scene_load: the flat-scene file, no OBJ parsing, image decoding or BVH build).
    scene load(const std::string& path) const {
        rt_scene* raw = nullptr;
        check(rt_scene_load(path.c_str(), device_, &raw), "scene_manager::load");
        return wrap(raw);
    }

private:
    static scene wrap(rt_scene* raw) {
        scene s;
        s.objects = std::shared_ptr<rt_scene>(raw, rt_scene_destroy);
        check(rt_scene_info_get(raw, &s.info), "rt_scene_info_get");
        for (int k = 0; k < 3; ++k) {
            s.lookfrom.e[k] = s.info.lookfrom[k];
            s.lookat.e[k] = s.info.lookat[k];
            s.background.e[k] = s.info.background[k];
        }
        s.vfov = s.info.vfov;
        s.aperture = s.info.aperture;
        return s;
    }
    std::string assets_;
    int device_;
};

// Writes a built or loaded scene as a versioned flat-scene file (rt_scene_save); scene_manager::load reads it back.
// Process-wide library options (rt_option_set / rt_option_get: builder experiments, the RCCL deadline, test fault points)
inline void set_option(const std::string& name, double value) { check(rt_option_set(name.c_str(), value), "rt_option_set"); }
inline double get_option(const std::string& name) {
    double v = 0;
    check(rt_option_get(name.c_str(), &v), "rt_option_get");
    return v;
}
inline void save_scene(const scene& world, const std::string& path) { check(rt_scene_save(world.objects.get(), path.c_str()), "save_scene"); }

// Ray queries (rt_query_rays): hittable_list::hit(r, 0.001, t_max[i], rec) of n rays {ox, oy, oz, dx, dy, dz, time}
// against a compiled world.  query_rays fills n * RT_HIT_DOUBLES doubles (t, normal, point, u, v, front_face, prim, mat;
// include/art.h); occluded_rays n bytes, 1 where some non-medium primitive lies in [0.001, t_max[i]].  t_max may be
// nullptr (+inf).  flags: RT_GLOBAL_SCENE, RT_Q_NO_MEDIA (closest mode), and RT_OUT_DEVICE with `stream` for device
// buffers -- the call then returns once the kernel is enqueued on a non-null stream.
inline void query_rays(const scene& world, const double* rays, const double* t_max, std::int64_t n, double* hits, std::int32_t flags = 0,
                       void* stream = nullptr) {
    rt_query_params q{};
    q.flags = flags & ~RT_Q_ANY_HIT;
    q.stream = stream;
    check(rt_query_rays(world.objects.get(), &q, rays, t_max, n, hits, nullptr), "query_rays");
}
inline void occluded_rays(const scene& world, const double* rays, const double* t_max, std::int64_t n, std::uint8_t* occluded,
                          std::int32_t flags = 0, void* stream = nullptr) {
    rt_query_params q{};
    q.flags = flags | RT_Q_ANY_HIT;
    q.stream = stream;
    check(rt_query_rays(world.objects.get(), &q, rays, t_max, n, nullptr, occluded), "occluded_rays");
}

// Path-traced radiance along caller-given rays (rt_radiance_rays): radiance receives n * 3 doubles, the f64 sums over
// o.spp paths per ray in sample order (sums, like the renderer's per-pixel sums; not means).  Path (i, s) runs
// engine::_ray_color (engine.h:447-466) on the PCG state rng[i * spp + s] when rng is given, else on the stream keyed
// (seed, id_base + i, sample_base + s).  flags: RT_GLOBAL_SCENE, and RT_OUT_DEVICE with `stream` for device buffers.
struct radiance_options {
    int spp = 1, max_depth = 50;
    std::uint64_t seed = 0, id_base = 0;
    std::uint32_t sample_base = 0;
    color background;
    std::int32_t flags = 0;
    void* stream = nullptr;
};
inline void radiance_rays(const scene& world, const double* rays, std::int64_t n, double* radiance, const radiance_options& o = {},
                          const std::uint64_t* rng = nullptr, rt_stats* stats = nullptr) {
    rt_radiance_params q{};
    q.flags = o.flags;
    q.spp = o.spp;
    q.max_depth = o.max_depth;
    q.sample_base = o.sample_base;
    q.seed = o.seed;
    q.id_base = o.id_base;
    q.stream = o.stream;
    for (int k = 0; k < 3; ++k) q.background[k] = o.background.e[k];
    check(rt_radiance_rays(world.objects.get(), &q, rays, rng, n, radiance, stats), "radiance_rays");
}
// radiance_rays' paths with the adjoint weights (n * 3 doubles) and the exact gradient of sum_i <weights[i], radiance[i]>
// with respect to the solid texture colours, the metal albedos and the background (rt_radiance_grad): grad_textures
// (T x RT_TEXTURE_DOUBLES) and grad_materials (M x RT_MATERIAL_DOUBLES) in the getters' row layout, grad_background (3);
// radiance and each gradient buffer may be nullptr.
inline void radiance_grad(const scene& world, const double* rays, const double* weights, std::int64_t n, double* radiance, double* grad_textures,
                          double* grad_materials, double* grad_background, const radiance_options& o = {}, const std::uint64_t* rng = nullptr,
                          rt_stats* stats = nullptr) {
    rt_radiance_params q{};
    q.flags = o.flags;
    q.spp = o.spp;
    q.max_depth = o.max_depth;
    q.sample_base = o.sample_base;
    q.seed = o.seed;
    q.id_base = o.id_base;
    q.stream = o.stream;
    for (int k = 0; k < 3; ++k) q.background[k] = o.background.e[k];
    check(rt_radiance_grad(world.objects.get(), &q, rays, rng, weights, n, radiance, grad_textures, grad_materials, grad_background, stats),
          "radiance_grad");
}
// ... and with respect to the texels of the world's image textures (rt_radiance_grad_texels): grad_texels (N x 3 doubles,
// N the texels of every image in scene_images' order; may be nullptr, and the call is then the one above) receives the
// derivative with respect to each texel's value, byte / 255 per channel.
inline void radiance_grad(const scene& world, const double* rays, const double* weights, std::int64_t n, double* radiance, double* grad_textures,
                          double* grad_materials, double* grad_background, double* grad_texels, const radiance_options& o = {},
                          const std::uint64_t* rng = nullptr, rt_stats* stats = nullptr) {
    rt_radiance_params q{};
    q.flags = o.flags;
    q.spp = o.spp;
    q.max_depth = o.max_depth;
    q.sample_base = o.sample_base;
    q.seed = o.seed;
    q.id_base = o.id_base;
    q.stream = o.stream;
    for (int k = 0; k < 3; ++k) q.background[k] = o.background.e[k];
    check(rt_radiance_grad_texels(world.objects.get(), &q, rays, rng, weights, n, radiance, grad_textures, grad_materials, grad_background, grad_texels,
                                  stats),
          "radiance_grad");
}
// The renderer's own camera rays as data (rt_camera_rays): entry (y * width + x) * k + j of rays_out (7 doubles) and
// rng_out (may be nullptr) is the ray render_engine starts at pixel (x, y) for sample sample_base + j with `seed`, and the
// PCG state after the camera's draws -- so the in-order sum of radiance_rays over a pixel's entries is that pixel's sum.
inline void camera_rays(const camera& cam, int width, int height, int k, double* rays_out, std::uint64_t* rng_out, std::uint32_t sample_base = 0,
                        std::uint64_t seed = 0, int device = 0) {
    rt_params p{};
    p.width = width;
    p.height = height;
    p.spp = k;
    p.seed = seed;
    p.fp_mode = RT_FP64;
    p.band_rows = height;
    p.band_count = 1;
    check(rt_camera_rays(&cam.raw(), &p, sample_base, device, rays_out, rng_out), "camera_rays");
}

// Many cameras of one scene in one call (rt_render_views): out_rgb8 receives cams.size() frames of width x height x 3
// bytes, view-major, each equal to render_engine's frame for that camera bit for bit; out_accum (may be nullptr) the f64
// sums.  seeds: one per view, or empty for o.seed in every view.  flags: RT_GLOBAL_SCENE, and RT_OUT_DEVICE with `stream`
// for device buffers.  Every view has the same size, samples and depth; frames of more than 2^31 paths take render_engine.
struct views_options {
    int spp = 100, max_depth = 50;
    std::uint64_t seed = 0;
    color background;
    std::int32_t flags = 0;
    void* stream = nullptr;
};
inline void render_views(const scene& world, const std::vector<camera>& cams, int width, int height, std::uint8_t* out_rgb8,
                         const views_options& o = {}, const std::vector<std::uint64_t>& seeds = {}, double* out_accum = nullptr,
                         rt_stats* stats = nullptr) {
    if (!seeds.empty() && seeds.size() != cams.size()) throw std::invalid_argument("render_views: one seed per camera, or none");
    std::vector<rt_camera> raw;
    raw.reserve(cams.size());
    for (const camera& c : cams) raw.push_back(c.raw());
    rt_params p{};
    p.width = width;
    p.height = height;
    p.spp = o.spp;
    p.max_depth = o.max_depth;
    p.seed = o.seed;
    p.fp_mode = RT_FP64;
    p.band_rows = height;
    p.band_count = 1;
    p.flags = o.flags;
    p.stream = o.stream;
    for (int k = 0; k < 3; ++k) p.background[k] = o.background.e[k];
    check(rt_render_views(world.objects.get(), raw.data(), seeds.empty() ? nullptr : seeds.data(), static_cast<std::int32_t>(raw.size()), &p, out_rgb8,
                          out_accum, stats),
          "render_views");
}

namespace detail {
// rt_scene_update_*: the params from flags and stream, the call, the check
template <class Fn>
void scene_update(Fn fn, const char* where, const scene& world, const double* v, std::int64_t first, std::int64_t n, std::int32_t flags, void* stream,
                  double* ms) {
    rt_update_params u{};
    u.flags = flags;
    u.stream = stream;
    check(fn(world.objects.get(), &u, v, first, n, ms), where);
}
// rt_scene_*_get: the count, then the fill of `width` doubles per record; get(out, cap) makes the call (out null: the count)
template <class Get>
std::vector<double> scene_get(Get get, const char* where, int width) {
    const std::int64_t n = get(nullptr, 0);
    check(n < 0 ? static_cast<int>(n) : RT_OK, where);
    std::vector<double> v(static_cast<std::size_t>(width * n));
    if (n > 0) {
        const std::int64_t got = get(v.data(), n);
        check(got < 0 ? static_cast<int>(got) : RT_OK, where);
    }
    return v;
}
// ... with the optional descriptions, desc_width int32 per record
template <class Fn>
std::vector<double> scene_get(Fn fn, const char* where, const scene& world, int width, std::vector<std::int32_t>* desc, int desc_width) {
    return scene_get([&](double* out, std::int64_t cap) {
        if (desc) desc->assign(static_cast<std::size_t>(desc_width * cap), 0);
        return fn(world.objects.get(), out, desc && out ? desc->data() : nullptr, cap);
    }, where, width);
}
}  // namespace detail

// Deforming a compiled scene (rt_scene_update_triangles).  scene_triangles: the world's triangles as it holds them now, 9
// doubles each (pt1, pt2, pt3) in compiled order.  update_triangles: new vertices p (9 doubles each, that order) for
// triangles [first, first + n), then a refit of every BVH box on the device; every later call on the world gives the bits
// a world compiled fresh from those vertices gives.  flags: RT_OUT_DEVICE with `stream` for a device buffer -- the call
// then returns once enqueued on a non-null stream unless ms (the device time of the update, milliseconds) is asked for.
inline std::vector<double> scene_triangles(const scene& world) {
    return detail::scene_get([&](double* out, std::int64_t cap) { return rt_scene_triangles_get(world.objects.get(), out, cap); }, "scene_triangles", 9);
}
inline void update_triangles(const scene& world, const double* p, std::int64_t first, std::int64_t n, std::int32_t flags = 0, void* stream = nullptr,
                             double* ms = nullptr) {
    detail::scene_update(rt_scene_update_triangles, "update_triangles", world, p, first, n, flags, stream, ms);
}
// The same for spheres (rt_scene_update_spheres): 4 doubles each (cx, cy, cz, r; center0 of a moving_sphere, whose motion
// stays) in compiled order; the BVH boxes and, where the world runs out of it, the LDS scene image are refitted.
inline std::vector<double> scene_spheres(const scene& world) {
    return detail::scene_get([&](double* out, std::int64_t cap) { return rt_scene_spheres_get(world.objects.get(), out, cap); }, "scene_spheres", 4);
}
inline void update_spheres(const scene& world, const double* s, std::int64_t first, std::int64_t n, std::int32_t flags = 0, void* stream = nullptr,
                           double* ms = nullptr) {
    detail::scene_update(rt_scene_update_spheres, "update_spheres", world, s, first, n, flags, stream, ms);
}
// A compiled world's materials and textures (rt_scene_materials_get / rt_scene_textures_get): RT_MATERIAL_DOUBLES /
// RT_TEXTURE_DOUBLES doubles per row, indexed by the graph's material / texture ids; desc (optional) receives the rows
// {type, tex} / {type, even, odd}.  update_materials / update_textures write new values for rows [first, first + n); each
// record takes what its type uses, and every device copy of a value follows (rt_scene_update_materials).
inline std::vector<double> scene_materials(const scene& world, std::vector<std::int32_t>* desc = nullptr) {
    return detail::scene_get(rt_scene_materials_get, "scene_materials", world, RT_MATERIAL_DOUBLES, desc, 2);
}
inline std::vector<double> scene_textures(const scene& world, std::vector<std::int32_t>* desc = nullptr) {
    return detail::scene_get(rt_scene_textures_get, "scene_textures", world, RT_TEXTURE_DOUBLES, desc, 3);
}
inline void update_materials(const scene& world, const double* m, std::int64_t first, std::int64_t n, std::int32_t flags = 0, void* stream = nullptr,
                             double* ms = nullptr) {
    detail::scene_update(rt_scene_update_materials, "update_materials", world, m, first, n, flags, stream, ms);
}
inline void update_textures(const scene& world, const double* t, std::int64_t first, std::int64_t n, std::int32_t flags = 0, void* stream = nullptr,
                            double* ms = nullptr) {
    detail::scene_update(rt_scene_update_textures, "update_textures", world, t, first, n, flags, stream, ms);
}
// A compiled world's images (rt_scene_images_get): {w, h, bpp} per image in the order the world's images were made, and
// (optional) each image's first global texel -- the rows of radiance_grad's texel gradient.  scene_texels: the h * w * bpp
// bytes of one image, top row first, as the world holds them now.  update_texels: new bytes for rows [first_row, first_row
// + n_rows) of one image in the same layout (rt_scene_update_texels); flags, stream and ms as update_triangles.
inline std::vector<std::int32_t> scene_images(const scene& world, std::vector<std::int64_t>* first_texel = nullptr) {
    const std::int64_t n = rt_scene_images_get(world.objects.get(), nullptr, nullptr, 0);
    check(n < 0 ? static_cast<int>(n) : RT_OK, "scene_images");
    std::vector<std::int32_t> desc(static_cast<std::size_t>(3 * n));
    if (first_texel) first_texel->assign(static_cast<std::size_t>(n), 0);
    if (n > 0) {
        const std::int64_t got = rt_scene_images_get(world.objects.get(), desc.data(), first_texel ? first_texel->data() : nullptr, n);
        check(got < 0 ? static_cast<int>(got) : RT_OK, "scene_images");
    }
    return desc;
}
inline std::vector<std::uint8_t> scene_texels(const scene& world, std::int32_t image) {
    const std::int64_t bytes = rt_scene_texels_get(world.objects.get(), image, nullptr, 0);
    check(bytes < 0 ? static_cast<int>(bytes) : RT_OK, "scene_texels");
    std::vector<std::uint8_t> out(static_cast<std::size_t>(bytes));
    if (bytes > 0) {
        const std::int64_t got = rt_scene_texels_get(world.objects.get(), image, out.data(), bytes);
        check(got < 0 ? static_cast<int>(got) : RT_OK, "scene_texels");
    }
    return out;
}
inline void update_texels(const scene& world, std::int32_t image, const std::uint8_t* texels, std::int64_t first_row, std::int64_t n_rows,
                          std::int32_t flags = 0, void* stream = nullptr, double* ms = nullptr) {
    rt_update_params u{};
    u.flags = flags;
    u.stream = stream;
    check(rt_scene_update_texels(world.objects.get(), &u, image, texels, first_row, n_rows, ms), "update_texels");
}
// A compiled world's rects, boxes and objects (rt_scene_rects_get / _boxes_get / _objects_get): RT_RECT_DOUBLES (a0, a1,
// b0, b1, k), RT_BOX_DOUBLES (min xyz, max xyz) and RT_OBJECT_DOUBLES (the parameters p: a translate's offset, a
// rotate_y's sin and cos, a constant_medium's -1 / density) per row in compiled order; desc (optional) receives the rows
// {axis, mat} / {mat} / {kind, a, b, world slot}.  update_rects / update_boxes write new extents for rows
// [first, first + n) and refit the BVH boxes; update_objects moves, turns or thins an instance without any refit
// (rt_scene_update_rects).
inline std::vector<double> scene_rects(const scene& world, std::vector<std::int32_t>* desc = nullptr) {
    return detail::scene_get(rt_scene_rects_get, "scene_rects", world, RT_RECT_DOUBLES, desc, 2);
}
inline std::vector<double> scene_boxes(const scene& world, std::vector<std::int32_t>* desc = nullptr) {
    return detail::scene_get(rt_scene_boxes_get, "scene_boxes", world, RT_BOX_DOUBLES, desc, 1);
}
inline std::vector<double> scene_objects(const scene& world, std::vector<std::int32_t>* desc = nullptr) {
    return detail::scene_get(rt_scene_objects_get, "scene_objects", world, RT_OBJECT_DOUBLES, desc, 4);
}
inline void update_rects(const scene& world, const double* v, std::int64_t first, std::int64_t n, std::int32_t flags = 0, void* stream = nullptr,
                         double* ms = nullptr) {
    detail::scene_update(rt_scene_update_rects, "update_rects", world, v, first, n, flags, stream, ms);
}
inline void update_boxes(const scene& world, const double* v, std::int64_t first, std::int64_t n, std::int32_t flags = 0, void* stream = nullptr,
                         double* ms = nullptr) {
    detail::scene_update(rt_scene_update_boxes, "update_boxes", world, v, first, n, flags, stream, ms);
}
inline void update_objects(const scene& world, const double* v, std::int64_t first, std::int64_t n, std::int32_t flags = 0, void* stream = nullptr,
                           double* ms = nullptr) {
    detail::scene_update(rt_scene_update_objects, "update_objects", world, v, first, n, flags, stream, ms);
}

// The engine with a runtime image size (the reference fixes W, H, C at compile time: engine<W,H,C> below); samples
// per pixel and max depth are the reference's tracer_constants (tracer_constants.h:12-13) as arguments with the same
// defaults.
class render_engine {
public:
    render_engine(int width, int height, const camera& cam, engine_mode mode, int samples_per_pixel = 100, int max_depth = 50,
                  uint64_t seed = 0)
        : w_(width), h_(height), cam_(cam), mode_(mode), spp_(samples_per_pixel), max_depth_(max_depth), seed_(seed) {}

    void set_scene(const scene& world, color background) {  // engine.h:24-28
        world_ = world;
        background_ = background;
    }

    // engine.h:30-54: blocking, fills W*H*3 bytes (row 0 = top); returns the elapsed milliseconds, or -1 for an empty
    // world.  single and parallel_stripes compute the same image; adaptive traces corners and interpolates
    // (engine.h:96-333); parallel_images sums four float images of spp/4 samples (engine.h:378-445).
    int run(std::uint8_t* out) {
        if (!world_.objects || world_.info.objects == 0) {
            std::fprintf(stderr, "Invalid input scene!\n");
            return -1;
        }
        const rt_params p = params();
        const int rc = rt_render(world_.objects.get(), &cam_.raw(), &p, out, nullptr, &stats_);
        if (rc == RT_E_INVALID && mode_ == engine_mode::adaptive) throw std::logic_error(rt_last_error());
        check(rc, "engine::run");
        return static_cast<int>(stats_.ms);
    }
    // Progressive rendering (the reference's live preview, gui.cpp:25-58, headless): passes of samples_per_pass samples
    // per pixel (0: spp / 8 rounded up); after each, `on_pass(samples_done, rgb)` sees the frame write_color'ed with the
    // samples so far (in `out`); returning false stops there.  The last snapshot equals run()'s image bit for bit.
    int run_progressive(std::uint8_t* out, const std::function<bool(int samples_done, const std::uint8_t* rgb)>& on_pass,
                        int samples_per_pass = 0) {
        if (!world_.objects || world_.info.objects == 0) {
            std::fprintf(stderr, "Invalid input scene!\n");
            return -1;
        }
        rt_params p = params();
        if (p.flags & (RT_ADAPTIVE | RT_PARALLEL_IMAGES)) throw std::logic_error("engine::run_progressive: adaptive and parallel_images are not progressive");
        p.samples_per_pass = samples_per_pass;
        struct ctx_t {
            const std::function<bool(int, const std::uint8_t*)>* fn;
            std::exception_ptr err;
        } ctx{&on_pass, nullptr};
        auto tramp = [](void* user, int32_t done, int32_t, const std::uint8_t* rgb, const double*) -> int {
            auto* c = static_cast<ctx_t*>(user);
            try {
                return (*c->fn)(done, rgb) ? 0 : 1;
            } catch (...) {  // no exception crosses the C ABI: stop the render, rethrow after it returns
                c->err = std::current_exception();
                return 1;
            }
        };
        const int rc = rt_render_progressive(world_.objects.get(), &cam_.raw(), &p, out, nullptr, tramp, &ctx, &stats_);
        if (ctx.err) std::rethrow_exception(ctx.err);
        check(rc, "engine::run_progressive");
        return static_cast<int>(stats_.ms);
    }
    // Denoised render (rt_render_denoised; the reference has no denoiser): two half-renders of spp / 2 samples (seeds
    // seed and seed + 1), the first-hit guide pass and the variance-guided a-trous filter, all on the device.  `out`
    // receives write_color of the filtered frame, `color` (optional, W*H*3 doubles) the frame itself; `dn` NULL = the
    // filter's defaults.  spp must be even; single / parallel_stripes only.  Returns the elapsed milliseconds of the
    // whole call, or -1 for an empty world.
    int run_denoised(std::uint8_t* out, double* color = nullptr, const rt_denoise_params* dn = nullptr) {
        if (!world_.objects || world_.info.objects == 0) {
            std::fprintf(stderr, "Invalid input scene!\n");
            return -1;
        }
        const rt_params p = params();
        if (p.flags & (RT_ADAPTIVE | RT_PARALLEL_IMAGES)) throw std::logic_error("engine::run_denoised: adaptive and parallel_images frames are not denoised");
        check(rt_render_denoised(world_.objects.get(), &cam_.raw(), &p, dn, out, color, &stats_), "engine::run_denoised");
        return static_cast<int>(stats_.ms);
    }
    // Noise-target render (rt_render_noise_target; the reference gives every pixel samples_per_pixel samples): every
    // pixel is traced until the standard error of its mean luminance is within noise.rel_tol, up to spp samples.  `out`
    // receives write_color of every pixel's sums with its own count, `counts` (optional, W*H) the samples per pixel;
    // `noise` zero-initialised = the defaults.  single / parallel_stripes only.  Returns the rounds, the converged pixels
    // and the samples traced (rounds = -1 for an empty world); stats().ms holds the elapsed milliseconds.
    rt_noise_result run_noise_target(std::uint8_t* out, const rt_noise_params& noise = rt_noise_params{}, std::int32_t* counts = nullptr) {
        rt_noise_result res{};
        if (!world_.objects || world_.info.objects == 0) {
            std::fprintf(stderr, "Invalid input scene!\n");
            res.rounds = -1;
            return res;
        }
        const rt_params p = params();
        if (p.flags & (RT_ADAPTIVE | RT_PARALLEL_IMAGES)) throw std::logic_error("engine::run_noise_target: adaptive and parallel_images frames have no noise target");
        check(rt_render_noise_target(world_.objects.get(), &cam_.raw(), &p, &noise, out, nullptr, counts, nullptr, &stats_, &res), "engine::run_noise_target");
        return res;
    }
    const rt_stats& stats() const { return stats_; }

private:
    rt_params params() const {
        rt_params p{};
        p.width = w_;
        p.height = h_;
        p.spp = spp_;
        p.max_depth = max_depth_;
        p.seed = seed_;
        p.fp_mode = RT_FP64;
        p.band_rows = h_;
        p.band_count = 1;
        p.band_index = 0;
        p.flags = mode_ == engine_mode::adaptive ? RT_ADAPTIVE : mode_ == engine_mode::parallel_images ? RT_PARALLEL_IMAGES : 0;
        for (int k = 0; k < 3; ++k) p.background[k] = background_.e[k];
        return p;
    }
    int w_, h_;
    camera cam_;
    engine_mode mode_;
    int spp_, max_depth_;
    uint64_t seed_;
    scene world_;
    color background_;
    rt_stats stats_{};
};

template <int W, int H, int C>
class engine : public render_engine {  // engine.h:19-54
    static_assert(C == 3, "libart writes RGB8 (color.h:6-22)");

public:
    engine(const camera& cam, engine_mode mode, int samples_per_pixel = 100, int max_depth = 50, uint64_t seed = 0)
        : render_engine(W, H, cam, mode, samples_per_pixel, max_depth, seed) {}
};

// The reference's CPU-parallel drivers (engine.h:335-376: row stripes on threads) over several GPUs of one process:
// the scene on every device, one RCCL communicator per device, each device rendering its row bands and one
// ncclGather assembling the frame on devices[0] (rt_render_multi).  Same image as engine::run for any device count.
class multi_engine {
public:
    multi_engine(const std::string& alias, const std::string& asset_dir, const std::vector<int>& devices, int width, int height,
                 const camera& cam, int samples_per_pixel = 100, int max_depth = 50, uint64_t seed = 0, int band_rows = 16)
        : w_(width), h_(height), cam_(cam), spp_(samples_per_pixel), max_depth_(max_depth), seed_(seed), band_rows_(band_rows) {
        rt_multi* raw = nullptr;
        check(rt_multi_create(alias.c_str(), asset_dir.c_str(), devices.data(), static_cast<int>(devices.size()), &raw), "multi_engine");
        m_ = std::shared_ptr<rt_multi>(raw, rt_multi_destroy);
    }
    void set_background(color background) { background_ = background; }
    // W*H*3 bytes of host memory, row 0 = top; returns the wall milliseconds of the call
    int run(std::uint8_t* out) {
        rt_params p{};
        p.width = w_;
        p.height = h_;
        p.spp = spp_;
        p.max_depth = max_depth_;
        p.seed = seed_;
        p.fp_mode = RT_FP64;
        p.band_rows = band_rows_;
        p.band_count = 1;
        p.band_index = 0;
        for (int k = 0; k < 3; ++k) p.background[k] = background_.e[k];
        check(rt_render_multi(m_.get(), &cam_.raw(), &p, out, &stats_), "multi_engine::run");
        return static_cast<int>(stats_.ms);
    }
    const rt_stats& stats() const { return stats_; }

private:
    std::shared_ptr<rt_multi> m_;
    int w_, h_;
    camera cam_;
    int spp_, max_depth_;
    uint64_t seed_;
    int band_rows_;
    color background_;
    rt_stats stats_{};
};

namespace imageio {  // utils/imageio.h: save_image writes a PNG (zlib deflate; stb_image_write in the reference)
// imageio::load_image (imageio.cpp:11-15, stbi_load(path, &w, &h, &c, 0)): JPEG / PNG through libart's decoder,
// the bytes stb_image v2.27 returns (rt_image_load); throws std::runtime_error on an unreadable file.
inline std::vector<std::uint8_t> load_image(const std::string& path, int& width, int& height, int& channels) {
    int32_t w = 0, h = 0, c = 0;
    std::uint8_t* px = nullptr;
    check(rt_image_load(path.c_str(), &w, &h, &c, &px), "imageio::load_image");
    std::vector<std::uint8_t> out(px, px + static_cast<size_t>(w) * h * c);
    rt_image_free(px);
    width = w;
    height = h;
    channels = c;
    return out;
}
inline bool save_image(const std::string& path, int width, int height, int bytes_per_pixel, const std::uint8_t* data) {
    const int color_type = bytes_per_pixel == 1 ? 0 : bytes_per_pixel == 2 ? 4 : bytes_per_pixel == 3 ? 2 : 6;
    std::vector<std::uint8_t> raw;
    const size_t stride = static_cast<size_t>(width) * bytes_per_pixel;
    raw.reserve((stride + 1) * height);
    for (int y = 0; y < height; ++y) {
        raw.push_back(0);  // filter: none
        raw.insert(raw.end(), data + y * stride, data + (y + 1) * stride);
    }
    uLongf zlen = compressBound(static_cast<uLong>(raw.size()));
    std::vector<std::uint8_t> z(zlen);
    if (compress2(z.data(), &zlen, raw.data(), static_cast<uLong>(raw.size()), 6) != Z_OK) return false;
    z.resize(zlen);
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    auto be32 = [](std::uint32_t v) {
        return std::vector<std::uint8_t>{std::uint8_t(v >> 24), std::uint8_t(v >> 16), std::uint8_t(v >> 8), std::uint8_t(v)};
    };
    auto chunk = [&](const char* tag, const std::vector<std::uint8_t>& payload) {
        std::vector<std::uint8_t> body(tag, tag + 4);
        body.insert(body.end(), payload.begin(), payload.end());
        const auto len = be32(static_cast<std::uint32_t>(payload.size()));
        const auto crc = be32(static_cast<std::uint32_t>(crc32(0L, body.data(), static_cast<uInt>(body.size()))));
        std::fwrite(len.data(), 1, 4, f);
        std::fwrite(body.data(), 1, body.size(), f);
        std::fwrite(crc.data(), 1, 4, f);
    };
    static const std::uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::fwrite(sig, 1, 8, f);
    std::vector<std::uint8_t> ihdr = be32(static_cast<std::uint32_t>(width));
    const auto h = be32(static_cast<std::uint32_t>(height));
    ihdr.insert(ihdr.end(), h.begin(), h.end());
    ihdr.insert(ihdr.end(), {8, static_cast<std::uint8_t>(color_type), 0, 0, 0});
    chunk("IHDR", ihdr);
    chunk("IDAT", z);
    chunk("IEND", {});
    return std::fclose(f) == 0;
}
}  // namespace imageio

}  // namespace art

#endif  // ART_ENGINE_HPP

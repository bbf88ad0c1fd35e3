// abi.cpp — the extern "C" boundary (include/art.h).  No exception crosses it.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "art.h"
#include "denoise.h"
#include "imagedec.h"
#include "multi.h"
#include "renderer.h"
#include "scenefile.h"
#include "objmesh.h"
#include "options.h"
#include "pass_plan.h"
#include "scene.h"

namespace art {
int device_count();  // renderer.hip
}

struct rt_scene {
    art::SceneGraph graph;       // empty for a scene loaded from a flat-scene file (has_graph false)
    bool has_graph = true;
    art::FlatScene flat;
    art::SceneView view;         // scene_manager::build's lookfrom / lookat / vfov / aperture
    int device = 0;
    std::unique_ptr<art::Renderer> renderer;  // created on first render (scene build/dump works without a GPU)
    art::Renderer& device_renderer() { return renderer ? *renderer : *(renderer = std::make_unique<art::Renderer>(flat, device)); }
    // the rt_scene_update_* calls leave `flat` stale: the renderer counts the updates, and whoever reads from `flat` what
    // an update writes (the getters through get_begin, rt_scene_save) takes it from the device first
    uint64_t synced = 0, synced_texels = 0;
    bool updated() const { return renderer && renderer->generation() > 0; }
    void sync_flat() {
        if (!renderer || renderer->generation() == synced) return;
        const art::FlatScene& now = renderer->current_flat();
        flat.spheres = now.spheres;
        flat.tris = now.tris;
        flat.nodes = now.nodes;
        flat.mats = now.mats;
        flat.texs = now.texs;
        flat.rects = now.rects;
        flat.boxes = now.boxes;
        flat.objs = now.objs;
        if (synced_texels != renderer->texel_generation()) flat.texels = now.texels;  // (the pool is large: only after a texel update)
        synced = renderer->generation(), synced_texels = renderer->texel_generation();
    }
};
struct rt_graph {
    art::SceneGraph g;
};
struct rt_multi {
    art::SceneGraph graph;
    art::FlatScene flat;
    std::unique_ptr<art::MultiRenderer> renderer;
};

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
template <class F>
int guard(int code_on_exception, F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(RT_E_INTERNAL, "out of memory");
    } catch (const std::exception& e) {
        return fail(code_on_exception, e.what());
    } catch (...) {
        return fail(RT_E_INTERNAL, "unknown error");
    }
}
art::Vec3 v3(const double* p) { return art::Vec3(p[0], p[1], p[2]); }
bool valid_params(const rt_params* p, std::string& why) {
    if (!p) { why = "params is NULL"; return false; }
    if (p->width < 2 || p->height < 2) { why = "width and height must be >= 2 (u = (i + r)/(W-1), engine.h:62-63)"; return false; }
    if (p->spp < 1) { why = "spp must be >= 1"; return false; }
    if (p->max_depth < 0) { why = "max_depth must be >= 0"; return false; }
    if (p->band_rows < 1 || p->band_count < 1 || p->band_index < 0 || p->band_index >= p->band_count) {
        why = "band partition must satisfy band_rows >= 1, band_count >= 1, 0 <= band_index < band_count";
        return false;
    }
    if (p->fp_mode != RT_FP64) { why = "fp_mode must be RT_FP64 (0): the reference's double arithmetic is the only mode"; return false; }
    if (static_cast<int64_t>(p->width) * p->height > (int64_t(1) << 31)) { why = "image too large"; return false; }
    return true;
}
art::RenderParams render_params(const rt_params* p) {
    art::RenderParams rp;
    rp.width = p->width;
    rp.height = p->height;
    rp.spp = p->spp;
    rp.max_depth = p->max_depth;
    rp.seed = p->seed;
    rp.fp_mode = p->fp_mode;
    rp.band_rows = p->band_rows;
    rp.band_count = p->band_count;
    rp.band_index = p->band_index;
    rp.samples_per_pass = p->samples_per_pass;
    rp.flags = p->flags;
    rp.stream = p->stream;
    for (int c = 0; c < 3; ++c) rp.background[c] = p->background[c];
    return rp;
}
void fill_stats(const art::RenderStats& st, rt_stats* stats) {
    if (!stats) return;
    std::memset(stats, 0, sizeof *stats);
    stats->segments = st.segments;
    stats->primary = st.primary;
    stats->ms = st.ms;
    stats->extend_ms = st.extend_ms;
    stats->shade_ms = st.shade_ms;
    stats->extend_launches = st.extend_launches;
    stats->shade_launches = st.shade_launches;
    stats->passes = st.passes;
    stats->samples_per_pass = st.samples_per_pass;
    stats->local_rows = st.local_rows;
    stats->extend_variant = st.extend_variant;
    stats->kernel_features = st.kernel_features;
    stats->kernel_textures = st.kernel_textures;
    stats->kernel_lds_mode = st.kernel_lds_mode;
}
art::CameraRec camera_of(const rt_camera* cam) {
    return art::make_camera(cam->lookfrom, cam->lookat, cam->vup, cam->vfov, cam->aspect, cam->aperture, cam->focus_dist, cam->time0, cam->time1);
}
int multi_from_graph(art::SceneGraph graph, const int* devices, int ngpus, rt_multi** out) {
    if (!devices || ngpus < 1) return fail(RT_E_INVALID, "devices must list ngpus >= 1 device ids");
    auto m = std::make_unique<rt_multi>();
    m->graph = std::move(graph);
    m->flat = art::compile_scene(m->graph);
    m->renderer = std::make_unique<art::MultiRenderer>(m->flat, std::vector<int>(devices, devices + ngpus));
    *out = m.release();
    return RT_OK;
}
int scene_from_graph(art::SceneGraph graph, int device, rt_scene** out) {
    auto s = std::make_unique<rt_scene>();
    s->graph = std::move(graph);
    s->flat = art::compile_scene(s->graph);
    for (int a = 0; a < 3; ++a) {
        s->view.lookfrom[a] = s->graph.lookfrom[a];
        s->view.lookat[a] = s->graph.lookat[a];
    }
    s->view.vfov = s->graph.vfov;
    s->view.aperture = s->graph.aperture;
    s->device = device;
    *out = s.release();
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
int rt_option_set(const char* name, double value) {
    if (!name) {
        art::opt_reset_all();
        return RT_OK;
    }
    const char* why = "";
    if (!art::opt_set(name, value, &why)) return fail(RT_E_INVALID, std::string("rt_option_set(") + name + "): " + why);
    return RT_OK;
}
int rt_option_get(const char* name, double* value) {
    if (!name || !value) return fail(RT_E_INVALID, "rt_option_get: name and value must be non-NULL");
    if (!art::opt_get(name, value)) return fail(RT_E_INVALID, std::string("rt_option_get(") + name + "): unknown option");
    return RT_OK;
}
const char* rt_last_error(void) { return g_err.c_str(); }
int rt_device_count(void) {
    return guard(RT_E_DEVICE, [] { return art::device_count(); });
}

int rt_scene_build(const char* name, const char* asset_dir, int device, rt_scene** out) {
    if (!name || !out) return fail(RT_E_INVALID, "name and out must be non-NULL");
    *out = nullptr;
    return guard(RT_E_SCENE, [&] {
        art::SceneGraph g;
        art::build_builtin_scene(g, name, asset_dir ? asset_dir : "assets");
        return scene_from_graph(std::move(g), device, out);
    });
}

static void fill_info(const art::SceneView& view, const art::FlatScene& flat, rt_scene_info* info) {
    std::memset(info, 0, sizeof *info);
    for (int a = 0; a < 3; ++a) {
        info->lookfrom[a] = view.lookfrom[a];
        info->lookat[a] = view.lookat[a];
        info->background[a] = flat.background[a];
    }
    info->vfov = view.vfov;
    info->aperture = view.aperture;
    info->spheres = static_cast<int64_t>(flat.spheres.size());
    info->triangles = static_cast<int64_t>(flat.tris.size());
    info->rects = static_cast<int64_t>(flat.rects.size());
    info->boxes = static_cast<int64_t>(flat.boxes.size());
    info->bvh_nodes = static_cast<int64_t>(flat.nodes.size());
    info->objects = static_cast<int64_t>(flat.world.size());
    info->materials = static_cast<int64_t>(flat.mats.size());
    info->textures = static_cast<int64_t>(flat.texs.size());
    info->has_media = flat.has_media ? 1 : 0;
    info->max_bvh_depth = flat.max_bvh_depth;
}

int rt_scene_info_get(const rt_scene* s, rt_scene_info* info) {
    if (!s || !info) return fail(RT_E_INVALID, "scene and info must be non-NULL");
    fill_info(s->view, s->flat, info);
    if (s->renderer) info->device_bytes_f64 = s->renderer->scene_bytes();
    return RT_OK;
}

size_t rt_scene_dump(const rt_scene* s, char* buf, size_t cap) {
    if (!s) {
        fail(RT_E_INVALID, "scene is NULL");
        return 0;
    }
    if (!s->has_graph) {
        fail(RT_E_INVALID, "a scene loaded from a flat-scene file has no object graph to dump");
        return 0;
    }
    if (s->updated()) {
        fail(RT_E_SCENE, "the scene was updated (rt_scene_update_triangles, _spheres, _materials, _textures, _texels, _rects, _boxes, _objects): its object graph no longer describes it");
        return 0;
    }
    try {
        std::string d = art::dump_scene(s->graph);
        if (buf && cap) {
            size_t n = std::min(cap - 1, d.size());
            std::memcpy(buf, d.data(), n);
            buf[n] = 0;
        }
        return d.size() + 1;
    } catch (const std::exception& e) {
        fail(RT_E_INTERNAL, e.what());
        return 0;
    }
}

int rt_scene_save(const rt_scene* s, const char* path) {
    if (!s || !path) return fail(RT_E_INVALID, "scene and path must be non-NULL");
    return guard(RT_E_INVALID, [&] {
        const_cast<rt_scene*>(s)->sync_flat();  // an updated scene is saved as the device holds it
        art::save_scene_file(path, s->flat, s->view);
        return RT_OK;
    });
}

// ---- rt_scene_update_* and rt_scene_*_get, driven by update_kinds.h's table
static_assert(art::kUpdateRows[2].width == RT_MATERIAL_DOUBLES && art::kUpdateRows[3].width == RT_TEXTURE_DOUBLES, "art.h's row widths are update_kinds.h's");

// Every refusal of an update call, all before any device work; RT_OK: go on
static int update_check(art::UpdateKind kind, rt_scene* s, const rt_update_params* u, const double* v, int64_t first, int64_t n) {
    const art::UpdateRow& row = art::update_row(kind);
    const std::string f = std::string("rt_scene_update_") + row.nouns;
    if (!s || !u) return fail(RT_E_INVALID, f + ": scene and params must be non-NULL");
    const int64_t count = static_cast<int64_t>(art::update_count(s->flat, kind));
    if (first < 0 || n < 0 || first > count || n > count - first)
        return fail(RT_E_INVALID, f + ": [first, first + n) must lie within the scene's " + std::to_string(count) + " " + row.nouns);
    if (u->flags & ~RT_OUT_DEVICE) return fail(RT_E_INVALID, f + " takes RT_OUT_DEVICE only");
    if (u->stream && !(u->flags & RT_OUT_DEVICE)) return fail(RT_E_INVALID, f + ": stream needs RT_OUT_DEVICE (host buffers run on the scene's own stream)");
    if (n > 0 && !v) return fail(RT_E_INVALID, f + ": the value buffer is NULL");
    if (u->flags & RT_OUT_DEVICE) return RT_OK;  // a device buffer is not inspected
    const auto refuse = [&](int64_t k, const std::string& subject, const char* fault) {
        return fail(RT_E_INVALID, f + ": " + subject + " of " + row.noun + " " + std::to_string(first + k) + " " + fault);
    };
    for (int64_t k = 0; k < n; ++k) {
        const double* record = v + row.width * static_cast<size_t>(k);
        for (size_t field = 0; field < row.width; ++field)
            if (!std::isfinite(record[field])) return refuse(k, "value " + std::to_string(field), "is not finite");
        if (row.ok && !row.ok(record)) return refuse(k, row.subject, row.fault);
    }
    return RT_OK;
}

static int scene_update(art::UpdateKind kind, rt_scene* s, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms) {
    const int rc = update_check(kind, s, u, v, first, n);
    if (rc != RT_OK) return rc;
    if (ms) *ms = 0;
    if (n == 0) return RT_OK;
    return guard(RT_E_DEVICE, [&] {
        s->device_renderer().update(kind, v, static_cast<size_t>(first), static_cast<size_t>(n), (u->flags & RT_OUT_DEVICE) != 0, u->stream, ms);
        return RT_OK;
    });
}

// A getter's common part: the count when no out pointer was passed (any_out false), the capacity check, then the host
// copy as the device holds it.  Returns the count (the caller fills its buffers when any_out) or the error.
static int64_t get_begin(art::UpdateKind kind, rt_scene* s, bool any_out, int64_t cap) {
    const art::UpdateRow& row = art::update_row(kind);
    const std::string f = std::string("rt_scene_") + row.nouns + "_get";
    if (!s) return fail(RT_E_INVALID, f + ": scene is NULL");
    const int64_t count = static_cast<int64_t>(art::update_count(s->flat, kind));
    if (!any_out) return count;
    if (cap < count)
        return fail(RT_E_INVALID, f + ": the out buffers hold " + std::to_string(cap) + " " + row.nouns + ", the scene has " + std::to_string(count));
    const int rc = guard(RT_E_DEVICE, [&] {
        s->sync_flat();
        return RT_OK;
    });
    return rc != RT_OK ? rc : count;
}

int64_t rt_scene_triangles_get(rt_scene* s, double* p_out, int64_t cap) {
    const int64_t count = get_begin(art::UpdateKind::Triangles, s, p_out != nullptr, cap);
    if (count < 0 || !p_out) return count;
    for (int64_t t = 0; t < count; ++t) std::memcpy(p_out + 9 * t, s->flat.tris[static_cast<size_t>(t)].p, 9 * sizeof(double));
    return count;
}

int rt_scene_update_triangles(rt_scene* s, const rt_update_params* u, const double* p, int64_t first, int64_t n, double* ms) {
    return scene_update(art::UpdateKind::Triangles, s, u, p, first, n, ms);
}

int64_t rt_scene_spheres_get(rt_scene* s, double* s_out, int64_t cap) {
    const int64_t count = get_begin(art::UpdateKind::Spheres, s, s_out != nullptr, cap);
    if (count < 0 || !s_out) return count;
    for (int64_t k = 0; k < count; ++k) {
        const art::SphereRec& sp = s->flat.spheres[static_cast<size_t>(k)];
        s_out[4 * k] = sp.c[0], s_out[4 * k + 1] = sp.c[1], s_out[4 * k + 2] = sp.c[2], s_out[4 * k + 3] = sp.r;
    }
    return count;
}

int rt_scene_update_spheres(rt_scene* s, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms) {
    return scene_update(art::UpdateKind::Spheres, s, u, v, first, n, ms);
}

int64_t rt_scene_lds_image_get(rt_scene* s, int32_t rebuilt, uint8_t* out, int64_t cap) {
    if (!s) return fail(RT_E_INVALID, "rt_scene_lds_image_get: scene is NULL");
    if (rebuilt != 0 && rebuilt != 1) return fail(RT_E_INVALID, "rt_scene_lds_image_get: rebuilt must be 0 or 1");
    int64_t bytes = 0;
    const int rc = guard(RT_E_DEVICE, [&] {
        art::Renderer& r = s->device_renderer();
        bytes = static_cast<int64_t>(r.lds_image_get(rebuilt != 0, nullptr));
        if (out && bytes > 0 && cap < bytes)
            return fail(RT_E_INVALID, "rt_scene_lds_image_get: out holds " + std::to_string(cap) + " bytes, the image has " + std::to_string(bytes));
        if (out && bytes > 0) r.lds_image_get(rebuilt != 0, out);
        return static_cast<int>(RT_OK);
    });
    return rc != RT_OK ? rc : bytes;
}

static_assert(RT_MAT_LAMBERTIAN == art::MAT_LAMBERTIAN && RT_MAT_METAL == art::MAT_METAL && RT_MAT_DIELECTRIC == art::MAT_DIELECTRIC &&
                  RT_MAT_DIFFUSE_LIGHT == art::MAT_LIGHT && RT_MAT_ISOTROPIC == art::MAT_ISOTROPIC,
              "art.h's RT_MAT_* are layout.h's MatType");
static_assert(RT_TEX_SOLID == art::TEX_SOLID && RT_TEX_CHECKER == art::TEX_CHECKER && RT_TEX_NOISE == art::TEX_NOISE && RT_TEX_IMAGE == art::TEX_IMAGE &&
                  RT_TEX_BARY_IMAGE == art::TEX_BARY_IMAGE,
              "art.h's RT_TEX_* are layout.h's TexType");

int64_t rt_scene_materials_get(rt_scene* s, double* params_out, int32_t* desc_out, int64_t cap) {
    const int64_t count = get_begin(art::UpdateKind::Materials, s, params_out || desc_out, cap);
    if (count < 0 || (!params_out && !desc_out)) return count;
    for (int64_t k = 0; k < count; ++k) {
        const art::MatRec& m = s->flat.mats[static_cast<size_t>(k)];
        if (params_out) {
            double* p = params_out + RT_MATERIAL_DOUBLES * k;
            p[0] = m.albedo[0], p[1] = m.albedo[1], p[2] = m.albedo[2], p[3] = m.fuzz, p[4] = m.ir;
        }
        if (desc_out) {
            const bool textured = m.type == art::MAT_LAMBERTIAN || m.type == art::MAT_LIGHT || m.type == art::MAT_ISOTROPIC;
            desc_out[2 * k] = static_cast<int32_t>(m.type), desc_out[2 * k + 1] = textured ? m.tex : -1;
        }
    }
    return count;
}

int64_t rt_scene_textures_get(rt_scene* s, double* params_out, int32_t* desc_out, int64_t cap) {
    const int64_t count = get_begin(art::UpdateKind::Textures, s, params_out || desc_out, cap);
    if (count < 0 || (!params_out && !desc_out)) return count;
    for (int64_t k = 0; k < count; ++k) {
        const art::TexRec& t = s->flat.texs[static_cast<size_t>(k)];
        if (params_out) {
            double* p = params_out + RT_TEXTURE_DOUBLES * k;
            p[0] = t.c[0], p[1] = t.c[1], p[2] = t.c[2], p[3] = t.scale;
        }
        if (desc_out) {
            const bool checker = t.type == art::TEX_CHECKER;
            desc_out[3 * k] = static_cast<int32_t>(t.type), desc_out[3 * k + 1] = checker ? t.even : -1, desc_out[3 * k + 2] = checker ? t.odd : -1;
        }
    }
    return count;
}

int rt_scene_update_materials(rt_scene* s, const rt_update_params* u, const double* m, int64_t first, int64_t n, double* ms) {
    return scene_update(art::UpdateKind::Materials, s, u, m, first, n, ms);
}

int rt_scene_update_textures(rt_scene* s, const rt_update_params* u, const double* t, int64_t first, int64_t n, double* ms) {
    return scene_update(art::UpdateKind::Textures, s, u, t, first, n, ms);
}

// ---- image texels: the images are the graph's in rt_tex_image order (compile_scene: one ImageRec per graph image)
static int64_t texel_count(const art::FlatScene& f) {
    int64_t n = 0;
    for (const art::ImageRec& im : f.images) n += static_cast<int64_t>(im.w) * static_cast<int64_t>(im.h);
    return n;
}

int64_t rt_scene_images_get(rt_scene* s, int32_t* desc_out, int64_t* first_texel_out, int64_t cap) {
    if (!s) return fail(RT_E_INVALID, "rt_scene_images_get: scene is NULL");
    const int64_t count = static_cast<int64_t>(s->flat.images.size());
    if (!desc_out && !first_texel_out) return count;
    if (cap < count)
        return fail(RT_E_INVALID, "rt_scene_images_get: the out buffers hold " + std::to_string(cap) + " images, the scene has " + std::to_string(count));
    int64_t first = 0;
    for (int64_t k = 0; k < count; ++k) {
        const art::ImageRec& im = s->flat.images[static_cast<size_t>(k)];
        if (desc_out) desc_out[3 * k] = im.w, desc_out[3 * k + 1] = im.h, desc_out[3 * k + 2] = im.bpp;
        if (first_texel_out) first_texel_out[k] = first;
        first += static_cast<int64_t>(im.w) * static_cast<int64_t>(im.h);
    }
    return count;
}

int64_t rt_scene_texture_images_get(rt_scene* s, int32_t* image_out, int64_t cap) {
    if (!s) return fail(RT_E_INVALID, "rt_scene_texture_images_get: scene is NULL");
    const int64_t count = static_cast<int64_t>(s->flat.texs.size());
    if (!image_out) return count;
    if (cap < count)
        return fail(RT_E_INVALID, "rt_scene_texture_images_get: image_out holds " + std::to_string(cap) + " textures, the scene has " + std::to_string(count));
    for (int64_t k = 0; k < count; ++k) {
        const art::TexRec& t = s->flat.texs[static_cast<size_t>(k)];
        image_out[k] = (t.type == art::TEX_IMAGE || t.type == art::TEX_BARY_IMAGE) ? t.image : -1;
    }
    return count;
}

int64_t rt_scene_texels_get(rt_scene* s, int32_t image, uint8_t* out, int64_t cap_bytes) {
    if (!s) return fail(RT_E_INVALID, "rt_scene_texels_get: scene is NULL");
    if (image < 0 || static_cast<size_t>(image) >= s->flat.images.size())
        return fail(RT_E_INVALID, "rt_scene_texels_get: image " + std::to_string(image) + " is not one of the scene's " + std::to_string(s->flat.images.size()) + " images");
    const art::ImageRec& im = s->flat.images[static_cast<size_t>(image)];
    const int64_t bytes = static_cast<int64_t>(im.w) * im.h * im.bpp;
    if (!out) return bytes;
    if (cap_bytes < bytes)
        return fail(RT_E_INVALID, "rt_scene_texels_get: out holds " + std::to_string(cap_bytes) + " bytes, the image has " + std::to_string(bytes));
    const int rc = guard(RT_E_DEVICE, [&] {
        s->sync_flat();
        return RT_OK;
    });
    if (rc != RT_OK) return rc;
    std::memcpy(out, s->flat.texels.data() + im.offset, static_cast<size_t>(bytes));
    return bytes;
}

int rt_scene_update_texels(rt_scene* s, const rt_update_params* u, int32_t image, const uint8_t* texels, int64_t first_row, int64_t n_rows, double* ms) {
    const std::string f = "rt_scene_update_texels";
    if (!s || !u) return fail(RT_E_INVALID, f + ": scene and params must be non-NULL");
    if (image < 0 || static_cast<size_t>(image) >= s->flat.images.size())
        return fail(RT_E_INVALID, f + ": image " + std::to_string(image) + " is not one of the scene's " + std::to_string(s->flat.images.size()) + " images");
    const int64_t h = s->flat.images[static_cast<size_t>(image)].h;
    if (first_row < 0 || n_rows < 0 || first_row > h || n_rows > h - first_row)
        return fail(RT_E_INVALID, f + ": [first_row, first_row + n_rows) must lie within the image's " + std::to_string(h) + " rows");
    if (u->flags & ~RT_OUT_DEVICE) return fail(RT_E_INVALID, f + " takes RT_OUT_DEVICE only");
    if (u->stream && !(u->flags & RT_OUT_DEVICE)) return fail(RT_E_INVALID, f + ": stream needs RT_OUT_DEVICE (host buffers run on the scene's own stream)");
    if (n_rows > 0 && !texels) return fail(RT_E_INVALID, f + ": the texel buffer is NULL");
    if (ms) *ms = 0;
    if (n_rows == 0) return RT_OK;
    return guard(RT_E_DEVICE, [&] {
        s->device_renderer().update_texels(static_cast<size_t>(image), texels, static_cast<size_t>(first_row), static_cast<size_t>(n_rows),
                                           (u->flags & RT_OUT_DEVICE) != 0, u->stream, ms);
        return RT_OK;
    });
}

static_assert(art::kUpdateRows[4].width == RT_RECT_DOUBLES && art::kUpdateRows[5].width == RT_BOX_DOUBLES && art::kUpdateRows[6].width == RT_OBJECT_DOUBLES,
              "art.h's row widths are update_kinds.h's");
static_assert(RT_OBJ_PRIM == art::OBJ_PRIM && RT_OBJ_BVH == art::OBJ_BVH && RT_OBJ_TRANSLATE == art::OBJ_TRANSLATE && RT_OBJ_ROTATE_Y == art::OBJ_ROTATE_Y &&
                  RT_OBJ_MEDIUM == art::OBJ_MEDIUM,
              "art.h's RT_OBJ_* are layout.h's ObjKind");

int64_t rt_scene_rects_get(rt_scene* s, double* values_out, int32_t* desc_out, int64_t cap) {
    const int64_t count = get_begin(art::UpdateKind::Rects, s, values_out || desc_out, cap);
    if (count < 0 || (!values_out && !desc_out)) return count;
    for (int64_t k = 0; k < count; ++k) {
        const art::RectRec& r = s->flat.rects[static_cast<size_t>(k)];
        if (values_out) {
            double* p = values_out + RT_RECT_DOUBLES * k;
            p[0] = r.a0, p[1] = r.a1, p[2] = r.b0, p[3] = r.b1, p[4] = r.k;
        }
        if (desc_out) desc_out[2 * k] = static_cast<int32_t>(r.axis), desc_out[2 * k + 1] = static_cast<int32_t>(r.mat);
    }
    return count;
}

int64_t rt_scene_boxes_get(rt_scene* s, double* values_out, int32_t* desc_out, int64_t cap) {
    const int64_t count = get_begin(art::UpdateKind::Boxes, s, values_out || desc_out, cap);
    if (count < 0 || (!values_out && !desc_out)) return count;
    for (int64_t k = 0; k < count; ++k) {
        const art::BoxRec& b = s->flat.boxes[static_cast<size_t>(k)];
        if (values_out)
            for (int a = 0; a < 3; ++a) values_out[RT_BOX_DOUBLES * k + a] = b.mn[a], values_out[RT_BOX_DOUBLES * k + 3 + a] = b.mx[a];
        if (desc_out) desc_out[k] = static_cast<int32_t>(b.mat);
    }
    return count;
}

int64_t rt_scene_objects_get(rt_scene* s, double* values_out, int32_t* desc_out, int64_t cap) {
    const int64_t count = get_begin(art::UpdateKind::Objects, s, values_out || desc_out, cap);
    if (count < 0 || (!values_out && !desc_out)) return count;
    for (int64_t k = 0; k < count; ++k) {
        const art::ObjRec& o = s->flat.objs[static_cast<size_t>(k)];
        if (values_out) std::memcpy(values_out + RT_OBJECT_DOUBLES * k, o.p, sizeof o.p);
        if (desc_out) desc_out[4 * k] = o.kind, desc_out[4 * k + 1] = o.a, desc_out[4 * k + 2] = o.b, desc_out[4 * k + 3] = -1;
    }
    if (desc_out)
        for (size_t w = 0; w < s->flat.world.size(); ++w) {
            const int32_t o = s->flat.world[w];
            if (o >= 0 && o < count) desc_out[4 * o + 3] = static_cast<int32_t>(w);
        }
    return count;
}

int rt_scene_update_rects(rt_scene* s, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms) {
    return scene_update(art::UpdateKind::Rects, s, u, v, first, n, ms);
}

int rt_scene_update_boxes(rt_scene* s, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms) {
    return scene_update(art::UpdateKind::Boxes, s, u, v, first, n, ms);
}

int rt_scene_update_objects(rt_scene* s, const rt_update_params* u, const double* v, int64_t first, int64_t n, double* ms) {
    return scene_update(art::UpdateKind::Objects, s, u, v, first, n, ms);
}

int rt_scene_bvh_get(rt_scene* s, void* nodes_out, int64_t node_cap, uint32_t* primrefs_out, int64_t ref_cap, int64_t* n_nodes, int64_t* n_primrefs) {
    if (!s) return fail(RT_E_INVALID, "rt_scene_bvh_get: scene is NULL");
    return guard(RT_E_DEVICE, [&] {
        size_t nn = 0, nr = 0;
        art::Renderer& r = s->device_renderer();
        r.bvh_get(nullptr, nullptr, nn, nr);
        if (n_nodes) *n_nodes = static_cast<int64_t>(nn);
        if (n_primrefs) *n_primrefs = static_cast<int64_t>(nr);
        if (nodes_out && node_cap < static_cast<int64_t>(nn))
            return fail(RT_E_INVALID, "rt_scene_bvh_get: nodes_out holds " + std::to_string(node_cap) + " nodes, the scene has " + std::to_string(nn));
        if (primrefs_out && ref_cap < static_cast<int64_t>(nr))
            return fail(RT_E_INVALID, "rt_scene_bvh_get: primrefs_out holds " + std::to_string(ref_cap) + " references, the scene has " + std::to_string(nr));
        if (nodes_out || primrefs_out) r.bvh_get(nodes_out, primrefs_out, nn, nr);
        return static_cast<int>(RT_OK);
    });
}

int rt_scene_load(const char* path, int device, rt_scene** out) {
    if (!path || !out) return fail(RT_E_INVALID, "path and out must be non-NULL");
    *out = nullptr;
    return guard(RT_E_SCENE, [&] {
        auto s = std::make_unique<rt_scene>();
        art::load_scene_file(path, s->flat, s->view);
        s->has_graph = false;
        s->device = device;
        *out = s.release();
        return RT_OK;
    });
}

void rt_scene_destroy(rt_scene* s) {
    try {
        delete s;
    } catch (...) {
    }
}

int rt_local_rows(const rt_params* p, int32_t* rows_out) {
    if (!p || p->height < 1 || p->band_rows < 1 || p->band_count < 1 || p->band_index < 0 || p->band_index >= p->band_count)
        return fail(RT_E_INVALID, "invalid band partition");
    const int n = art::band_local_rows(p->height, p->band_rows, p->band_count, p->band_index);
    if (rows_out)
        for (int ly = 0; ly < n; ++ly) rows_out[ly] = art::band_global_row(ly, p->band_rows, p->band_count, p->band_index);
    return n;
}

int rt_band_block_rows(int32_t height, int32_t band_rows, int32_t n) {
    if (height < 1 || band_rows < 1 || n < 1) return fail(RT_E_INVALID, "height, band_rows and n must be >= 1");
    return art::band_block_rows(height, band_rows, n);
}

int rt_unpack_bands(const uint8_t* packed, size_t packed_bytes, uint8_t* frame, size_t frame_bytes, int32_t width, int32_t height,
                    int32_t band_rows, int32_t n, int32_t flags, void* stream) {
    if (!packed || !frame) return fail(RT_E_INVALID, "packed and frame must be non-NULL");
    if (width < 1 || height < 1 || band_rows < 1 || n < 1) return fail(RT_E_INVALID, "width, height, band_rows and n must be >= 1");
    if (static_cast<int64_t>(width) * height > (int64_t(1) << 31)) return fail(RT_E_INVALID, "image too large");
    const size_t row_bytes = static_cast<size_t>(width) * 3;
    const size_t want_packed = static_cast<size_t>(n) * static_cast<size_t>(art::band_block_rows(height, band_rows, n)) * row_bytes;
    const size_t want_frame = static_cast<size_t>(height) * row_bytes;
    if (packed_bytes != want_packed)
        return fail(RT_E_INVALID, "packed holds " + std::to_string(packed_bytes) + " bytes, the layout needs n * band_block_rows * width * 3 = " +
                                      std::to_string(want_packed) + " (every rank's padded block)");
    if (frame_bytes != want_frame)
        return fail(RT_E_INVALID, "frame holds " + std::to_string(frame_bytes) + " bytes, height * width * 3 = " + std::to_string(want_frame));
    return guard(RT_E_DEVICE, [&] {
        art::unpack_bands(packed, frame, width, height, band_rows, n, (flags & RT_OUT_DEVICE) != 0, stream);
        return RT_OK;
    });
}

int rt_render(rt_scene* s, const rt_camera* cam, const rt_params* p, uint8_t* out_rgb8, double* out_accum, rt_stats* stats) {
    std::string why;
    if (!s || !cam) return fail(RT_E_INVALID, "scene and camera must be non-NULL");
    if (!valid_params(p, why)) return fail(RT_E_INVALID, why);
    if ((p->flags & RT_ADAPTIVE) && (p->flags & RT_PARALLEL_IMAGES)) return fail(RT_E_INVALID, "RT_ADAPTIVE and RT_PARALLEL_IMAGES are two engine modes");
    if (p->flags & RT_ADAPTIVE) {
        const int rows = rt_local_rows(p, nullptr);
        if (p->width % 12 != 0 || rows % 12 != 0 || (p->band_count > 1 && p->band_rows % 12 != 0))
            return fail(RT_E_INVALID, "for adaptive strategy image size should perfectly fit big square size for now!! (engine.h:178-179: "
                                      "width and local rows multiples of 12, band_rows a multiple of 12 when bands are interleaved)");
        if (out_accum) return fail(RT_E_INVALID, "adaptive mode has no per-pixel radiance sums: out_accum must be NULL");
    }
    return guard(RT_E_DEVICE, [&] {
        art::RenderStats st;
        s->device_renderer().render(camera_of(cam), render_params(p), out_rgb8, out_accum, st);
        fill_stats(st, stats);
        return RT_OK;
    });
}

int rt_render_progressive(rt_scene* s, const rt_camera* cam, const rt_params* p, uint8_t* out_rgb8, double* out_accum, rt_progress_fn cb,
                          void* user, rt_stats* stats) {
    std::string why;
    if (!s || !cam || !cb || !out_rgb8) return fail(RT_E_INVALID, "scene, camera, callback and out_rgb8 must be non-NULL");
    if (!valid_params(p, why)) return fail(RT_E_INVALID, why);
    if (p->flags & (RT_ADAPTIVE | RT_PARALLEL_IMAGES))
        return fail(RT_E_INVALID, "progressive rendering traces whole frames of consecutive samples (no RT_ADAPTIVE or RT_PARALLEL_IMAGES)");
    return guard(RT_E_DEVICE, [&] {
        art::RenderParams rp = render_params(p);
        if (rp.samples_per_pass <= 0) rp.samples_per_pass = (rp.spp + 7) / 8;
        const int spp = rp.spp;
        rp.on_pass = [&](int done) { return cb(user, done, spp, out_rgb8, out_accum) == 0; };
        art::RenderStats st;
        s->device_renderer().render(camera_of(cam), rp, out_rgb8, out_accum, st);
        fill_stats(st, stats);
        return RT_OK;
    });
}

int rt_trace_rays(rt_scene* s, const double* rays, int64_t n, int32_t flags, double* t_out, double* normal_out) {
    if (!s || n < 0 || (n > 0 && (!rays || !t_out))) return fail(RT_E_INVALID, "scene, rays and t_out must be non-NULL, n >= 0");
    return guard(RT_E_DEVICE, [&] {
        std::vector<double> nrm(normal_out ? 0 : 3 * static_cast<size_t>(n));
        s->device_renderer().trace_rays(rays, static_cast<size_t>(n), (flags & RT_GLOBAL_SCENE) != 0, t_out, normal_out ? normal_out : nrm.data());
        return RT_OK;
    });
}

int rt_query_rays(rt_scene* s, const rt_query_params* q, const double* rays, const double* t_max, int64_t n, double* hits, uint8_t* occluded) {
    if (!s || !q) return fail(RT_E_INVALID, "rt_query_rays: scene and params must be non-NULL");
    if (n < 0 || n > (int64_t(1) << 30)) return fail(RT_E_INVALID, "rt_query_rays: n must be in [0, 2^30]");
    if (q->flags & ~(RT_OUT_DEVICE | RT_GLOBAL_SCENE | RT_Q_ANY_HIT | RT_Q_NO_MEDIA))
        return fail(RT_E_INVALID, "rt_query_rays takes RT_OUT_DEVICE, RT_GLOBAL_SCENE, RT_Q_ANY_HIT and RT_Q_NO_MEDIA only");
    if ((hits != nullptr) == (occluded != nullptr))
        return fail(RT_E_INVALID, "rt_query_rays: give exactly one of hits (closest mode) and occluded (RT_Q_ANY_HIT)");
    const bool any_hit = (q->flags & RT_Q_ANY_HIT) != 0;
    if (any_hit != (occluded != nullptr))
        return fail(RT_E_INVALID, any_hit ? "rt_query_rays: RT_Q_ANY_HIT writes occluded, not hits" : "rt_query_rays: occluded needs RT_Q_ANY_HIT");
    if (n == 0) return RT_OK;
    if (!rays) return fail(RT_E_INVALID, "rt_query_rays: rays is NULL");
    return guard(RT_E_DEVICE, [&] {
        s->device_renderer().query_rays(rays, t_max, static_cast<size_t>(n), (q->flags & RT_OUT_DEVICE) != 0, (q->flags & RT_GLOBAL_SCENE) != 0, any_hit,
                                        (q->flags & RT_Q_NO_MEDIA) != 0, q->stream, hits, occluded);
        return RT_OK;
    });
}

int rt_radiance_rays(rt_scene* s, const rt_radiance_params* q, const double* rays, const uint64_t* rng, int64_t n, double* radiance,
                     rt_stats* stats) {
    if (!s || !q) return fail(RT_E_INVALID, "rt_radiance_rays: scene and params must be non-NULL");
    if (n < 0 || n > (int64_t(1) << 30)) return fail(RT_E_INVALID, "rt_radiance_rays: n must be in [0, 2^30]");
    if (q->flags & ~(RT_OUT_DEVICE | RT_GLOBAL_SCENE)) return fail(RT_E_INVALID, "rt_radiance_rays takes RT_OUT_DEVICE and RT_GLOBAL_SCENE only");
    if (q->spp < 0) return fail(RT_E_INVALID, "rt_radiance_rays: spp must be >= 1 (0 is taken as 1)");
    if (q->max_depth < 1) return fail(RT_E_INVALID, "rt_radiance_rays: max_depth must be >= 1");
    if (q->stream && !(q->flags & RT_OUT_DEVICE)) return fail(RT_E_INVALID, "rt_radiance_rays: stream needs RT_OUT_DEVICE (host buffers run on the scene's own stream)");
    const int64_t spp = q->spp > 0 ? q->spp : 1;
    if (static_cast<uint64_t>(n) * static_cast<uint64_t>(spp) > art::kMaxPassSlots)
        return fail(RT_E_INVALID, "rt_radiance_rays: n * spp = " + std::to_string(n * spp) + " exceeds kMaxPassSlots = 2^31 paths per call: chunk the "
                                  "rays with id_base, or the samples with sample_base");
    if (!rng && (q->id_base > (uint64_t(1) << 32) || q->id_base + static_cast<uint64_t>(n) > (uint64_t(1) << 32)))
        return fail(RT_E_INVALID, "rt_radiance_rays: id_base + n must be <= 2^32 (stream ids are 32 bits)");
    if (n == 0) return RT_OK;
    if (!rays || !radiance) return fail(RT_E_INVALID, "rt_radiance_rays: rays and radiance must be non-NULL");
    return guard(RT_E_DEVICE, [&] {
        art::RadianceParams rp;
        rp.spp = static_cast<int>(spp), rp.max_depth = q->max_depth, rp.sample_base = q->sample_base;
        rp.seed = q->seed, rp.id_base = rng ? 0 : q->id_base;
        rp.device = (q->flags & RT_OUT_DEVICE) != 0, rp.global_scene = (q->flags & RT_GLOBAL_SCENE) != 0;
        rp.stream = q->stream;
        for (int c = 0; c < 3; ++c) rp.background[c] = q->background[c];
        art::RenderStats st;
        s->device_renderer().radiance_rays(rp, rays, rng, static_cast<size_t>(n), radiance, stats ? &st : nullptr);
        if (stats) {
            fill_stats(st, stats);
            stats->extend_variant = stats->kernel_lds_mode = -1;  // neither an extend variant nor a k_paths_g instantiation
        }
        return RT_OK;
    });
}

// rt_radiance_grad and rt_radiance_grad_texels (`f`: the name in messages; grad_texels null: the former)
static int radiance_grad(const std::string& f, rt_scene* s, const rt_radiance_params* q, const double* rays, const uint64_t* rng, const double* weights,
                         int64_t n, double* radiance, double* grad_textures, double* grad_materials, double* grad_background, double* grad_texels,
                         rt_stats* stats) {
    if (!s || !q) return fail(RT_E_INVALID, f + ": scene and params must be non-NULL");
    if (n < 0 || n > (int64_t(1) << 30)) return fail(RT_E_INVALID, f + ": n must be in [0, 2^30]");
    if (q->flags & ~(RT_OUT_DEVICE | RT_GLOBAL_SCENE)) return fail(RT_E_INVALID, f + " takes RT_OUT_DEVICE and RT_GLOBAL_SCENE only");
    if (q->spp < 0) return fail(RT_E_INVALID, f + ": spp must be >= 1 (0 is taken as 1)");
    if (q->max_depth < 1) return fail(RT_E_INVALID, f + ": max_depth must be >= 1");
    if (q->stream && !(q->flags & RT_OUT_DEVICE)) return fail(RT_E_INVALID, f + ": stream needs RT_OUT_DEVICE (host buffers run on the scene's own stream)");
    const int64_t spp = q->spp > 0 ? q->spp : 1;
    if (static_cast<uint64_t>(n) * static_cast<uint64_t>(spp) > art::kMaxPassSlots)
        return fail(RT_E_INVALID, f + ": n * spp = " + std::to_string(n * spp) + " exceeds kMaxPassSlots = 2^31 paths per call: chunk the "
                                  "rays with id_base, or the samples with sample_base (gradients of chunks add)");
    if (!rng && (q->id_base > (uint64_t(1) << 32) || q->id_base + static_cast<uint64_t>(n) > (uint64_t(1) << 32)))
        return fail(RT_E_INVALID, f + ": id_base + n must be <= 2^32 (stream ids are 32 bits)");
    if (n == 0) return RT_OK;
    if (!rays || !weights) return fail(RT_E_INVALID, f + ": rays and weights must be non-NULL");
    if (!radiance && !grad_textures && !grad_materials && !grad_background && !grad_texels) return RT_OK;
    if (grad_texels) {  // a vertex record's row is 32 bits: T + M + 1 + N rows, and kGradNoRow
        const uint64_t rows = s->flat.texs.size() + s->flat.mats.size() + 1 + static_cast<uint64_t>(texel_count(s->flat));
        if (rows > 0xFFFFFFFFull)
            return fail(RT_E_INVALID, f + ": textures + materials + 1 + texels = " + std::to_string(rows) + " rows do not fit the 32-bit row of a vertex record");
    }
    return guard(RT_E_DEVICE, [&] {
        art::RadianceParams rp;
        rp.spp = static_cast<int>(spp), rp.max_depth = q->max_depth, rp.sample_base = q->sample_base;
        rp.seed = q->seed, rp.id_base = rng ? 0 : q->id_base;
        rp.device = (q->flags & RT_OUT_DEVICE) != 0, rp.global_scene = (q->flags & RT_GLOBAL_SCENE) != 0;
        rp.stream = q->stream;
        for (int c = 0; c < 3; ++c) rp.background[c] = q->background[c];
        art::RenderStats st;
        s->device_renderer().radiance_grad(rp, rays, rng, weights, static_cast<size_t>(n), radiance, grad_textures, grad_materials, grad_background,
                                           grad_texels, stats ? &st : nullptr);
        if (stats) {
            fill_stats(st, stats);
            stats->extend_variant = stats->kernel_lds_mode = -1;
        }
        return RT_OK;
    });
}

int rt_radiance_grad(rt_scene* s, const rt_radiance_params* q, const double* rays, const uint64_t* rng, const double* weights, int64_t n,
                     double* radiance, double* grad_textures, double* grad_materials, double* grad_background, rt_stats* stats) {
    return radiance_grad("rt_radiance_grad", s, q, rays, rng, weights, n, radiance, grad_textures, grad_materials, grad_background, nullptr, stats);
}

int rt_radiance_grad_texels(rt_scene* s, const rt_radiance_params* q, const double* rays, const uint64_t* rng, const double* weights, int64_t n,
                            double* radiance, double* grad_textures, double* grad_materials, double* grad_background, double* grad_texels,
                            rt_stats* stats) {
    return radiance_grad("rt_radiance_grad_texels", s, q, rays, rng, weights, n, radiance, grad_textures, grad_materials, grad_background, grad_texels,
                         stats);
}

int rt_render_views(rt_scene* s, const rt_camera* cams, const uint64_t* seeds, int32_t nviews, const rt_params* p, uint8_t* out_rgb8,
                    double* out_accum, rt_stats* stats) {
    if (!s || !cams || !p) return fail(RT_E_INVALID, "rt_render_views: scene, cams and params must be non-NULL");
    if (nviews < 0) return fail(RT_E_INVALID, "rt_render_views: nviews must be >= 0");
    if (p->flags & ~(RT_OUT_DEVICE | RT_GLOBAL_SCENE)) return fail(RT_E_INVALID, "rt_render_views takes RT_OUT_DEVICE and RT_GLOBAL_SCENE only");
    if (p->width < 2 || p->height < 2) return fail(RT_E_INVALID, "rt_render_views: width and height must be >= 2 (u = (i + r)/(W-1), engine.h:62-63)");
    if (p->spp < 1) return fail(RT_E_INVALID, "rt_render_views: spp must be >= 1");
    if (p->max_depth < 1) return fail(RT_E_INVALID, "rt_render_views: max_depth must be >= 1");
    if (p->fp_mode != RT_FP64) return fail(RT_E_INVALID, "fp_mode must be RT_FP64 (0): the reference's double arithmetic is the only mode");
    if (p->band_count != 1 || p->band_index != 0)
        return fail(RT_E_INVALID, "rt_render_views renders whole frames: band_count must be 1 (and band_index 0)");
    if (p->stream && !(p->flags & RT_OUT_DEVICE))
        return fail(RT_E_INVALID, "rt_render_views: stream needs RT_OUT_DEVICE (host buffers run on the scene's own stream)");
    const uint64_t view_paths = static_cast<uint64_t>(p->width) * static_cast<uint64_t>(p->height) * static_cast<uint64_t>(p->spp);
    if (view_paths > art::kMaxPassSlots)
        return fail(RT_E_INVALID, "rt_render_views: one view of width * height * spp = " + std::to_string(view_paths) + " paths exceeds kMaxPassSlots = "
                                  "2^31 paths per launch: render such frames with rt_render, which splits a frame into passes");
    if (nviews == 0) return RT_OK;
    if (!out_rgb8) return fail(RT_E_INVALID, "rt_render_views: out_rgb8 must be non-NULL");
    return guard(RT_E_DEVICE, [&] {
        std::vector<art::CameraRec> recs(static_cast<size_t>(nviews));
        for (int32_t v = 0; v < nviews; ++v) recs[static_cast<size_t>(v)] = camera_of(&cams[v]);
        art::RenderStats st;
        s->device_renderer().render_views(recs.data(), seeds, static_cast<size_t>(nviews), render_params(p), out_rgb8, out_accum, stats ? &st : nullptr);
        if (stats) {
            fill_stats(st, stats);
            stats->extend_variant = stats->kernel_lds_mode = -1;  // neither an extend variant nor a k_paths_g instantiation
        }
        return RT_OK;
    });
}

int rt_tile_candidates(rt_scene* s, const rt_camera* cam, const rt_params* p, uint16_t* counts_out, int64_t cap) {
    std::string why;
    if (!s || !cam) return fail(RT_E_INVALID, "rt_tile_candidates: scene and camera must be non-NULL");
    if (!valid_params(p, why)) return fail(RT_E_INVALID, why);
    if (counts_out && cap < 0) return fail(RT_E_INVALID, "rt_tile_candidates: cap must be >= 0");
    if (counts_out) {
        const int64_t rows = art::band_local_rows(p->height, p->band_rows, p->band_count, p->band_index);
        const int64_t tiles = static_cast<int64_t>((p->width + 7) / 8) * ((rows + 7) / 8);
        if (cap < tiles) return fail(RT_E_INVALID, "rt_tile_candidates: counts_out holds " + std::to_string(cap) + " entries, the frame has " +
                                                       std::to_string(tiles) + " tiles");
    }
    return guard(RT_E_DEVICE, [&] {
        return s->device_renderer().tile_candidates(camera_of(cam), render_params(p), counts_out, static_cast<size_t>(counts_out ? cap : 0));
    });
}

int rt_camera_rays(const rt_camera* cam, const rt_params* p, uint32_t sample_base, int device, double* rays_out, uint64_t* rng_out) {
    std::string why;
    if (!cam || !rays_out) return fail(RT_E_INVALID, "rt_camera_rays: camera and rays_out must be non-NULL");
    if (!p) return fail(RT_E_INVALID, "params is NULL");
    if (device < 0) return fail(RT_E_INVALID, "device must be >= 0");
    rt_params q = *p;  // max_depth, samples_per_pass and background are ignored
    q.max_depth = 0;
    if (!valid_params(&q, why)) return fail(RT_E_INVALID, why);
    if (p->flags & ~RT_OUT_DEVICE) return fail(RT_E_INVALID, "rt_camera_rays takes RT_OUT_DEVICE only");
    if (p->stream && !(p->flags & RT_OUT_DEVICE)) return fail(RT_E_INVALID, "rt_camera_rays: stream needs RT_OUT_DEVICE");
    const uint64_t rows = static_cast<uint64_t>(art::band_local_rows(p->height, p->band_rows, p->band_count, p->band_index));
    const uint64_t npix_pad = static_cast<uint64_t>((p->width + 7) / 8) * ((rows + 7) / 8) * 64u;  // 8x8 tiles, as rt_render's slots
    if (npix_pad * static_cast<uint64_t>(p->spp) > art::kMaxPassSlots)
        return fail(RT_E_INVALID, "rt_camera_rays: padded local pixels * spp exceeds kMaxPassSlots = 2^31 per call: fewer samples per call, with sample_base");
    return guard(RT_E_DEVICE, [&] {
        art::Renderer::camera_rays(device, camera_of(cam), render_params(&q), sample_base, rays_out, rng_out);
        return RT_OK;
    });
}

int rt_render_guides(rt_scene* s, const rt_camera* cam, const rt_params* p, double* guides, double* rays_out) {
    std::string why;
    if (!s || !cam || !guides) return fail(RT_E_INVALID, "scene, camera and guides must be non-NULL");
    if (!p) return fail(RT_E_INVALID, "params is NULL");
    rt_params q = *p;  // spp, seed, max_depth and samples_per_pass are ignored
    q.spp = 1;
    q.max_depth = 0;
    if (!valid_params(&q, why)) return fail(RT_E_INVALID, why);
    if (p->flags & ~(RT_OUT_DEVICE | RT_GLOBAL_SCENE)) return fail(RT_E_INVALID, "rt_render_guides takes RT_OUT_DEVICE and RT_GLOBAL_SCENE only");
    return guard(RT_E_DEVICE, [&] {
        s->device_renderer().render_guides(camera_of(cam), render_params(&q), guides, rays_out);
        return RT_OK;
    });
}

namespace {
// rt_denoise_params -> DenoiseParams with the defaults filled in; false (why) for a value outside its range
bool denoise_params(const rt_denoise_params* p, int width, int height, art::DenoiseParams& d, std::string& why) {
    d.width = width;
    d.height = height;
    if (width < 1 || height < 1) { why = "width and height must be >= 1"; return false; }
    if (static_cast<int64_t>(width) * height > (int64_t(1) << 31)) { why = "image too large"; return false; }
    if (!p) return true;
    if (p->iterations < 0 || p->iterations > 8) { why = "iterations must be 1..8 (0 = the default, 5)"; return false; }
    if (p->normal_squarings < 0 || p->normal_squarings > 10) { why = "normal_squarings must be 1..10 (0 = the default, 6)"; return false; }
    if (!(p->sigma_color >= 0) || !(p->sigma_plane >= 0) || !(p->albedo_floor >= 0) || std::isinf(p->sigma_color) || std::isinf(p->sigma_plane) ||
        std::isinf(p->albedo_floor)) {
        why = "sigma_color, sigma_plane and albedo_floor must be finite and >= 0 (0 = the default)";
        return false;
    }
    if (p->flags & ~(RT_OUT_DEVICE | RT_DN_NO_DEMODULATE)) { why = "rt_denoise_params.flags takes RT_OUT_DEVICE and RT_DN_NO_DEMODULATE only"; return false; }
    if (p->iterations) d.iterations = p->iterations;
    if (p->normal_squarings) d.normal_squarings = p->normal_squarings;
    if (p->sigma_color != 0) d.sigma_color = p->sigma_color;
    if (p->sigma_plane != 0) d.sigma_plane = p->sigma_plane;
    if (p->albedo_floor != 0) d.albedo_floor = p->albedo_floor;
    d.demodulate = !(p->flags & RT_DN_NO_DEMODULATE);
    d.stream = p->stream;
    return true;
}
}  // namespace

int rt_denoise(int device, const rt_denoise_params* p, const double* accum_a, const double* accum_b, int32_t spp_each, const double* guides,
               double* out_color, uint8_t* out_rgb8, double* ms) {
    if (!p || !accum_a || !accum_b || !guides || !out_color) return fail(RT_E_INVALID, "params, accum_a, accum_b, guides and out_color must be non-NULL");
    if (spp_each < 1) return fail(RT_E_INVALID, "spp_each must be >= 1");
    if (device < 0) return fail(RT_E_INVALID, "device must be >= 0");
    art::DenoiseParams d;
    std::string why;
    if (!denoise_params(p, p->width, p->height, d, why)) return fail(RT_E_INVALID, why);
    return guard(RT_E_DEVICE, [&] {
        art::denoise(device, d, accum_a, accum_b, spp_each, guides, out_color, out_rgb8, (p->flags & RT_OUT_DEVICE) != 0, ms);
        return RT_OK;
    });
}

int rt_render_denoised(rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_params* dn, uint8_t* out_rgb8, double* out_color,
                       rt_stats* stats) {
    std::string why;
    if (!s || !cam || !out_rgb8) return fail(RT_E_INVALID, "scene, camera and out_rgb8 must be non-NULL");
    if (!valid_params(p, why)) return fail(RT_E_INVALID, why);
    if (p->band_count != 1) return fail(RT_E_INVALID, "rt_render_denoised filters a whole frame: band_count must be 1");
    if (p->spp < 2 || p->spp % 2 != 0) return fail(RT_E_INVALID, "rt_render_denoised splits spp into two half-renders: spp must be even and >= 2");
    if (p->flags & (RT_ADAPTIVE | RT_PARALLEL_IMAGES)) return fail(RT_E_INVALID, "rt_render_denoised renders engine_mode::single frames (no RT_ADAPTIVE or RT_PARALLEL_IMAGES)");
    art::DenoiseParams d;
    if (!denoise_params(dn, p->width, p->height, d, why)) return fail(RT_E_INVALID, why);
    if (!d.stream) d.stream = p->stream;
    return guard(RT_E_DEVICE, [&] {
        const auto t0 = std::chrono::steady_clock::now();
        art::Renderer& renderer = s->device_renderer();
        const art::DenoiseFrame fb = art::denoise_reserve(s->device, p->width, p->height);
        art::RenderParams rp = render_params(p);
        rp.spp = p->spp / 2;
        rp.flags |= RT_OUT_DEVICE;
        art::RenderStats st[2];
        for (int half = 0; half < 2; ++half) {
            rp.seed = p->seed + static_cast<uint64_t>(half);
            renderer.render(camera_of(cam), rp, nullptr, half ? fb.accum_b : fb.accum_a, st[half]);
        }
        art::RenderParams gp = rp;
        gp.flags = RT_OUT_DEVICE | (p->flags & RT_GLOBAL_SCENE);
        renderer.render_guides(camera_of(cam), gp, fb.guides, nullptr);
        art::denoise_reserved(s->device, d, rp.spp, out_color, out_rgb8, (p->flags & RT_OUT_DEVICE) != 0, nullptr);
        art::RenderStats sum = st[1];
        sum.segments += st[0].segments;
        sum.primary += st[0].primary;
        sum.extend_ms += st[0].extend_ms;
        sum.shade_ms += st[0].shade_ms;
        sum.extend_launches += st[0].extend_launches;
        sum.shade_launches += st[0].shade_launches;
        sum.passes += st[0].passes;
        sum.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fill_stats(sum, stats);
        return RT_OK;
    });
}

int rt_render_noise_target(rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_noise_params* noise, uint8_t* out_rgb8, double* out_accum,
                           int32_t* out_count, double* out_moments, rt_stats* stats, rt_noise_result* result) {
    std::string why;
    if (!s || !cam || !out_rgb8) return fail(RT_E_INVALID, "scene, camera and out_rgb8 must be non-NULL");
    if (!valid_params(p, why)) return fail(RT_E_INVALID, why);
    if (p->flags & (RT_ADAPTIVE | RT_PARALLEL_IMAGES | RT_WAVEFRONT | RT_SPLIT_SHADE))
        return fail(RT_E_INVALID, "rt_render_noise_target traces engine_mode::single samples through the persistent-path kernels "
                                  "(no RT_ADAPTIVE, RT_PARALLEL_IMAGES, RT_WAVEFRONT or RT_SPLIT_SHADE)");
    art::NoiseParams np;
    if (noise) {
        if (noise->min_spp < 0 || noise->min_spp == 1) return fail(RT_E_INVALID, "min_spp must be >= 2 (the variance needs two samples; 0 = the default, 32)");
        if (noise->step_spp < 0) return fail(RT_E_INVALID, "step_spp must be >= 1 (0 = the default, 32)");
        if (noise->dilate != 0 && noise->dilate != 1) return fail(RT_E_INVALID, "dilate must be 0 or 1");
        if (!(noise->rel_tol >= 0) || !(noise->lum_floor >= 0) || std::isinf(noise->rel_tol) || std::isinf(noise->lum_floor))
            return fail(RT_E_INVALID, "rel_tol and lum_floor must be finite and >= 0 (0 = the default)");
        if (noise->min_spp) np.min_spp = noise->min_spp;
        if (noise->step_spp) np.step_spp = noise->step_spp;
        np.dilate = noise->dilate == 1;
        if (noise->rel_tol != 0) np.rel_tol = noise->rel_tol;
        if (noise->lum_floor != 0) np.lum_floor = noise->lum_floor;
    }
    if (np.min_spp > p->spp) return fail(RT_E_INVALID, "min_spp (" + std::to_string(np.min_spp) + ") exceeds the per-pixel cap spp (" + std::to_string(p->spp) + ")");
    if (np.dilate && p->band_count > 1)
        return fail(RT_E_INVALID, "dilate = 1 needs the whole frame (band_count 1): a pixel's 3x3 neighbourhood would depend on the partition");
    return guard(RT_E_DEVICE, [&] {
        art::RenderStats st;
        art::NoiseResult nr;
        s->device_renderer().render_noise_target(camera_of(cam), render_params(p), np, out_rgb8, out_accum, out_count, out_moments, st, nr);
        fill_stats(st, stats);
        if (result) {
            result->rounds = nr.rounds;
            result->converged_pixels = nr.converged_pixels;
            result->samples = nr.samples;
        }
        return RT_OK;
    });
}

int rt_image_load(const char* path, int32_t* width, int32_t* height, int32_t* channels, uint8_t** pixels) {
    if (!path || !width || !height || !channels || !pixels) return fail(RT_E_INVALID, "NULL argument");
    *pixels = nullptr;
    return guard(RT_E_INVALID, [&] {
        art::DecodedImage d = art::load_image_file(path);
        uint8_t* p = static_cast<uint8_t*>(std::malloc(d.data.size()));
        if (!p) throw std::bad_alloc();
        std::memcpy(p, d.data.data(), d.data.size());
        *width = d.w;
        *height = d.h;
        *channels = d.channels;
        *pixels = p;
        return RT_OK;
    });
}
void rt_image_free(uint8_t* pixels) { std::free(pixels); }

// ---------------------------------------------------------------------------------------------- multi-GPU
int rt_multi_create(const char* name, const char* asset_dir, const int* devices, int ngpus, rt_multi** out) {
    if (!name || !out) return fail(RT_E_INVALID, "name and out must be non-NULL");
    *out = nullptr;
    art::SceneGraph g;
    const int rc = guard(RT_E_SCENE, [&] {
        art::build_builtin_scene(g, name, asset_dir ? asset_dir : "assets");
        return RT_OK;
    });
    if (rc != RT_OK) return rc;
    return guard(RT_E_DEVICE, [&] { return multi_from_graph(std::move(g), devices, ngpus, out); });
}
int rt_multi_from_graph(rt_graph* g, const int* devices, int ngpus, rt_multi** out) {
    if (!g || !out) return fail(RT_E_INVALID, "graph and out must be non-NULL");
    *out = nullptr;
    return guard(RT_E_DEVICE, [&] { return multi_from_graph(g->g, devices, ngpus, out); });
}
void rt_multi_destroy(rt_multi* m) {
    try {
        delete m;
    } catch (...) {
    }
}
int rt_render_multi(rt_multi* m, const rt_camera* cam, const rt_params* p, uint8_t* out_rgb8, rt_stats* stats) {
    std::string why;
    if (!m || !cam || !out_rgb8) return fail(RT_E_INVALID, "multi, camera and out_rgb8 must be non-NULL");
    if (!valid_params(p, why)) return fail(RT_E_INVALID, why);
    if (p->flags & RT_ADAPTIVE) return fail(RT_E_INVALID, "rt_render_multi renders engine_mode::single frames (no RT_ADAPTIVE)");
    return guard(RT_E_DEVICE, [&] {
        art::RenderStats st;
        m->renderer->render(camera_of(cam), render_params(p), out_rgb8, (p->flags & RT_OUT_DEVICE) != 0, st);
        fill_stats(st, stats);
        return RT_OK;
    });
}

int rt_multi_device_stats(const rt_multi* m, int k, rt_stats* stats) {
    if (!m || !stats) return fail(RT_E_INVALID, "multi and stats must be non-NULL");
    art::RenderStats st;
    if (!m->renderer->device_stats(k, st)) return fail(RT_E_INVALID, "no such device index, or no render yet");
    fill_stats(st, stats);
    return RT_OK;
}
int rt_multi_scene_info(const rt_multi* m, rt_scene_info* info) {
    if (!m || !info) return fail(RT_E_INVALID, "multi and info must be non-NULL");
    art::SceneView view;
    for (int a = 0; a < 3; ++a) {
        view.lookfrom[a] = m->graph.lookfrom[a];
        view.lookat[a] = m->graph.lookat[a];
    }
    view.vfov = m->graph.vfov;
    view.aperture = m->graph.aperture;
    fill_info(view, m->flat, info);
    info->device_bytes_f64 = m->renderer->scene_bytes();
    return RT_OK;
}
int rt_multi_times_get(const rt_multi* m, rt_multi_times* out) {
    if (!m || !out) return fail(RT_E_INVALID, "multi and out must be non-NULL");
    const art::MultiTimes& t = m->renderer->times();
    std::memset(out, 0, sizeof *out);
    out->total_ms = t.total_ms;
    out->render_ms_max = t.render_ms_max;
    out->render_ms_min = t.render_ms_min;
    out->gather_ms = t.gather_ms;
    out->unpack_ms = t.unpack_ms;
    out->wait_ms = t.wait_ms;
    out->collectives = t.collectives;
    out->slowest_device = t.slowest_device;
    out->ngpus = t.ngpus;
    return RT_OK;
}
int rt_multi_ngpus(const rt_multi* m) {
    if (!m) return fail(RT_E_INVALID, "multi is NULL");
    return m->renderer->ngpus();
}

// ---------------------------------------------------------------------------------------------- graph builder
rt_graph* rt_graph_new(void) {
    try {
        return new rt_graph();
    } catch (...) {
        fail(RT_E_INTERNAL, "out of memory");
        return nullptr;
    }
}
void rt_graph_free(rt_graph* g) { delete g; }

#define GRAPH_CALL(expr)                                                \
    do {                                                                \
        if (!g) return fail(RT_E_INVALID, "graph is NULL");             \
        return guard(RT_E_INVALID, [&] { return static_cast<int>(expr); }); \
    } while (0)

namespace {
void check_tex(const rt_graph* g, int t) {
    if (t < 0 || t >= static_cast<int>(g->g.textures.size())) throw std::runtime_error("bad texture id");
}
void check_mat(const rt_graph* g, int m) {
    if (m < 0 || m >= static_cast<int>(g->g.materials.size())) throw std::runtime_error("bad material id");
}
void check_obj(const rt_graph* g, int o) {
    if (o < 0 || o >= static_cast<int>(g->g.nodes.size())) throw std::runtime_error("bad object id");
}
std::vector<int> items_of(const rt_graph* g, int n, const int* items) {
    if (n < 0 || (n > 0 && !items)) throw std::runtime_error("bad item list");
    std::vector<int> v(items, items + n);
    for (int o : v) check_obj(g, o);
    return v;
}
}  // namespace

int rt_graph_random_double(rt_graph* g, double* out) {
    if (!g || !out) return fail(RT_E_INVALID, "graph/out is NULL");
    *out = g->g.rng.d();
    return RT_OK;
}
int rt_tex_solid(rt_graph* g, double r, double gr, double b) { GRAPH_CALL(g->g.solid(art::Vec3(r, gr, b))); }
int rt_tex_checker(rt_graph* g, int even, int odd) {
    GRAPH_CALL((check_tex(g, even), check_tex(g, odd), g->g.checker(even, odd)));
}
int rt_tex_noise(rt_graph* g, double scale) { GRAPH_CALL(g->g.noise(scale)); }
int rt_tex_image(rt_graph* g, int w, int h, int bpp, const uint8_t* texels) {
    GRAPH_CALL(([&] {
        if (w <= 0 || h <= 0 || bpp < 3 || !texels) throw std::runtime_error("bad image");
        art::Image im;
        im.w = w;
        im.h = h;
        im.bpp = bpp;
        im.data.assign(texels, texels + static_cast<size_t>(w) * h * bpp);
        return g->g.image(std::move(im));
    }()));
}
int rt_tex_bary_image(rt_graph* g, const double uv[6], int image_tex) {
    GRAPH_CALL(([&] {
        if (!uv) throw std::runtime_error("uv is NULL");
        check_tex(g, image_tex);
        if (g->g.textures[image_tex].type != art::TEX_IMAGE) throw std::runtime_error("image_tex must be an rt_tex_image texture");
        return g->g.bary_image(uv[0], uv[1], uv[2], uv[3], uv[4], uv[5], image_tex);
    }()));
}
int rt_mesh_parse(const char* obj_path, int64_t* triangles, int64_t* shapes) {
    if (!obj_path) return fail(RT_E_INVALID, "obj_path is NULL");
    return guard(RT_E_SCENE, [&] {
        const art::ObjMesh m = art::load_obj(obj_path);
        if (triangles) *triangles = static_cast<int64_t>(m.tri.size() / 3);
        if (shapes) *shapes = static_cast<int64_t>(m.shapes);
        return RT_OK;
    });
}
int rt_mesh_build(rt_graph* g, const char* obj_path, int* first_id) {
    if (!g || !obj_path) return fail(RT_E_INVALID, "graph/obj_path is NULL");
    return guard(RT_E_SCENE, [&] {
        const std::vector<int> ids = art::build_mesh(g->g, art::load_obj(obj_path));
        if (first_id) *first_id = ids.empty() ? static_cast<int>(g->g.nodes.size()) : ids.front();
        return static_cast<int>(ids.size());
    });
}
int rt_mat_lambertian(rt_graph* g, int tex) { GRAPH_CALL((check_tex(g, tex), g->g.lambertian(tex))); }
int rt_mat_metal(rt_graph* g, double r, double gr, double b, double fuzz) { GRAPH_CALL(g->g.metal(art::Vec3(r, gr, b), fuzz)); }
int rt_mat_dielectric(rt_graph* g, double ir) { GRAPH_CALL(g->g.dielectric(ir)); }
int rt_mat_diffuse_light(rt_graph* g, int tex) { GRAPH_CALL((check_tex(g, tex), g->g.diffuse_light(tex))); }
int rt_obj_sphere(rt_graph* g, const double c[3], double r, int mat) { GRAPH_CALL((check_mat(g, mat), g->g.sphere(v3(c), r, mat))); }
int rt_obj_moving_sphere(rt_graph* g, const double c0[3], const double c1[3], double t0, double t1, double r, int mat) {
    GRAPH_CALL((check_mat(g, mat), g->g.moving_sphere(v3(c0), v3(c1), t0, t1, r, mat)));
}
int rt_obj_triangle(rt_graph* g, const double p1[3], const double p2[3], const double p3[3], int mat) {
    GRAPH_CALL((check_mat(g, mat), g->g.triangle(v3(p1), v3(p2), v3(p3), mat)));
}
int rt_obj_rect(rt_graph* g, int axis, double a0, double a1, double b0, double b1, double k, int mat) {
    GRAPH_CALL(([&] {
        if (axis < 0 || axis > 2) throw std::runtime_error("rect axis must be 0 (xy), 1 (xz) or 2 (yz)");
        check_mat(g, mat);
        return g->g.rect(axis, a0, a1, b0, b1, k, mat);
    }()));
}
int rt_obj_box(rt_graph* g, const double p0[3], const double p1[3], int mat) { GRAPH_CALL((check_mat(g, mat), g->g.box(v3(p0), v3(p1), mat))); }
int rt_obj_list(rt_graph* g, int n, const int* items) { GRAPH_CALL(g->g.list(items_of(g, n, items))); }
int rt_obj_bvh(rt_graph* g, int n, const int* items) { GRAPH_CALL(g->g.bvh(items_of(g, n, items))); }
int rt_obj_translate(rt_graph* g, int child, const double offset[3]) { GRAPH_CALL((check_obj(g, child), g->g.translate(child, v3(offset)))); }
int rt_obj_rotate_y(rt_graph* g, int child, double degrees) { GRAPH_CALL((check_obj(g, child), g->g.rotate_y(child, degrees))); }
int rt_obj_constant_medium(rt_graph* g, int boundary, double density, int tex) {
    GRAPH_CALL((check_obj(g, boundary), check_tex(g, tex), g->g.constant_medium(boundary, density, tex)));
}
int rt_graph_add_world(rt_graph* g, int obj) {
    GRAPH_CALL((check_obj(g, obj), g->g.world.push_back(obj), static_cast<int>(g->g.world.size()) - 1));
}
int rt_graph_clear_world(rt_graph* g) {
    if (!g) return fail(RT_E_INVALID, "graph is NULL");
    g->g.world.clear();
    return RT_OK;
}
int rt_graph_set_view(rt_graph* g, const double lookfrom[3], const double lookat[3], double vfov, double aperture, const double background[3]) {
    if (!g || !lookfrom || !lookat || !background) return fail(RT_E_INVALID, "NULL argument");
    g->g.lookfrom = v3(lookfrom);
    g->g.lookat = v3(lookat);
    g->g.vfov = vfov;
    g->g.aperture = aperture;
    g->g.background = v3(background);
    return RT_OK;
}
int rt_graph_compile(rt_graph* g, int device, rt_scene** out) {
    if (!g || !out) return fail(RT_E_INVALID, "graph and out must be non-NULL");
    *out = nullptr;
    return guard(RT_E_SCENE, [&] { return scene_from_graph(g->g, device, out); });
}

}  // extern "C"

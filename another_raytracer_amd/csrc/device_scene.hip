// device_scene.hip — FlatScene -> DeviceScene: the layout.h LDS scene image, the leaf layouts the kernels read and
// the upload.  Host code only.
#include "device_scene.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <unordered_map>

#include "lds_image.h"
#include "options.h"
#include "tile_lists.h"

namespace art {

// Builds the layout.h LDS scene image when the f64 scene qualifies: spheres only, every BVH node and leaf slot within
// the plane capacities, and image + stack within one CU's LDS.  Returns an empty vector otherwise.  What follows a
// sphere's centre and radius or a node's boxes is lds_image.h's text, which rt_scene_update_spheres' kernels run too.
std::vector<uint8_t> build_lds_image(const FlatScene& f, uint32_t& nmov, bool& shade_ok, uint32_t& tile_reps) {
    std::vector<uint8_t> img;
    nmov = 0;
    tile_reps = 0;
    shade_ok = false;
    if ((f.features & ~kFeatSpheres) != 0 || f.nodes.empty() || f.nodes.size() > kLdsNodeCap || f.primrefs.size() > kLdsSlotCap ||
        f.world.size() > kPathsWorldCap || f.objs.size() > kPathsWorldCap ||
        f.spheres.size() > kLdsRefIndexMask || std::max(extend_lds_bytes(true, stack_rows(f.max_stack)), paths_lds_bytes(stack_rows(f.max_stack))) > kLdsPerCu)
        return img;
    // k_paths shades a hit by its LDS leaf slot: every world object must be a BVH over the image's slots (a loose
    // OBJ_PRIM object, e.g. with option compile.world_merge = 0 or from a flat-scene file, takes the HBM kernels)
    for (int32_t w : f.world)
        if (w < 0 || static_cast<size_t>(w) >= f.objs.size() || f.objs[w].kind != OBJ_BVH) return img;
    for (uint32_t ref : f.primrefs) {
        if (primref_type(ref) != PRIM_SPHERE) return img;
        const SphereRec& sp = f.spheres[primref_index(ref)];
        if (sp.flags & SPH_MOVING) {
            // the image's moving spheres span the unit shutter (every moving_sphere of the reference scenes,
            // scene_manager.cpp:34-35, :201): their centre fraction is the ray time itself (hit_lds_slot); and they
            // move along y only (scene_manager.cpp:33): the image keeps one dy per leaf slot (layout.h)
            if (sp.t0 != 0.0 || sp.dt != 1.0 || sp.d[0] != 0.0 || sp.d[2] != 0.0) return img;
            ++nmov;
        }
    }
    if (nmov > kLdsMovCap) return img;
    for (const BvhNode& b : f.nodes)
        for (int c = 0; c < 4; ++c)
            if (b.child[c] < 0 && b.child[c] != kNodeEmpty && leaf_count(b.child[c]) > kLdsLeafMaxCount) return img;
    img.assign(kLdsImageBytes, 0);
    auto put = [&](uint32_t off, const void* v, size_t n) { std::memcpy(img.data() + off, v, n); };
    for (size_t n = 0; n < f.nodes.size(); ++n) {
        const BvhNode& b = f.nodes[n];
        int32_t child[4];
        for (int c = 0; c < 4; ++c) {
            // an empty slot becomes an empty leaf behind image_put_node_boxes' point box
            const bool empty = b.child[c] == kNodeEmpty;
            // inner nodes by their byte offset in a plane (index * 16: device.h traverse), leaves as lds_leaf codes
            child[c] = empty ? kLdsEmptyChild : b.child[c] >= 0 ? b.child[c] * 16 : lds_leaf(leaf_first(b.child[c]), leaf_count(b.child[c]));
        }
        // the nine box planes, then the child codes as int16
        const uint32_t nn = static_cast<uint32_t>(n);
        image_put_node_boxes(img.data(), nn, b);
        const int16_t c16[8] = {static_cast<int16_t>(child[0]), static_cast<int16_t>(child[1]), static_cast<int16_t>(child[2]),
                                static_cast<int16_t>(child[3]), 0, 0, 0, 0};
        put(kLdsOffNodes + (kLdsNodePlaneChild * kLdsNodeCap + nn) * 16, c16, 16);
    }
    // shading table: one entry per material (two for a checker of solid colours); anything else keeps the scene off
    // the fused variant (shade_ok = false), which shades from the global scene records instead.  Which entry a material
    // gets and what the entry holds are lds_image.h's text, which rt_scene_update_materials / _textures run too.
    std::vector<int32_t> entry(f.mats.size(), -1);
    image_material_entries(f.primrefs.data(), f.primrefs.size(), f.spheres.data(), f.mats.data(), f.mats.size(), f.texs.data(), f.texs.size(),
                           entry.data(), shade_ok);
    for (size_t k = 0; k < f.mats.size(); ++k) image_put_material(img.data(), entry[k], f.mats[k], f.texs.data());
    uint32_t m = 0;
    for (size_t slot = 0; slot < f.primrefs.size(); ++slot) {
        const uint32_t idx = primref_index(f.primrefs[slot]);
        const auto& sp = f.spheres[idx];
        const bool moving = (sp.flags & SPH_MOVING) != 0;
        const uint32_t sl = static_cast<uint32_t>(slot);
        image_put_sphere(img.data(), sl, sp);
        uint32_t code = idx | (f.mats[sp.mat].type << kLdsRefMatShift);
        const double dy = moving ? sp.d[1] : -0.0;
        put(kLdsOffMov + sl * 8, &dy, 8);
        if (moving) {
            code |= (m + 1) << kLdsRefMovShift;
            ++m;
        }
        put(kLdsOffRef + sl * 4, &code, 4);
        const uint16_t mi = static_cast<uint16_t>(entry[sp.mat] < 0 ? 0 : entry[sp.mat]);
        put(kLdsOffMatIdx + sl * 2, &mi, 2);
    }
    // Behind the image: one representative slot per sphere (tile_lists.h TileReps; spatial splits put a sphere into
    // several leaves), the lowest slot whose index field names it.  k_paths' tile lists test representatives only and
    // shade by them, so every slot of a sphere must hold the representative's bytes in every per-slot plane; the
    // world holds nothing but BVHs over these slots (checked above).  Otherwise n stays 0: no lists.
    TileReps reps{};
    {
        std::unordered_map<uint32_t, uint32_t> first;  // sphere index -> representative slot
        bool same = shade_ok;
        auto eq = [&](uint32_t off, uint32_t stride, uint32_t a, uint32_t b) { return std::memcmp(img.data() + off + a * stride, img.data() + off + b * stride, stride) == 0; };
        for (uint32_t sl = 0; sl < f.primrefs.size(); ++sl) {
            const uint32_t idx = primref_index(f.primrefs[sl]);
            const auto it = first.find(idx);
            if (it == first.end()) {
                first.emplace(idx, sl);
                reps.slot[reps.n++] = static_cast<uint16_t>(sl);
                continue;
            }
            const uint32_t r = it->second;
            same = same && eq(kLdsOffSph, 16, sl, r) && eq(kLdsOffSph + kLdsSlotCap * 16, 16, sl, r) && eq(kLdsOffMov, 8, sl, r) &&
                   eq(kLdsOffRef, 4, sl, r) && eq(kLdsOffMatIdx, 2, sl, r) && eq(kLdsOffInvR, 8, sl, r);
        }
        if (!same) reps.n = 0;
    }
    img.resize(kLdsImageBytes + sizeof(TileReps));
    std::memcpy(img.data() + kLdsImageBytes, &reps, sizeof reps);
    tile_reps = reps.n;
    return img;
}


// The 16-bit child codes (layout.h make_leaf16) of a BVH whose leaves start past slot 8191 (more than 8192 primitive
// references: the capsule's 10 200 triangles) do not fit; with every leaf moved to an even slot of a padded copy of
// the primitive references they do, as first / 2 (F_LEAF2).  Rewrites the device copies of the leaf codes (nodes and
// hoisted leaves) and returns the padded references (pad[i]: slot i belongs to no leaf, its records stay zero), or
// an empty vector when the leaves overlap or the padded codes still do not fit.  A leaf tests the same primitives in
// the same order, so every closest hit, and the image, is unchanged.
static std::vector<uint32_t> pair_align_leaves(const std::vector<uint32_t>& primrefs, std::vector<BvhNode>& nodes,
                                               std::vector<ObjRec>& objs, std::vector<uint8_t>& pad) {
    std::vector<std::pair<uint32_t, uint32_t>> leaves;  // (first, count)
    for (const BvhNode& b : nodes)
        for (int c = 0; c < 4; ++c)
            if (b.child[c] < 0 && b.child[c] != kNodeEmpty) leaves.emplace_back(leaf_first(b.child[c]), leaf_count(b.child[c]));
    for (const auto& o : objs)
        if (o.kind == OBJ_BVH && o.b != kNodeEmpty) leaves.emplace_back(leaf_first(o.b), leaf_count(o.b));
    std::sort(leaves.begin(), leaves.end());
    leaves.erase(std::unique(leaves.begin(), leaves.end()), leaves.end());
    std::unordered_map<uint32_t, uint32_t> moved;  // old first -> new first
    std::vector<uint32_t> out;
    pad.clear();
    uint32_t next = 0;  // first old slot not yet copied
    for (const auto& lf : leaves) {
        if (lf.first < next || lf.second < 1 || lf.second > 4 || lf.first + lf.second > primrefs.size()) return {};
        for (; next < lf.first; ++next) {  // slots outside every leaf keep their order
            out.push_back(primrefs[next]);
            pad.push_back(0);
        }
        if (out.size() & 1u) {
            out.push_back(0u);
            pad.push_back(1);
        }
        moved[lf.first] = static_cast<uint32_t>(out.size());
        if (!leaf16_ok(static_cast<uint32_t>(out.size()) >> 1, lf.second)) return {};
        for (uint32_t k = 0; k < lf.second; ++k) {
            out.push_back(primrefs[lf.first + k]);
            pad.push_back(0);
        }
        next = lf.first + lf.second;
    }
    for (; next < primrefs.size(); ++next) {
        out.push_back(primrefs[next]);
        pad.push_back(0);
    }
    auto remap = [&](int32_t c) { return make_leaf(moved.at(leaf_first(c)), leaf_count(c)); };
    for (BvhNode& b : nodes)
        for (int c = 0; c < 4; ++c)
            if (b.child[c] < 0 && b.child[c] != kNodeEmpty) b.child[c] = remap(b.child[c]);
    for (auto& o : objs)
        if (o.kind == OBJ_BVH && o.b != kNodeEmpty) o.b = remap(o.b);
    return out;
}

void build_device_scene(const FlatScene& f0, DeviceScene& ds) {
    // the device copy of the BVH arrays, with leaves pair-aligned where 16-bit codes need it (pair_align_leaves)
    FlatScene f = f0;
    std::vector<uint8_t> slot_pad(f.primrefs.size(), 0);
    {
        bool fit = f.nodes.size() <= 32768u;
        for (const BvhNode& b : f.nodes)
            for (int c = 0; c < 4; ++c)
                if (b.child[c] < 0 && b.child[c] != kNodeEmpty) fit = fit && leaf16_ok(leaf_first(b.child[c]), leaf_count(b.child[c]));
        for (const auto& o : f.objs)
            if (o.kind == OBJ_BVH && o.b != kNodeEmpty) fit = fit && leaf16_ok(leaf_first(o.b), leaf_count(o.b));
        ds.leaf_shift = 0;
        // only where an F_LEAF2 kernel exists (mesh feature sets with triangles: launch_paths_g); other kernels decode
        // 16-bit leaves unshifted
        const bool mesh = (f.features & ~kFeatMesh) == 0 && (f.features & F_TRI) != 0;
        if (!fit && mesh && f.nodes.size() <= 32768u && opt(Opt::Leaf2) != 0) {
            std::vector<BvhNode> nodes = f.nodes;
            std::vector<ObjRec> objs = f.objs;
            std::vector<uint8_t> pad;
            std::vector<uint32_t> refs = pair_align_leaves(f.primrefs, nodes, objs, pad);
            if (!refs.empty()) {
                f.primrefs = std::move(refs);
                f.nodes = std::move(nodes);
                f.objs = std::move(objs);
                slot_pad = std::move(pad);
                ds.leaf_shift = 1;
            }
        }
    }
    // the records go up as the flat scene holds them (f64 throughout), with their pad words zeroed
    for (auto& t : f.tris) t.pad = 0;
    for (auto& b : f.boxes) b.pad = 0;
    for (auto& o : f.objs) o.pad = 0;
    for (auto& t : f.texs) t.pad = 0;
    const std::vector<SphereRec>& sph = f.spheres;
    const std::vector<TriRec>& tri = f.tris;
    const std::vector<RectRec>& rect = f.rects;
    const std::vector<BoxRec>& box = f.boxes;
    const std::vector<ObjRec>& objs = f.objs;
    std::vector<MatRec> mats = f.mats;
    for (MatRec& m : mats) {
        m.pad = 0;
        m.flags &= ~static_cast<uint32_t>(MATF_SOLID);
        const int32_t t = m.tex;
        if ((m.type == MAT_LAMBERTIAN || m.type == MAT_LIGHT || m.type == MAT_ISOTROPIC) && t >= 0 && static_cast<size_t>(t) < f.texs.size() &&
            f.texs[t].type == TEX_SOLID) {
            // the solid colour itself: tex_value's ld3(t.c), the same doubles
            for (int a = 0; a < 3; ++a) m.albedo[a] = f.texs[t].c[a];
            m.flags |= MATF_SOLID;
        }
    }
    ds.view.spheres = ds.upload(sph);
    ds.view.tris = ds.upload(tri);
    ds.view.rects = ds.upload(rect);
    ds.view.boxes = ds.upload(box);
    ds.view.primrefs = ds.upload(f.primrefs);
    ds.slot_refs = f.primrefs;
    ds.slot_pad = slot_pad;
    {  // every scene with a BVH: any kernel instantiated with triangles reads it, whatever the scene holds
        std::vector<TriRec> lt(f.primrefs.size());
        for (size_t i = 0; i < lt.size(); ++i)
            if (!slot_pad[i] && primref_type(f.primrefs[i]) == PRIM_TRIANGLE) lt[i] = tri[primref_index(f.primrefs[i])];
        ds.view.leaf_tris = ds.upload(lt);
        {
            // TriRec112: the plane of each leaf triangle by the device's operations in its order (device.h cross, dot;
            // -ffp-contract=off on both sides): n = cross(p2 - p1, p3 - p1), dd = -dot(n, p1), bit for bit
            std::vector<TriRec112> l112(lt.size());
            for (size_t i = 0; i < lt.size(); ++i) {
                const double* q = lt[i].p;
                const double ux = q[3] - q[0], uy = q[4] - q[1], uz = q[5] - q[2];
                const double vx = q[6] - q[0], vy = q[7] - q[1], vz = q[8] - q[2];
                const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
                for (int k = 0; k < 9; ++k) l112[i].p[k] = q[k];
                l112[i].n[0] = nx;
                l112[i].n[1] = ny;
                l112[i].n[2] = nz;
                l112[i].dd = -(nx * q[0] + ny * q[1] + nz * q[2]);
                l112[i].mat = lt[i].mat;
                l112[i].pad = 0;
            }
            ds.view.leaf_tris112 = ds.upload(l112);
        }
        std::vector<PrimRec80> lp(f.primrefs.size());  // every primitive type in leaf order (triangle-free kernels)
        for (size_t i = 0; i < lp.size(); ++i) {
            if (slot_pad[i]) continue;
            const uint32_t ref = f.primrefs[i], idx = primref_index(ref);
            switch (primref_type(ref)) {
                case PRIM_SPHERE: std::memcpy(lp[i].b, &sph[idx], sizeof(sph[idx])); break;
                case PRIM_TRIANGLE: std::memcpy(lp[i].b, &tri[idx], sizeof(tri[idx])); break;
                case PRIM_RECT: std::memcpy(lp[i].b, &rect[idx], sizeof(rect[idx])); break;
                default: std::memcpy(lp[i].b, &box[idx], sizeof(box[idx])); break;
            }
        }
        ds.view.leaf_prims = ds.upload(lp);
    }
    {  // BvhNode::pad: the 16-bit child codes (layout.h make_leaf16), derived here from the 32-bit ones (never read
       // from a scene file); codes16 when every inner index, leaf and hoisted leaf fits them
        std::vector<BvhNode> nodes = f.nodes;
        bool ok = nodes.size() <= 32768u;
        for (BvhNode& b : nodes) {
            int32_t c16[4];
            for (int c = 0; c < 4; ++c) {
                const int32_t x = b.child[c];
                if (x >= 0) {
                    c16[c] = x;
                } else if (x == kNodeEmpty) {
                    c16[c] = kNodeEmpty;
                } else {
                    ok = ok && leaf16_ok(leaf_first(x) >> ds.leaf_shift, leaf_count(x));
                    c16[c] = ok ? make_leaf16(leaf_first(x) >> ds.leaf_shift, leaf_count(x)) : kNodeEmpty;
                }
            }
            b.pad[0] = static_cast<int32_t>((static_cast<uint32_t>(c16[1]) << 16) | (static_cast<uint32_t>(c16[0]) & 0xFFFFu));
            b.pad[1] = static_cast<int32_t>((static_cast<uint32_t>(c16[3]) << 16) | (static_cast<uint32_t>(c16[2]) & 0xFFFFu));
            b.pad[2] = b.pad[3] = 0;
        }
        for (const auto& o : f.objs)
            if (o.kind == OBJ_BVH && o.b != kNodeEmpty) ok = ok && leaf16_ok(leaf_first(o.b) >> ds.leaf_shift, leaf_count(o.b));
        // option render.codes16 = 0 (read per upload; tests): take the 32-bit-code kernels as a scene whose codes do
        // not fit would (a parity probe of that path on scenes that fit)
        if (opt(Opt::Codes16) == 0) ok = false;
        ds.codes16 = ok;
        if (!ok) ds.leaf_shift = 0;  // the 32-bit codes (child[]) address the padded slots directly
        ds.view.nodes = ds.upload(nodes);
    }
    ds.view.objs = ds.upload(objs);
    {  // obj_prims[o]: prim object o's primitive record (device.h hit_object)
        std::vector<PrimRec80> op(objs.size());
        for (size_t i = 0; i < objs.size(); ++i) {
            if (objs[i].kind != OBJ_PRIM) continue;
            const uint32_t ref = static_cast<uint32_t>(objs[i].a), idx = primref_index(ref);
            switch (primref_type(ref)) {
                case PRIM_SPHERE: std::memcpy(op[i].b, &sph[idx], sizeof(sph[idx])); break;
                case PRIM_TRIANGLE: std::memcpy(op[i].b, &tri[idx], sizeof(tri[idx])); break;
                case PRIM_RECT: std::memcpy(op[i].b, &rect[idx], sizeof(rect[idx])); break;
                default: std::memcpy(op[i].b, &box[idx], sizeof(box[idx])); break;
            }
        }
        ds.view.obj_prims = ds.upload(op);
    }
    ds.view.world = ds.upload(f.world);
    ds.view.mats = ds.upload(mats);
    ds.view.texs = ds.upload(f.texs);
    ds.view.perlins = ds.upload(f.perlins);
    {  // [sphere_uv.h's table][image records]: device.h uv_table reads the table in front of DevScene::images
        std::vector<uint8_t> ib(kUvTableBytes + sizeof(ImageRec) * f.images.size(), 0);
        std::memcpy(ib.data(), glibc_trig_data::kTrigHost, sizeof(glibc_trig_data::kTrigHost));
        if (!f.images.empty()) std::memcpy(ib.data() + kUvTableBytes, f.images.data(), sizeof(ImageRec) * f.images.size());
        ds.view.images = reinterpret_cast<const ImageRec*>(ds.upload(ib) + kUvTableBytes);
    }
    ds.view.texels = ds.upload(f.texels);
    {
        uint32_t nmov = 0;
        bool shade_ok = false;
        uint32_t tile_reps = 0;
        const std::vector<uint8_t> img = ds.leaf_shift ? std::vector<uint8_t>() : build_lds_image(f, nmov, shade_ok, tile_reps);
        ds.tile_reps = img.empty() ? 0 : tile_reps;
        if (!img.empty()) {
            ds.view.lds_image = ds.upload(img);
            ds.lds_scene = true;
            ds.lds_shade = shade_ok;
        }
    }
    ds.view.n_nodes = static_cast<uint32_t>(f.nodes.size());
    ds.view.n_objs = static_cast<uint32_t>(f.objs.size());
    ds.view.n_mats = static_cast<uint32_t>(f.mats.size());
    ds.view.n_primrefs = static_cast<uint32_t>(f.primrefs.size());
    ds.view.n_tris = static_cast<uint32_t>(f.tris.size());
    ds.view.nworld = static_cast<int32_t>(f.world.size());
    for (int a = 0; a < 3; ++a) ds.view.bg[a] = f.background[a];
    ds.media = f.has_media;
    ds.features = f.features;
    ds.max_stack = f.max_stack;
    ds.tex_basic = true;
    for (const auto& t : f.texs) ds.tex_basic = ds.tex_basic && (t.type == TEX_SOLID || t.type == TEX_CHECKER);
    {  // TF_BARY: the texture trees the materials reach hold only solid, checker and barycentric-image nodes (a
       // mesh's bary_image refers to its image texture, which no material samples directly), and no primitive but a
       // triangle samples u, v
        bool bary = !ds.tex_basic;
        std::function<bool(int32_t, int)> tree_ok = [&](int32_t t, int depth) -> bool {
            if (t < 0 || static_cast<size_t>(t) >= f.texs.size()) return true;
            const uint32_t ty = f.texs[t].type;
            if (ty == TEX_SOLID || ty == TEX_BARY_IMAGE) return true;
            return ty == TEX_CHECKER && depth < 4 && tree_ok(f.texs[t].even, depth + 1) && tree_ok(f.texs[t].odd, depth + 1);
        };
        for (const auto& m : f.mats)
            if (m.type == MAT_LAMBERTIAN || m.type == MAT_LIGHT || m.type == MAT_ISOTROPIC) bary = bary && tree_ok(m.tex, 0);
        auto needs_uv = [&](uint32_t m) { return m < f.mats.size() && (f.mats[m].flags & MATF_NEEDS_UV) != 0; };
        for (const auto& p : f.spheres) bary = bary && !needs_uv(p.mat);
        for (const auto& p : f.rects) bary = bary && !needs_uv(p.mat);
        for (const auto& p : f.boxes) bary = bary && !needs_uv(p.mat);
        ds.tex_bary = bary && opt(Opt::TexBary) != 0;
    }
    ds.mat_types = 0;
    for (const auto& m : f.mats) ds.mat_types |= 1u << m.type;
}

}  // namespace art

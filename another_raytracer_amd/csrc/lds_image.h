// lds_image.h — the parts of the layout.h LDS scene image that follow a sphere's centre and radius and a node's child
// boxes, for host (g++, hipcc's host pass) and device code alike: device_scene.hip's builder and refit.hip's
// rt_scene_update_spheres kernels run one text, so an updated image is the image a fresh build makes, byte for byte.
// The same for a material's entry of the shading table (image_put_material: the builder and rt_scene_update_materials /
// _textures' derive pass) and for which entry a material gets (image_material_entries: host only).
// No HIP types (tests/native/lds_image_check.cpp, lds_material_check.cpp).
//
// Both sides compile this with -ffp-contract=off: every expression below is one IEEE operation per operator; the
// division is the language's own (correctly rounded on both sides), not a reciprocal sequence.
#pragma once
#include <cstddef>
#include <cstdint>

#include "layout.h"

namespace art {

// Slot `slot` of the image's sphere planes: (cx, cy), (cz, r * r) and 1 / r.  A moving sphere's x and z at time tm are
// c + tm * (+-0) (moving_sphere.h:72-74) == c + d: the image stores that value (it differs from c only for c = -0 and
// d = +0), and the device adds tm * dy to y alone.  The motion, reference and material planes do not depend on c or r.
ART_HD void image_put_sphere(uint8_t* img, uint32_t slot, const SphereRec& s) {
    const bool moving = (s.flags & SPH_MOVING) != 0;
    const double cx = moving ? s.c[0] + s.d[0] : s.c[0], cz = moving ? s.c[2] + s.d[2] : s.c[2];
    double* p0 = reinterpret_cast<double*>(img + kLdsOffSph + slot * 16);
    double* p1 = reinterpret_cast<double*>(img + kLdsOffSph + (kLdsSlotCap + slot) * 16);
    double* inv_r = reinterpret_cast<double*>(img + kLdsOffInvR + slot * 8);
    p0[0] = cx, p0[1] = s.c[1];
    p1[0] = cz, p1[1] = s.r * s.r;
    *inv_r = 1.0 / s.r;
}

// The nine box planes of node n: per axis lo, hi, lo (layout.h kLdsNodePlanes).  An empty slot becomes a point box at
// (3e38, 3e38, 3e38): no slab test of it needs a child check, and the astronomically rare ray whose three slab times
// coincide there finds no primitives (its child code is an empty leaf).  The child-code plane is the builder's alone.
ART_HD void image_put_plane(uint8_t* img, uint32_t j, uint32_t n, const BvhNode& b, const float v[4]) {
    float* plane = reinterpret_cast<float*>(img + kLdsOffNodes + (j * kLdsNodeCap + n) * 16);
    for (int c = 0; c < 4; ++c) plane[c] = b.child[c] == kNodeEmpty ? kLdsEmptyBox : v[c];
}
ART_HD void image_put_node_boxes(uint8_t* img, uint32_t n, const BvhNode& b) {
    image_put_plane(img, 0, n, b, b.lox), image_put_plane(img, 1, n, b, b.hix), image_put_plane(img, 2, n, b, b.lox);
    image_put_plane(img, 3, n, b, b.loy), image_put_plane(img, 4, n, b, b.hiy), image_put_plane(img, 5, n, b, b.loy);
    image_put_plane(img, 6, n, b, b.loz), image_put_plane(img, 7, n, b, b.hiz), image_put_plane(img, 8, n, b, b.loz);
}

// Entry e of the shading table: (c.x, c.y), (c.z, param), 32 bytes.  An entry past the table's capacity is not written
// (the builder then keeps the scene off the fused variant: image_material_entries' `complete`).
ART_HD void image_put_entry(uint8_t* img, uint32_t e, const double c[3], double param) {
    if (e >= kLdsMatCap) return;
    double* v = reinterpret_cast<double*>(img + kLdsOffMat + e * 32);
    v[0] = c[0], v[1] = c[1], v[2] = c[2], v[3] = param;
}

// The shading-table entries of material m from its record and the textures, at the entry `code` image_material_entries
// gave it (-1: none; entry | kLdsMatChecker: a checker of two solid colours, even at entry, odd at entry + 1):
// a lambertian's / diffuse_light's solid colour (or its checker's two), a metal's albedo and fuzz, a dielectric's
// (1 / ir, r0 front, r0 back, ir) -- material.h:63-99: reflectance()'s r0 = ((1 - ratio) / (1 + ratio))^2 for both
// faces, in IEEE double arithmetic, one operation per operator.
ART_HD void image_put_material(uint8_t* img, int32_t code, const MatRec& m, const TexRec* texs) {
    if (code < 0) return;
    const uint32_t e = static_cast<uint32_t>(code) & ~kLdsMatChecker;
    if (m.type == MAT_LAMBERTIAN || m.type == MAT_LIGHT) {
        const TexRec& t = texs[m.tex];
        if (static_cast<uint32_t>(code) & kLdsMatChecker) {
            image_put_entry(img, e, texs[t.even].c, 0.0);
            image_put_entry(img, e + 1, texs[t.odd].c, 0.0);
        } else {
            image_put_entry(img, e, t.c, 0.0);
        }
    } else if (m.type == MAT_METAL) {
        image_put_entry(img, e, m.albedo, m.fuzz);
    } else if (m.type == MAT_DIELECTRIC) {
        const double inv = 1.0 / m.ir;
        double r0f = (1.0 - inv) / (1.0 + inv), r0b = (1.0 - m.ir) / (1.0 + m.ir);
        r0f = r0f * r0f;
        r0b = r0b * r0b;
        const double d3[3] = {inv, r0f, r0b};
        image_put_entry(img, e, d3, m.ir);
    }
}

// Which entry each material gets (host only): entries are handed out in the order the leaf slots first meet a material --
// one for a lambertian / diffuse_light over a solid colour, for a metal and for a dielectric, two for a lambertian /
// diffuse_light over a checker of two solid colours; any other material met gets none and makes the table incomplete, a
// material no slot uses gets none.  entry[m] (n_mats of them) receives -1 or entry | kLdsMatChecker.  Returns the number
// of entries handed out; complete: every material met has its entries and all of them fit the table.
inline uint32_t image_material_entries(const uint32_t* primrefs, size_t n_slots, const SphereRec* spheres, const MatRec* mats, size_t n_mats,
                                       const TexRec* texs, size_t n_texs, int32_t* entry, bool& complete) {
    for (size_t m = 0; m < n_mats; ++m) entry[m] = -1;
    uint32_t nent = 0;
    complete = true;
    auto solid = [&](int32_t t) { return t >= 0 && static_cast<size_t>(t) < n_texs && texs[t].type == TEX_SOLID; };
    for (size_t slot = 0; slot < n_slots; ++slot) {
        const uint32_t mi = spheres[primref_index(primrefs[slot])].mat;
        if (entry[mi] >= 0) continue;
        const MatRec& mat = mats[mi];
        if (mat.type == MAT_LAMBERTIAN || mat.type == MAT_LIGHT) {
            const TexRec& t = texs[mat.tex];
            if (t.type == TEX_SOLID) {
                entry[mi] = static_cast<int32_t>(nent++);
            } else if (t.type == TEX_CHECKER && solid(t.even) && solid(t.odd)) {
                entry[mi] = static_cast<int32_t>(nent | kLdsMatChecker);
                nent += 2;
            } else {
                complete = false;
            }
        } else if (mat.type == MAT_METAL || mat.type == MAT_DIELECTRIC) {
            entry[mi] = static_cast<int32_t>(nent++);
        } else {
            complete = false;
        }
    }
    if (nent > kLdsMatCap) complete = false;
    return nent;
}

}  // namespace art

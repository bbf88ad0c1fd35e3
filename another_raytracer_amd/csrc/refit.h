// refit.h — the arithmetic a BVH refit shares with the builder, for host (g++) and device (hipcc) code alike: the
// conservative f32 box of an f64 interval (bvh.cpp's boxes and k_refit_level's are one text), the f64 box of a primitive
// from its record (a scene loaded from a file has no graph to ask), the union and the four-child reduction of
// k_refit_level, and the per-level node ranges of a FlatScene.  No HIP types (tests/native/refit_check.cpp).
//
// Both sides compile this with -ffp-contract=off: every expression below is one IEEE operation per operator.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "layout.h"

namespace art {

// (std::max / fmaxf differ on signed zeros and in the headers they need; these are the same text on both sides)
ART_HD float refit_maxf(float a, float b) { return a < b ? b : a; }
ART_HD double refit_min(double a, double b) { return b < a ? b : a; }
ART_HD double refit_max(double a, double b) { return a < b ? b : a; }

// One axis of the conservative box the traversal tests: [mn, mx] converted to f32, stepped one float outward where the
// conversion rounded inward, then padded by 1e-6 of the larger of its magnitude and its extent (the f32 rounding of the
// ray origin / direction and of the slab arithmetic) plus 1e-30.
ART_HD void conservative_interval(double mn, double mx, float& lo, float& hi) {
    float l = static_cast<float>(mn);
    float h = static_cast<float>(mx);
    if (static_cast<double>(l) > mn) l = nextafterf(l, -INFINITY);
    if (static_cast<double>(h) < mx) h = nextafterf(h, INFINITY);
    const float pad = 1e-6f * refit_maxf(refit_maxf(fabsf(l), fabsf(h)), h - l) + 1e-30f;
    lo = l - pad;
    hi = h + pad;
}
ART_HD void conservative_box(const double mn[3], const double mx[3], float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) conservative_interval(mn[k], mx[k], lo[k], hi[k]);
}

// ---------------------------------------------------------------------------------------------- primitive boxes
// b = {min xyz, max xyz}: what SceneGraph::bounding_box(idx, 0, 1) gives the primitive the record was compiled from.
ART_HD void sphere_box(const SphereRec& s, double b[6]) {
    if (s.flags & SPH_MOVING) {  // moving_sphere.h:61-70 over the unit shutter: the boxes at t = 0 and t = 1
        const double f0 = (0.0 - s.t0) / s.dt, f1 = (1.0 - s.t0) / s.dt;
        for (int a = 0; a < 3; ++a) {
            const double c0 = s.c[a] + f0 * s.d[a], c1 = s.c[a] + f1 * s.d[a];
            b[a] = refit_min(c0 - s.r, c1 - s.r);
            b[3 + a] = refit_max(c0 + s.r, c1 + s.r);
        }
        return;
    }
    for (int a = 0; a < 3; ++a) {
        b[a] = s.c[a] - s.r;
        b[3 + a] = s.c[a] + s.r;
    }
}
ART_HD void tri_box(const double p[9], double b[6]) {
    for (int a = 0; a < 3; ++a) {
        b[a] = refit_min(p[a], refit_min(p[3 + a], p[6 + a]));
        b[3 + a] = refit_max(p[a], refit_max(p[3 + a], p[6 + a]));
    }
}
ART_HD void rect_box(const RectRec& r, double b[6]) {  // aarect.h:16-21, :37-42, :58-63
    const int ka = r.axis == 0 ? 2 : r.axis == 1 ? 1 : 0;
    const int ia = r.axis == 2 ? 1 : 0;
    const int ib = r.axis == 0 ? 1 : 2;
    b[ia] = r.a0, b[3 + ia] = r.a1;
    b[ib] = r.b0, b[3 + ib] = r.b1;
    b[ka] = r.k - 0.0001, b[3 + ka] = r.k + 0.0001;
}
ART_HD void box_box(const BoxRec& x, double b[6]) {
    for (int a = 0; a < 3; ++a) {
        b[a] = x.mn[a];
        b[3 + a] = x.mx[a];
    }
}
ART_HD void empty_box6(double b[6]) {
    for (int a = 0; a < 3; ++a) {
        b[a] = INFINITY;
        b[3 + a] = -INFINITY;
    }
}
ART_HD void grow_box6(double b[6], const double o[6]) {
    for (int a = 0; a < 3; ++a) {
        b[a] = refit_min(b[a], o[a]);
        b[3 + a] = refit_max(b[3 + a], o[3 + a]);
    }
}

// ---------------------------------------------------------------------------------------------- one child of a node
// Child c of node n, refitted from what lies below it (k_refit_level's lane; the host model of the tests runs the same
// text).  A leaf: the conservative box of the union of its slots' f64 boxes.  An inner child: the component-wise
// min / max over the four child boxes of its node, which are padded f32 boxes already -- their union is exact in f32
// and needs no second pad; empty slots hold +FLT_MAX / -FLT_MAX and drop out.  An empty child, and a code that points
// outside the arrays, keeps its box.
ART_HD void refit_child(BvhNode* nodes, uint32_t n_nodes, const double* slot_box, uint32_t n_slots, uint32_t n, int c) {
    BvhNode& me = nodes[n];
    const int32_t code = me.child[c];
    if (code == kNodeEmpty) return;
    float lo[3], hi[3];
    if (code < 0) {
        const uint32_t first = leaf_first(code), count = leaf_count(code);
        if (count == 0 || first + count > n_slots) return;
        double b[6];
        empty_box6(b);
        for (uint32_t k = 0; k < count; ++k) grow_box6(b, slot_box + 6 * static_cast<size_t>(first + k));
        conservative_box(b, b + 3, lo, hi);
    } else {
        if (static_cast<uint32_t>(code) >= n_nodes || static_cast<uint32_t>(code) <= n) return;
        const BvhNode& k = nodes[code];
        lo[0] = k.lox[0], hi[0] = k.hix[0];
        lo[1] = k.loy[0], hi[1] = k.hiy[0];
        lo[2] = k.loz[0], hi[2] = k.hiz[0];
        for (int j = 1; j < 4; ++j) {
            lo[0] = k.lox[j] < lo[0] ? k.lox[j] : lo[0], hi[0] = hi[0] < k.hix[j] ? k.hix[j] : hi[0];
            lo[1] = k.loy[j] < lo[1] ? k.loy[j] : lo[1], hi[1] = hi[1] < k.hiy[j] ? k.hiy[j] : hi[1];
            lo[2] = k.loz[j] < lo[2] ? k.loz[j] : lo[2], hi[2] = hi[2] < k.hiz[j] ? k.hiz[j] : hi[2];
        }
    }
    me.lox[c] = lo[0], me.hix[c] = hi[0];
    me.loy[c] = lo[1], me.hiy[c] = hi[1];
    me.loz[c] = lo[2], me.hiz[c] = hi[2];
}

// ---------------------------------------------------------------------------------------------- levels (host)
// Level l of the node array is [begin[l], begin[l + 1]): scene.cpp's relabel_level_major stores the nodes of all BVHs
// in BFS order over all roots, so a level is a contiguous range and every inner child has a higher index than its
// parent.  A refit runs the levels from the last to the first.  Throws when the array is not in that order (a node
// below its parent's level range, a child index not above its parent's).
inline std::vector<uint32_t> refit_levels(const std::vector<BvhNode>& nodes, const std::vector<ObjRec>& objs) {
    const size_t n = nodes.size();
    std::vector<uint32_t> begin;
    if (n == 0) return begin;
    std::vector<int32_t> depth(n, -1);
    for (const ObjRec& o : objs)
        if (o.kind == OBJ_BVH && o.a >= 0 && static_cast<size_t>(o.a) < n) depth[static_cast<size_t>(o.a)] = 0;
    int32_t last = 0;
    for (size_t i = 0; i < n; ++i) {
        if (depth[i] < 0) depth[i] = last;  // a node no root reaches: harmless wherever it is refitted
        if (depth[i] < last) throw std::runtime_error("refit: the BVH nodes are not stored level by level");
        if (depth[i] > last || begin.empty()) begin.push_back(static_cast<uint32_t>(i));
        last = depth[i];
        for (int c = 0; c < 4; ++c) {
            const int32_t k = nodes[i].child[c];
            if (k < 0) continue;
            if (static_cast<size_t>(k) <= i || static_cast<size_t>(k) >= n) throw std::runtime_error("refit: a BVH child does not lie below its parent");
            depth[static_cast<size_t>(k)] = depth[i] + 1;
        }
    }
    begin.push_back(static_cast<uint32_t>(n));
    return begin;
}

}  // namespace art

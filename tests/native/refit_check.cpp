// refit.h on the host (g++ -ffp-contract=off, as the library builds it): conservative_box against an independent
// restatement over a sweep of doubles, and a host model of the level refit on a hand-made three-level node array with an
// empty slot and a four-primitive leaf.  Prints "ok" or the first failure.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "refit.h"

using namespace art;

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// The documented formula restated with long-double compares and arithmetic: l is the largest float <= mn, h the smallest
// float >= mx, pad = fl(fl(1e-6f * max(max(|l|, |h|), fl(h - l))) + 1e-30f), lo = fl(l - pad), hi = fl(h + pad).  Every
// product, sum and difference of two floats formed here is exact in long double (a float pair's exponents lie within
// its 64 bits wherever the smaller operand can still change the rounded result), so one conversion rounds once.
static bool check_interval(double mn, double mx) {
    float lo, hi;
    conservative_interval(mn, mx, lo, hi);
    const long double lmn = mn, lmx = mx;
    float l = static_cast<float>(mn), h = static_cast<float>(mx);
    while (static_cast<long double>(l) > lmn) l = nextafterf(l, -INFINITY);
    while (static_cast<long double>(nextafterf(l, INFINITY)) <= lmn) l = nextafterf(l, INFINITY);
    while (static_cast<long double>(h) < lmx) h = nextafterf(h, INFINITY);
    while (static_cast<long double>(nextafterf(h, -INFINITY)) >= lmx) h = nextafterf(h, -INFINITY);
    const long double ext = static_cast<float>(static_cast<long double>(h) - static_cast<long double>(l));
    long double m = std::fabs(static_cast<long double>(l));
    if (std::fabs(static_cast<long double>(h)) > m) m = std::fabs(static_cast<long double>(h));
    if (ext > m) m = ext;
    const float prod = static_cast<float>(static_cast<long double>(1e-6f) * m);
    const float pad = static_cast<float>(static_cast<long double>(prod) + static_cast<long double>(1e-30f));
    const float want_lo = static_cast<float>(static_cast<long double>(l) - static_cast<long double>(pad));
    const float want_hi = static_cast<float>(static_cast<long double>(h) + static_cast<long double>(pad));
    if (!same_bits(lo, want_lo) || !same_bits(hi, want_hi)) {
        std::printf("FAIL formula [%a, %a]: got [%a, %a], the formula gives [%a, %a]\n", mn, mx, lo, hi, want_lo, want_hi);
        return false;
    }
    if (!(static_cast<long double>(lo) < lmn && static_cast<long double>(hi) > lmx)) {
        std::printf("FAIL containment [%a, %a] in [%a, %a]\n", mn, mx, lo, hi);
        return false;
    }
    return true;
}

static bool check_conservative_box() {
    std::vector<double> vals = {0.0, -0.0, 1e30, -1e30, 1e-30, -1e-30};
    const float seeds[] = {1.0f, 1.5f, 0.1f, 3.14159274f, 1000.0f, 123456.789f, 16777216.0f, 1e-6f, 5e-20f, 7.25e12f, 0.333333343f, 2.0f};
    for (float f : seeds)
        for (int sign = 0; sign < 2; ++sign) {
            const double v = sign ? -static_cast<double>(f) : static_cast<double>(f);
            vals.push_back(v);                               // exactly an f32
            vals.push_back(std::nextafter(v, INFINITY));     // one f64 ulp either side of it
            vals.push_back(std::nextafter(v, -INFINITY));
            vals.push_back(v * (1.0 + 0x1p-30));             // between two floats, nearer the lower
            vals.push_back(v * (1.0 + 0x1.8p-24));           // ... and nearer the upper
        }
    size_t n = 0;
    for (double a : vals)
        for (double b : vals) {
            if (a > b) continue;
            if (!check_interval(a, b)) return false;
            ++n;
        }
    if (n < 1000) {
        std::printf("FAIL the sweep holds %zu intervals\n", n);
        return false;
    }
    // the three-axis form is the interval per axis
    const double mn[3] = {-1.0000000001, 2.5, -1e30}, mx[3] = {1.0000000001, 2.5, 1e-30};
    float lo[3], hi[3];
    conservative_box(mn, mx, lo, hi);
    for (int k = 0; k < 3; ++k) {
        float l, h;
        conservative_interval(mn[k], mx[k], l, h);
        if (!same_bits(l, lo[k]) || !same_bits(h, hi[k])) {
            std::printf("FAIL conservative_box axis %d\n", k);
            return false;
        }
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ the level refit
static void child_box(const BvhNode& n, int c, float lo[3], float hi[3]) {
    lo[0] = n.lox[c], hi[0] = n.hix[c], lo[1] = n.loy[c], hi[1] = n.hiy[c], lo[2] = n.loz[c], hi[2] = n.hiz[c];
}
// every slot below child c of node n lies inside [lo, hi]
static bool contains_below(const std::vector<BvhNode>& nodes, const std::vector<double>& slot_box, uint32_t n, int c, const float lo[3], const float hi[3]) {
    const int32_t code = nodes[n].child[c];
    if (code == kNodeEmpty) return true;
    if (code < 0) {
        for (uint32_t s = leaf_first(code); s < leaf_first(code) + leaf_count(code); ++s)
            for (int a = 0; a < 3; ++a)
                if (!(static_cast<double>(lo[a]) < slot_box[6 * s + a] && static_cast<double>(hi[a]) > slot_box[6 * s + 3 + a])) return false;
        return true;
    }
    for (int j = 0; j < 4; ++j)
        if (!contains_below(nodes, slot_box, static_cast<uint32_t>(code), j, lo, hi)) return false;
    return true;
}

static bool check_level_refit() {
    // 13 slots with hand-made f64 boxes (values that are no floats, a degenerate flat one, far-apart ones)
    std::vector<double> slot_box;
    for (int s = 0; s < 13; ++s) {
        const double x = -7.1 + 1.3 * s, y = 0.1 * s * s - 3.3, z = (s % 3) * 1e3 + 1.0 / 3.0;
        const double b[6] = {x, y, z, x + 0.7 + 0.01 * s, s == 5 ? y : y + 2.0 / 7.0, z + 1e-9 * (s + 1)};
        slot_box.insert(slot_box.end(), b, b + 6);
    }
    // level 0: node 0; level 1: nodes 1, 2; level 2: node 3
    std::vector<BvhNode> nodes(4);
    const int32_t codes[4][4] = {{1, 2, make_leaf(0, 1), kNodeEmpty},
                                 {3, make_leaf(1, 4), make_leaf(5, 2), kNodeEmpty},
                                 {make_leaf(7, 1), make_leaf(8, 2), kNodeEmpty, kNodeEmpty},
                                 {make_leaf(10, 1), make_leaf(11, 1), make_leaf(12, 1), kNodeEmpty}};
    for (int n = 0; n < 4; ++n)
        for (int c = 0; c < 4; ++c) {
            nodes[n].child[c] = codes[n][c];
            const bool empty = codes[n][c] == kNodeEmpty;
            // stale boxes: a point at the origin, which contains nothing below; empty slots as the builder leaves them
            nodes[n].lox[c] = nodes[n].loy[c] = nodes[n].loz[c] = empty ? FLT_MAX : 0.0f;
            nodes[n].hix[c] = nodes[n].hiy[c] = nodes[n].hiz[c] = empty ? -FLT_MAX : 0.0f;
        }
    std::vector<ObjRec> objs(1);
    objs[0].kind = OBJ_BVH, objs[0].a = 0, objs[0].b = kNodeEmpty;
    const std::vector<uint32_t> levels = refit_levels(nodes, objs);
    const std::vector<uint32_t> want = {0, 1, 3, 4};
    if (levels != want) {
        std::printf("FAIL level table:");
        for (uint32_t v : levels) std::printf(" %u", v);
        std::printf("\n");
        return false;
    }
    for (size_t l = 0; l + 1 < levels.size(); ++l)  // contiguous, and children lie in the next level
        for (uint32_t n = levels[l]; n < levels[l + 1]; ++n)
            for (int c = 0; c < 4; ++c) {
                const int32_t k = nodes[n].child[c];
                if (k >= 0 && !(l + 2 < levels.size() && static_cast<uint32_t>(k) >= levels[l + 1] && static_cast<uint32_t>(k) < levels[l + 2])) {
                    std::printf("FAIL child %d of node %u is not in the level below\n", k, n);
                    return false;
                }
            }
    for (size_t l = levels.size(); l-- > 1;)
        for (uint32_t n = levels[l - 1]; n < levels[l]; ++n)
            for (int c = 0; c < 4; ++c) refit_child(nodes.data(), 4, slot_box.data(), 13, n, c);
    for (uint32_t n = 0; n < 4; ++n)
        for (int c = 0; c < 4; ++c) {
            float lo[3], hi[3];
            child_box(nodes[n], c, lo, hi);
            const int32_t code = nodes[n].child[c];
            if (code == kNodeEmpty) {
                for (int a = 0; a < 3; ++a)
                    if (lo[a] != FLT_MAX || hi[a] != -FLT_MAX) {
                        std::printf("FAIL the empty child %d of node %u changed\n", c, n);
                        return false;
                    }
                continue;
            }
            if (!contains_below(nodes, slot_box, n, c, lo, hi)) {
                std::printf("FAIL child %d of node %u does not contain the boxes below it\n", c, n);
                return false;
            }
            float wl[3], wh[3];
            if (code < 0) {  // a leaf: the conservative box of the union of its slots
                double b[6];
                empty_box6(b);
                for (uint32_t s = leaf_first(code); s < leaf_first(code) + leaf_count(code); ++s) grow_box6(b, slot_box.data() + 6 * s);
                conservative_box(b, b + 3, wl, wh);
            } else {  // an inner child: min / max of its node's non-empty child boxes
                for (int a = 0; a < 3; ++a) wl[a] = FLT_MAX, wh[a] = -FLT_MAX;
                for (int j = 0; j < 4; ++j) {
                    if (nodes[code].child[j] == kNodeEmpty) continue;
                    float kl[3], kh[3];
                    child_box(nodes[code], j, kl, kh);
                    for (int a = 0; a < 3; ++a) wl[a] = std::fmin(wl[a], kl[a]), wh[a] = std::fmax(wh[a], kh[a]);
                }
            }
            for (int a = 0; a < 3; ++a)
                if (!same_bits(lo[a], wl[a]) || !same_bits(hi[a], wh[a])) {
                    std::printf("FAIL child %d of node %u axis %d: [%a, %a], expected [%a, %a]\n", c, n, a, lo[a], hi[a], wl[a], wh[a]);
                    return false;
                }
        }
    // an array that is not level-major is refused
    std::vector<BvhNode> bad = nodes;
    bad[3].child[3] = 1;
    bool threw = false;
    try {
        refit_levels(bad, objs);
    } catch (const std::exception&) {
        threw = true;
    }
    if (!threw) {
        std::printf("FAIL a child above its parent was accepted\n");
        return false;
    }
    return true;
}

// the primitive boxes are the graph's (SceneGraph::bounding_box over the unit shutter), worked out by hand
static bool check_prim_boxes() {
    double b[6];
    SphereRec s{};
    s.c[0] = 1, s.c[1] = 2, s.c[2] = 3, s.r = 0.5;
    sphere_box(s, b);
    const double ws[6] = {0.5, 1.5, 2.5, 1.5, 2.5, 3.5};
    if (std::memcmp(b, ws, sizeof b) != 0) return std::printf("FAIL sphere box\n"), false;
    s.flags = SPH_MOVING, s.d[1] = 0.25, s.t0 = 0, s.dt = 1;  // centre y from 2 to 2.25
    sphere_box(s, b);
    const double wm[6] = {0.5, 1.5, 2.5, 1.5, 2.75, 3.5};
    if (std::memcmp(b, wm, sizeof b) != 0) return std::printf("FAIL moving sphere box\n"), false;
    const double p[9] = {0, 5, -1, 2, -3, 4, -2, 1, 0.5};
    tri_box(p, b);
    const double wt[6] = {-2, -3, -1, 2, 5, 4};
    if (std::memcmp(b, wt, sizeof b) != 0) return std::printf("FAIL triangle box\n"), false;
    const RectRec r{1, 2, 3, 4, 5, 1, 0};  // xz_rect: a = x, b = z, k on y
    rect_box(r, b);
    const double wr[6] = {1, 5 - 0.0001, 3, 2, 5 + 0.0001, 4};
    if (std::memcmp(b, wr, sizeof b) != 0) return std::printf("FAIL rect box\n"), false;
    BoxRec x{};
    x.mn[0] = -1, x.mn[1] = -2, x.mn[2] = -3, x.mx[0] = 1, x.mx[1] = 2, x.mx[2] = 3;
    box_box(x, b);
    const double wb[6] = {-1, -2, -3, 1, 2, 3};
    if (std::memcmp(b, wb, sizeof b) != 0) return std::printf("FAIL box box\n"), false;
    return true;
}

int main() {
    if (!check_conservative_box() || !check_level_refit() || !check_prim_boxes()) return 1;
    std::printf("ok\n");
    return 0;
}

// lds_image.h on the host (g++ -ffp-contract=off, as the library builds it): image_put_sphere and image_put_node_boxes
// against literal expectations -- a static sphere, a moving sphere with c = -0.0 and d = +0.0, a node with an empty
// child, a node updated twice -- and that neither writes a byte outside the planes it owns.  Prints "ok" or the first
// failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lds_image.h"

using namespace art;

static std::vector<uint8_t> g_img(kLdsImageBytes);

static double rd(uint32_t off) {
    double v;
    std::memcpy(&v, g_img.data() + off, 8);
    return v;
}
static float rf(uint32_t off) {
    float v;
    std::memcpy(&v, g_img.data() + off, 4);
    return v;
}
static bool bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool bitsf(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
            return false;                                        \
        }                                                        \
    } while (0)

// every byte outside [lo, hi) ranges listed in `own` still holds the fill
static bool untouched(const std::vector<std::pair<uint32_t, uint32_t>>& own, uint8_t fill) {
    for (uint32_t i = 0; i < kLdsImageBytes; ++i) {
        bool mine = false;
        for (const auto& r : own) mine = mine || (i >= r.first && i < r.second);
        if (!mine && g_img[i] != fill) {
            std::printf("FAIL: byte %u outside the written planes changed\n", i);
            return false;
        }
    }
    return true;
}
static std::vector<std::pair<uint32_t, uint32_t>> sphere_ranges(uint32_t s) {
    return {{kLdsOffSph + s * 16, kLdsOffSph + s * 16 + 16},
            {kLdsOffSph + (kLdsSlotCap + s) * 16, kLdsOffSph + (kLdsSlotCap + s) * 16 + 16},
            {kLdsOffInvR + s * 8, kLdsOffInvR + s * 8 + 8}};
}

static bool check_static_sphere() {
    std::fill(g_img.begin(), g_img.end(), 0xA5);
    SphereRec s{};
    s.c[0] = 1.25, s.c[1] = -2.5, s.c[2] = 1e-3, s.r = 3.0;
    s.d[0] = 7.0, s.d[1] = 8.0, s.d[2] = 9.0;  // not moving: d is ignored
    s.mat = 5, s.flags = 0;
    const uint32_t slot = 37;
    image_put_sphere(g_img.data(), slot, s);
    CHECK(bits(rd(kLdsOffSph + slot * 16), 1.25) && bits(rd(kLdsOffSph + slot * 16 + 8), -2.5));
    CHECK(bits(rd(kLdsOffSph + (kLdsSlotCap + slot) * 16), 1e-3) && bits(rd(kLdsOffSph + (kLdsSlotCap + slot) * 16 + 8), 9.0));
    CHECK(bits(rd(kLdsOffInvR + slot * 8), 0x1.5555555555555p-2));  // 1 / 3, correctly rounded
    return untouched(sphere_ranges(slot), 0xA5);
}

static bool check_moving_sphere_signed_zero() {
    std::fill(g_img.begin(), g_img.end(), 0x00);
    SphereRec s{};
    s.c[0] = -0.0, s.c[1] = 0.2, s.c[2] = -0.0, s.r = 0.2;
    s.d[0] = 0.0, s.d[1] = 0.375, s.d[2] = 0.0;
    s.t0 = 0.0, s.dt = 1.0, s.flags = SPH_MOVING;
    const uint32_t slot = kLdsSlotCap - 1;  // the last slot: the planes' far ends
    image_put_sphere(g_img.data(), slot, s);
    // c + d: -0 + +0 = +0, what the reference's centre(tm) gives at every tm; y stays c.y (dy lives in the Mov plane)
    CHECK(bits(rd(kLdsOffSph + slot * 16), 0.0) && !std::signbit(rd(kLdsOffSph + slot * 16)));
    CHECK(bits(rd(kLdsOffSph + slot * 16 + 8), 0.2));
    CHECK(bits(rd(kLdsOffSph + (kLdsSlotCap + slot) * 16), 0.0) && !std::signbit(rd(kLdsOffSph + (kLdsSlotCap + slot) * 16)));
    CHECK(bits(rd(kLdsOffSph + (kLdsSlotCap + slot) * 16 + 8), 0x1.47ae147ae147cp-5));  // fl(0.2 * 0.2)
    CHECK(bits(rd(kLdsOffInvR + slot * 8), 5.0));
    if (!untouched(sphere_ranges(slot), 0x00)) return false;
    // the same record, not moving: -0 stays -0
    s.flags = 0;
    image_put_sphere(g_img.data(), 0, s);
    CHECK(std::signbit(rd(kLdsOffSph)) && std::signbit(rd(kLdsOffSph + kLdsSlotCap * 16)));
    // a moving sphere with x and z motion (never in an image scene, but the text is the builder's): c + d
    s.flags = SPH_MOVING, s.c[0] = 1.0, s.d[0] = 0.5, s.c[2] = 2.0, s.d[2] = -4.0;
    image_put_sphere(g_img.data(), 1, s);
    CHECK(bits(rd(kLdsOffSph + 16), 1.5) && bits(rd(kLdsOffSph + (kLdsSlotCap + 1) * 16), -2.0));
    return true;
}

static BvhNode node_of(float base) {
    BvhNode b{};
    for (int c = 0; c < 4; ++c) {
        b.lox[c] = base + c, b.hix[c] = base + c + 0.5f;
        b.loy[c] = -base - c, b.hiy[c] = -base - c + 0.25f;
        b.loz[c] = 10 * base + c, b.hiz[c] = 10 * base + c + 2.0f;
        b.child[c] = make_leaf(4 * c, 4);
        b.pad[c] = 0x7777;
    }
    return b;
}
static float plane(uint32_t j, uint32_t n, int c) { return rf(kLdsOffNodes + (j * kLdsNodeCap + n) * 16 + 4 * c); }

static bool node_is(uint32_t n, const BvhNode& b) {
    const float* src[9] = {b.lox, b.hix, b.lox, b.loy, b.hiy, b.loy, b.loz, b.hiz, b.loz};  // per axis: lo, hi, lo
    for (uint32_t j = 0; j < 9; ++j)
        for (int c = 0; c < 4; ++c) {
            const float want = b.child[c] == kNodeEmpty ? 3.0e38f : src[j][c];
            if (!bitsf(plane(j, n, c), want)) {
                std::printf("FAIL node %u plane %u child %d: %a, expected %a\n", n, j, c, plane(j, n, c), want);
                return false;
            }
        }
    return true;
}

static bool check_nodes() {
    std::fill(g_img.begin(), g_img.end(), 0x5A);
    std::vector<std::pair<uint32_t, uint32_t>> own;
    const uint32_t n = kLdsNodeCap - 1;
    for (uint32_t j = 0; j < 9; ++j) own.push_back({kLdsOffNodes + (j * kLdsNodeCap + n) * 16, kLdsOffNodes + (j * kLdsNodeCap + n) * 16 + 16});
    BvhNode b = node_of(1.0f);
    b.child[1] = 7;           // an inner child: its box is copied like a leaf's
    b.child[2] = kNodeEmpty;  // an empty child: the point box at 3e38 on all nine planes, whatever the node holds there
    image_put_node_boxes(g_img.data(), n, b);
    if (!node_is(n, b)) return false;
    CHECK(bitsf(plane(0, n, 0), 1.0f) && bitsf(plane(1, n, 0), 1.5f) && bitsf(plane(2, n, 0), 1.0f));
    CHECK(bitsf(plane(3, n, 3), -4.0f) && bitsf(plane(4, n, 3), -3.75f) && bitsf(plane(5, n, 3), -4.0f));
    CHECK(bitsf(plane(6, n, 1), 11.0f) && bitsf(plane(7, n, 1), 13.0f) && bitsf(plane(8, n, 1), 11.0f));
    for (uint32_t j = 0; j < 9; ++j) CHECK(bitsf(plane(j, n, 2), kLdsEmptyBox));
    // the child-code plane (and everything else) keeps its bytes
    if (!untouched(own, 0x5A)) return false;
    // updated twice: the second boxes replace the first on every plane, the empty child stays the point box
    BvhNode b2 = node_of(-3.5f);
    b2.child[1] = 7, b2.child[2] = kNodeEmpty;
    image_put_node_boxes(g_img.data(), n, b2);
    if (!node_is(n, b2)) return false;
    CHECK(bitsf(plane(2, n, 3), -0.5f) && bitsf(plane(7, n, 0), -33.0f));
    if (!untouched(own, 0x5A)) return false;
    // node 0 sits at the planes' near ends
    image_put_node_boxes(g_img.data(), 0, b);
    return node_is(0, b) && node_is(n, b2);
}

int main() {
    if (!check_static_sphere() || !check_moving_sphere_signed_zero() || !check_nodes()) return 1;
    std::printf("ok\n");
    return 0;
}

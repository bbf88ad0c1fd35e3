// lds_image.h — the parts of the layout.h LDS scene image that follow a sphere's centre and radius and a node's child
// boxes, for host (g++, hipcc's host pass) and device code alike: device_scene.hip's builder and refit.hip's
// rt_scene_update_spheres kernels run one text, so an updated image is the image a fresh build makes, byte for byte.
// No HIP types (tests/native/lds_image_check.cpp).
//
// Both sides compile this with -ffp-contract=off: every expression below is one IEEE operation per operator; the
// division is the language's own (correctly rounded on both sides), not a reciprocal sequence.
#pragma once
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

}  // namespace art

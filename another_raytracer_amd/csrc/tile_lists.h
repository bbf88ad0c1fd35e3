// tile_lists.h — which spheres the camera rays of one 8x8-pixel tile can reach (pure host/device code, no HIP header:
// g++ compiles it for tests/native/tile_lists_check.cpp, hipcc for k_tile_lists).
//
// A k_paths batch traces 64 camera rays of one tile.  Every camera ray cam_ray (path_work.h) forms for a pixel of the
// tile is
//     P(t) = o + t d = O + t (F - O) + (1 - t) off,
// with O the camera origin, off = lens_radius (px u + py v), px^2 + py^2 < 1, the lens offset, and
// F = llc + s horizontal + t' vertical its point on the focus plane, s in [8 tx, 8 tx + 8] / (W - 1) and t' in
// [(H - 1 - gmax), (H - gmin)] / (H - 1) for the tile's smallest and largest global row.  With Fc the centre of that
// rectangle and D = Fc - O, the bundle's axis is A(t) = O + t D, and
//     |P(t) - A(t)| = |t (F - Fc) + (1 - t) off| <= rho(t) = t R_tile + |1 - t| R_lens        (t >= 0)
// where R_tile >= |F - Fc| (the half extents of the rectangle, added) and R_lens >= |off|.  sphere_root accepts a root
// t >= 0.001 of |P(t) - c| = r, so a sphere the tile can hit has |A(t) - c| <= r + rho(t) for some t >= 0: the bundle
// is a fat ray.  Both sides are non-negative and their squares are quadratics in t on [0, 1] and on [1, inf), so the
// test is the sign of a quadratic's minimum over each piece.
//
// Conservative: the bound is taken with r + pad in place of r, pad = 1e-6 (|r| + |O - c| + |D|) (kTilePad).  What it
// has to cover are the roundings of cam_ray (s, t', the lens offset, o, d: a few ulp of scene-scale doubles, 1e-16
// relative) and of sphere_root, whose discriminant |d|^2 (r^2 - p^2), p the ray's distance from the centre, carries an
// absolute error of a few ulp of |d|^2 |o - c|^2: a ray is accepted at most at p <= r + 8 ulp |o - c|^2 / r.  That is
// below the pad while |O - c| / r < 1e8; a sphere farther away than that in units of its radius is a candidate of
// every tile (kTileFar).  The arithmetic here is f64 with errors of the same 1e-16 relative size, far below the pad.
#pragma once
#include <cmath>
#include <cstdint>

#include "layout.h"

namespace art {

constexpr uint32_t kTileK = 15;             // slots a tile's record holds
constexpr uint16_t kTileOverflow = 0xFFFF;  // TileRec::n of a tile with more candidates: its batches traverse the tree
constexpr double kTilePad = 1e-6, kTileFar = 1e8;
// One tile's candidates: the representative leaf slots (layout.h LDS scene image) of the spheres its rays can reach,
// nearest first.  32 B, read by k_paths as one scalar load.
struct alignas(32) TileRec {
    uint16_t n;
    uint16_t slot[kTileK];
};
static_assert(sizeof(TileRec) == 32, "a tile record is 32 B");
// The representative slots of an LDS scene image, uploaded behind it (at lds_image + kLdsImageBytes): one slot per
// sphere, the lowest whose kLdsOffRef index names it.  n == 0: the scene gets no lists.
struct TileReps {
    uint32_t n;
    uint16_t slot[kLdsSlotCap];
    uint16_t pad[6];
};
static_assert(sizeof(TileReps) % 16 == 0, "uploaded behind the 16-B aligned image");

struct TileFrame {  // the frame geometry of PassGeom the tiles depend on
    int32_t W, H, band_rows, band_count, band_index;
    uint32_t tiles_x;
};
struct TileBundle {  // the fat ray of one tile
    double O[3], D[3];
    double DD;              // |D|^2
    double r_lens, r_tile;
    double t_mid, t_half;   // the shutter [time0, time1]: its midpoint and half length
};

ART_HD TileBundle tile_bundle(const CameraRec& cam, const TileFrame& g, uint32_t tile) {
    const uint32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const double s0 = static_cast<double>(8 * tx) / static_cast<double>(g.W - 1), s1 = static_cast<double>(8 * tx + 8) / static_cast<double>(g.W - 1);
    // the tile's eight local rows (padding rows of a bottom tile included: the bound only widens); band_global_row is
    // increasing in the local row
    const int gmin = band_global_row(static_cast<int>(8 * ty), g.band_rows, g.band_count, g.band_index);
    const int gmax = band_global_row(static_cast<int>(8 * ty + 7), g.band_rows, g.band_count, g.band_index);
    const double t0 = static_cast<double>(g.H - 1 - gmax) / static_cast<double>(g.H - 1), t1 = static_cast<double>(g.H - gmin) / static_cast<double>(g.H - 1);
    const double sc = 0.5 * (s0 + s1), tc = 0.5 * (t0 + t1), sh = 0.5 * (s1 - s0), th = 0.5 * (t1 - t0);
    TileBundle b;
    double hh = 0, vv = 0, uu = 0, ww = 0, uw = 0;
    b.DD = 0;
    for (int a = 0; a < 3; ++a) {
        b.O[a] = cam.origin[a];
        b.D[a] = cam.llc[a] + sc * cam.horizontal[a] + tc * cam.vertical[a] - cam.origin[a];
        b.DD += b.D[a] * b.D[a];
        hh += cam.horizontal[a] * cam.horizontal[a];
        vv += cam.vertical[a] * cam.vertical[a];
        uu += cam.u[a] * cam.u[a];
        ww += cam.v[a] * cam.v[a];
        uw += cam.u[a] * cam.v[a];
    }
    b.r_tile = sh * std::sqrt(hh) + th * std::sqrt(vv);
    // |px u + py v|^2 <= (max(|u|^2, |v|^2) + |u.v|) (px^2 + py^2): no assumption that u and v are orthonormal
    b.r_lens = std::fabs(cam.lens_radius) * std::sqrt((uu > ww ? uu : ww) + std::fabs(uw));
    b.t_mid = 0.5 * (cam.time0 + cam.time1);
    b.t_half = 0.5 * std::fabs(cam.time1 - cam.time0);
    return b;
}

// Is |w + t D|^2 <= (k0 + t k1)^2 for some t in [lo, hi] (hi < 0: [lo, inf))?  k0 + t k1 >= 0 on the piece.  first: a
// lower bound of the smallest such t.
ART_HD bool tile_piece(double ww, double wD, double DD, double k0, double k1, double lo, double hi, double& first) {
    const double a = DD - k1 * k1, hb = wD - k0 * k1, c = ww - k0 * k0;  // g(t) = a t^2 + 2 hb t + c
    first = lo;
    if ((a * lo + 2.0 * hb) * lo + c <= 0.0) return true;
    if (hi >= 0.0 && (a * hi + 2.0 * hb) * hi + c <= 0.0) return true;
    if (!(a > 0.0)) return hi < 0.0;  // concave or linear: the minimum is at an end; towards inf it is reached (or taken to be)
    const double tv = -hb / a;        // convex: the vertex, if inside
    if (!(tv > lo) || (hi >= 0.0 && !(tv < hi))) return false;
    const double disc = hb * hb - a * c;
    if (disc < 0.0) return false;
    first = (-hb - std::sqrt(disc)) / a;  // g(lo) > 0 and the vertex is inside: the smaller root lies in (lo, tv]
    if (!(first > lo)) first = lo;
    return true;
}

// Can a ray of the bundle hit the sphere (centre c, radius r, y motion dy over the unit shutter: centre c + tm dy at
// ray time tm) at t >= 0.001?  Never false for a sphere that sphere_root accepts for a ray of the tile (see above).
// key: a lower bound of the parameter t at which the bundle reaches the sphere (the sort key: nearest first).
ART_HD bool tile_reaches(const TileBundle& b, double cx, double cy, double cz, double r, double dy, double& key) {
    // a moving sphere over the camera's shutter: the centre's midpoint, the radius widened by half its travel
    const double my = cy + b.t_mid * dy, rad = std::fabs(r) + b.t_half * std::fabs(dy);
    const double w[3] = {b.O[0] - cx, b.O[1] - my, b.O[2] - cz};
    const double ww = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], wD = w[0] * b.D[0] + w[1] * b.D[1] + w[2] * b.D[2];
    key = 0.0;
    if (!(ww < kTileFar * kTileFar * rad * rad)) return true;  // too far for the pad's argument (or not a number)
    const double R = rad + kTilePad * (rad + std::sqrt(ww) + std::sqrt(b.DD));
    // [0, 1]: rho = R_lens + t (R_tile - R_lens); [1, inf): rho = -R_lens + t (R_tile + R_lens)
    double f0, f1;
    const bool p0 = tile_piece(ww, wD, b.DD, R + b.r_lens, b.r_tile - b.r_lens, 0.0, 1.0, f0);
    const bool p1 = tile_piece(ww, wD, b.DD, R - b.r_lens, b.r_tile + b.r_lens, 1.0, -1.0, f1);
    key = p0 ? f0 : f1;
    return p0 || p1;
}

}  // namespace art

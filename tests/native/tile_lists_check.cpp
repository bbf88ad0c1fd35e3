// tile_lists.h's conservative test (which spheres can the camera rays of an 8x8 tile reach?) against brute force: for
// every case and sampled tile, a few thousand rays formed exactly as cam_ray (path_work.h) forms them -- s, t and the lens
// offset at random and at their extremes -- are tested against every sphere with sphere_root's root selection on
// [0.001, inf), and every sphere that accepts must be a candidate of the tile.  Also the precondition of the speed-up
// on the benchmark-like layout at 1920x1080: no tile overflows kTileK and the mean count is below 4.
// Prints the statistics, then "ok" or the first failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tile_lists.h"

using namespace art;

struct V {
    double x, y, z;
};
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(double s, V a) { return {s * a.x, s * a.y, s * a.z}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V unit(V a) { return (1.0 / std::sqrt(dot(a, a))) * a; }
static V ld(const double* p) { return {p[0], p[1], p[2]}; }
static void st(double* p, V a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }

struct Rng {
    uint64_t s;
    double next() {  // [0, 1)
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return static_cast<double>(s >> 11) * 0x1p-53;
    }
    double range(double a, double b) { return a + (b - a) * next(); }
};

// camera::camera (camera.h) in f64
static CameraRec make_camera(V from, V at, V vup, double vfov, double aspect, double aperture, double focus, double t0, double t1) {
    const double pi = 3.1415926535897932385;
    const double h = std::tan(vfov * pi / 180.0 / 2.0), vh = 2.0 * h, vw = aspect * vh;
    const V w = unit(from - at), u = unit(cross(vup, w)), v = cross(w, u);
    CameraRec c{};
    const V hor = (focus * vw) * u, ver = (focus * vh) * v;
    st(c.origin, from), st(c.horizontal, hor), st(c.vertical, ver), st(c.u, u), st(c.v, v);
    st(c.llc, from - 0.5 * hor - 0.5 * ver - focus * w);
    c.lens_radius = aperture / 2.0, c.time0 = t0, c.time1 = t1;
    return c;
}

struct Sph {
    V c;
    double r, dy;
};

// sphere_root (device.h) on [0.001, inf) for the sphere at ray time tm
static bool accepts(const Sph& s, V o, V d, double tm) {
    const V center{s.c.x, s.c.y + tm * s.dy, s.c.z};
    const V oc = o - center;
    const double a = dot(d, d), half_b = dot(oc, d), c = dot(oc, oc) - s.r * s.r;
    const double disc = half_b * half_b - a * c;
    if (disc < 0.0) return false;
    const double sq = std::sqrt(disc);
    double root = (-half_b - sq) / a;
    if (root < 0.001) {
        root = (-half_b + sq) / a;
        if (root < 0.001) return false;
    }
    return true;
}

struct Case {
    const char* name;
    CameraRec cam;
    TileFrame g;
    std::vector<Sph> sph;
    uint32_t tile_stride;  // every tile_stride-th tile is sampled
    int rays;
    int must_hit = -1;     // a sphere the sampled rays have to hit somewhere (the case is the one meant)
    int must_skip = -1;    // a sphere that is no tile's candidate
};

static std::vector<Sph> random_layout(uint64_t seed, bool moving) {
    Rng r{seed};
    std::vector<Sph> s;
    s.push_back({{0, -1000, 0}, 1000, 0});
    for (int a = -11; a < 11; ++a)
        for (int b = -11; b < 11; ++b) {
            const V c{a + 0.9 * r.next(), 0.2, b + 0.9 * r.next()};
            const V d = c - V{4, 0.2, 0};
            const double dy = (moving && r.next() < 0.5) ? r.range(0.0, 0.5) : 0.0;
            if (std::sqrt(dot(d, d)) > 0.9) s.push_back({c, 0.2, dy});
        }
    s.push_back({{0, 1, 0}, 1, 0});
    s.push_back({{-4, 1, 0}, 1, 0});
    s.push_back({{4, 1, 0}, 1, 0});
    return s;
}

static int check_case(const Case& cs) {
    const TileFrame& g = cs.g;
    const int rows = band_local_rows(g.H, g.band_rows, g.band_count, g.band_index);
    const uint32_t tiles_y = static_cast<uint32_t>((rows + 7) / 8), ntiles = g.tiles_x * tiles_y;
    const V O = ld(cs.cam.origin), llc = ld(cs.cam.llc), hor = ld(cs.cam.horizontal), ver = ld(cs.cam.vertical), cu = ld(cs.cam.u), cv = ld(cs.cam.v);
    const double one = std::nextafter(1.0, 0.0);
    Rng rng{0x9E3779B97F4A7C15ull};
    std::vector<char> cand(cs.sph.size());
    bool hit_must = cs.must_hit < 0;
    uint64_t sum = 0, max = 0, over = 0, hits = 0;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
        const TileBundle b = tile_bundle(cs.cam, g, tile);
        uint32_t n = 0;
        for (size_t i = 0; i < cs.sph.size(); ++i) {
            double key;
            cand[i] = tile_reaches(b, cs.sph[i].c.x, cs.sph[i].c.y, cs.sph[i].c.z, cs.sph[i].r, cs.sph[i].dy, key) ? 1 : 0;
            if (cand[i] && !(key >= 0.0)) return std::printf("FAIL %s: tile %u sphere %zu key %g\n", cs.name, tile, i, key), 1;
            n += cand[i];
        }
        if (cs.must_skip >= 0 && cand[cs.must_skip]) return std::printf("FAIL %s: sphere %d is a candidate of tile %u\n", cs.name, cs.must_skip, tile), 1;
        sum += n, max = n > max ? n : max, over += n > kTileK;
        if (tile % cs.tile_stride != 0) continue;
        const uint32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        for (int k = 0; k < cs.rays; ++k) {
            // a pixel of the tile inside the frame (the kernel traces no padding pixel), extremes first
            int lx = static_cast<int>(8 * tx) + (k & 1 ? 7 : (k & 2 ? 0 : static_cast<int>(rng.next() * 8)));
            int ly = static_cast<int>(8 * ty) + (k & 4 ? 7 : (k & 8 ? 0 : static_cast<int>(rng.next() * 8)));
            if (lx > g.W - 1) lx = g.W - 1;
            if (ly > rows - 1) ly = rows - 1;
            const int gy = band_global_row(ly, g.band_rows, g.band_count, g.band_index);
            const double ru = k & 16 ? (k & 32 ? 0.0 : one) : rng.next(), rv = k & 64 ? (k & 128 ? 0.0 : one) : rng.next();
            const double s = (static_cast<double>(lx) + ru) / static_cast<double>(g.W - 1);
            const double t = (static_cast<double>(g.H - 1 - gy) + rv) / static_cast<double>(g.H - 1);
            double px, py;
            if (k & 256) {  // on the rim of the lens disk (cam_ray keeps len2(p) < 1)
                const double ang = rng.range(0.0, 6.283185307179586);
                px = one * std::cos(ang), py = one * std::sin(ang);
                if (px * px + py * py >= 1.0) px *= one, py *= one;
            } else {
                do px = rng.range(-1.0, 1.0), py = rng.range(-1.0, 1.0);
                while (px * px + py * py >= 1.0);
            }
            const V rd{cs.cam.lens_radius * px, cs.cam.lens_radius * py, 0.0};
            const V offset = rd.x * cu + rd.y * cv;
            const V o = O + offset, d = llc + s * hor + t * ver - O - offset;
            const double tm = k & 512 ? (k & 1024 ? cs.cam.time0 : cs.cam.time1) : rng.range(cs.cam.time0, cs.cam.time1);
            for (size_t i = 0; i < cs.sph.size(); ++i) {
                if (!accepts(cs.sph[i], o, d, tm)) continue;
                ++hits;
                if (static_cast<int>(i) == cs.must_hit) hit_must = true;
                if (!cand[i])
                    return std::printf("FAIL %s: tile %u (%u, %u) pixel (%d, %d) ray %d hits sphere %zu, which is no candidate\n", cs.name, tile, tx, ty,
                                       lx, ly, k, i), 1;
            }
        }
    }
    std::printf("%s: %u tiles, mean %.3f max %llu overflow %llu, %llu sampled hits\n", cs.name, ntiles, double(sum) / ntiles,
                static_cast<unsigned long long>(max), static_cast<unsigned long long>(over), static_cast<unsigned long long>(hits));
    if (!hit_must) return std::printf("FAIL %s: no sampled ray hit sphere %d\n", cs.name, cs.must_hit), 1;
    if (hits == 0) return std::printf("FAIL %s: no sampled ray hit anything\n", cs.name), 1;
    if (cs.g.W == 1920 && (over != 0 || !(double(sum) / ntiles < 4.0)))
        return std::printf("FAIL %s: the 1080p layout needs no overflow and a mean below 4\n", cs.name), 1;
    return 0;
}

static TileFrame frame(int W, int H, int band_rows = 0, int band_count = 1, int band_index = 0) {
    return TileFrame{W, H, band_rows ? band_rows : H, band_count, band_index, static_cast<uint32_t>((W + 7) / 8)};
}

int main() {
    const V from{13, 2, 3}, at{0, 0, 0}, up{0, 1, 0};
    const std::vector<Sph> layout = random_layout(12345, false);
    std::vector<Case> cases;
    cases.push_back({"layout 1920x1080", make_camera(from, at, up, 20, 1920.0 / 1080.0, 0.1, 10, 0, 1), frame(1920, 1080), layout, 211, 1500});
    cases.push_back({"layout 72x40", make_camera(from, at, up, 20, 72.0 / 40.0, 0.1, 10, 0, 1), frame(72, 40), layout, 1, 2500});
    cases.push_back({"aperture 0", make_camera(from, at, up, 20, 72.0 / 40.0, 0.0, 10, 0, 1), frame(72, 40), layout, 1, 2500});
    cases.push_back({"aperture 2", make_camera(from, at, up, 20, 72.0 / 40.0, 2.0, 10, 0, 1), frame(72, 40), layout, 1, 2500});
    cases.push_back({"moving spheres", make_camera(from, at, up, 20, 72.0 / 40.0, 0.1, 10, 0, 1), frame(72, 40), random_layout(777, true), 1, 2500});
    for (int bi = 0; bi < 3; ++bi)
        cases.push_back({"band_rows 4, 3 bands", make_camera(from, at, up, 20, 72.0 / 40.0, 0.1, 10, 0, 1), frame(72, 40, 4, 3, bi), layout, 1, 2500});
    {  // the camera inside a sphere (the mirror room of the GPU tests): a candidate of every tile, hit by every ray
        std::vector<Sph> room = {{{0, 0, 0}, 12, 0}, {{0, -4, 0}, 2.5, 0}, {{-4.5, 1, -2}, 1.5, 0}, {{4.5, 1, -2}, 1.5, 0}, {{0, 7, 0}, 3, 0}};
        cases.push_back({"camera inside a sphere", make_camera({0, 1, 8}, {0, 1.5, 0}, up, 70, 64.0 / 40.0, 0.0, 10, 0, 1), frame(64, 40), room, 1, 1500, 0});
    }
    {  // a sphere straddling the lens plane (centre 0.2 in front of the lens and 0.3 to its side, radius 0.3), which rays
       // of the right half hit, and one wholly behind the camera, which none can
        const CameraRec cam = make_camera(from, at, up, 20, 72.0 / 40.0, 0.1, 10, 0, 1);
        const V w = unit(from - at), u = ld(cam.u);
        std::vector<Sph> s = layout;
        s.push_back({from + 0.3 * u - 0.2 * w, 0.3, 0});
        s.push_back({from + 5.0 * w, 1.0, 0});
        cases.push_back({"lens plane", cam, frame(72, 40), s, 1, 2500, static_cast<int>(s.size()) - 2, static_cast<int>(s.size()) - 1});
    }
    {  // a sphere tangent to the edge of a tile's bundle: it touches (to 1e-9 of its radius) the ray through the corner
       // s = 8 / 71, t = 16 / 39 of tile (1, 2), from outside the bundle; a pinhole camera, so that the corner ray is one
       // of the sampled extremes (ray 246)
        const CameraRec cam = make_camera(from, at, up, 20, 72.0 / 40.0, 0.0, 10, 0, 1);
        const V O = ld(cam.origin), u = ld(cam.u);
        const double s0 = 8.0 / 71.0, t0 = (39.0 - 23.0) / 39.0;  // pixel (8, 23), ru = rv = 0: the tile's lower left corner
        const V offset = (-std::nextafter(1.0, 0.0) * cam.lens_radius) * u;
        const V o = O + offset, d = ld(cam.llc) + s0 * ld(cam.horizontal) + t0 * ld(cam.vertical) - O - offset;
        const V p = o + 0.8 * d, side = unit(cross(d, ld(cam.v)));  // towards smaller s: out of the bundle
        const double r = 0.05;
        std::vector<Sph> s = {{{0, -1000, 0}, 1000, 0}, {p + ((side.x * u.x + side.y * u.y + side.z * u.z) < 0 ? 1.0 : -1.0) * (r * (1.0 - 1e-9)) * side, r, 0}};
        cases.push_back({"tangent sphere", cam, frame(72, 40), s, 1, 4096, 1});
    }
    for (const Case& c : cases)
        if (check_case(c)) return 1;
    std::printf("ok\n");
    return 0;
}

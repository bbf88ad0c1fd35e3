// A host run of rt_scene_update_spheres' refit (refit.h, g++ -ffp-contract=off as the library builds it): 40 spheres, 7
// of them moving, are given new centres and radii; every slot's box is sphere_box of the updated record, and
// refit_child runs over refit_levels of two node arrays, deepest level first: a three-level tree of ten four-sphere
// leaves with two empty slots, and one node of four ten-sphere leaves.  Checked here: every refitted box contains the
// swept extent of every sphere below it (long double), empty slots keep their boxes.  Printed for
// tests/test_update_spheres_model.py, which restates the boxes in numpy: "ok", the updated records, both trees' boxes.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "refit.h"

using namespace art;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform(double lo, double hi) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (hi - lo) * static_cast<double>(g_state >> 11) * 0x1p-53;
}

static BvhNode blank_node() {
    BvhNode b{};
    for (int c = 0; c < 4; ++c) {
        b.lox[c] = b.loy[c] = b.loz[c] = FLT_MAX;  // the builder's empty slot; stale garbage for the others
        b.hix[c] = b.hiy[c] = b.hiz[c] = -FLT_MAX;
        b.child[c] = kNodeEmpty;
    }
    return b;
}

// the spheres of slots [first, first + count) lie inside child c of node n, at both ends of the shutter
static bool contains(const BvhNode& b, int c, const std::vector<SphereRec>& sph, uint32_t first, uint32_t count) {
    const float lo[3] = {b.lox[c], b.loy[c], b.loz[c]}, hi[3] = {b.hix[c], b.hiy[c], b.hiz[c]};
    for (uint32_t k = first; k < first + count; ++k)
        for (int a = 0; a < 3; ++a)
            for (int end = 0; end < 2; ++end) {
                long double c0 = sph[k].c[a];
                if (sph[k].flags & SPH_MOVING) c0 += (static_cast<long double>(end) - sph[k].t0) / sph[k].dt * sph[k].d[a];
                if (!(static_cast<long double>(lo[a]) < c0 - sph[k].r && static_cast<long double>(hi[a]) > c0 + sph[k].r)) {
                    std::printf("FAIL: sphere %u axis %d end %d outside its box [%a, %a]\n", k, a, end, lo[a], hi[a]);
                    return false;
                }
            }
    return true;
}

static void refit(std::vector<BvhNode>& nodes, const std::vector<double>& slot_box, uint32_t n_slots) {
    std::vector<ObjRec> objs(1);
    objs[0] = ObjRec{};
    objs[0].kind = OBJ_BVH, objs[0].a = 0, objs[0].b = kNodeEmpty;
    const std::vector<uint32_t> level = refit_levels(nodes, objs);
    for (size_t l = level.size(); l-- > 1;)
        for (uint32_t n = level[l - 1]; n < level[l]; ++n)
            for (int c = 0; c < 4; ++c) refit_child(nodes.data(), static_cast<uint32_t>(nodes.size()), slot_box.data(), n_slots, n, c);
}

static void print_nodes(const char* tag, const std::vector<BvhNode>& nodes) {
    for (size_t n = 0; n < nodes.size(); ++n)
        for (int c = 0; c < 4; ++c)
            std::printf("%s %zu %d %d %a %a %a %a %a %a\n", tag, n, c, nodes[n].child[c], nodes[n].lox[c], nodes[n].loy[c], nodes[n].loz[c], nodes[n].hix[c],
                        nodes[n].hiy[c], nodes[n].hiz[c]);
}

int main() {
    const uint32_t N = 40;
    std::vector<SphereRec> sph(N);
    for (uint32_t k = 0; k < N; ++k) {  // S0: the compiled records
        SphereRec& s = sph[k];
        s = SphereRec{};
        for (int a = 0; a < 3; ++a) s.c[a] = uniform(-10.0, 10.0);
        s.r = uniform(0.1, 1.0);
        s.mat = k % 3;
        if (k % 6 == 1) {  // 7 moving spheres: y motion over the unit shutter, one along x, one over a shorter shutter
            s.flags = SPH_MOVING;
            s.t0 = 0.0, s.dt = 1.0;
            s.d[1] = uniform(0.0, 0.5);
            if (k == 13) s.d[0] = -0.75, s.d[1] = 0.0;
            if (k == 25) s.t0 = 0.25, s.dt = 0.5, s.d[2] = 0.3;
        }
    }
    const std::vector<SphereRec> before = sph;
    std::vector<double> slot_box(6 * N);
    for (uint32_t k = 0; k < N; ++k) {  // the update: c and r change, everything else stays; then the slot's box
        for (int a = 0; a < 3; ++a) sph[k].c[a] += uniform(-2.0, 2.0) * sph[k].r;
        sph[k].r *= uniform(0.6, 1.5);
        sphere_box(sph[k], slot_box.data() + 6 * k);
    }
    for (uint32_t k = 0; k < N; ++k)
        if (sph[k].mat != before[k].mat || sph[k].flags != before[k].flags || sph[k].d[1] != before[k].d[1] || sph[k].dt != before[k].dt) return 2;

    // tree 1: root 0 -> nodes 1, 2, 3 (and an empty slot); node 1: leaves 0..3, node 2: leaves 4..7, node 3: leaves 8, 9
    std::vector<BvhNode> t1(4, blank_node());
    for (int c = 0; c < 3; ++c) t1[0].child[c] = c + 1;
    for (uint32_t leaf = 0; leaf < 10; ++leaf) t1[1 + leaf / 4].child[leaf % 4] = make_leaf(4 * leaf, 4);
    refit(t1, slot_box, N);
    for (uint32_t leaf = 0; leaf < 10; ++leaf)
        if (!contains(t1[1 + leaf / 4], static_cast<int>(leaf % 4), sph, 4 * leaf, 4)) return 1;
    for (int c = 0; c < 3; ++c)
        if (!contains(t1[0], c, sph, 16 * c, c < 2 ? 16 : 8)) return 1;
    for (int n : {0, 3})
        for (int c = n == 0 ? 3 : 2; c < 4; ++c)
            if (t1[n].lox[c] != FLT_MAX || t1[n].hiz[c] != -FLT_MAX) {
                std::printf("FAIL: the empty slot %d of node %d changed\n", c, n);
                return 1;
            }
    // tree 2: one node of four ten-sphere leaves
    std::vector<BvhNode> t2(1, blank_node());
    for (int c = 0; c < 4; ++c) t2[0].child[c] = make_leaf(10 * c, 10);
    refit(t2, slot_box, N);
    for (int c = 0; c < 4; ++c)
        if (!contains(t2[0], c, sph, 10 * c, 10)) return 1;

    std::printf("ok\n");
    for (uint32_t k = 0; k < N; ++k)
        std::printf("S %u %a %a %a %a %a %a %a %a %a %u\n", k, sph[k].c[0], sph[k].c[1], sph[k].c[2], sph[k].r, sph[k].d[0], sph[k].d[1], sph[k].d[2],
                    sph[k].t0, sph[k].dt, sph[k].flags);
    print_nodes("T1", t1);
    print_nodes("T2", t2);
    return 0;
}

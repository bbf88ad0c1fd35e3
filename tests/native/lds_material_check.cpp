// lds_image.h's shading-table text on the host (g++ -ffp-contract=off, as the library builds it): image_put_material
// for a solid entry, a checker pair, two metals and two dielectrics, and image_material_entries for a small slot
// sequence.  Prints, for tests/test_lds_material_model.py to compare with values restated in numpy:
//   entry <name> <e> <4 doubles as hex bit patterns>     one per shading-table entry written
//   codes <one int per material>                          image_material_entries' codes, then "nent <n> complete <0|1>"
// and checks itself that no byte outside the written entries changes.  Ends with "ok" or the first failure.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lds_image.h"

using namespace art;

static std::vector<uint8_t> g_img(kLdsImageBytes);

static void print_entry(const char* name, uint32_t e) {
    uint64_t v[4];
    std::memcpy(v, g_img.data() + kLdsOffMat + e * 32, 32);
    std::printf("entry %s %u %016llx %016llx %016llx %016llx\n", name, e, static_cast<unsigned long long>(v[0]), static_cast<unsigned long long>(v[1]),
                static_cast<unsigned long long>(v[2]), static_cast<unsigned long long>(v[3]));
}

// every byte outside entries [e, e + count) still holds the fill
static bool untouched(uint32_t e, uint32_t count, uint8_t fill) {
    for (uint32_t i = 0; i < kLdsImageBytes; ++i) {
        const bool mine = i >= kLdsOffMat + e * 32 && i < kLdsOffMat + (e + count) * 32;
        if (!mine && g_img[i] != fill) {
            std::printf("FAIL: byte %u outside entries [%u, %u) changed\n", i, e, e + count);
            return false;
        }
    }
    return true;
}

static TexRec solid_tex(double r, double g, double b) {
    TexRec t{};
    t.type = TEX_SOLID, t.even = t.odd = t.perlin = t.image = -1;
    t.c[0] = r, t.c[1] = g, t.c[2] = b;
    t.scale = 123.0;  // not a solid texture's: never in an entry
    return t;
}
static MatRec mat_of(uint32_t type, int32_t tex) {
    MatRec m{};
    m.type = type, m.tex = tex;
    m.albedo[0] = -1.0, m.albedo[1] = -2.0, m.albedo[2] = -3.0, m.fuzz = -4.0, m.ir = -5.0;  // overwritten where the type uses them
    return m;
}

int main() {
    // textures: 0 solid, 1 solid, 2 checker(0, 1), 3 solid, 4 noise, 5 checker(3, 4): not two solid colours
    std::vector<TexRec> texs = {solid_tex(0.125, 0.3, 0.7), solid_tex(0.9, 0.1, 1e-3), TexRec{}, solid_tex(4.0, 5.5, 7.25), TexRec{}, TexRec{}};
    texs[2].type = TEX_CHECKER, texs[2].even = 0, texs[2].odd = 1;
    texs[4].type = TEX_NOISE, texs[4].scale = 4.0;
    texs[5].type = TEX_CHECKER, texs[5].even = 3, texs[5].odd = 4;

    // ---- image_put_material
    struct Case { const char* name; MatRec m; int32_t code; uint32_t e, count; };
    std::vector<Case> cases;
    cases.push_back({"solid", mat_of(MAT_LAMBERTIAN, 0), 7, 7, 1});
    cases.push_back({"light", mat_of(MAT_LIGHT, 3), 0, 0, 1});
    cases.push_back({"checker", mat_of(MAT_LAMBERTIAN, 2), static_cast<int32_t>(40 | kLdsMatChecker), 40, 2});
    MatRec metal = mat_of(MAT_METAL, -1);
    metal.albedo[0] = 0.7, metal.albedo[1] = 0.6, metal.albedo[2] = 0.5, metal.fuzz = 0.25;
    cases.push_back({"metal", metal, 3, 3, 1});
    metal.fuzz = 1.0;  // 1.5 as the caller clamps it (SceneGraph::metal, k_update_materials)
    cases.push_back({"metal_clamped", metal, static_cast<int32_t>(kLdsMatCap - 1), kLdsMatCap - 1, 1});
    MatRec glass = mat_of(MAT_DIELECTRIC, -1);
    glass.ir = 1.5;
    cases.push_back({"glass_1.5", glass, 11, 11, 1});
    glass.ir = 0.75;
    cases.push_back({"glass_0.75", glass, 12, 12, 1});
    for (const Case& c : cases) {
        std::fill(g_img.begin(), g_img.end(), 0xA5);
        image_put_material(g_img.data(), c.code, c.m, texs.data());
        for (uint32_t k = 0; k < c.count; ++k) print_entry(c.name, c.e + k);
        if (!untouched(c.e, c.count, 0xA5)) return 1;
    }
    // no entry: nothing is written; a checker whose odd entry would lie past the table writes the even one only
    std::fill(g_img.begin(), g_img.end(), 0x5A);
    image_put_material(g_img.data(), -1, metal, texs.data());
    image_put_material(g_img.data(), -1, mat_of(MAT_ISOTROPIC, 0), texs.data());
    if (!untouched(0, 0, 0x5A)) return 1;
    image_put_material(g_img.data(), static_cast<int32_t>((kLdsMatCap - 1) | kLdsMatChecker), mat_of(MAT_LAMBERTIAN, 2), texs.data());
    print_entry("checker_at_the_end", kLdsMatCap - 1);
    if (!untouched(kLdsMatCap - 1, 1, 0x5A)) return 1;

    // ---- image_material_entries: materials 0 lambertian(solid 0), 1 metal, 2 lambertian(checker 2), 3 dielectric,
    // 4 light(solid 3), 5 lambertian(solid 0) that no slot uses, 6 lambertian(checker 5: a noise child), 7 isotropic
    std::vector<MatRec> mats = {mat_of(MAT_LAMBERTIAN, 0), mat_of(MAT_METAL, -1), mat_of(MAT_LAMBERTIAN, 2), mat_of(MAT_DIELECTRIC, -1),
                                mat_of(MAT_LIGHT, 3), mat_of(MAT_LAMBERTIAN, 0), mat_of(MAT_LAMBERTIAN, 5), mat_of(MAT_ISOTROPIC, 0)};
    const uint32_t sphere_mat[7] = {3, 2, 2, 0, 4, 1, 0};  // sphere k's material
    std::vector<SphereRec> spheres(7);
    for (int k = 0; k < 7; ++k) spheres[k].mat = sphere_mat[k];
    // slots name spheres 1, 0, 2, 1, 5, 3, 4, 6: materials 2, 3, 2, 2, 1, 0, 4, 0 in first-encounter order 2, 3, 1, 0, 4
    const uint32_t order[8] = {1, 0, 2, 1, 5, 3, 4, 6};
    std::vector<uint32_t> refs;
    for (uint32_t k : order) refs.push_back(make_primref(PRIM_SPHERE, k));
    std::vector<int32_t> entry(mats.size(), 77);
    bool complete = false;
    uint32_t nent = image_material_entries(refs.data(), refs.size(), spheres.data(), mats.data(), mats.size(), texs.data(), texs.size(), entry.data(), complete);
    std::printf("codes");
    for (int32_t e : entry) std::printf(" %d", e);
    std::printf("\nnent %u complete %d\n", nent, complete ? 1 : 0);
    // a slot of material 6 (a checker with a noise child) or 7 (isotropic): no entry, and the table is incomplete
    for (uint32_t bad : {6u, 7u}) {
        spheres[6].mat = bad;
        nent = image_material_entries(refs.data(), refs.size(), spheres.data(), mats.data(), mats.size(), texs.data(), texs.size(), entry.data(), complete);
        std::printf("codes");
        for (int32_t e : entry) std::printf(" %d", e);
        std::printf("\nnent %u complete %d\n", nent, complete ? 1 : 0);
    }
    std::printf("ok\n");
    return 0;
}

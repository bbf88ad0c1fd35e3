// Stand-alone check of the oracle's scene-dump loader (oracle/restate.cpp build_scene on a text that starts with '{'):
// linked with restate.cpp and run directly, under -fsanitize=address,undefined by tests/test_oracle_dump_scenes.py.
// A good dump loads, renders and dumps back to itself; every truncation of a dump and every malformed case is an error
// with a message -- never a crash or an out-of-bounds read, which is what the sanitizers watch.
// argv[1]: the asset directory (builtin scene 7 needs none; kept for orc_set_asset_dir).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "restate.h"

static int g_failed = 0;
#define CHECK(cond, what)                                                   \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, std::string(what).c_str()); \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

// one of every object, material and texture kind that needs no image, with consistent bvh `nodes` / `box`
static const char* kSmall = R"({"lookfrom":[0,0,9],"lookat":[3,0,0],"vfov":60,"aperture":0.1,"background":[0.5,0.25,0.125],"objects":[
{"type":"bvh","nodes":3,"box":[[-1,-1,-1],[7,1.5,1]],"items":[
{"type":"sphere","center":[0,0,0],"radius":1,"mat":{"type":"metal","albedo":[0.5,0.5,0.5],"fuzz":0.25}},
{"type":"moving_sphere","center0":[3,0,0],"center1":[3,0.5,0],"time0":0,"time1":1,"radius":1,"mat":{"type":"dielectric","ir":1.5}},
{"type":"triangle","p":[[5,-1,0],[7,-1,0],[6,1,0.5]],"mat":{"type":"lambertian","tex":{"type":"checker","even":{"type":"solid","c":[0,0,0]},"odd":{"type":"solid","c":[1,1,1]}}}}]},
{"type":"list","items":[{"type":"xz_rect","a0":"-inf","a1":"inf","b0":-50,"b1":50,"k":-2.5,"mat":{"type":"diffuse_light","tex":{"type":"solid","c":[2,2,2]}}}]},
{"type":"translate","offset":[0,3,0],"child":{"type":"constant_medium","neg_inv_density":-2,"phase":{"type":"isotropic","tex":{"type":"solid","c":[1,1,1]}},"boundary":{"type":"sphere","center":[0,0,0],"radius":1,"mat":{"type":"dielectric","ir":1.5}}}}]}
)";

static std::string dump_of(const std::string& scene) {
    const size_t n = orc_dump(scene.c_str(), nullptr, 0);
    if (n == 0) return "";
    std::vector<char> buf(n);
    orc_dump(scene.c_str(), buf.data(), n);
    return std::string(buf.data());
}

static std::string replaced(const std::string& text, const std::string& from, const std::string& to) {
    const size_t at = text.find(from);
    if (at == std::string::npos) {
        std::fprintf(stderr, "FAIL the test's own pattern is missing: %s\n", from.c_str());
        ++g_failed;
        return text;
    }
    return text.substr(0, at) + to + text.substr(at + from.size());
}

static std::string rstrip(std::string s) {
    while (!s.empty() && (s.back() == '\n' || s.back() == ' ')) s.pop_back();
    return s;
}

// a dump that must be refused with a message containing `expect`
static void refused(const std::string& text, const char* expect, const char* what) {
    const size_t n = orc_dump(text.c_str(), nullptr, 0);
    const std::string err = orc_last_error();
    CHECK(n == 0, std::string(what) + ": loaded");
    CHECK(n != 0 || err.find(expect) != std::string::npos, std::string(what) + ": message '" + err + "' lacks '" + expect + "'");
}

static void every_truncation_is_refused(const std::string& whole, const char* what) {
    const std::string text = rstrip(whole);
    for (size_t n = 0; n < text.size(); ++n) {
        const std::string cut = text.substr(0, n);
        if (orc_dump(cut.c_str(), nullptr, 0) != 0 || !*orc_last_error()) {
            CHECK(false, std::string(what) + ": truncation to " + std::to_string(n) + " bytes loaded or gave no message");
            return;
        }
    }
}

int main(int argc, char** argv) {
    if (argc > 1) orc_set_asset_dir(argv[1]);

    // good dumps: the hand-written one and a builder-made one (rects, boxes, rotate_y, translate, media, a light)
    const std::string small = dump_of(kSmall);
    CHECK(!small.empty(), std::string("the small dump does not load: ") + orc_last_error());
    CHECK(dump_of(small) == small, "the small dump does not dump back to itself");
    CHECK(small.find("\"-inf\"") != std::string::npos && small.find("\"inf\"") != std::string::npos, "infinities lost");
    const std::string smoke = dump_of("7");
    CHECK(!smoke.empty() && dump_of(smoke) == smoke, "scene 7 does not round-trip");
    CHECK(dump_of("  \n" + smoke) == smoke, "leading blanks");

    // renders and traces like a named scene; pcg only
    const int W = 8, H = 6;
    std::vector<double> a(W * H * 3), b(W * H * 3);
    long long sa = 0, sb = 0;
    CHECK(orc_render("7", W, H, 2, 8, ORC_PCG, 1, 0, H, 2, nullptr, a.data(), &sa, nullptr) == 0, "render by name");
    CHECK(orc_render(smoke.c_str(), W, H, 2, 8, ORC_PCG, 1, 0, H, 2, nullptr, b.data(), &sb, nullptr) == 0, "render by dump");
    CHECK(sa == sb && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0, "dump render differs from the named one");
    CHECK(orc_render(small.c_str(), W, H, 2, 8, ORC_PCG, 1, 0, H, 2, nullptr, a.data(), &sa, nullptr) == 0 && sa >= 2 * W * H, "small render");
    const double ray[7] = {0, 0, 9, 0, 0, -1, 0.5};
    double t = 0, nrm[3];
    CHECK(orc_trace_rays(small.c_str(), ray, 1, &t, nrm) == 0 && t == 8.0 && nrm[2] == 1.0, "trace into the small dump");
    CHECK(orc_render(small.c_str(), W, H, 2, 8, ORC_MT, 1, 0, H, 1, nullptr, a.data(), &sa, nullptr) != 0 &&
              std::strstr(orc_last_error(), "pcg mode only"), "mt mode with a dump must be refused");
    CHECK(orc_render_adaptive(small.c_str(), 12, 12, 2, 8, ORC_MT, 1, 1, nullptr, nullptr, nullptr) != 0, "adaptive mt with a dump");
    CHECK(orc_render_images(small.c_str(), W, H, 4, 8, ORC_MT, 1, 1, nullptr, nullptr, nullptr, nullptr) != 0, "images mt with a dump");
    double probe[2];
    CHECK(orc_probe(small.c_str(), 2, probe) != 0, "probe of a dump");

    // images: unresolved names the hash; registered resolves
    std::vector<unsigned char> texels(4 * 2 * 3);
    for (size_t i = 0; i < texels.size(); ++i) texels[i] = static_cast<unsigned char>(37 * i + 11);
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : texels) { h ^= c; h *= 1099511628211ull; }
    char hex[32];
    std::snprintf(hex, sizeof hex, "%016llx", static_cast<unsigned long long>(h));
    const std::string image = std::string("{\"type\":\"image\",\"w\":4,\"h\":2,\"bpp\":3,\"fnv1a\":\"") + hex + "\"}";
    const std::string textured = replaced(replaced(small, "{\"type\":\"solid\",\"c\":[2,2,2]}", image), "{\"type\":\"solid\",\"c\":[0,0,0]}",
                                          "{\"type\":\"bary_image\",\"a\":[0,0],\"b\":[1,0],\"c\":[0,1],\"tex\":" + image + "}");
    refused(textured, hex, "unregistered image");
    CHECK(orc_register_image(4, 2, 3, texels.data()) == 0, "register");
    CHECK(orc_register_image(0, 2, 3, texels.data()) != 0 && orc_register_image(4, 2, 3, nullptr) != 0, "bad image accepted");
    CHECK(dump_of(textured) == textured, std::string("registered image does not resolve: ") + orc_last_error());
    refused(replaced(textured, "\"w\":4", "\"w\":5"), "not registered", "image of another size");

    // malformed input
    every_truncation_is_refused(small, "small");
    every_truncation_is_refused(textured, "textured");
    every_truncation_is_refused(smoke, "scene 7");
    refused(replaced(small, "\"type\":\"moving_sphere\"", "\"type\":\"torus\""), "unknown object type", "unknown object");
    refused(replaced(small, "\"type\":\"dielectric\"", "\"type\":\"glass\""), "unknown material type", "unknown material");
    refused(replaced(small, "\"type\":\"checker\"", "\"type\":\"marble\""), "unknown texture type", "unknown texture");
    refused(replaced(small, "\"radius\":1,", ""), "missing key \"radius\"", "missing key");
    refused(replaced(small, "\"vfov\":60,", ""), "missing key \"vfov\"", "missing header key");
    refused(replaced(small, "\"fuzz\":0.25", "\"fuzzy\":0.25"), "missing key \"fuzz\"", "misnamed key");
    refused(replaced(small, "\"center\":[0,0,0]", "\"center\":[0,0]"), "wrong array length", "short vector");
    refused(replaced(small, "\"center\":[0,0,0]", "\"center\":[0,0,0,0]"), "wrong array length", "long vector");
    refused(replaced(small, "[6,1,0.5]]", "[6,1,0.5],[0,0,0]]"), "wrong array length", "four triangle corners");
    refused(replaced(small, ",[7,1.5,1]]", "]"), "wrong array length", "one-cornered box");
    refused(replaced(smoke, "\"sides\":[", "\"sides\":[" + std::string("{\"type\":\"xy_rect\",\"a0\":0,\"a1\":1,\"b0\":0,\"b1\":1,\"k\":0,\"mat\":{\"type\":\"dielectric\",\"ir\":1.5}},")),
            "wrong array length", "seven box sides");
    refused(rstrip(small) + "x", "trailing garbage", "trailing garbage");
    refused(rstrip(small) + "{}", "trailing garbage", "a second value");
    refused(replaced(small, "\"nodes\":3", "\"nodes\":2"), "node count", "bvh node count");
    refused(replaced(small, "[7,1.5,1]", "[7,1.25,1]"), "bvh box", "bvh box");
    refused(replaced(small, "\"items\":[\n{\"type\":\"sphere\"", "\"items\":[],\"was\":[\n{\"type\":\"sphere\""), "empty list", "empty bvh");
    refused(replaced(smoke, "\"max\":[165,330,165]", "\"max\":[165,331,165]"), "box sides disagree", "box sides");
    refused(replaced(small, "\"ir\":1.5", "\"ir\":1.5.5"), "bad number", "bad number");
    refused(replaced(small, "\"ir\":1.5", "\"ir\":\"nan\""), "bad number", "nan");
    refused(replaced(small, "\"ir\":1.5", "\"ir\":\"1\\u0035\""), "unsupported character", "escape");
    refused(replaced(small, "\"vfov\":60", "\"vfov\":"), "expected a number", "missing value");
    std::string deep = "{\"type\":\"sphere\",\"center\":[0,0,0],\"radius\":1,\"mat\":{\"type\":\"dielectric\",\"ir\":1.5}}";
    for (int i = 0; i < 1000; ++i) deep = "{\"type\":\"list\",\"items\":[" + deep + "]}";
    refused(replaced(small, "\"objects\":[", "\"objects\":[" + deep + ","), "nesting deeper", "deep nesting");
    std::string nested = "{\"type\":\"solid\",\"c\":[1,1,1]}";
    for (int i = 0; i < 80; ++i) nested = "{\"type\":\"checker\",\"even\":" + nested + ",\"odd\":{\"type\":\"solid\",\"c\":[0,0,0]}}";
    refused(replaced(small, "{\"type\":\"solid\",\"c\":[2,2,2]}", nested), "nesting deeper", "deep textures");

    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("dump loader ok");
    return 0;
}

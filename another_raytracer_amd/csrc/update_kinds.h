// update_kinds.h — what rt_scene_update_triangles / _spheres / _materials / _textures update, as one table: the ABI's
// refusals and getters (abi.cpp) and the renderer's update call (Renderer::update) are driven by it.  Host only.
#pragma once
#include <cstddef>

#include "scene.h"

namespace art {

enum class UpdateKind { Triangles, Spheres, Materials, Textures };

struct UpdateRow {
    const char *noun, *nouns;  // a record in a message; rt_scene_update_<nouns>, rt_scene_<nouns>_get
    size_t width;              // doubles per record
    bool geometry;             // moves boxes (the slot boxes and the refit) or recolours (the material entry codes)
    // beside "every value finite", a rule for a record of a host buffer (ok null: none); refused as
    // "<subject> of <noun> K <fault>"
    bool (*ok)(const double* record);
    const char *subject, *fault;
};
inline constexpr UpdateRow kUpdateRows[] = {
    {"triangle", "triangles", 9, true, nullptr, nullptr, nullptr},  // three vertices
    {"sphere", "spheres", 4, true, [](const double* s) { return s[3] > 0.0; }, "the radius", "is not positive"},  // cx, cy, cz, r
    {"material", "materials", 5, false, nullptr, nullptr, nullptr},  // albedo r, g, b; fuzz; ir (RT_MATERIAL_DOUBLES)
    {"texture", "textures", 4, false, nullptr, nullptr, nullptr},    // colour r, g, b; scale (RT_TEXTURE_DOUBLES)
};
inline const UpdateRow& update_row(UpdateKind kind) { return kUpdateRows[static_cast<int>(kind)]; }

// the records of the kind a compiled scene holds (an update changes no count)
inline size_t update_count(const FlatScene& f, UpdateKind kind) {
    switch (kind) {
        case UpdateKind::Triangles: return f.tris.size();
        case UpdateKind::Spheres: return f.spheres.size();
        case UpdateKind::Materials: return f.mats.size();
        default: return f.texs.size();
    }
}

}  // namespace art

// update_kinds.h — what rt_scene_update_triangles / _spheres / _materials / _textures / _rects / _boxes / _objects update,
// as one table: the ABI's refusals and getters (abi.cpp) and the renderer's update call (Renderer::update) are driven by
// it.  Host only.
#pragma once
#include <cstddef>

#include "scene.h"

namespace art {

enum class UpdateKind { Triangles, Spheres, Materials, Textures, Rects, Boxes, Objects };
// What a kind's first update prepares and what follows its kernel: Refit -- it moves boxes (the slot boxes, then the
// refit of every level); Appearance -- it recolours (the material entry codes of an image scene); None -- neither (an
// object's parameters: a transformed object and a medium have no box anywhere)
enum class UpdateClass { Refit, Appearance, None };

struct UpdateRow {
    const char *noun, *nouns;  // a record in a message; rt_scene_update_<nouns>, rt_scene_<nouns>_get
    size_t width;              // doubles per record
    UpdateClass cls;
    // beside "every value finite", a rule for a record of a host buffer (ok null: none); refused as
    // "<subject> of <noun> K <fault>"
    bool (*ok)(const double* record);
    const char *subject, *fault;
};
inline constexpr UpdateRow kUpdateRows[] = {
    {"triangle", "triangles", 9, UpdateClass::Refit, nullptr, nullptr, nullptr},  // three vertices
    {"sphere", "spheres", 4, UpdateClass::Refit, [](const double* s) { return s[3] > 0.0; }, "the radius", "is not positive"},  // cx, cy, cz, r
    {"material", "materials", 5, UpdateClass::Appearance, nullptr, nullptr, nullptr},  // albedo r, g, b; fuzz; ir (RT_MATERIAL_DOUBLES)
    {"texture", "textures", 4, UpdateClass::Appearance, nullptr, nullptr, nullptr},    // colour r, g, b; scale (RT_TEXTURE_DOUBLES)
    {"rect", "rects", 5, UpdateClass::Refit, nullptr, nullptr, nullptr},               // a0, a1, b0, b1, k (RT_RECT_DOUBLES)
    {"box", "boxes", 6, UpdateClass::Refit, nullptr, nullptr, nullptr},                // min xyz, max xyz (RT_BOX_DOUBLES)
    {"object", "objects", 4, UpdateClass::None, nullptr, nullptr, nullptr},            // ObjRec::p (RT_OBJECT_DOUBLES)
};
inline const UpdateRow& update_row(UpdateKind kind) { return kUpdateRows[static_cast<int>(kind)]; }

// the records of the kind a compiled scene holds (an update changes no count)
inline size_t update_count(const FlatScene& f, UpdateKind kind) {
    switch (kind) {
        case UpdateKind::Triangles: return f.tris.size();
        case UpdateKind::Spheres: return f.spheres.size();
        case UpdateKind::Materials: return f.mats.size();
        case UpdateKind::Textures: return f.texs.size();
        case UpdateKind::Rects: return f.rects.size();
        case UpdateKind::Boxes: return f.boxes.size();
        default: return f.objs.size();
    }
}

}  // namespace art

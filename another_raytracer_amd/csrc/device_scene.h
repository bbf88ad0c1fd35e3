// device_scene.h — the scene as the kernels see it: the uploaded arrays behind a DevScene view, and the properties
// the launchers choose kernels by.  Built from a FlatScene by build_device_scene (device_scene.hip).
#pragma once
#include <algorithm>
#include <vector>

#include "hip_check.h"
#include "path_work.h"
#include "scene.h"

namespace art {

struct DeviceScene {
    std::vector<void*> allocs;
    DevScene view{};
    bool media = false;
    uint32_t features = F_ALL;
    int max_stack = kMaxStackDepth;
    uint32_t mat_types = (1u << kNumMatTypes) - 1;  // bit m: some material of type m exists
    bool tex_basic = false;                          // only solid and checker textures
    bool lds_scene = false;                          // view.lds_image holds the layout.h LDS scene image
    bool lds_shade = false;                          // ... including a complete shading table (fused variant)
    uint32_t tile_reps = 0;                          // > 0: the representative slots behind the image (tile_lists.h TileReps)
    bool codes16 = false;                            // every node's child codes fit BvhNode::pad's 16-bit form
    uint32_t leaf_shift = 0;                         // 1: 16-bit leaf codes count slot pairs (F_LEAF2; leaves on even slots)
    bool tex_bary = false;                           // image textures are barycentric ones on triangles only (TF_BARY)
    size_t bytes = 0;
    // rt_scene_update_triangles: the host copy of view.primrefs (slot_pad[i]: slot i belongs to no leaf), and what the
    // scene's first update makes: the f64 box of every slot's primitive on the device and the level ranges of the nodes
    std::vector<uint32_t> slot_refs;
    std::vector<uint8_t> slot_pad;
    double* slot_box = nullptr;
    const uint8_t* slot_pad_dev = nullptr;  // slot_pad on the device (k_update_spheres skips pad slots)
    std::vector<uint32_t> level_begin;
    // rt_scene_update_materials / _textures: what the first of them makes of a scene with an image -- each material's
    // shading-table entry code (lds_image.h image_material_entries) on the device
    const int32_t* mat_entry_dev = nullptr;

    template <class T>
    const T* upload(const std::vector<T>& v) {
        if (v.empty()) return nullptr;
        void* p = nullptr;
        HIP_OK(hipMalloc(&p, v.size() * sizeof(T)));
        HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        allocs.push_back(p);
        bytes += v.size() * sizeof(T);
        return static_cast<const T*>(p);
    }
    void release() {
        for (void* p : allocs) (void)hipFree(p);
        allocs.clear();
    }
};

constexpr size_t kLdsPerCu = 160 * 1024;  // gfx950

// Traversal stack rows per lane: the worst-case depth + the sentinel row + the spare row of branchless pushes.
inline uint32_t stack_rows(int max_stack) { return static_cast<uint32_t>(std::max(1, max_stack)) + 2u; }
inline size_t extend_lds_bytes(bool L, uint32_t stack) { return extend_pre_offset(L, stack) + 4 * (kShards + 1); }

void build_device_scene(const FlatScene& f0, DeviceScene& ds);  // device_scene.hip
// The layout.h LDS scene image of f with its TileReps behind it (kLdsImageBytes + sizeof(TileReps) bytes), or an empty
// vector when f does not qualify; nmov: its moving spheres, shade_ok: the shading table is complete, tile_reps: the
// representative slots (0: no tile lists).  build_device_scene uploads it; rt_scene_lds_image_get rebuilds it.
std::vector<uint8_t> build_lds_image(const FlatScene& f, uint32_t& nmov, bool& shade_ok, uint32_t& tile_reps);

}  // namespace art

// refit.hip — rt_scene_update_triangles on the device: k_update_tris writes the new vertices into every array that holds
// a triangle (the records, the three leaf-ordered copies, the prim objects' copies) and the f64 box of every leaf slot
// it touches; k_refit_level then recomputes the child boxes of one tree level from what lies below it (refit.h).  One
// launch per level, deepest first, on one stream: stream order is the only dependency between the levels.
// rt_scene_update_spheres: k_update_spheres does the same for centres and radii (the records, the leaf-ordered copy,
// the prim objects' copies, the slot boxes and the sphere planes of the LDS scene image, lds_image.h), and after the
// levels k_image_nodes rewrites the image's box planes from the refitted nodes.
// rt_scene_update_materials / rt_scene_update_textures: k_update_materials / k_update_textures write the fields a record's
// type takes, then k_derive_materials refreshes, for every material of the scene, the two copies made of them at upload:
// the solid colour inlined into a MATF_SOLID record and the image's shading-table entries (lds_image.h).
// rt_scene_update_rects / rt_scene_update_boxes: k_update_rects / k_update_boxes are k_update_spheres without an image
// (the records, the leaf-ordered copy, the prim objects' copies, the slot boxes), followed by the levels.
// rt_scene_update_objects: k_update_objects writes ObjRec::p by the object's kind -- where an instance stands, how it is
// turned, how dense a medium is; none of those has a box, so nothing is refitted.
#include "launch.h"
#include "lds_image.h"
#include "refit.h"

namespace art {

constexpr int kRefitBlock = 256;

// The nine doubles of a triangle into a record's p[] (TriRec, TriRec112 and a PrimRec80 holding a TriRec start with them)
__device__ __forceinline__ void put9(double* dst, const double v[9]) {
    for (int k = 0; k < 9; ++k) dst[k] = v[k];
}

__global__ void __launch_bounds__(kRefitBlock) k_update_tris(UpdateJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < j.n_slots) {  // leaf slot i: a pad slot of the pair-aligned copy holds reference 0, a sphere
        const uint32_t ref = j.primrefs[i];
        const uint32_t t = primref_index(ref) - j.first;  // (wraps above n for a triangle below `first`)
        if (primref_type(ref) == PRIM_TRIANGLE && t < j.n) {
            double v[9];
            for (int k = 0; k < 9; ++k) v[k] = j.p[9 * static_cast<size_t>(t) + k];
            put9(j.leaf_tris[i].p, v);
            // the plane as device_scene.hip makes it: n = cross(pt2 - pt1, pt3 - pt1), dd = -dot(n, pt1)
            const V3 p1 = ld3(v), nn = cross(ld3(v + 3) - p1, ld3(v + 6) - p1);
            TriRec112& r = j.leaf_tris112[i];
            put9(r.p, v);
            r.n[0] = nn.x, r.n[1] = nn.y, r.n[2] = nn.z;
            r.dd = -dot(nn, p1);
            put9(reinterpret_cast<double*>(j.leaf_prims[i].b), v);
            tri_box(v, j.slot_box + 6 * static_cast<size_t>(i));
        }
    }
    if (i < j.n) {  // triangle first + i: its record (mat stays)
        double v[9];
        for (int k = 0; k < 9; ++k) v[k] = j.p[9 * static_cast<size_t>(i) + k];
        put9(j.tris[j.first + i].p, v);
    }
    if (i < j.n_objs && j.objs[i].kind == OBJ_PRIM) {  // a loose triangle of the world: obj_prims[i] is its record
        const uint32_t ref = static_cast<uint32_t>(j.objs[i].a);
        const uint32_t t = primref_index(ref) - j.first;
        if (primref_type(ref) == PRIM_TRIANGLE && t < j.n) {
            double v[9];
            for (int k = 0; k < 9; ++k) v[k] = j.p[9 * static_cast<size_t>(t) + k];
            put9(reinterpret_cast<double*>(j.obj_prims[i].b), v);
        }
    }
}

// (cx, cy, cz, r) into a sphere record; mat, flags and a moving sphere's d, t0, dt stay: it translates with its motion
__device__ __forceinline__ void put_sphere(SphereRec& r, const double* v) {
    r.c[0] = v[0], r.c[1] = v[1], r.c[2] = v[2];
    r.r = v[3];
}

__global__ void __launch_bounds__(kRefitBlock) k_update_spheres(SphereJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    // leaf slot i.  A pad slot of the pair-aligned copy holds reference 0, which reads as sphere 0: it belongs to no leaf,
    // its records stay zero and its box stays empty.  Every slot of a sphere that spatial splits put into several leaves
    // gets the same bytes (tile_lists.h TileReps).
    if (i < j.n_slots && !j.slot_pad[i]) {
        const uint32_t ref = j.primrefs[i];
        const uint32_t t = primref_index(ref) - j.first;  // (wraps above n for a sphere below `first`)
        if (primref_type(ref) == PRIM_SPHERE && t < j.n) {
            SphereRec& r = *reinterpret_cast<SphereRec*>(j.leaf_prims[i].b);
            put_sphere(r, j.s + 4 * static_cast<size_t>(t));
            const SphereRec now = r;
            sphere_box(now, j.slot_box + 6 * static_cast<size_t>(i));
            if (j.image) image_put_sphere(j.image, i, now);  // (an image scene has no pad slots: its slots are these)
        }
    }
    if (i < j.n) put_sphere(j.spheres[j.first + i], j.s + 4 * static_cast<size_t>(i));  // sphere first + i: its record
    if (i < j.n_objs && j.objs[i].kind == OBJ_PRIM) {  // a loose sphere of the world, or a constant_medium's boundary
        const uint32_t ref = static_cast<uint32_t>(j.objs[i].a);
        const uint32_t t = primref_index(ref) - j.first;
        if (primref_type(ref) == PRIM_SPHERE && t < j.n) put_sphere(*reinterpret_cast<SphereRec*>(j.obj_prims[i].b), j.s + 4 * static_cast<size_t>(t));
    }
}

// One thread per node: the image's box planes from the refitted node (the child-code plane stays: topology does)
__global__ void __launch_bounds__(kRefitBlock) k_image_nodes(uint8_t* image, const BvhNode* nodes, uint32_t n_nodes) {
    const uint32_t n = blockIdx.x * kRefitBlock + threadIdx.x;
    if (n < n_nodes) image_put_node_boxes(image, n, nodes[n]);
}

// One thread per record of [first, first + n).  A metal takes albedo and fuzz (clamped as SceneGraph::metal clamps it,
// material.h:47), a dielectric ir; a lambertian's, a light's and an isotropic's colour is their texture's.
__global__ void __launch_bounds__(kRefitBlock) k_update_materials(AppearanceJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= j.n) return;
    const double* v = j.v + 5 * static_cast<size_t>(i);
    MatRec& m = j.mats[j.first + i];
    if (m.type == MAT_METAL) {
        m.albedo[0] = v[0], m.albedo[1] = v[1], m.albedo[2] = v[2];
        m.fuzz = v[3] < 1.0 ? v[3] : 1.0;
    } else if (m.type == MAT_DIELECTRIC) {
        m.ir = v[4];
    }
}

// A solid texture takes the colour, a noise texture the scale (its perlin table stays); the others nothing
__global__ void __launch_bounds__(kRefitBlock) k_update_textures(AppearanceJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= j.n) return;
    const double* v = j.v + 4 * static_cast<size_t>(i);
    TexRec& t = j.texs[j.first + i];
    if (t.type == TEX_SOLID) {
        t.c[0] = v[0], t.c[1] = v[1], t.c[2] = v[2];
    } else if (t.type == TEX_NOISE) {
        t.scale = v[3];
    }
}

// One thread per material of the scene, whatever range was updated: a texture may be shared by materials outside it
__global__ void __launch_bounds__(kRefitBlock) k_derive_materials(AppearanceJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= j.n_mats) return;
    MatRec& m = j.mats[i];
    if (m.flags & MATF_SOLID) {  // (set at upload for a valid solid texture only)
        const TexRec& t = j.texs[m.tex];
        m.albedo[0] = t.c[0], m.albedo[1] = t.c[1], m.albedo[2] = t.c[2];
    }
    if (j.image) image_put_material(j.image, j.entry[i], m, j.texs);
}

// (a0, a1, b0, b1, k) into a rect record, (min xyz, max xyz) into a box record; axis and mat stay
__device__ __forceinline__ void put_rect(RectRec& r, const double* v) { r.a0 = v[0], r.a1 = v[1], r.b0 = v[2], r.b1 = v[3], r.k = v[4]; }
__device__ __forceinline__ void put_box(BoxRec& x, const double* v) {
    for (int a = 0; a < 3; ++a) x.mn[a] = v[a], x.mx[a] = v[3 + a];
}

// k_update_spheres' shape for rects: thread i is leaf slot i, rect first + i and object i at once.  No image: an image
// scene holds spheres only.
__global__ void __launch_bounds__(kRefitBlock) k_update_rects(RigidJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < j.n_slots && !j.slot_pad[i]) {
        const uint32_t ref = j.primrefs[i];
        const uint32_t t = primref_index(ref) - j.first;  // (wraps above n for a rect below `first`)
        if (primref_type(ref) == PRIM_RECT && t < j.n) {
            RectRec& r = *reinterpret_cast<RectRec*>(j.leaf_prims[i].b);
            put_rect(r, j.v + 5 * static_cast<size_t>(t));
            const RectRec now = r;
            rect_box(now, j.slot_box + 6 * static_cast<size_t>(i));
        }
    }
    if (i < j.n) put_rect(j.rects[j.first + i], j.v + 5 * static_cast<size_t>(i));  // rect first + i: its record
    if (i < j.n_objs && j.objs[i].kind == OBJ_PRIM) {  // a loose rect of the world, or one under a transform chain
        const uint32_t ref = static_cast<uint32_t>(j.objs[i].a);
        const uint32_t t = primref_index(ref) - j.first;
        if (primref_type(ref) == PRIM_RECT && t < j.n) put_rect(*reinterpret_cast<RectRec*>(j.obj_prims[i].b), j.v + 5 * static_cast<size_t>(t));
    }
}

// ... and for boxes (a box under a transform chain, a constant_medium's boundary included, is an OBJ_PRIM object)
__global__ void __launch_bounds__(kRefitBlock) k_update_boxes(RigidJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < j.n_slots && !j.slot_pad[i]) {
        const uint32_t ref = j.primrefs[i];
        const uint32_t t = primref_index(ref) - j.first;
        if (primref_type(ref) == PRIM_BOX && t < j.n) {
            BoxRec& x = *reinterpret_cast<BoxRec*>(j.leaf_prims[i].b);
            put_box(x, j.v + 6 * static_cast<size_t>(t));
            const BoxRec now = x;
            box_box(now, j.slot_box + 6 * static_cast<size_t>(i));
        }
    }
    if (i < j.n) put_box(j.boxes[j.first + i], j.v + 6 * static_cast<size_t>(i));
    if (i < j.n_objs && j.objs[i].kind == OBJ_PRIM) {
        const uint32_t ref = static_cast<uint32_t>(j.objs[i].a);
        const uint32_t t = primref_index(ref) - j.first;
        if (primref_type(ref) == PRIM_BOX && t < j.n) put_box(*reinterpret_cast<BoxRec*>(j.obj_prims[i].b), j.v + 6 * static_cast<size_t>(t));
    }
}

// One thread per record of [first, first + n): p by the object's kind; kind, a and b stay
__global__ void __launch_bounds__(kRefitBlock) k_update_objects(ObjectJob j) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= j.n) return;
    const double* v = j.v + 4 * static_cast<size_t>(i);
    ObjRec& o = j.objs[j.first + i];
    if (o.kind == OBJ_TRANSLATE) {
        o.p[0] = v[0], o.p[1] = v[1], o.p[2] = v[2];
    } else if (o.kind == OBJ_ROTATE_Y) {
        o.p[0] = v[0], o.p[1] = v[1];
    } else if (o.kind == OBJ_MEDIUM) {
        o.p[0] = v[0];
    }
}

// Four lanes per node of [begin, end), one per child
__global__ void __launch_bounds__(kRefitBlock) k_refit_level(BvhNode* nodes, uint32_t n_nodes, const double* slot_box, uint32_t n_slots,
                                                             uint32_t begin, uint32_t end) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    const uint32_t n = begin + (i >> 2);
    if (n < end) refit_child(nodes, n_nodes, slot_box, n_slots, n, static_cast<int>(i & 3u));
}

// One thread per item in blocks of kRefitBlock; nothing to do is no launch
template <class... Params, class... Args>
static void launch_1d(void (*kernel)(Params...), uint32_t threads, hipStream_t st, const Args&... args) {
    if (threads == 0) return;
    hipLaunchKernelGGL(kernel, dim3((threads + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, args...);
}

void launch_update_tris(hipStream_t st, const UpdateJob& j) { launch_1d(k_update_tris, std::max(std::max(j.n_slots, j.n), j.n_objs), st, j); }

void launch_update_spheres(hipStream_t st, const SphereJob& j) { launch_1d(k_update_spheres, std::max(std::max(j.n_slots, j.n), j.n_objs), st, j); }

void launch_image_nodes(hipStream_t st, uint8_t* image, const BvhNode* nodes, uint32_t n_nodes) {
    if (image) launch_1d(k_image_nodes, n_nodes, st, image, nodes, n_nodes);
}

void launch_update_materials(hipStream_t st, const AppearanceJob& j) {
    if (j.n == 0) return;
    launch_1d(k_update_materials, j.n, st, j);
    launch_1d(k_derive_materials, j.n_mats, st, j);
}

void launch_update_textures(hipStream_t st, const AppearanceJob& j) {
    if (j.n == 0) return;
    launch_1d(k_update_textures, j.n, st, j);
    launch_1d(k_derive_materials, j.n_mats, st, j);
}

void launch_update_rects(hipStream_t st, const RigidJob& j) { launch_1d(k_update_rects, std::max(std::max(j.n_slots, j.n), j.n_objs), st, j); }

void launch_update_boxes(hipStream_t st, const RigidJob& j) { launch_1d(k_update_boxes, std::max(std::max(j.n_slots, j.n), j.n_objs), st, j); }

void launch_update_objects(hipStream_t st, const ObjectJob& j) { launch_1d(k_update_objects, j.n, st, j); }

void launch_refit_levels(hipStream_t st, BvhNode* nodes, uint32_t n_nodes, const double* slot_box, uint32_t n_slots,
                         const std::vector<uint32_t>& level_begin) {
    for (size_t l = level_begin.size(); l-- > 1;) {
        const uint32_t begin = level_begin[l - 1], end = level_begin[l];
        if (end > begin) launch_1d(k_refit_level, 4u * (end - begin), st, nodes, n_nodes, slot_box, n_slots, begin, end);
    }
}

}  // namespace art

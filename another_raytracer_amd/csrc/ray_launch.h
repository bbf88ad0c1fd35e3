// ray_launch.h — what the objects with ray kernels share on the host side (kernels.hip: k_trace_rays, k_guides,
// k_query_rays, k_occlude_rays; radiance_rays.hip: k_radiance_rays, k_radiance_views): the choice of instantiation and the launch of a
// one-thread-per-item kernel.  Host templates only; included by .hip files.
#pragma once
#include <type_traits>

#include "launch.h"

namespace art {

// The choice: the LDS scene image where the scene has one (spheres only) and global_scene does not rule it out, else
// the smallest HBM-scene feature set that covers the scene's features & MASK.  fn(f, l) receives F and L as
// compile-time values (std::integral_constant).
template <uint32_t MASK = ~0u, class Fn>
static void with_ray_features(const DeviceScene& ds, bool global_scene, Fn&& fn) {
    const uint32_t feat = ds.features & MASK;
    if (ds.lds_scene && !global_scene && (ds.features & ~kFeatSpheres) == 0) fn(std::integral_constant<uint32_t, kFeatSpheres>{}, std::true_type{});
    else if ((feat & ~kFeatSpheres) == 0) fn(std::integral_constant<uint32_t, kFeatSpheres>{}, std::false_type{});
    else if ((feat & ~kFeatMesh) == 0) fn(std::integral_constant<uint32_t, kFeatMesh & MASK>{}, std::false_type{});
    else fn(std::integral_constant<uint32_t, F_ALL & MASK>{}, std::false_type{});
}
// The launch of `kernel` over n items: a block's traversal stacks in dynamic LDS, behind the scene image when L (more
// than 64 KiB then: blocks_per_cu sets the attribute; and the image must start at LDS address 0).
template <auto kernel, bool L, class... Args>
static void launch_ray_kernel(const DeviceScene& ds, hipStream_t st, uint32_t n, const Args&... args) {
    const uint32_t stack = stack_rows(ds.max_stack);
    constexpr int B = L ? kBlockL : kBlock;
    const size_t lds = L ? kLdsImageBytes + paths_stack_bytes(stack) : sizeof(int32_t) * stack * kBlock;
    if constexpr (L) {
        static const bool checked = static_lds_is_zero(reinterpret_cast<const void*>(kernel));
        (void)checked;
        (void)blocks_per_cu(reinterpret_cast<const void*>(kernel), B, lds);
    }
    hipLaunchKernelGGL(kernel, dim3((n + B - 1) / B), dim3(B), lds, st, args...);
}

}  // namespace art

// hip_check.h — HIP_OK(call): throws std::runtime_error("<call>: <hipGetErrorString>") unless the call returns hipSuccess;
// HipAlloc: the device allocator of workspace.h's DeviceBuffer.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define HIP_OK(x)                                                                                         \
    do {                                                                                                  \
        hipError_t e_ = (x);                                                                              \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace art {
struct HipAlloc {
    static void* alloc(size_t bytes) { void* p = nullptr; HIP_OK(hipMalloc(&p, bytes)); return p; }
    static void free(void* old) { HIP_OK(hipFree(old)); }
    static void drop(void* p) noexcept { (void)hipFree(p); }  // on paths that cannot report
};
}  // namespace art

// hip_check.h — HIP_OK(call): throws std::runtime_error("<call>: <hipGetErrorString>") unless the call returns hipSuccess.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define HIP_OK(x)                                                                                         \
    do {                                                                                                  \
        hipError_t e_ = (x);                                                                              \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

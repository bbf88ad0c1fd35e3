// workspace.h — the grow-only device buffer behind the renderer's and the denoiser's workspaces and rt_multi's gather
// buffers, and the carver that lays typed sub-buffers out in one (host side).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "options.h"

namespace art {

// Grow-only device allocation.  The old buffer is released before the larger one is requested (both need not fit), and
// data() / size() describe a live allocation at every point: a refused growth leaves {nullptr, 0}, so the next call
// allocates again instead of handing out offsets from a null base.  The owner has the buffer's device current.  Dev is
// the allocator: HipAlloc (hip_check.h: hipMalloc / hipFree), or tests/native/workspace_check.cpp's counting stand-in.
template <class Dev>
class GrowBuffer {
public:
    // fault_point (the renderer's and the denoiser's workspaces): option test.fault_workspace_bytes = N > 0 makes every
    // growth beyond N bytes fail as a refused hipMalloc would, after the old buffer is released
    explicit GrowBuffer(bool fault_point = false) : fault_point_(fault_point) {}
    GrowBuffer(GrowBuffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_), fault_point_(o.fault_point_) { o.p_ = nullptr, o.bytes_ = 0; }
    GrowBuffer(const GrowBuffer&) = delete;
    GrowBuffer& operator=(const GrowBuffer&) = delete;
    ~GrowBuffer() { release(); }

    void* data() const { return p_; }
    size_t size() const { return bytes_; }
    void* reserve(size_t bytes) {
        if (bytes <= bytes_) return p_;
        const double lim = fault_point_ ? opt(Opt::FaultWorkspaceBytes) : 0;
        if (lim > 0 && static_cast<double>(bytes) > lim) {
            release();
            throw std::runtime_error("workspace allocation of " + std::to_string(bytes) + " bytes refused (test.fault_workspace_bytes)");
        }
        if (void* old = p_) {
            p_ = nullptr, bytes_ = 0;
            Dev::free(old);
        }
        p_ = Dev::alloc(bytes);
        bytes_ = bytes;
        return p_;
    }
    void release() {
        if (p_) Dev::drop(p_);
        p_ = nullptr, bytes_ = 0;
    }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
    bool fault_point_;
};
struct HipAlloc;
using DeviceBuffer = GrowBuffer<HipAlloc>;

// Lays sub-buffers out from `base`, each named once with its element type and count: take() returns the typed pointer
// and advances by the aligned size (a part that is off takes no room), total() is what the layout needs.  A layout
// function runs twice: over a null base for the size, then over the allocation for the pointers.
class Carver {
public:
    explicit Carver(void* base, size_t align = 256) : base_(reinterpret_cast<uintptr_t>(base)), align_(align) {}
    template <class T>
    T* take(size_t count, bool on = true) {
        T* p = reinterpret_cast<T*>(base_ + off_);
        if (on) off_ += (sizeof(T) * count + align_ - 1) / align_ * align_;
        return p;
    }
    size_t total() const { return off_; }

private:
    uintptr_t base_;
    size_t align_, off_ = 0;
};

}  // namespace art

// workspace.h's GrowBuffer over a counting stand-in for HipAlloc and its own opt() (the class's only dependencies):
// every allocation is freed exactly once, the old one before the new one is requested, and a refused or failed growth
// leaves {nullptr, 0}.  A host program of its own, meant for the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I another_raytracer_amd/csrc
//       tests/native/workspace_check.cpp -o workspace_check && ./workspace_check
// Prints "ok" or the first failure.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <stdexcept>
#include <string>

#include "workspace.h"

// ---- stand-ins (the stand-in allocations are real host blocks, so a double free or a leak is the sanitizer's to see)
static std::set<void*> g_live;
static int g_mallocs = 0, g_frees = 0, g_bad_frees = 0;
static bool g_fail_next_malloc = false;
static size_t g_live_at_malloc_max = 0;  // allocations alive while a new one was requested
struct CountingAlloc {
    static void* alloc(size_t bytes) {
        if (g_live.size() > g_live_at_malloc_max) g_live_at_malloc_max = g_live.size();
        if (g_fail_next_malloc) {
            g_fail_next_malloc = false;
            throw std::runtime_error("hipMalloc(&p, bytes): out of memory");
        }
        void* p = std::malloc(bytes);
        g_live.insert(p);
        ++g_mallocs;
        return p;
    }
    static void drop(void* p) noexcept {
        if (g_live.erase(p) != 1) ++g_bad_frees;
        else std::free(p);
        ++g_frees;
    }
    static void free(void* old) { drop(old); }
};
namespace art {
static double g_fault_bytes = 0;
double opt(Opt) { return g_fault_bytes; }  // options.h's, defined here: only test.fault_workspace_bytes is asked for
}  // namespace art
using Buffer = art::GrowBuffer<CountingAlloc>;

static int failures = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);    \
            ++failures;                                          \
        }                                                        \
    } while (0)

static bool empty(const Buffer& b) { return b.data() == nullptr && b.size() == 0; }
static bool throws(Buffer& b, size_t bytes, const char* text) {
    try {
        b.reserve(bytes);
    } catch (const std::runtime_error& e) {
        return std::string(e.what()).find(text) != std::string::npos;
    }
    return false;
}

int main() {
    {  // grow, refuse, grow again
        Buffer b(true);
        CHECK(empty(b));
        void* p = b.reserve(1000);
        CHECK(p && b.data() == p && b.size() == 1000 && g_live.size() == 1);
        CHECK(b.reserve(10) == p && b.reserve(1000) == p && g_mallocs == 1);  // grow-only: no call below the size
        art::g_fault_bytes = 4096;
        CHECK(b.reserve(4096) && b.size() == 4096 && g_mallocs == 2 && g_frees == 1);  // at the limit: allowed
        CHECK(throws(b, 4097, "workspace allocation of 4097 bytes refused (test.fault_workspace_bytes)"));
        CHECK(empty(b) && g_live.empty() && g_mallocs == 2 && g_frees == 2);  // the old buffer was released first
        CHECK(throws(b, 5000, "refused") && empty(b) && g_frees == 2);      // refused again: nothing to free
        art::g_fault_bytes = 0;
        CHECK(b.reserve(5000) && b.size() == 5000 && g_live.size() == 1 && g_mallocs == 3);
    }
    CHECK(g_live.empty() && g_frees == 3);  // the destructor frees
    {  // grow, failed allocation, grow again
        Buffer b(true);
        CHECK(b.reserve(100) && g_mallocs == 4);
        g_fail_next_malloc = true;
        CHECK(throws(b, 200, "hipMalloc"));
        CHECK(empty(b) && g_live.empty() && g_frees == 4);
        CHECK(b.reserve(50) && b.size() == 50 && g_mallocs == 5);  // from {nullptr, 0} every size is a growth
        g_fail_next_malloc = true;
        CHECK(throws(b, 300, "hipMalloc") && empty(b) && g_frees == 5);
        CHECK(b.reserve(300) && b.size() == 300 && g_mallocs == 6);
        b.release();  // release twice
        CHECK(empty(b) && g_frees == 6);
        b.release();
        CHECK(empty(b) && g_frees == 6);
        CHECK(b.reserve(1) && g_mallocs == 7);
    }
    CHECK(g_live.empty() && g_frees == 7);
    {  // without the fault point (rt_multi's buffers) the option refuses nothing; a moved-from buffer owns nothing
        art::g_fault_bytes = 16;
        Buffer a;
        CHECK(a.reserve(64) && a.size() == 64);
        Buffer b(std::move(a));
        CHECK(empty(a) && b.size() == 64 && g_live.size() == 1);
        art::g_fault_bytes = 0;
    }
    CHECK(g_live.empty() && g_mallocs == 8 && g_frees == 8 && g_bad_frees == 0);
    CHECK(g_live_at_malloc_max == 0);  // never two allocations at once: the old one goes before the new one is requested
    {  // the carver: 256-B parts in order, a part that is off takes no room, the same layout over a null base
        char block[2048];
        for (char* base : {static_cast<char*>(nullptr), block}) {
            art::Carver c(base);
            double* a = c.take<double>(3);
            char* off = c.take<char>(1000, false);
            int* i = c.take<int>(65);
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(base);
            CHECK(reinterpret_cast<uintptr_t>(a) == b0 && reinterpret_cast<uintptr_t>(off) == b0 + 256 && reinterpret_cast<uintptr_t>(i) == b0 + 256);
            CHECK(c.total() == 256 + 512);
        }
        art::Carver packed(block, 1);
        CHECK(packed.take<double>(7) == reinterpret_cast<double*>(block) && packed.take<char>(3) == block + 56 && packed.total() == 59);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

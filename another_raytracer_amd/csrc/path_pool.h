// path_pool.h — the index arithmetic of k_paths' per-wave path pool (k_paths.hip, PathPool), host and device: what a
// round pops, whether a batch of camera rays is due, and where entries go.  tools/path_pool_check.cpp drives exactly
// these functions on the CPU.
#pragma once
#include <cstdint>

#include "layout.h"

namespace art {

// ART_POOL_RING: pool entries per wave (the stride between two waves' pools).  The pool never holds more than
// kPoolBound entries; the capacity only spaces the pools in memory.
#ifndef ART_POOL_RING
#define ART_POOL_RING 64
#endif
constexpr uint32_t kPoolCap = ART_POOL_RING;
static_assert(kPoolCap >= 64 && kPoolCap <= 128, "pool entries per wave");
// A batch is due when this many idle lanes find the pool empty.
constexpr uint32_t kBatchIdle = 1;
static_assert(kBatchIdle >= 1 && kBatchIdle <= 64, "idle lanes that trigger a batch");
// A batch pushes the busy lanes' paths, and it runs only when the idle lanes outnumber the entries by kBatchIdle:
// entries + busy <= idle - kBatchIdle + busy = 64 - kBatchIdle.
constexpr uint32_t kPoolBound = 64u - kBatchIdle;
static_assert(kPoolBound <= kPoolCap, "the pool holds every path a batch can displace");

// entries the round's `idle` lanes can take from a pool of `count`
ART_HD uint32_t pool_pop_count(uint32_t count, uint32_t idle) { return count < idle ? count : idle; }
// a batch replaces the round: the pass has slots left and at least kBatchIdle idle lanes would get no entry
ART_HD bool pool_batch_due(bool exhausted, uint32_t count, uint32_t idle) {
    return !exhausted && idle - pool_pop_count(count, idle) >= kBatchIdle;
}
// LIFO: the idle lane of rank r (< pool_pop_count) takes the r-th entry from the top
ART_HD uint32_t pool_pop_pos(uint32_t count, uint32_t rank) { return count - 1u - rank; }
// the busy lane of rank r pushes above the top
ART_HD uint32_t pool_push_pos(uint32_t count, uint32_t rank) { return count + rank; }

}  // namespace art

// path_pool_check.cpp — drives the index arithmetic of k_paths' per-wave path pool (csrc/path_pool.h) on the CPU: one
// wave of 64 lanes runs the kernel's round structure (csrc/k_paths.hip) over passes of random length with random finish
// patterns, with path ids in place of path states.  Checks, for at least the given number of rounds: the pool never
// holds more than kPoolBound entries and no position leaves the capacity, every pushed entry is popped exactly once
// and by no lane that holds a path, every slot of a pass is traced to its end exactly once, and every pass terminates.
//   g++ -std=c++17 -O1 -I another_raytracer_amd/csrc tools/path_pool_check.cpp -o path_pool_check && ./path_pool_check 100000
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "path_pool.h"

using namespace art;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "path_pool_check: %s failed (line %d, round %llu)\n", #c, __LINE__, rounds); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

int main(int argc, char** argv) {
    const unsigned long long want = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100000ull;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    unsigned long long rounds = 0, batches = 0, pushed = 0, popped = 0, passes = 0;
    uint32_t high = 0;
    constexpr int kMaxDepth = 50;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    while (rounds < want) {
        // a pass: P slots, of which a wave sees batches of 64 (the last one partial), and a probability to go on
        const uint32_t P = 1u + static_cast<uint32_t>(rng() % 6000u);
        const double p_cont = static_cast<double>(rng() % 97u) / 100.0;
        const int max_depth = (rng() % 4u == 0) ? 1 + static_cast<int>(rng() % 3u) : kMaxDepth;
        std::vector<int> state(P, 0);  // 0 = not started, 1 = in a lane, 2 = in the pool, 3 = ended
        std::vector<uint32_t> pool(kPoolCap, kNone);
        uint32_t lane_path[64];
        int lane_depth[64];
        std::vector<int> pool_depth(kPoolCap, 0);
        bool busy[64] = {false};
        uint32_t count = 0, cur = 0;
        bool exhausted = false;
        const unsigned long long limit = rounds + 64ull * P * kMaxDepth + 64;  // every round but the last ends or advances a path
        for (;;) {
            CHECK(rounds < limit);
            uint32_t n_idle = 0;
            for (int l = 0; l < 64; ++l) n_idle += !busy[l];
            const bool fb = pool_batch_due(exhausted, count, n_idle);
            bool act[64];
            if (fb) {
                uint32_t rank = 0;
                for (int l = 0; l < 64; ++l)
                    if (busy[l]) {
                        const uint32_t pos = pool_push_pos(count, rank++);
                        CHECK(pos < kPoolCap && pos < kPoolBound);
                        CHECK(pool[pos] == kNone);
                        CHECK(state[lane_path[l]] == 1);
                        pool[pos] = lane_path[l];
                        pool_depth[pos] = lane_depth[l];
                        state[lane_path[l]] = 2;
                        ++pushed;
                    }
                count += rank;
                CHECK(count <= kPoolBound);
                if (count > high) high = count;
                const uint32_t b = cur;
                cur += 64;
                if (b + 64u >= P) exhausted = true;
                for (int l = 0; l < 64; ++l) {
                    act[l] = b + l < P;
                    if (act[l]) {
                        CHECK(state[b + l] == 0);
                        state[b + l] = 1;
                        lane_path[l] = b + l;
                    }
                    lane_depth[l] = 0;
                }
                ++batches;
            } else {
                const uint32_t npop = pool_pop_count(count, n_idle);
                CHECK(npop <= count && npop <= n_idle);
                if (npop) {
                    uint32_t rank = 0;
                    for (int l = 0; l < 64; ++l)
                        if (!busy[l]) {
                            if (rank < npop) {
                                const uint32_t pos = pool_pop_pos(count, rank);
                                CHECK(pos < count);
                                CHECK(pool[pos] != kNone && state[pool[pos]] == 2);
                                lane_path[l] = pool[pos];
                                lane_depth[l] = pool_depth[pos];
                                CHECK(lane_depth[l] >= 1);
                                state[lane_path[l]] = 1;
                                pool[pos] = kNone;
                                busy[l] = true;
                                ++popped;
                            }
                            ++rank;
                        }
                    count -= npop;
                } else if (n_idle == 64) {
                    CHECK(exhausted && count == 0);
                    ++rounds;
                    break;
                }
                for (int l = 0; l < 64; ++l) act[l] = busy[l];
            }
            // entries below the count are live, entries above it are free
            for (uint32_t i = 0; i < kPoolCap; ++i) CHECK((pool[i] != kNone) == (i < count));
            for (int l = 0; l < 64; ++l) {
                if (!(fb || act[l])) continue;
                bool cont = false;
                if (act[l]) {
                    CHECK(state[lane_path[l]] == 1);
                    cont = lane_depth[l] + 1 < max_depth && static_cast<double>(rng() % 1000u) / 1000.0 < p_cont;
                    if (!cont) state[lane_path[l]] = 3;
                }
                busy[l] = cont;
                ++lane_depth[l];
            }
            ++rounds;
        }
        for (uint32_t s = 0; s < P; ++s) CHECK(state[s] == 3);
        CHECK(count == 0);
        ++passes;
    }
    CHECK(pushed == popped);
    std::printf("path_pool_check ok: %llu rounds, %llu passes, %llu batches, %llu entries pushed and popped, most entries at once %u (bound %u, capacity %u)\n",
                rounds, passes, batches, pushed, high, kPoolBound, kPoolCap);
    return 0;
}

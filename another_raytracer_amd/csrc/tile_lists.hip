// tile_lists.hip — k_tile_lists and its launcher: the per-tile sphere lists k_paths' batches test instead of walking
// the tree (tile_lists.h).  One launch per rt_render call, before the first pass; its own object (MAIN_SCHED).
#include "launch.h"
#include "tile_lists.h"

namespace art {

constexpr int kTileBlock = 256, kTileWaves = kTileBlock / 64;

// One wave per 8x8 tile, lanes over the representative slots behind the LDS scene image (TileReps): lane i tests slot
// reps[i], reps[i + 64], ... against the tile's fat ray (tile_reaches) and the candidates are gathered, in slot order,
// into the wave's LDS row; at most kTileK of them are then ranked by their key (ties by position: a total order) and
// written nearest first.  A tile with more candidates gets kTileOverflow.  Block-wide barriers only: every wave of
// the block runs the same trip counts (a wave past the last tile works on tile 0 and writes nothing).
__global__ __launch_bounds__(kTileBlock) void k_tile_lists(const uint8_t* image, CameraRec cam, TileFrame g, uint32_t ntiles, TileRec* out) {
    __shared__ double s_key[kTileWaves][kTileK + 1];
    __shared__ uint16_t s_slot[kTileWaves][kTileK + 1];
    __shared__ uint16_t s_out[kTileWaves][kTileK + 1];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tile_w = blockIdx.x * kTileWaves + wv;
    const bool live = tile_w < ntiles;
    const uint32_t tile = live ? tile_w : 0u;
    const TileReps* reps = reinterpret_cast<const TileReps*>(image + kLdsImageBytes);
    const uint32_t n = reps->n <= kLdsSlotCap ? reps->n : 0u;
    const TileBundle b = tile_bundle(cam, g, tile);
    const uint64_t below = (1ull << lane) - 1ull;
    if (lane <= kTileK) s_out[wv][lane] = 0;
    uint32_t count = 0;  // wave-uniform
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        bool cand = false;
        double key = 0.0;
        uint32_t slot = 0;
        if (i < n) {
            slot = reps->slot[i] & (kLdsSlotCap - 1);
            const double2 a = reinterpret_cast<const double2*>(image + kLdsOffSph)[slot];
            const double2 c = reinterpret_cast<const double2*>(image + kLdsOffSph)[kLdsSlotCap + slot];  // (cz, r * r)
            const double dy = reinterpret_cast<const double*>(image + kLdsOffMov)[slot];
            cand = tile_reaches(b, a.x, a.y, c.x, sqrt(c.y), dy, key);
        }
        const uint64_t m = __ballot(cand);
        const uint32_t rank = count + static_cast<uint32_t>(__popcll(m & below));
        if (cand && rank <= kTileK) {
            s_key[wv][rank] = key;
            s_slot[wv][rank] = static_cast<uint16_t>(slot);
        }
        count += static_cast<uint32_t>(__popcll(m));
    }
    __syncthreads();
    const bool over = count > kTileK;
    if (!over && lane < count) {
        const double key = s_key[wv][lane];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < count; ++j) {
            const double kj = s_key[wv][j];
            rank += (kj < key || (kj == key && j < lane)) ? 1u : 0u;
        }
        s_out[wv][1u + rank] = s_slot[wv][lane];
    }
    __syncthreads();
    if (live && lane <= kTileK) {
        uint16_t* rec = reinterpret_cast<uint16_t*>(out + tile);
        rec[lane] = lane == 0 ? (over ? kTileOverflow : static_cast<uint16_t>(count)) : (over ? uint16_t(0) : s_out[wv][lane]);
    }
}

void launch_tile_lists(hipStream_t st, const DevScene& S, const PassGeom& g, const CameraRec& cam, void* tiles) {
    const uint32_t ntiles = g.npix_pad / 64u;
    const TileFrame tf{g.W, g.H, g.band_rows, g.band_count, g.band_index, g.tiles_x};
    hipLaunchKernelGGL(k_tile_lists, dim3((ntiles + kTileWaves - 1) / kTileWaves), dim3(kTileBlock), 0, st, S.lds_image, cam, tf, ntiles,
                       static_cast<TileRec*>(tiles));
}

}  // namespace art

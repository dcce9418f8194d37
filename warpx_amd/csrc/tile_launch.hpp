// What the two LDS-tile kernels (deposit_tile.hip, gather_tile.hip) share on the way to a launch: the tiles of the last
// cell sort, the queue of the particles that leave their tile, and the host-side preamble that fills both.
#ifndef WXA_TILE_LAUNCH_HPP_
#define WXA_TILE_LAUNCH_HPP_

#include "heavy_tiles.hpp"
#include "workspace.hpp"

#ifndef WXA_STRAGGLER_BLOCKS
// workgroups of 256 lanes of the straggler kernels (a grid-stride loop over a list whose length only the device
// knows).  512 workgroups are two waves per SIMD; 2048 were measured for the gather's and change nothing (0.19-0.62 ms per
// launch either way at 256^3 x 8 per cell, profiles/round5/README.md): the kernel is not short of waves in flight
#define WXA_STRAGGLER_BLOCKS 512
#endif

namespace wxa {

struct TileGeom {
    int nt[3];        // tiles per direction
    int cell_lo[3];   // global index of the brick's first cell
};

// Particles whose stencil leaves the LDS tile (stale sort, particles outside the domain before
// the periodic wrap) are queued and handled by the kernel's straggler twin with global loads / atomics:
// keeping that path out of the tile kernel saves registers and instruction cache.
struct StragglerQueue {
    int* __restrict__ idx;
    unsigned* __restrict__ count;
    unsigned* __restrict__ next = nullptr;   // the next launch's counter, zeroed by this one (wxa::flip_counter)
    __device__ __forceinline__ void push(int ip) const { idx[atomicAdd(count, 1u)] = ip; }
};

struct TileLaunch {
    TileGeom tg;
    long ntiles = 0;
    const int* offsets = nullptr;   // first particle of every cell, tile-major (ws->offsets)
    StragglerQueue sq{nullptr, nullptr, nullptr};
    HeavyUnits hu;                  // tiles with far more particles than the others are shared by several workgroups (heavy_tiles.hpp)
    unsigned groups = 0;            // workgroups of the tile kernel: the regular grid and the heavy tiles' extra units
};

// The launch of a tile kernel over the `np` sorted particles of ws->sorted.  The straggler count is the two-slot counter at
// words `counter_word`, `counter_word + 1` of ws->counters, flipped `flips` times so far.  Everything that can fail comes
// first and the flip last: a launch that is not made leaves the counter protocol where it was.  On `st`, in this order:
// the planning of the heavy tiles (its memset and kernel, if any tile can be heavy), then -- once per workspace -- the
// memset of the counters; the caller's tile kernel follows.
inline wxa_status plan_tile_launch(wxa_workspace* ws, long np, CounterWord counter_word, unsigned& flips, hipStream_t st, TileLaunch& tl) {
    for (int d = 0; d < 3; ++d) {
        tl.tg.nt[d] = ws->sorted.tiles(d);
        tl.tg.cell_lo[d] = ws->sorted.cell_lo[d];
    }
    tl.ntiles = (long)tl.tg.nt[0] * tl.tg.nt[1] * tl.tg.nt[2];
    tl.offsets = (const int*)ws->offsets.p;
    wxa_status rc;
    if ((rc = ws->stragglers.reserve(sizeof(int) * (size_t)np + 64)) != WXA_OK) return rc;
    long extra_groups = 0;
    if ((rc = plan_heavy_tiles(ws, tl.offsets, tl.ntiles, np, tl.hu, extra_groups, st)) != WXA_OK) return rc;
    tl.groups = (unsigned)(xcd_grid_size(tl.ntiles) + extra_groups);
    unsigned *cnt_now = nullptr, *cnt_next = nullptr;
    if ((rc = flip_counter(ws, counter_word, flips, st, cnt_now, cnt_next)) != WXA_OK) return rc;
    tl.sq = StragglerQueue{(int*)ws->stragglers.p, cnt_now, cnt_next};
    return WXA_OK;
}

}  // namespace wxa
#endif

// bcp_ego_route.h -- which kernel draws an egocentric call, and with what launch shape: the LDS arithmetic of the kernels
// of bcp_ego.h, the cost model of the sparse route, and the route decision as pure functions of the call's shape.  No HIP in
// here (the C ABI's header names the routes, BCP_EGO_*): bcp_ego.h and bcp_ego_host.h include it, and so does a stand-alone
// host program (tests/c_abi/ego_route_main.cpp) that checks the decision table without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/bcplan.h"

namespace bcp {

constexpr int kEgoWaves = 8;        // wavefronts (= images in flight) per workgroup of ego_costmap_kernel
constexpr int kEgoBoundInts = 16;   // behind the tables: {first live row, first inside row, inside end, live end} per wave
constexpr int kEgoCellCapMin = 512; // least stride of a list (a RandomMiniEnv world: <= 2 x 183 cells; pool entries change)
constexpr int kEgoHeld = 768;       // cells a wave can hold back in LDS between the culling pass and the patches

// the LDS a route may ask for: a staged map with its tables (gfx950 gives a workgroup up to 160 KB; a big copy costs
// occupancy, but LDS sampling still wins), the window route, the sparse routes
constexpr size_t kEgoStageLds = 150 * 1024, kEgoWindowLds = 60 * 1024, kEgoSparseLds = 64 * 1024;

// LDS copy of a map with a border ring; one table of the sampling kernels (row terms, row bounds); a map that can be staged
// whole beside the four tables of the binned kernel
static inline size_t ego_map_bytes(int rows, int cols) { return ((size_t)(rows + 2) * (cols + 2) + 7) & ~(size_t)7; }
static inline size_t ego_row_bytes(int drows) { return ((size_t)drows * 2 + kEgoBoundInts) * sizeof(int32_t); }
static inline bool ego_fits_lds(int rows, int cols, int drows) { return ego_map_bytes(rows, cols) + 4 * ego_row_bytes(drows) <= kEgoStageLds; }

// the part of a map a window can see: at most the window's diagonal (+ 2 px of rounding, + ring) squared
static inline size_t ego_win_bytes(int drows, int dcols)
{
    const double diag = std::sqrt((double)drows * drows + (double)dcols * dcols);
    const size_t side = (size_t)std::ceil(diag) + 5;
    return (side * side + 7) & ~(size_t)7;
}

// LDS of ego_sparse_kernel, per wave: cv::hal::warpAffine's column terms {adelta, bdelta}(x) = {sat(M0 x 1024), sat(M3 x 1024)}
// for every column of the window, its row terms {sat((M1 y + M2) 1024) + 512, sat((M4 y + M5) 1024) + 512} for every row,
// and the list of cells held back.
static inline size_t ego_sparse_lds_bytes(int drows, int dcols, int waves)
{
    return (size_t)waves * ((size_t)(drows + dcols) * 8 + (size_t)kEgoHeld * 4);
}

// LDS of ego_pooled_sparse_kernel, per wave: the tables and the held list of ego_sparse_kernel, then one 32-bit word per
// pooled cell (the LDS maximum works on words), an even number of them so that the next wave's tables stay 8-byte aligned
static inline size_t ego_pooled_lds_bytes(int drows, int dcols, int prows, int pcols, int waves)
{
    return (size_t)waves * ((size_t)(drows + dcols) * 8 + (size_t)kEgoHeld * 4 + (((size_t)prows * pcols + 1) & ~(size_t)1) * 4);
}

// The cost model of the sparse route (tools/bench_ego_cells.py measures both sides on the box): per image the fill-and-patch
// kernel pays ~0.4 instructions per listed cell for the culling pass and ~2.5 per cell that meets the window, the sampling
// kernels ~0.1 per destination pixel when the map is staged in LDS whole and five times that when every workgroup stages the
// part of the map its window sees.  BCP_TUNE_EGO_SPARSE >= 2 is an explicit limit (tests, sweeps).
static inline int32_t ego_sparse_limit(int32_t tuning, int64_t pixels, bool fits_lds)
{
    if (tuning >= 2) return tuning;
    const int64_t lim = fits_lds ? pixels / 8 : pixels / 2;
    return (int32_t)std::max<int64_t>(kEgoCellCapMin, std::min<int64_t>(lim, 16384));
}

// The shape of one call, as far as the route depends on it.
struct EgoCall {
    int rows, cols;     // allocation shape of one map
    bool shared;
    int drows, dcols;   // window, in pixels
    int border;
    int pool;           // 1: full-resolution images
    int64_t n;          // images
};

// waves per workgroup of ego_pooled_sparse_kernel: as many of kEgoWaves as fit the 64 KB the sparse route budgets (a small
// `pool` on a large window leaves many words per image); 0 = not even one, the sampled route takes the call
static inline int ego_pooled_sparse_waves(int drows, int dcols, int pool)
{
    const size_t one = ego_pooled_lds_bytes(drows, dcols, (drows + pool - 1) / pool, (dcols + pool - 1) / pool, 1);
    return (int)std::min<size_t>(kEgoWaves, kEgoSparseLds / one);
}

// ... and of the sparse kernel this call would run; 0: its tables do not fit, the sampling routes take the call
static inline int ego_sparse_waves(const EgoCall& c)
{
    if (c.pool > 1) return ego_pooled_sparse_waves(c.drows, c.dcols, c.pool);
    return ego_sparse_lds_bytes(c.drows, c.dcols, kEgoWaves) <= kEgoSparseLds ? kEgoWaves : 0;
}

// Sparse maps and a zero border (extract_egocentric_costmap's default): zero fill + one patch per non-zero source cell
// (ego_sparse_kernel) can serve this call -- whether it does is decided from the counts of non-zero cells (EgoCells).
// tuning: BCP_TUNE_EGO_SPARSE; refused: the lists could not be allocated once.  (A cell is packed as row << 12 | column.)
static inline bool ego_sparse_candidate(const EgoCall& c, int32_t tuning, bool refused)
{
    return c.border == 0 && c.rows <= 4095 && c.cols <= 4095 && !refused && tuning && ego_sparse_waves(c) > 0;
}

struct EgoPlan {
    int32_t route;           // BCP_EGO_*
    int waves;               // wavefronts per workgroup
    size_t lds_bytes;        // dynamic LDS of the launch
    int32_t stage_map;       // EgoArgs::stage_map
    int32_t win_lds_bytes;   // EgoArgs::win_lds_bytes
    int px;                  // pixels per lane of the sampling kernels: 8 (one 64-bit store), narrow windows fall back to 4
};

// The route of a call.  What it knows of the cell lists: `usable` -- they exist and describe the maps --, the largest
// `count` of any entry, the `limit` in force.  Maps with more cells than that, a non-zero border or no lists keep the
// sampling kernels.
static inline EgoPlan ego_route_of(const EgoCall& c, bool usable, int32_t count, int32_t limit)
{
    EgoPlan p = {BCP_EGO_NONE, kEgoWaves, 0, 0, 0, c.dcols >= 8 ? 8 : 4};
    const size_t map_bytes = ego_map_bytes(c.rows, c.cols), row_bytes = ego_row_bytes(c.drows);
    const bool fits_lds = ego_fits_lds(c.rows, c.cols, c.drows);
    if (ego_sparse_candidate(c, 1, false) && usable && count >= 0 && count <= limit) {
        // one image per wave; pooled: nothing but the pooled bytes goes to HBM
        p.route = c.pool > 1 ? BCP_EGO_POOLED_SPARSE : BCP_EGO_SPARSE;
        p.waves = ego_sparse_waves(c);
        p.lds_bytes = c.pool > 1 ? ego_pooled_lds_bytes(c.drows, c.dcols, (c.drows + c.pool - 1) / c.pool, (c.dcols + c.pool - 1) / c.pool, p.waves)
                                 : ego_sparse_lds_bytes(c.drows, c.dcols, p.waves);   // (<= 64 KB)
    } else if (c.pool > 1) {
        p.route = BCP_EGO_POOLED_SAMPLED;   // any map, any border value: every pooled cell samples its block from global memory
    } else if (!c.shared && fits_lds && c.n < ((int64_t)1 << 31)) {
        // private / pooled maps that fit LDS: group the images by map entry, then one workgroup per entry at a time
        p.route = BCP_EGO_BINNED;
        p.waves = 4;
        p.lds_bytes = map_bytes + 4 * row_bytes;
        p.stage_map = 1;
    } else {
        // shared map (staged in LDS when it fits) or maps too large for LDS: persistent workgroups
        p.stage_map = (c.shared && fits_lds) ? 1 : 0;
        const size_t win_bytes = ego_win_bytes(c.drows, c.dcols);
        if (!p.stage_map && win_bytes + row_bytes <= kEgoWindowLds) {
            // too large: each workgroup stages just the part of the map its window can see
            p.route = BCP_EGO_WINDOW;
            p.waves = 4;
            p.win_lds_bytes = (int32_t)win_bytes;
            p.lds_bytes = win_bytes + row_bytes;
        } else {
            p.route = p.stage_map ? BCP_EGO_STAGED : BCP_EGO_GLOBAL;
            p.lds_bytes = kEgoWaves * row_bytes + (p.stage_map ? map_bytes : 0);
        }
    }
    return p;
}

}  // namespace bcp

// bcp_goal_plan.h -- everything a goal_field_kernel launch decides before it touches the device: where the masks and the
// plane live, the threads of a workgroup, the grid, the dynamic LDS and the scratch the global route needs.  Pure
// arithmetic, no HIP in here: goal_launch (bcp_goal_host.h) asks it for every launch of every form, goal_field_kernel
// (bcp_goal.h) takes its LDS offsets from goal_lds_bytes, and a stand-alone host program (tests/c_abi/goal_plan_main.cpp)
// prints a table of plans without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BCP_HD __host__ __device__
#else
#define BCP_HD
#endif

namespace bcp {

constexpr int kGoalFixedWords = 128 + 4;   // half-widths [128], pass flags [3], counter

// dynamic LDS of the kernel: the fixed words, and on the LDS route both masks and the plane; cost: behind them the table
// [256] uint16 (on either route) and, on the LDS route, the map's bytes
BCP_HD inline size_t goal_lds_bytes(int rows, int cols, int wpr, bool in_lds, bool cost = false)
{
    const size_t fixed = (size_t)kGoalFixedWords * 4, cells = (size_t)rows * cols;
    const size_t plain = in_lds ? fixed + (size_t)2 * rows * wpr * 4 + ((cells * 2 + 3) & ~(size_t)3) : fixed;
    return cost ? plain + 512 + (in_lds ? (cells + 3) & ~(size_t)3 : 0) : plain;
}

constexpr size_t kGoalMaxLds = 150 * 1024;         // the library's limit on dynamic LDS (kMaxDynamicLds, bcp_host.h)
constexpr int64_t kGoalLdsGrid = 16384;            // LDS route: workgroups at most ...
constexpr int64_t kGoalBoundGrid = 1024;           // ... and in the bound form, whose grid never depends on the device-side count
// Global route: two masks per workgroup in scratch, so the grid is what sizes it (as for bcp_inflate_costmaps).
constexpr int64_t kGoalGlobalGrid = 512;
constexpr int64_t kGoalScratchBytes = 256ll << 20;

struct GoalPlan {
    bool in_lds;             // masks and plane in LDS; else masks in scratch and the plane in `out`
    unsigned threads;        // of a workgroup
    int64_t grid;            // workgroups (0 without trips: nothing is launched)
    size_t lds_bytes;        // dynamic LDS of the launch
    int64_t scratch_words;   // uint32 words of scratch the launch needs: grid * 2 * rows * wpr on the global route, else 0
};

// trips: maps (bcp_goal_field) or listed entries (bound) the launch walks; forced_global: BCP_TUNE_GOAL_ROUTE = 2
inline GoalPlan plan_goal(int32_t rows, int32_t cols, int64_t trips, bool bound, bool cost, bool forced_global)
{
    GoalPlan p;
    const int32_t wpr = (cols + 31) / 32;
    p.in_lds = goal_lds_bytes(rows, cols, wpr, true, cost) <= kGoalMaxLds && !forced_global;
    // a workgroup's threads: enough cells each to be worth their barriers
    p.threads = (int64_t)rows * cols >= 128 * 128 ? 1024u : 256u;
    p.lds_bytes = goal_lds_bytes(rows, cols, wpr, p.in_lds, cost);
    if (p.in_lds) {
        const int64_t cap = bound ? kGoalBoundGrid : kGoalLdsGrid;
        p.grid = trips < cap ? trips : cap;
        p.scratch_words = 0;
        return p;
    }
    const int64_t mask_words = (int64_t)2 * rows * wpr;
    const int64_t fit = kGoalScratchBytes / (mask_words * (int64_t)sizeof(uint32_t));
    const int64_t cap = fit < 1 ? 1 : (fit < kGoalGlobalGrid ? fit : kGoalGlobalGrid);
    p.grid = trips < cap ? trips : cap;
    p.scratch_words = p.grid * mask_words;
    return p;
}

}  // namespace bcp

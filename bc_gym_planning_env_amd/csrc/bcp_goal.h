// bcp_goal.h -- goal_field_kernel and goal_sample_kernel: the geodesic cost-to-go of bcp_goal_field and its per-row reads
// (include/bcplan.h).  The arithmetic of a cell -- the pull relaxation, the widening of a mask word, the carrot walk -- is
// bcp_goal_cell.h, which has no HIP in it and which the host tests run as it stands; this file decides who works on which
// cell and where the words live.
//
// goal_field_kernel: one workgroup per map (a grid stride over maps), phases with a barrier between them:
//   0  clear the 1-bit lethal mask [rows][wpr], the pass flags and the counter
//   1  read the map ONCE, four cells per aligned dword, as inflate_kernel does; a lethal byte inside the valid shape sets its bit
//   2  `closed` [rows][wpr] = the lethal mask dilated by the clearance disc, OR everything outside the valid shape: per
//      destination word the OR over the source rows |dr| <= reach of the words around it widened by that row's half-width
//      (goal_widen_word: shifts on 64-bit words).  A thread per word.
//   3  the uint16 plane = kGoalNone everywhere; then the seeds inside the valid shape: value 0, their closed bit cleared
//   4  passes: a wave per row, a lane per column; a thread PULLS for its own cells (eight neighbour reads, goal_relax_cell)
//      and writes only those, with ordinary stores.  A read may see a neighbour's value of this pass or of the last one:
//      values only fall and every value is the length of an admissible route, so either is right.  A thread that lowered a
//      cell raises the pass's flag; after the barrier a pass that raised none ends the loop -- everything it read was written
//      before the barrier in front of it, so nothing can change any more.  The flags rotate over three words: the word of
//      pass p + 1 is cleared during pass p, when its last readers (after pass p - 2) are two barriers behind.
//   5  copy the plane to `out` and count the cells that hold a value; info = {count, gave_up}
// The masks and the plane live in LDS when they fit (kLds); otherwise the masks are a slice of handle-owned scratch per
// workgroup and the plane IS the map's slab of `out`.  A workgroup runs on one CU and its barriers order its own global
// stores and loads (workgroup scope); no workgroup touches another's map.  The code is one template: the bytes are the same.
// kBound (bcp_goal_field_bound / bcp_refresh_goal_fields): the same phases on the handle's own binding.  The trip counter
// walks a selection of entries (EntrySelect: all of them, or a device-side list with a device-side count) instead of
// 0 .. n_maps - 1, and phase 3 takes the entry's one seed from the last way point of its bound path.  Entries that are not
// worked on keep their slab of `out` and their row of `info`.  The grid never depends on the count: a workgroup without a
// trip leaves at once.
// kCost (bcp_goal_field_cost / bcp_goal_field_cost_bound): the same phases; phase 4 adds the relaxed cell's extra
// (goal_relax_cell_cost), looked up in a table staged in LDS by the map's byte, which phase 1 kept in LDS (kLds) or which is
// read from `data` again.  The four kernels without kCost are, instruction for instruction, what they were without it.
#pragma once

#include "bcp_device.h"
#include "bcp_goal_cell.h"
#include "bcp_goal_plan.h"   // goal_lds_bytes, kGoalFixedWords: the LDS the host plans is the LDS the kernel lays out
#include "bcp_step.h"   // EntrySelect

namespace bcp {

typedef __attribute__((address_space(3))) uint16_t* GoalLdsU16;
typedef __attribute__((address_space(3))) uint8_t* GoalLdsU8;

struct GoalArgs {
    const uint8_t* data;         // [n_maps][rows][cols], or [rows][cols] when shared
    const int32_t* valid_rows;   // optional [n_maps], with valid_cols
    const int32_t* valid_cols;
    const int32_t* seeds;        // [n_maps][n_seeds][2] (row, col)
    uint16_t* out;               // [n_maps][rows][cols]
    int32_t* info;               // optional [n_maps][2]
    uint32_t* scratch;           // global route: [gridDim.x][2][rows][wpr]
    int64_t n_maps;
    int32_t rows, cols, wpr, shared;
    int32_t n_seeds, clearance_d2, reach, max_passes;   // reach = floor(sqrt(clearance_d2)); max_passes >= 1
};

// The bound form (bcp_goal_field_bound, bcp_refresh_goal_fields): the extra words behind GoalArgs.  The maps, valid shapes,
// `out` and `info` are GoalArgs' (the handle's own binding, shared = 0, n_maps = the entry count); the entries worked on are
// a selection, and each entry's one seed is the last way point of its bound path.
struct GoalBound {
    EntrySelect sel;             // {list, count, n_list}: list == nullptr = entries 0 .. n_list - 1
    const double* paths;         // [n_maps][max_len][3], as given to bcp_set_paths
    const int32_t* lens;         // [n_maps]
    const double* origins;       // [n_maps][2], or nullptr: (ox, oy)
    double ox, oy, inv_res;
    int32_t max_len, pad;
};

// The cost form (bcp_goal_field_cost, bcp_goal_field_cost_bound): the table of extras per map byte, by value -- a launch
// keeps the table it was made with, and nothing is uploaded.
struct GoalCost {
    uint16_t extra[256];
};

// The kernel's argument: GoalArgs as it is, behind it the bound part for the kBound kernels only and the table for the
// kCost kernels only -- the others take what they always took.
template <bool kBound, bool kCost = false> struct GoalKernelArgs;
template <> struct GoalKernelArgs<false, false> {
    GoalArgs g;
};
template <> struct GoalKernelArgs<true, false> {
    GoalArgs g;
    GoalBound b;
};
template <> struct GoalKernelArgs<false, true> {
    GoalArgs g;
    GoalCost c;
};
template <> struct GoalKernelArgs<true, true> {
    GoalArgs g;
    GoalBound b;
    GoalCost c;
};

template <bool kLds> struct GoalMem;
template <> struct GoalMem<true> {
    typedef LdsU32 Words;
    typedef GoalLdsU16 Plane;
};
template <> struct GoalMem<false> {
    typedef uint32_t* Words;
    typedef uint16_t* Plane;
};

template <typename Plane>
struct GoalPlaneGet {
    Plane p;
    int32_t cols;
    __device__ __forceinline__ uint16_t operator()(int32_t r, int32_t c) const { return p[r * cols + c]; }
};

// kCost: the field weighted by the map's costs (goal_relax_cell_cost).  Phase 1 keeps every byte it reads in a uint8 plane
// in LDS (kLds; on the global route phase 4 reads the byte from `data`, which nobody writes during the call), the table is
// staged in LDS once per workgroup, and phase 4 reads one byte and one table entry per cell it relaxes.  Only cells that
// are open are relaxed, and everything outside the valid shape is closed: the bytes of the padding never reach the table.
template <bool kLds, bool kBound, bool kCost = false>
__global__ void __launch_bounds__(1024) goal_field_kernel(const GoalKernelArgs<kBound, kCost> ka)
{
    const GoalArgs& a = ka.g;
    typedef typename GoalMem<kLds>::Words Words;
    typedef typename GoalMem<kLds>::Plane Plane;
    const int rows = a.rows, cols = a.cols, wpr = a.wpr, cells = rows * cols, n_words = rows * wpr;
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, n_waves = nthr >> 6;
    const LdsU32 half_width = (LdsU32)lds_dyn;     // [reach + 1]
    const LdsU32 flags = half_width + 128;         // [3]
    const LdsU32 counter = flags + 3;
    Words lethal, closed;
    Plane plane;
    if constexpr (kLds) {
        lethal = counter + 1;
        closed = lethal + n_words;
        plane = (GoalLdsU16)(closed + n_words);
    } else {
        lethal = a.scratch + (int64_t)blockIdx.x * 2 * n_words;
        closed = lethal + n_words;
        plane = nullptr;
    }
    for (int dr = tid; dr <= a.reach; dr += nthr) half_width[dr] = (uint32_t)goal_half_width(a.clearance_d2, dr);
    [[maybe_unused]] GoalLdsU16 extra_of = nullptr;   // kCost: [256], behind the plane (kLds) or the fixed words
    [[maybe_unused]] GoalLdsU8 bytes = nullptr;       // kCost && kLds: [cells], the map as phase 1 read it
    if constexpr (kCost) {
        if constexpr (kLds) extra_of = (GoalLdsU16)((LdsU32)lds_dyn + (goal_lds_bytes(rows, cols, wpr, true) >> 2));
        else extra_of = (GoalLdsU16)(counter + 1);
        bytes = (GoalLdsU8)(extra_of + 256);
        for (int i = tid; i < 256; i += nthr) extra_of[i] = ka.c.extra[i];   // (the first barrier of a trip is ahead of phase 4)
    }

    // trips: the maps 0 .. n_maps - 1, or (kBound) the selection's entries -- *count clamped to [0, n_list], so the loop is
    // bounded by n_list whatever the word holds; an id outside [0, n_maps) is skipped by the whole workgroup
    int64_t trips = a.n_maps;
    if constexpr (kBound) trips = ka.b.sel.list && ka.b.sel.count ? min(max(ka.b.sel.size(), (int64_t)0), ka.b.sel.n) : ka.b.sel.n;
    for (int64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        int64_t m = trip;
        if constexpr (kBound) {
            m = ka.b.sel.entry(trip);
            if (m < 0 || m >= a.n_maps) continue;
        }
        uint16_t* const dst = a.out + m * (int64_t)cells;
        if constexpr (!kLds) plane = dst;
        int vr = rows, vc = cols;
        if (a.valid_rows) {
            vr = min(max(a.valid_rows[m], 0), rows);
            vc = min(max(a.valid_cols[m], 0), cols);
        }
        // ---- 0: clear (the previous map's phases 4 and 5 read neither the lethal mask nor, after thread 0 is done, the counter)
        for (int i = tid; i < n_words; i += nthr) lethal[i] = 0u;
        if (tid == 0) flags[0] = flags[1] = flags[2] = *counter = 0u;
        __syncthreads();
        // ---- 1: the map, once.  Dword j of the aligned run that covers the map holds cells 4 j - head .. 4 j - head + 3
        {
            const uint8_t* src = a.data + (a.shared ? 0 : m) * (int64_t)cells;
            const int head = (int)((uintptr_t)src & 3u);
            const uint32_t* words = reinterpret_cast<const uint32_t*>(src - head);
            const int n_dwords = (cells + head + 3) >> 2;
            for (int j = tid; j < n_dwords; j += nthr) {
                const uint32_t y = words[j] ^ 0xFEFEFEFEu;   // a zero byte = a lethal cell
                if constexpr (kCost && kLds) {               // keep the bytes of the map's own cells
                    for (int b = 0; b < 4; ++b) {
                        const int p = 4 * j - head + b;
                        if (p >= 0 && p < cells) bytes[p] = (uint8_t)((y >> (8 * b)) ^ 0xFEu);
                    }
                }
                if (((y - 0x01010101u) & ~y & 0x80808080u) == 0u) continue;
                for (int b = 0; b < 4; ++b) {
                    const int p = 4 * j - head + b;          // (bytes before and after the map belong to others: skipped)
                    if (((y >> (8 * b)) & 255u) != 0u || p < 0 || p >= cells) continue;
                    const int r = p / cols, c = p - r * cols;
                    if (r < vr && c < vc)
                        __hip_atomic_fetch_or(lethal + r * wpr + (c >> 5), 1u << (c & 31), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // ---- 2: closed = blocked, or outside the valid shape
        for (int i = tid; i < n_words; i += nthr) {
            const int r = i / wpr, w = i - r * wpr, first = 32 * w;
            const uint32_t inside = r < vr && vc > first ? (vc - first >= 32 ? ~0u : (1u << (vc - first)) - 1u) : 0u;
            uint32_t acc = 0u;
            if (inside) {
                const int lo = max(r - a.reach, 0), hi = min(r + a.reach, vr - 1);
                for (int rr = lo; rr <= hi; ++rr) {
                    const int hw = (int)half_width[rr > r ? rr - r : r - rr], kw = (hw + 31) >> 5;
                    const int k0 = max(w - kw, 0), k1 = min(w + kw, wpr - 1);
                    for (int k = k0; k <= k1; ++k) acc |= goal_widen_word(lethal[rr * wpr + k], 32 * (k - w), hw);
                }
            }
            closed[i] = (acc & inside) | ~inside;
        }
        // ---- 3: the plane and the seeds
        for (int i = tid; i < cells; i += nthr) plane[i] = (uint16_t)kGoalNone;
        __syncthreads();
        if constexpr (kBound) {   // one seed: the goal of the entry's path, on the entry's origin (goal_seed_of_path)
            const GoalBound& b = ka.b;
            const int32_t len = min(b.lens[m], b.max_len);
            if (tid == 0 && len >= 1) {
                const double* goal = b.paths + (m * b.max_len + (len - 1)) * 3;
                const double ox = b.origins ? b.origins[2 * m] : b.ox, oy = b.origins ? b.origins[2 * m + 1] : b.oy;
                int32_t sr = 0, sc = 0;
                if (goal_seed_of_path(goal[0], goal[1], ox, oy, b.inv_res, vr, vc, sr, sc)) {
                    plane[sr * cols + sc] = (uint16_t)0;
                    closed[sr * wpr + (sc >> 5)] &= ~(1u << (sc & 31));   // (thread 0 alone, between two barriers)
                }
            }
        } else {
            for (int s = tid; s < a.n_seeds; s += nthr) {
                const int32_t* seed = a.seeds + (m * a.n_seeds + s) * 2;
                const int sr = seed[0], sc = seed[1];
                if ((uint32_t)sr < (uint32_t)vr && (uint32_t)sc < (uint32_t)vc) {
                    plane[sr * cols + sc] = (uint16_t)0;
                    __hip_atomic_fetch_and(closed + sr * wpr + (sc >> 5), ~(1u << (sc & 31)), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // ---- 4: passes
        int gave_up = 0;
        {
            const GoalPlaneGet<Plane> get = {plane, cols};
            int mine = 0, next = 1;   // flag words of this pass and of the one after it
            for (int pass = 0;; ++pass) {
                if (pass == a.max_passes) {   // (the pass before this one lowered a cell)
                    gave_up = 1;
                    break;
                }
                if (tid == 0) flags[next] = 0u;
                bool lowered = false;
                for (int r = wave; r < vr; r += n_waves) {
                    for (int c = lane; c < vc; c += 64) {
                        if ((closed[r * wpr + (c >> 5)] >> (c & 31)) & 1u) continue;
                        const int32_t own = plane[r * cols + c];
                        if (own == 0) continue;
                        int32_t now;
                        if constexpr (kCost) {
                            int32_t cost;
                            if constexpr (kLds) cost = bytes[r * cols + c];
                            else cost = a.data[(a.shared ? 0 : m) * (int64_t)cells + r * cols + c];
                            now = goal_relax_cell_cost(get, vr, vc, r, c, own, (int32_t)extra_of[cost]);
                        } else {
                            now = goal_relax_cell(get, vr, vc, r, c, own);
                        }
                        if (now != own) {
                            plane[r * cols + c] = (uint16_t)now;
                            lowered = true;
                        }
                    }
                }
                if (lowered) flags[mine] = 1u;
                __syncthreads();
                if (flags[mine] == 0u) break;
                mine = next;
                next = next == 2 ? 0 : next + 1;
            }
        }
        // ---- 5: out and info
        {
            uint32_t n_set = 0u;
            for (int i = tid; i < cells; i += nthr) {
                const uint16_t v = plane[i];
                if constexpr (kLds) dst[i] = v;
                n_set += v != (uint16_t)kGoalNone ? 1u : 0u;
            }
            if (a.info) {
                if (n_set) __hip_atomic_fetch_add(counter, n_set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __syncthreads();
                if (tid == 0) {
                    a.info[2 * m] = (int32_t)*counter;
                    a.info[2 * m + 1] = gave_up;
                }
            }
        }
        // (no barrier here: phase 0 of the next map writes the lethal mask, the flags and -- thread 0 alone, after its read
        //  above -- the counter; its barrier keeps closed and the plane intact until every thread has left phase 5)
    }
}

// ---- per-row reads of finished fields ---------------------------------------------------------------------------
// Whose row reads what: the part of the arguments that goal_sample_kernel and goal_route_kernel share, and the one
// statement of how a row finds its env, its entry, the entry's origin and valid shape, and its field (goal_row_entry).
struct GoalRows {
    const uint16_t* field;       // [n_fields][rows][cols]
    int64_t n_fields, n_entries;   // n_entries: pool entries, or n_envs without a pool
    int32_t rows, cols, shared, pad;
    const int32_t* valid_rows;   // per entry, or nullptr: the allocated shape
    const int32_t* valid_cols;
    const double* origins;       // per entry, or nullptr: (ox, oy)
    double ox, oy, inv_res, resolution;
    const double* poses;         // [n][3] or nullptr: sx, sy, sth
    const double *sx, *sy, *sth;
    const int32_t* entry;        // entry of an env (pool entry, or env of a record's slot), or nullptr: the env index itself
    const int32_t* row_env;      // env of row i, or nullptr: i % n_envs
    int64_t n_envs, n;
};

struct GoalSampleArgs {
    GoalRows src;
    int32_t carrot_cells, pad;
    double max_dist;
    const int32_t* live;         // rows beyond min(*live, n) are left alone, or nullptr
    float* out3;
    int32_t* cell_value;         // or nullptr
    int32_t* carrot;             // or nullptr
};

struct GoalFieldGet {
    const uint16_t* p;
    int32_t cols;
    __device__ __forceinline__ uint16_t operator()(int32_t r, int32_t c) const { return p[r * cols + c]; }
};

// the entry a row stands on
struct GoalRowEntry {
    int64_t slot;                // the env's entry among the non-shared arrays: it picks the field and the bound path
    double ox, oy;
    int32_t vr, vc;
    GoalFieldGet get;
};

// false: the row's env or its entry is out of range, and `e` is untouched
__device__ __forceinline__ bool goal_row_entry(const GoalRows& a, int64_t i, GoalRowEntry& e)
{
    const int64_t me = a.row_env ? (int64_t)a.row_env[i] : i % a.n_envs;
    if (me < 0 || me >= a.n_envs) return false;
    // the env's entry among the non-shared arrays: it picks the field; the map it is read on is entry 0 when shared
    const int64_t slot = a.entry ? (int64_t)a.entry[me] : me;
    if (slot < 0 || slot >= a.n_entries) return false;
    const int64_t g = a.shared ? 0 : slot;
    e.slot = slot;
    e.ox = a.origins ? a.origins[2 * g] : a.ox;
    e.oy = a.origins ? a.origins[2 * g + 1] : a.oy;
    e.vr = a.valid_rows ? max(0, min(a.valid_rows[g], a.rows)) : a.rows;
    e.vc = a.valid_cols ? max(0, min(a.valid_cols[g], a.cols)) : a.cols;
    e.get.p = a.field + (a.n_fields == 1 ? 0 : slot) * ((int64_t)a.rows * a.cols);
    e.get.cols = a.cols;
    return true;
}

__device__ __forceinline__ void goal_row_pose(const GoalRows& a, int64_t i, double pose[3])
{
    pose[0] = a.poses ? a.poses[3 * i] : a.sx[i];
    pose[1] = a.poses ? a.poses[3 * i + 1] : a.sy[i];
    pose[2] = a.poses ? a.poses[3 * i + 2] : a.sth[i];
}

__device__ __forceinline__ bool goal_pose_finite(const double pose[3])
{
    const double lim = 1.7976931348623157e308;   // (a NaN fails every comparison)
    return pose[0] >= -lim && pose[0] <= lim && pose[1] >= -lim && pose[1] <= lim && pose[2] >= -lim && pose[2] <= lim;
}

__global__ void __launch_bounds__(256) goal_sample_kernel(GoalSampleArgs a)
{
    const GoalRows& R = a.src;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_rows = a.live ? min(R.n, (int64_t)max(*a.live, 0)) : R.n;
    if (i >= n_rows) return;
    GoalSample s = goal_no_sample(a.max_dist);
    GoalRowEntry e;
    if (goal_row_entry(R, i, e)) {
        double pose[3];
        goal_row_pose(R, i, pose);
        const bool finite = goal_pose_finite(pose);
        const double ct = finite ? cos(pose[2]) : 0.0, st = finite ? sin(pose[2]) : 0.0;
        s = goal_sample_row(e.get, e.vr, e.vc, pose[0], pose[1], ct, st, finite, e.ox, e.oy, R.inv_res, R.resolution,
                            a.carrot_cells, a.max_dist);
    }
    a.out3[3 * i] = s.out3[0];
    a.out3[3 * i + 1] = s.out3[1];
    a.out3[3 * i + 2] = s.out3[2];
    if (a.cell_value) a.cell_value[i] = s.cell_value;
    if (a.carrot) {
        a.carrot[2 * i] = s.carrot_row;
        a.carrot[2 * i + 1] = s.carrot_col;
    }
}

// ---- routes -----------------------------------------------------------------------------------------------------------
// goal_route_kernel: one lane per row.  A row's walk is a chain of dependent 3 x 3 reads of a plane that L2 holds; the
// parallelism is the rows', and nothing is staged.  A row's way points are its own: it writes them with plain stores, reads
// them back for the headings and the provider state (the same lane, program order), and nobody else touches them.
struct GoalRouteArgs {
    GoalRows src;
    const double* goals;         // [n][3], or nullptr: the last way point of the bound path of the row's entry
    const double* src_paths;     // the bound paths [.][src_max_len][3] (one [src_max_len][3] when src_lens is nullptr), or nullptr
    const int32_t* src_lens;
    int32_t src_max_len, bound;  // bound: row m is entry m and starts at its bound path[0]
    int32_t stride, max_len, pure_pursuit, pad;
    double sp, ap;
    double* paths;               // [n][max_len][3]
    int32_t* lens;               // [n]
    double* init;                // [n][2], or nullptr
    int32_t* status;             // [n]
};

__global__ void __launch_bounds__(256) goal_route_kernel(GoalRouteArgs a)
{
    const GoalRows& R = a.src;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n) return;
    double* const wp = a.paths + i * (int64_t)a.max_len * 3;
    int32_t len = 0, status = kGoalRouteNoRoute;
    double init[2] = {0.0, 0.0};
    bool routed = false;
    GoalRowEntry e;
    if (goal_row_entry(R, i, e)) {
        // the bound path of the row's entry: its last way point is the goal (and, in the bound form, its first the start)
        const double* src = nullptr;
        int32_t src_len = 0;
        if (a.src_paths) {
            src = a.src_paths + (a.src_lens ? e.slot : 0) * (int64_t)a.src_max_len * 3;
            src_len = a.src_lens ? min(a.src_lens[e.slot], a.src_max_len) : a.src_max_len;
        }
        const bool need_src = a.bound || !a.goals;
        if (!need_src || src_len >= 1) {
            double start[3], goal[3];
            if (a.bound) {
                start[0] = src[0];
                start[1] = src[1];
                start[2] = src[2];
            } else {
                goal_row_pose(R, i, start);
            }
            const double* g = a.goals ? a.goals + 3 * i : src + 3 * (int64_t)(src_len - 1);
            goal[0] = g[0];
            goal[1] = g[1];
            goal[2] = g[2];
            const bool finite = goal_pose_finite(start) && goal_pose_finite(goal);
            status = goal_route_row(e.get, e.vr, e.vc, start, goal, finite, e.ox, e.oy, R.inv_res, R.resolution, a.stride,
                                    a.max_len, a.sp, a.ap, a.pure_pursuit, DeviceNormalizeAngle(), wp, len, init);
            routed = true;
        }
    }
    if (!routed)
        for (int32_t j = 0; j < 3 * a.max_len; ++j) wp[j] = 0.0;
    a.lens[i] = len;
    a.status[i] = status;
    if (a.init) {
        a.init[2 * i] = init[0];
        a.init[2 * i + 1] = init[1];
    }
}

}  // namespace bcp

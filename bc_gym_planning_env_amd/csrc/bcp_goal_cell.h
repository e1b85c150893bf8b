// bcp_goal_cell.h -- the goal field's arithmetic (bcp_goal_field, bcp_goal_field_sample; include/bcplan.h): the argument
// checks, the half-widths of the clearance disc and the widening of one mask word, the pull relaxation of one cell -- plain, and
// weighted by the map's costs (goal_relax_cell_cost, bcp_goal_field_cost) --, the field at a pose, the seed cell of a bound
// path (bcp_goal_field_bound), the sampling of one row with its carrot walk, and the route of one row (bcp_goal_route: the
// walk written out as a path).  Plain C++ with no HIP in it.  Who calls this, on the device: goal_field_kernel,
// goal_sample_kernel and goal_route_kernel (bcp_goal.h), and mppi_kernel's terminal read (bcp_mppi.h).  On the host, under
// sanitizers and through bounds-checked accessors: tests/c_abi/goal_sweep.h (for goal_field_main.cpp and goal_cost_main.cpp),
// goal_seed_main.cpp, goal_route_main.cpp and mppi_field_main.cpp call the same functions, and there is no other copy of
// them.  What is NOT here is who works on which word: the loops of goal_field_kernel's phases 2 (the `closed` word) and 3
// (the seeds) are the kernel's, and goal_sweep.h restates them once around goal_half_width and goal_widen_word.  The float64
// arithmetic rounds every product, quotient, root and sum on its own (-ffp-contract=off).
//
// A field is a uint16 plane [rows][cols]: kGoalNone where no route exists (blocked, outside the valid shape, not connected
// to a seed), else min(length of the cheapest admissible route to a seed, kGoalFar) with steps of kGoalOrtho to an edge
// neighbour and kGoalDiag to a corner neighbour.  A corner step is admissible only if both edge neighbours it passes
// between are free.  While the plane is being relaxed "free" is read off the plane itself: a cell counts as free once it
// holds a value.  That only delays a corner step until both edge cells are reached -- and they are reached whenever the
// corner's far end is, being edge neighbours of it -- so the fixed point is the same, and every intermediate value is
// still the length of an admissible route.
#pragma once

#include <cmath>
#include <cstdint>

#include "bcp_path_init.h"   // path_initial_reward: the provider state of a routed path (goal_route_row)

#if defined(__HIPCC__)
#define BCP_HD __host__ __device__
#else
#define BCP_HD
#endif

namespace bcp {

constexpr int32_t kGoalOrtho = 12;
constexpr int32_t kGoalDiag = 17;
constexpr int32_t kGoalFar = 65534;
constexpr int32_t kGoalNone = 65535;
constexpr int32_t kGoalMaxSide = 2048;
constexpr int32_t kGoalMaxSeeds = 4096;
constexpr int32_t kGoalMaxClearance = 127 * 127;   // BCP_MAX_KERNEL_HALF squared
constexpr int32_t kGoalMaxCarrot = 256;

// neighbour k: E, NE, N, NW, W, SW, S, SE
BCP_HD inline int32_t goal_dcol(int k) { return k == 0 || k == 1 || k == 7 ? 1 : (k == 2 || k == 6 ? 0 : -1); }
BCP_HD inline int32_t goal_drow(int k) { return k >= 1 && k <= 3 ? 1 : (k == 0 || k == 4 ? 0 : -1); }

// what bcp_goal_field refuses with BCP_E_INVALID, in the order it looks
enum GoalRefusal {
    kGoalOk = 0, kGoalHandle = 1, kGoalMaps = 2, kGoalShape = 3, kGoalSeeds = 4, kGoalClearance = 5, kGoalPasses = 6,
    kGoalValidPair = 7, kGoalValidShared = 8, kGoalPointers = 9
};

BCP_HD inline int goal_field_check_args(bool have_handle, int64_t n_maps, bool have_data, bool have_seeds, bool have_out,
                                        int32_t rows, int32_t cols, int32_t n_seeds, int32_t clearance_d2, int32_t max_passes,
                                        bool have_valid_rows, bool have_valid_cols, bool shared)
{
    if (!have_handle) return kGoalHandle;
    if (n_maps < 0) return kGoalMaps;
    if (rows < 1 || rows > kGoalMaxSide || cols < 1 || cols > kGoalMaxSide) return kGoalShape;
    if (n_seeds < 1 || n_seeds > kGoalMaxSeeds) return kGoalSeeds;
    if (clearance_d2 < 0 || clearance_d2 > kGoalMaxClearance) return kGoalClearance;
    if (max_passes < 0) return kGoalPasses;
    if (have_valid_rows != have_valid_cols) return kGoalValidPair;
    if (shared && have_valid_rows) return kGoalValidShared;
    if (n_maps > 0 && (!have_data || !have_seeds || !have_out)) return kGoalPointers;
    return kGoalOk;
}

// ... and bcp_goal_field_sample.  n_entries: fields the binding has (0 while no costmaps are bound: the comparisons with the
// binding are then the caller's BCP_E_STATE); final_form: the rows are the record's, n is not the caller's to choose
enum GoalSampleRefusal {
    kGoalSampleOk = 0, kGoalSampleNull = 1, kGoalSampleCarrot = 2, kGoalSampleDist = 3, kGoalSampleRows = 4,
    kGoalSampleRowEnv = 5, kGoalSampleShape = 6, kGoalSampleFields = 7
};

BCP_HD inline int goal_sample_check_args(bool have_handle, bool have_field, bool have_out3, int32_t carrot_cells, double max_dist,
                                         int64_t n, int64_t n_envs, bool have_poses, bool have_row_env, bool final_form,
                                         int32_t rows, int32_t cols, int32_t map_rows, int32_t map_cols, int64_t n_fields,
                                         int64_t n_entries)
{
    if (!have_handle || !have_field || !have_out3) return kGoalSampleNull;
    if (carrot_cells < 1 || carrot_cells > kGoalMaxCarrot) return kGoalSampleCarrot;
    if (!(max_dist > 0.0)) return kGoalSampleDist;   // (a NaN fails the comparison; +inf passes)
    if (!final_form && (n <= 0 || (!have_poses && n != n_envs))) return kGoalSampleRows;
    if (!have_poses && have_row_env) return kGoalSampleRowEnv;
    if (n_entries > 0 && (rows != map_rows || cols != map_cols)) return kGoalSampleShape;
    if (n_entries > 0 && n_fields != 1 && n_fields != n_entries) return kGoalSampleFields;
    return kGoalSampleOk;
}

BCP_HD inline int32_t goal_isqrt(int32_t n)   // floor(sqrt(n)), 0 <= n <= kGoalMaxClearance
{
    int32_t r = 0;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// half-width of the clearance disc `dr` rows from its centre, |dr| <= goal_isqrt(clearance_d2)
BCP_HD inline int32_t goal_half_width(int32_t clearance_d2, int32_t dr) { return goal_isqrt(clearance_d2 - dr * dr); }

// One word of a bit row widened by `hw` to either side, as seen in the word `d` columns to its left (d = 32 * (source word -
// destination word)): bit j of the result is set iff the source has a bit b with |d + b - j| <= hw.
BCP_HD inline uint32_t goal_widen_word(uint32_t x, int32_t d, int32_t hw)
{
    const int32_t a = d - hw > -31 ? d - hw : -31, b = d + hw < 31 ? d + hw : 31;   // the shifts that land in the word
    if (x == 0u || a > b) return 0u;
    uint64_t y = (uint64_t)x << 32;              // the destination word is the upper half: right shifts keep their bits
    y = a >= 0 ? y << a : y >> -a;
    for (int32_t cover = 0, n = b - a; cover < n;) {   // y covers the shifts a .. a + cover
        const int32_t s = cover + 1 < n - cover ? cover + 1 : n - cover;
        y |= y << s;
        cover += s;
    }
    return (uint32_t)(y >> 32);
}

// The pull relaxation of cell (r, c) of a plane whose valid shape is (vr, vc): the smallest of its own value and, over its
// admissible neighbours, the neighbour's value plus the step, saturating at kGoalFar.  get(row, col) reads the plane and is
// only ever called inside the valid shape.  The caller sees to it that a blocked cell is never relaxed.
template <typename Get>
BCP_HD inline int32_t goal_relax_cell(const Get& get, int32_t vr, int32_t vc, int32_t r, int32_t c, int32_t own)
{
    int32_t v[8];
    for (int k = 0; k < 8; ++k) {
        const int32_t rr = r + goal_drow(k), cc = c + goal_dcol(k);
        v[k] = (uint32_t)rr < (uint32_t)vr && (uint32_t)cc < (uint32_t)vc ? (int32_t)get(rr, cc) : kGoalNone;
    }
    const int32_t nothing = 0x7FFFFFFF;
    int32_t best = own == kGoalNone ? nothing : own;
    for (int k = 0; k < 8; k += 2)
        if (v[k] != kGoalNone) best = v[k] + kGoalOrtho < best ? v[k] + kGoalOrtho : best;
    for (int k = 1; k < 8; k += 2)   // a corner step passes between edge neighbours k - 1 and k + 1
        if (v[k] != kGoalNone && v[k - 1] != kGoalNone && v[(k + 1) & 7] != kGoalNone)
            best = v[k] + kGoalDiag < best ? v[k] + kGoalDiag : best;
    if (best == nothing) return kGoalNone;
    return best < kGoalFar ? best : kGoalFar;   // (the sums stop at kGoalFar: a longer route reads kGoalFar, never kGoalNone)
}

// ---- fields weighted by the map's costs (bcp_goal_field_cost, bcp_goal_field_cost_bound) --------------------------------
// With a table extra_of_cost[256] of uint16, each <= kGoalMaxExtra, and e(c) = extra_of_cost[data[c]]:
//     v(seed) = 0,   v(c) = min over admissible neighbours n of sat(v(n) + step(n, c) + e(c))   for a free, non-seed cell c
// The extra belongs to the cell that is entered on the way from the goal, i.e. the cell being relaxed: in the pull form it
// is one addition behind the minimum over the eight neighbours.  Everything else is the plain field's: obstacles (== 254
// only), clearance, seeds (value 0 and free whatever stood there: their extra is never charged), the valid shape, the
// corner rule, the steps, the saturation at kGoalFar, kGoalNone.  An all-zero table gives the plain field bit for bit.
// The weights stay positive integers and the sum monotone and saturating, so the fixed point is unique and does not depend
// on the order of evaluation, and every intermediate value is still the cost of an admissible route.
// e(c) is the same for every neighbour of c, so goal_walk_step's argmin(field + step) is the true successor on a weighted
// field too: goal_walk_step, goal_sample_row, goal_route_row, goal_value_at and mppi_kernel's terminal read consume a
// weighted field UNCHANGED.  Below kGoalFar every cell's successor is strictly cheaper (the step is >= 12), so a walk still
// lowers a uint16 on every trip; on a saturated stretch it ends in kGoalRouteStuck, as on a saturated plain field.
constexpr int32_t kGoalMaxExtra = 4095;

// The pull relaxation of a weighted field: goal_relax_cell's minimum over the neighbours alone, plus `extra` (the relaxed
// cell's own, 0 .. kGoalMaxExtra), saturating at kGoalFar; then the smaller of that and the cell's own value.
template <typename Get>
BCP_HD inline int32_t goal_relax_cell_cost(const Get& get, int32_t vr, int32_t vc, int32_t r, int32_t c, int32_t own, int32_t extra)
{
    const int32_t via = goal_relax_cell(get, vr, vc, r, c, kGoalNone);   // kGoalNone, or <= kGoalFar
    if (via == kGoalNone) return own;
    const int32_t now = via + extra < kGoalFar ? via + extra : kGoalFar;
    return own == kGoalNone || now < own ? now : own;
}

// what bcp_goal_field_cost refuses on top of goal_field_check_args (those come first, in their order): a NULL table, then
// the first entry above kGoalMaxExtra -- all 256 are looked at, 254 and 255 too, although a lethal byte is never looked up
enum GoalCostRefusal { kGoalCostOk = 0, kGoalCostTable = 1, kGoalCostEntry = 2 };

// bad_index: the first offending entry when the answer is kGoalCostEntry
BCP_HD inline int goal_cost_check_args(const uint16_t* extra_of_cost, int32_t& bad_index)
{
    if (!extra_of_cost) return kGoalCostTable;
    for (int32_t i = 0; i < 256; ++i)
        if ((int32_t)extra_of_cost[i] > kGoalMaxExtra) {
            bad_index = i;
            return kGoalCostEntry;
        }
    return kGoalCostOk;
}

// One step of the carrot walk on a finished field from (r, c): the admissible neighbour k that minimises field + step, ties
// to the lowest k; -1 if no neighbour is admissible.
template <typename Get>
BCP_HD inline int goal_walk_step(const Get& get, int32_t vr, int32_t vc, int32_t r, int32_t c)
{
    int32_t v[8];
    for (int k = 0; k < 8; ++k) {
        const int32_t rr = r + goal_drow(k), cc = c + goal_dcol(k);
        v[k] = (uint32_t)rr < (uint32_t)vr && (uint32_t)cc < (uint32_t)vc ? (int32_t)get(rr, cc) : kGoalNone;
    }
    int best_k = -1;
    int32_t best = 0;
    for (int k = 0; k < 8; ++k) {
        if (v[k] == kGoalNone) continue;
        if ((k & 1) && (v[k - 1] == kGoalNone || v[(k + 1) & 7] == kGoalNone)) continue;
        const int32_t cost = v[k] + ((k & 1) ? kGoalDiag : kGoalOrtho);
        if (best_k < 0 || cost < best) {
            best_k = k;
            best = cost;
        }
    }
    return best_k;
}

struct GoalSample {
    float out3[3];         // min(distance, max_dist) in metres, direction to the carrot in the robot frame
    int32_t cell_value;    // the field at the pose's cell, kGoalNone for a row without a result
    int32_t carrot_row, carrot_col;   // (-1, -1) for a row without a result
};

BCP_HD inline GoalSample goal_no_sample(double max_dist)
{
    GoalSample s;
    s.out3[0] = (float)max_dist;
    s.out3[1] = s.out3[2] = 0.0f;
    s.cell_value = kGoalNone;
    s.carrot_row = s.carrot_col = -1;
    return s;
}

// The field at a pose: (col, row) = half-to-even of ((x - ox) * inv_res, (y - oy) * inv_res) on a field with origin
// (ox, oy) and valid shape (vr, vc); kGoalNone where `finite` is false (the caller's word on x and y) or the cell lies
// outside the valid shape -- get is then not called.  (r, c): the cell, set whenever it lies inside.  The one statement of
// the rule: goal_sample_row (below) and mppi_kernel's terminal read (bcp_mppi.h) both go through it.
template <typename Get>
BCP_HD inline int32_t goal_value_at(const Get& get, int32_t vr, int32_t vc, double x, double y, bool finite, double ox,
                                    double oy, double inv_res, int32_t& r, int32_t& c)
{
    if (!finite) return kGoalNone;
    const double fc = __builtin_rint((x - ox) * inv_res), fr = __builtin_rint((y - oy) * inv_res);   // half to even
    if (!(fc >= 0.0 && fc < (double)vc && fr >= 0.0 && fr < (double)vr)) return kGoalNone;
    r = (int32_t)fr;
    c = (int32_t)fc;
    return (int32_t)get(r, c);
}

template <typename Get>
BCP_HD inline int32_t goal_value_at(const Get& get, int32_t vr, int32_t vc, double x, double y, bool finite, double ox,
                                    double oy, double inv_res)
{
    int32_t r = 0, c = 0;
    return goal_value_at(get, vr, vc, x, y, finite, ox, oy, inv_res, r, c);
}

// The seed of a bound path's last way point (x, y) on an entry with origin (ox, oy) and valid shape (vr, vc): the cell of
// goal_value_at, by the same statement of the rule.  false -- and (row, col) untouched -- where x or y is not finite or the
// cell lies outside the valid shape.  The range test is made on the rounded float64, before anything is converted: 1e300
// is merely "outside".
struct GoalAnyCell {
    BCP_HD uint16_t operator()(int32_t, int32_t) const { return (uint16_t)0; }
};

BCP_HD inline bool goal_seed_of_path(double x, double y, double ox, double oy, double inv_res, int32_t vr, int32_t vc,
                                     int32_t& row, int32_t& col)
{
    const double lim = 1.7976931348623157e308;
    const bool finite = x >= -lim && x <= lim && y >= -lim && y <= lim;   // (a NaN fails every comparison)
    return goal_value_at(GoalAnyCell(), vr, vc, x, y, finite, ox, oy, inv_res, row, col) != kGoalNone;
}

// what bcp_goal_field_bound and bcp_refresh_goal_fields refuse, in the order they look: 1 .. 6 with BCP_E_INVALID, 7 .. 10
// with BCP_E_STATE.  refresh_form: bcp_refresh_goal_fields -- the list is the ring's, not the caller's, and a refresh must
// be pending.  n_entries: the handle's entry count (pool entries, or n_envs without a pool).
enum GoalBoundRefusal {
    kGoalBoundOk = 0, kGoalBoundHandle = 1, kGoalBoundField = 2, kGoalBoundList = 3, kGoalBoundCount = 4,
    kGoalBoundClearance = 5, kGoalBoundPasses = 6, kGoalBoundUnbound = 7, kGoalBoundShared = 8, kGoalBoundShape = 9,
    kGoalBoundNoRefresh = 10
};

BCP_HD inline int goal_bound_check_args(bool have_handle, bool have_field, int64_t n_list, int64_t n_entries, bool have_entries,
                                        bool have_count, int32_t clearance_d2, int32_t max_passes, bool have_map,
                                        bool have_path, bool shared_map, bool shared_path, int32_t rows, int32_t cols,
                                        bool refresh_form, bool refresh_pending)
{
    if (!have_handle) return kGoalBoundHandle;
    if (!have_field) return kGoalBoundField;
    if (!refresh_form && (n_list < 0 || n_list > n_entries)) return kGoalBoundList;
    if (!refresh_form && have_count && !have_entries) return kGoalBoundCount;
    if (clearance_d2 < 0 || clearance_d2 > kGoalMaxClearance) return kGoalBoundClearance;
    if (max_passes < 0) return kGoalBoundPasses;
    if (!have_map || !have_path) return kGoalBoundUnbound;
    if (shared_map || shared_path) return kGoalBoundShared;
    if (rows < 1 || rows > kGoalMaxSide || cols < 1 || cols > kGoalMaxSide) return kGoalBoundShape;
    if (refresh_form && !refresh_pending) return kGoalBoundNoRefresh;
    return kGoalBoundOk;
}

// metres to go of a cell value, float64, the product and the quotient rounded on their own
BCP_HD inline double goal_metres(int32_t v, double resolution) { return ((double)v * resolution) / 12.0; }

// One row of bcp_goal_field_sample: pose (x, y) with heading (cos, sin) = (ct, st) on a field with origin (ox, oy) and valid
// shape (vr, vc); `finite`: x, y and the heading are finite numbers.
template <typename Get>
BCP_HD inline GoalSample goal_sample_row(const Get& get, int32_t vr, int32_t vc, double x, double y, double ct, double st,
                                         bool finite, double ox, double oy, double inv_res, double resolution,
                                         int32_t carrot_cells, double max_dist)
{
    int32_t r = 0, c = 0;
    int32_t v = goal_value_at(get, vr, vc, x, y, finite, ox, oy, inv_res, r, c);
    if (v == kGoalNone) return goal_no_sample(max_dist);
    const int32_t r0 = r, c0 = c;
    GoalSample s;
    const double dist = goal_metres(v, resolution);
    s.out3[0] = (float)(dist < max_dist ? dist : max_dist);
    s.cell_value = v;
    for (int32_t step = 0; step < carrot_cells && v != 0; ++step) {
        const int k = goal_walk_step(get, vr, vc, r, c);
        if (k < 0) break;
        r += goal_drow(k);
        c += goal_dcol(k);
        v = (int32_t)get(r, c);
    }
    s.carrot_row = r;
    s.carrot_col = c;
    if (r == r0 && c == c0) {
        s.out3[1] = s.out3[2] = 0.0f;
        return s;
    }
    const double dx = (ox + (double)c * resolution) - x, dy = (oy + (double)r * resolution) - y;
    const double norm = __builtin_sqrt(dx * dx + dy * dy);
    const double ux = dx / norm, uy = dy / norm;
    s.out3[1] = (float)(ux * ct + uy * st);
    s.out3[2] = (float)(uy * ct - ux * st);
    return s;
}

// ---- routes: the walk down a field written out as a path (bcp_goal_route, bcp_goal_route_bound) --------------------
constexpr int32_t kGoalRouteMaxStride = 64;
constexpr int32_t kGoalRouteMaxLen = 32766;   // bcp_set_paths' limit

// the bits of a row's status
constexpr int32_t kGoalRouteLong = 1;       // truncated: the first max_len - 1 way points, then the goal
constexpr int32_t kGoalRouteTooClose = 2;   // path_initial_reward's "Goal pose too close to initial pose"
constexpr int32_t kGoalRouteNoRoute = 4;    // no path at all: len 0, every slot zero, init (0, 0)
constexpr int32_t kGoalRouteStuck = 8;      // the plane is not a goal field here: the walk could not descend

// what bcp_goal_route and bcp_goal_route_bound refuse with BCP_E_INVALID, in the order they look.  bound_form: the rows are
// the binding's entries -- n is not the caller's to choose, there are no poses, and every entry needs a field of its own.
enum GoalRouteRefusal {
    kGoalRouteOk = 0, kGoalRouteNull = 1, kGoalRouteStride = 2, kGoalRouteMaxLenRange = 3, kGoalRouteRows = 4,
    kGoalRouteRowEnv = 5, kGoalRouteShape = 6, kGoalRouteFields = 7
};

BCP_HD inline int goal_route_check_args(bool have_handle, bool have_field, bool have_paths, bool have_lens, bool have_status,
                                        int32_t stride, int32_t max_len, int64_t n, int64_t n_envs, bool have_poses,
                                        bool have_row_env, bool bound_form, int32_t rows, int32_t cols, int32_t map_rows,
                                        int32_t map_cols, int64_t n_fields, int64_t n_entries)
{
    if (!have_handle || !have_field || !have_paths || !have_lens || !have_status) return kGoalRouteNull;
    if (stride < 1 || stride > kGoalRouteMaxStride) return kGoalRouteStride;
    if (max_len < 2 || max_len > kGoalRouteMaxLen) return kGoalRouteMaxLenRange;
    if (!bound_form && (n <= 0 || (!have_poses && n != n_envs))) return kGoalRouteRows;
    if (!bound_form && !have_poses && have_row_env) return kGoalRouteRowEnv;
    if (n_entries > 0 && (rows != map_rows || cols != map_cols)) return kGoalRouteShape;
    if (n_entries > 0 && n_fields != n_entries && (bound_form || n_fields != 1)) return kGoalRouteFields;
    return kGoalRouteOk;
}

// One row of bcp_goal_route: the route from the pose `start` (x, y, theta) down the field to a cell of value 0, written as
// way points wp[0 .. len) of [max_len][3]: the start pose bit for bit, the centre of every stride-th cell the walk enters
// before it arrives, the pose `goal` bit for bit.  Interior way points head for their successor; slots len .. max_len - 1
// are zeros.  init = (min_spat_dist_so_far, target_idx) of the reward provider on that path (path_initial_reward).  Returns
// the status bits.  `finite`: every number of start and goal is finite.  Every trip of the loop ends it or lowers v, which
// a uint16 gave: at most 65534 trips whatever the plane holds.
template <typename Get, typename Normalize>
BCP_HD inline int32_t goal_route_row(const Get& get, int32_t vr, int32_t vc, const double start[3], const double goal[3],
                                     bool finite, double ox, double oy, double inv_res, double resolution, int32_t stride,
                                     int32_t max_len, double sp, double ap, int pure_pursuit, const Normalize& normalize,
                                     double* wp, int32_t& len, double init[2])
{
    int32_t r = 0, c = 0;
    int32_t v = goal_value_at(get, vr, vc, start[0], start[1], finite, ox, oy, inv_res, r, c);
    if (v == kGoalNone) {
        for (int32_t j = 0; j < 3 * max_len; ++j) wp[j] = 0.0;
        len = 0;
        init[0] = init[1] = 0.0;
        return kGoalRouteNoRoute;
    }
    int32_t status = 0, k = 1, steps = 0;
    wp[0] = start[0];
    wp[1] = start[1];
    wp[2] = start[2];
    while (v != 0) {
        const int q = goal_walk_step(get, vr, vc, r, c);
        if (q < 0) {
            status |= kGoalRouteStuck;
            break;
        }
        const int32_t nr = r + goal_drow(q), nc = c + goal_dcol(q);
        const int32_t nv = (int32_t)get(nr, nc);
        if (nv >= v) {   // not a goal field
            status |= kGoalRouteStuck;
            break;
        }
        r = nr;
        c = nc;
        v = nv;
        ++steps;
        if (v != 0 && steps % stride == 0) {
            if (k == max_len - 1) {   // the last slot is the goal's
                status |= kGoalRouteLong;
                break;
            }
            wp[3 * k] = ox + (double)c * resolution;
            wp[3 * k + 1] = oy + (double)r * resolution;
            ++k;
        }
    }
    wp[3 * k] = goal[0];
    wp[3 * k + 1] = goal[1];
    wp[3 * k + 2] = goal[2];
    ++k;
    for (int32_t j = 1; j + 1 < k; ++j) {
        const double dx = wp[3 * (j + 1)] - wp[3 * j], dy = wp[3 * (j + 1) + 1] - wp[3 * j + 1];
        wp[3 * j + 2] = dx == 0.0 && dy == 0.0 ? goal[2] : atan2(dy, dx);
    }
    for (int32_t j = 3 * k; j < 3 * max_len; ++j) wp[j] = 0.0;
    len = k;
    double min_dist = 0.0;
    int target = 0, rc = 0;
    path_initial_reward(wp, k, sp, ap, pure_pursuit, min_dist, target, rc, normalize);
    if (rc == 2) status |= kGoalRouteTooClose;
    init[0] = min_dist;
    init[1] = (double)target;
    return status;
}

}  // namespace bcp

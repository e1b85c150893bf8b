// bcp_smooth.h -- smooth_kernel: bcp_smooth_route (include/bcplan.h), a cell chain pulled taut and blended into a path a
// tracker can follow.  The arithmetic -- the line-of-sight walk, a corner's blend, the pieces of a row -- is
// bcp_smooth_cell.h, which has no HIP in it and which the host tests run as it stands (smooth_row is the row as a sequential
// program); this file decides which lane tests which candidate, corner and piece.
//
// One wave per row, one wave per workgroup.  A row of m way points has work for a wave where goal_route_kernel's had work
// for a lane: up to `look` line-of-sight walks per anchor, a blend test per corner, and a few hundred way points to write.
//   0  stage: a lane per way point reads its three numbers, votes on "finite", and keeps the way point's cell in LDS
//      (int16 row, col; -1: no cell)
//   1  pull: per anchor k the 64 lanes test 64 candidates j per trip, the farthest chunk first; a ballot, and the highest
//      set lane is the next anchor.  The loop moves k on every trip: at most m - 1 anchors of at most ceil(look / 64) trips.
//      The vertices go to LDS as uint16 (anchor index | level << 12).
//   2  blends: a lane per corner (smooth_blend_level: at most 9 sizes); the level goes into the vertex's word
//   3  count: a lane per piece, a wave sum per 64 pieces.  LONG is decided here, before anything is written.
//   4  write: a lane per piece again; an exclusive prefix sum over the pieces' counts gives every lane its slots.  The
//      pieces are recomputed from the vertices, not kept: a piece is two corners' worth of arithmetic.  Then the zero tail.
//   5  headings: a lane per way point reads its successor, which another lane may have written: the stores of phase 4 are
//      made visible first by a workgroup-scope fence with the barrier (nothing is recomputed).  The same again ahead of
//      6  lane 0's path_initial_reward over the written row, the very function goal_route_row calls.
// LDS: 6 bytes per slot of paths_in, dynamic: 24 KB at max_len_in = 4096 (6 workgroups of one wave per CU by LDS), 6 KB at
// 1024 (26 per CU; the CU's 32 wave slots are the limit from about 800 slots down).  More waves per workgroup would share
// nothing: a row's LDS is its own.
#pragma once

#include "bcp_device.h"
#include "bcp_goal.h"          // GoalRows, goal_row_entry: whose row stands on which entry
#include "bcp_smooth_cell.h"

namespace bcp {

struct SmoothArgs {
    GoalRows src;                // poses unused; entry == nullptr and n_envs == n_entries when rows are entries
    const double* paths_in;      // [n][max_len_in][3]
    const int32_t* lens_in;      // [n]
    int32_t max_len_in, max_len, pure_pursuit, pad;
    SmoothParams prm;
    double sp, ap;
    double* paths;               // [n][max_len][3]
    int32_t* lens;               // [n]
    double* init;                // [n][2], or nullptr
    int32_t* status;             // [n]
    int32_t* info;               // [n][4], or nullptr
};

typedef __attribute__((address_space(3))) int16_t* SmoothLdsS16;
typedef __attribute__((address_space(3))) uint16_t* SmoothLdsU16;

struct SmoothIn {
    const double* p;
    __device__ __forceinline__ double operator()(int32_t k, int32_t e) const { return p[3 * k + e]; }
};
struct SmoothCellLds {
    SmoothLdsS16 cells;
    __device__ __forceinline__ bool operator()(int32_t k, int32_t& r, int32_t& c) const
    {
        r = cells[2 * k];
        c = cells[2 * k + 1];
        return r >= 0;
    }
};
struct SmoothVertexLds {
    SmoothLdsU16 v;
    __device__ __forceinline__ uint16_t operator()(int32_t t) const { return v[t]; }
};

// the sum of v over the wave's lanes below this one, and (total) over all of them
__device__ __forceinline__ int32_t smooth_exclusive_scan(int32_t v, int lane, int32_t& total)
{
    int32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t up = __shfl_up(inc, off);
        if (lane >= off) inc += up;
    }
    total = __shfl(inc, 63);
    return inc - v;
}

__global__ void __launch_bounds__(64) smooth_kernel(const SmoothArgs a)
{
    const GoalRows& R = a.src;
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const SmoothLdsS16 cells = (SmoothLdsS16)lds_dyn;                        // [max_len_in][2]
    const SmoothLdsU16 vertices = (SmoothLdsU16)(cells + 2 * a.max_len_in);  // [max_len_in]
    const int32_t max_len = a.max_len;
    double* const wp = a.paths + row * (int64_t)max_len * 3;
    const SmoothIn in = {a.paths_in + row * (int64_t)a.max_len_in * 3};
    const int32_t m = max(min(a.lens_in[row], a.max_len_in), 0);
    const SmoothParams prm = a.prm;

    GoalRowEntry e;
    bool ok = goal_row_entry(R, row, e) && m >= 2;   // (the row's own words: wave-uniform)
    SmoothMap<GoalFieldGet> map;
    if (ok) {
        map.get = e.get;
        map.vr = e.vr;
        map.vc = e.vc;
        map.ox = e.ox;
        map.oy = e.oy;
        map.inv_res = R.inv_res;
    }
    // ---- 0: stage
    if (ok) {
        bool finite = true;
        for (int32_t k = lane; k < m; k += 64) {
            const double x = in(k, 0), y = in(k, 1);
            finite = finite && smooth_finite(x) && smooth_finite(y) && smooth_finite(in(k, 2));
            int32_t r = -1, c = -1;
            if (!map.cell_of(x, y, r, c)) r = c = -1;
            cells[2 * k] = (int16_t)r;
            cells[2 * k + 1] = (int16_t)c;
        }
        ok = __ballot(!finite) == 0;
    }
    int32_t status = ok ? 0 : kGoalRouteNoRoute, M = 0, total = 0;
    int32_t n_full = 0, n_reduced = 0, n_sharp = 0;
    const SmoothCellLds cell = {cells};
    const SmoothVertexLds vertex = {vertices};
    if (ok) {
        __syncthreads();   // (ok is wave-uniform and the workgroup is one wave)
        // ---- 1: pull
        if (lane == 0) vertices[0] = (uint16_t)(kSmoothSharp << 12);
        for (int32_t k = 0; k < m - 1;) {
            const int32_t hi = min(k + prm.look, m - 1);
            int32_t next = -1;
            for (int32_t top = hi; top > k && next < 0; top -= 64) {   // candidates top - 63 .. top, lane 63 the farthest
                const int32_t j = top - 63 + lane;
                const uint64_t seen = __ballot(j > k && smooth_sees(map, cell, k, j));
                if (seen) next = top - __builtin_clzll(seen);
            }
            if (next < 0) {
                next = k + 1;
                status |= kSmoothBlocked;
            }
            ++M;
            if (lane == 0) vertices[M] = (uint16_t)(next | (kSmoothSharp << 12));
            k = next;
        }
        __syncthreads();
        // ---- 2: blends.  A lane writes its own vertex's word alone; the neighbours' indices it reads do not change.
        for (int32_t base = 1; base < M; base += 64) {
            const int32_t t = base + lane;
            int32_t level = -1;
            if (t < M) {
                const int32_t kp = vertices[t - 1] & 4095, kv = vertices[t] & 4095, kn = vertices[t + 1] & 4095;
                const double p[2] = {in(kp, 0), in(kp, 1)}, v[2] = {in(kv, 0), in(kv, 1)}, n[2] = {in(kn, 0), in(kn, 1)};
                level = smooth_blend_level(map, p, v, n, prm.blend, prm.delta, prm.halvings);
            }
            __syncthreads();   // (every lane has read its neighbours' words)
            if (t < M) vertices[t] = (uint16_t)((vertices[t] & 4095) | (level << 12));
            n_full += __popcll(__ballot(level == 0));
            n_sharp += __popcll(__ballot(level == kSmoothSharp));
            n_reduced += __popcll(__ballot(level > 0 && level != kSmoothSharp));
        }
        __syncthreads();
        // ---- 3: count
        total = 1;
        for (int32_t base = 0; base < 2 * M - 1; base += 64) {
            const int32_t piece = base + lane;
            int32_t count = piece < 2 * M - 1 ? smooth_piece(in, vertex, M, piece, prm.blend, prm.delta).count : 0;
            for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
            total += count;
        }
        if (total > max_len) {
            status |= kGoalRouteLong;
            ok = false;
        }
    }
    if (!ok) {   // NO_ROUTE or LONG: every slot zero
        for (int32_t j = lane; j < 3 * max_len; j += 64) wp[j] = 0.0;
        if (lane == 0) {
            a.lens[row] = 0;
            a.status[row] = status;
            if (a.init) a.init[2 * row] = a.init[2 * row + 1] = 0.0;
            if (a.info) {
                a.info[4 * row] = status & kGoalRouteLong ? M + 1 : 0;
                a.info[4 * row + 1] = n_full;
                a.info[4 * row + 2] = n_reduced;
                a.info[4 * row + 3] = n_sharp;
            }
        }
        return;
    }
    // ---- 4: write.  total <= max_len: every slot written below lies inside the row.
    const double goal_heading = in(m - 1, 2);
    if (lane == 0) {
        wp[0] = in(0, 0);
        wp[1] = in(0, 1);
        wp[2] = in(0, 2);
        wp[3 * (total - 1) + 2] = goal_heading;
    }
    int32_t at = 1;
    for (int32_t base = 0; base < 2 * M - 1; base += 64) {
        const int32_t piece = base + lane;
        SmoothPiece o;
        o.count = 0;
        if (piece < 2 * M - 1) o = smooth_piece(in, vertex, M, piece, prm.blend, prm.delta);
        int32_t chunk = 0;
        const int32_t first = at + smooth_exclusive_scan(o.count, lane, chunk);
        for (int32_t i = 1; i <= o.count; ++i) {
            double xy[2];
            smooth_piece_point(o, i, xy);
            wp[3 * (first + i - 1)] = xy[0];
            wp[3 * (first + i - 1) + 1] = xy[1];
        }
        at += chunk;
    }
    for (int32_t j = 3 * total + lane; j < 3 * max_len; j += 64) wp[j] = 0.0;
    __threadfence_block();
    __syncthreads();
    // ---- 5: headings (way points 0 and total - 1 keep the input's)
    for (int32_t j = 1 + lane; j + 1 < total; j += 64) wp[3 * j + 2] = smooth_heading(wp, j, goal_heading);
    __threadfence_block();
    __syncthreads();
    // ---- 6: the provider's state on the written row
    if (lane == 0) {
        double min_dist = 0.0;
        int target = 0, rc = 0;
        path_initial_reward(wp, total, a.sp, a.ap, a.pure_pursuit, min_dist, target, rc, DeviceNormalizeAngle());
        if (rc == 2) status |= kGoalRouteTooClose;
        a.lens[row] = total;
        a.status[row] = status;
        if (a.init) {
            a.init[2 * row] = min_dist;
            a.init[2 * row + 1] = (double)target;
        }
        if (a.info) {
            a.info[4 * row] = M + 1;
            a.info[4 * row + 1] = n_full;
            a.info[4 * row + 2] = n_reduced;
            a.info[4 * row + 3] = n_sharp;
        }
    }
}

}  // namespace bcp

// bcp_path_window.h -- the reward side of a step: the window of way points a pose can reach, the scans for the last reached
// one, the three reward providers, and the delay queues.  The step kernels and the roll-out core (bcp_lookahead.h) use them.
#pragma once

#include "bcp_bind_kernels.h"

// find_last_reached restricted to j >= target (utilities/path_tools.py:408-448): the reward only asks whether the
// LAST reached index is >= target_idx (envs/base/reward.py:234), so indices below target never matter.
// A way point can only be reached when |x_j - x| and |y_j - y| are both below spatial_precision, so the scan is
// confined to the index window the two bucket tables allow for this pose (usually a handful of way points).
// index window [lo, hi] of the way points that can be within spatial_precision of (x, y); empty when lo > hi
struct PathWindow {
    int lo, hi;
};

// bbox: the eight leading values of a path record -- the f32 words of the record itself, or a copy widened to doubles
// (the LDS copy of a shared path); either way the arithmetic below is on the same doubles
template <typename BoxPtr, typename IndexPtr>
__device__ __forceinline__ PathWindow path_window(const DevParams& P, BoxPtr bbox, IndexPtr index, double x, double y)
{
    PathWindow w;
    w.lo = 0;
    w.hi = -1;
    if (x < (double)bbox[0] - P.sp_prune || x > (double)bbox[1] + P.sp_prune || y < (double)bbox[2] - P.sp_prune ||
        y > (double)bbox[3] + P.sp_prune)
        return w;  // farther than spatial_precision from the bounding box of the whole path
    const int bx = min(max((int)floor((x - (double)bbox[4]) * (double)bbox[5]), 0), kPathBuckets - 1);
    const int by = min(max((int)floor((y - (double)bbox[6]) * (double)bbox[7]), 0), kPathBuckets - 1);
    const IndexPtr ix = index + 2 * bx;
    const IndexPtr iy = index + 2 * (kPathBuckets + by);
    w.lo = max((int)ix[0], (int)iy[0]);
    w.hi = min((int)ix[1], (int)iy[1]);
    return w;
}

// the same look-up in the compact tables of a private path (tables: the record's uint16 words from kBoxIndexU16 on;
// shift: its int32 word kBoxLenWord + 1) -- a superset of the window the 64-bucket tables would give
template <typename BoxPtr, typename TablePtr>
__device__ __forceinline__ PathWindow path_window_compact(const DevParams& P, BoxPtr bbox, TablePtr tables, int shift, double x,
                                                          double y)
{
    PathWindow w;
    w.lo = 0;
    w.hi = -1;
    if (x < (double)bbox[0] - P.sp_prune || x > (double)bbox[1] + P.sp_prune || y < (double)bbox[2] - P.sp_prune ||
        y > (double)bbox[3] + P.sp_prune)
        return w;
    const int bx = min(max((int)floor((x - (double)bbox[4]) * (double)bbox[5]), 0), kPathBucketsCompact - 1);
    const int by = min(max((int)floor((y - (double)bbox[6]) * (double)bbox[7]), 0), kPathBucketsCompact - 1);
    const uint32_t ix = tables[bx], iy = tables[kPathBucketsCompact + by];
    w.lo = (int)max(ix & 0xFFu, iy & 0xFFu) << shift;
    w.hi = (int)(((min(ix >> 8, iy >> 8) + 1u) << shift) - 1u);
    return w;
}

// the window of entry g's path for a pose, whichever tables the path has (everything but the step kernels' hot paths)
__device__ __forceinline__ PathWindow path_window_of(const DevParams& P, bool shared, const double* bbox, const int16_t* index,
                                                     int64_t g, double x, double y)
{
    if (shared) return path_window(P, reinterpret_cast<const float*>(bbox), index, x, y);
    const float* rec = reinterpret_cast<const float*>(bbox + g * kBoxDoubles);
    return path_window_compact(P, rec, reinterpret_cast<const uint16_t*>(rec) + kBoxIndexU16,
                               reinterpret_cast<const int32_t*>(rec)[kBoxLenWord + 1], x, y);
}

// one candidate way point (its five values already in registers) against the three reach conditions of
// path_tools.py:419-427; they are independent predicates, so the cheap ones go first
__device__ __forceinline__ bool way_point_reached(const DevParams& P, double sx, double sy, double sth, double sc, double ss,
                                                  double x, double y, double th)
{
    const double dx = sx - x, dy = sy - y;
    if (fabs(dx) > P.sp_prune || fabs(dy) > P.sp_prune) return false;   // then hypot(dx,dy) >= sp
    const double par = sc * (x - sx) + ss * (y - sy);                   // path_tools.py:405
    if (!(par >= P.par_thr)) return false;
    const double q = dx * dx + dy * dy;
    bool near = q < P.sp2_lo;
    if (!near && q <= P.sp2_hi) near = hypot(dx, dy) < P.sp;            // too close to call from q
    return near && fabs(normalize_angle(th - sth)) < P.ap;
}

// way points in LDS (shared path): one candidate at a time, first hit from the top wins
// (four at a time, like the global-memory form below, measured no faster: the scan is not bound by the LDS round trip)
template <typename PathPtr>
__device__ __forceinline__ int last_reached_from(const DevParams& P, PathPtr path, PathWindow w, int m, int target,
                                                 double x, double y, double th, int stride = 1)
{
    if (target > m - 1) return -1;
    const int lo = max(w.lo, target);
    const int hi = min(w.hi, m - 1);
    for (int j = hi; j >= lo; j -= stride) {
        const PathPtr s = path + 5 * j;
        // all five values of the way point are fetched up front (one latency instead of three dependent ones)
        if (way_point_reached(P, s[0], s[1], s[2], s[3], s[4], x, y, th)) return j;
    }
    return -1;
}

// way points in global memory (private / pooled paths, cold after the kernel boundary): four candidates are fetched
// together, so the scan pays one memory round trip per four way points instead of one each
// (TRIP candidates per round trip: four hold 40 vector registers while they are in flight -- where the caller is short of
//  registers, the finishing code of the configurations with delay queues, two)
template <int TRIP = 4>
__device__ __forceinline__ int last_reached_from(const DevParams& P, const double* __restrict__ path, PathWindow w, int m,
                                                 int target, double x, double y, double th)
{
    if (target > m - 1) return -1;
    const int lo = max(w.lo, target);
    const int hi = min(w.hi, m - 1);
    for (int j = hi; j >= lo; j -= TRIP) {
        double v[TRIP][5];
#pragma unroll
        for (int u = 0; u < TRIP; ++u) {
            const double* s = path + 5 * max(j - u, lo);   // (below lo: a harmless repeat of way point lo)
#pragma unroll
            for (int k = 0; k < 5; ++k) v[u][k] = s[k];
        }
#pragma unroll
        for (int u = 0; u < TRIP; ++u)
            if (j - u >= lo && way_point_reached(P, v[u][0], v[u][1], v[u][2], v[u][3], v[u][4], x, y, th)) return j - u;
    }
    return -1;
}

// find_last_reached for ONE pose by all 64 lanes of a wave (way points in LDS): lane l takes candidate hi - l, the first
// lane that reports "reached" holds the last reached index.  Wave-uniform arguments and result.
__device__ __forceinline__ int coop_last_reached(const DevParams& P, LdsF64 path, PathWindow w, int m, int target, double x,
                                                 double y, double th)
{
    if (target > m - 1) return -1;
    const int lo = max(w.lo, target), hi = min(w.hi, m - 1);
    const int ln = (int)__lane_id();
    for (int top = hi; top >= lo; top -= 64) {
        const int j = top - ln;
        bool ok = false;
        if (j >= lo) {
            const LdsF64 s = path + 5 * j;
            ok = way_point_reached(P, s[0], s[1], s[2], s[3], s[4], x, y, th);
        }
        const uint64_t mask = __ballot(ok);
        if (mask) return top - ((int)__ffsll((unsigned long long)mask) - 1);
    }
    return -1;
}

// way points in global memory with the quantised prefilter record of private paths (PathDesc::pre, 8 bytes: x, y as uint16
// steps from the corner of the path's box, cos / sin of the heading as int16 / 32767; path_trig_kernel): eight candidates per
// trip cost eight 8-byte loads out of one or two 64-byte sectors (float32 records of 16 bytes until round 4: four per trip
// out of the same sectors; float64 before that: twenty 8-byte loads out of three per four candidates), and float32
// arithmetic; only a candidate the prefilter cannot rule out fetches its float64 record for the exact test.
// The prefilter works in steps: xr = (x - corner) / step is below 2^17 in magnitude for every pose whose window is not empty
// (the box test of path_window, step >= sp_prune / kQuantReach), so xr as a float32 is good to 2^-8 step and qx - xr to as much again;
// the reciprocal of the step as float32 adds 6e-8 * 2^17 < 0.01 step, the way point's own rounding 0.5: each coordinate
// difference is within 0.52 step of the true one, the distance within 0.74 -- the position limits carry +1.  "Not behind the
// way point" (path_tools.py:405): cos and sin are off by 1.53e-5 each, times a difference of at most kQuantReach + 1 steps =
// 0.25 step per term, plus 0.52 (|cos| + |sin|) <= 0.74 for the differences and ~0.002 of float32 rounding: below 1.3 -- the
// limit carries -2.  The heading (path_tools.py:419, |normalize(th - th_j)| < ap  <=>  cos(th - th_j) > cos ap for ap < pi): the
// cosine of the difference from the record's cos / sin and float32 cos / sin of the pose's heading is within 2.5e-5 of the true
// one -- its limit, DevParams::ap_cos_min, carries -1e-4.  (Without it a pose that is near a way point but turned away from it
// went through the exact test of every such way point, one memory round trip each: the waves that scan the part of the window
// next to the target took 9 k cycles longer than the others on C4.)
// The pose's heading is rounded to float32 before its cos / sin are taken.  For |th| < 32 rad that is half an ulp = 1e-6 and the
// 2.5e-5 above stands (2.16e-5 from the record's cos / sin, the rest float32 rounding).  A heading is only normalised by a
// step that moves the robot: one written into the state (set_state, state.robot[2], path[0] after a reset) arrives here as it is
// when that step collides and rolls the pose back.  Up to |th| < 2048 rad half an ulp is 6.1e-5, the cosine is within 8.3e-5
// and the -1e-4 of ap_cos_min still covers it; from 2048 rad on it does not.  No such heading gets here unflagged: a step from th
// is free of BCP_ERR_ANGLE_JUMP only if |w| dt >= |th| - 3 pi (path_velocity corrects the difference to the normalised new
// heading by one turn), i.e. for a robot that turns by more than 2000 rad in one step; every other one carries the error word,
// which says that the reference raised there.  tests/headings.py keeps robot headings within 51 turns (320 rad).
// So whatever the prefilter rejects fails the float64 test too: the result is the exact scan's, bit for bit.
#ifndef BCP_PREFILTER_TRIP
#define BCP_PREFILTER_TRIP 8
#endif
__device__ __forceinline__ int last_reached_prefiltered(const DevParams& P, const double* __restrict__ path,
                                                        const uint32_t* __restrict__ pre, PathWindow w, int m, int target,
                                                        double x, double y, double th, double ox, double oy, float inv_step)
{
    if (target > m - 1) return -1;
    const int lo = max(w.lo, target);
    const int hi = min(w.hi, m - 1);
    const double inv = (double)inv_step;
    const float xr = (float)((x - ox) * inv), yr = (float)((y - oy) * inv);
    const float lim = (float)(P.sp * inv) + 1.0f, par_min = (float)(P.par_thr * inv) - 2.0f;
    const float q_max = lim * lim * 1.000001f;
    float sin_th, cos_th;
    sincosf((float)th, &sin_th, &cos_th);
    const float cos_min = P.ap_cos_min * 32767.0f;
    constexpr int TRIP = BCP_PREFILTER_TRIP;
    for (int j = hi; j >= lo; j -= TRIP) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        u32x2 p[TRIP];
#pragma unroll
        for (int u = 0; u < TRIP; ++u) p[u] = as_global(reinterpret_cast<const u32x2*>(pre))[max(j - u, lo)];   // (below lo: a repeat of lo)
        // the candidates the prefilter lets through, as a bit mask (straight-line code), then the exact test from the top
        uint32_t maybe = 0;
#pragma unroll
        for (int u = 0; u < TRIP; ++u) {
            const float dx = (float)(p[u].x & 0xFFFFu) - xr, dy = (float)(p[u].x >> 16) - yr;
            const float qc = (float)(int16_t)(p[u].y & 0xFFFFu), qs = (float)((int32_t)p[u].y >> 16);
            const float par = -(qc * dx + qs * dy) * (1.0f / 32767.0f);
            const bool out = fabsf(dx) > lim || fabsf(dy) > lim || dx * dx + dy * dy > q_max || par < par_min ||
                             qc * cos_th + qs * sin_th < cos_min || j - u < lo;
            maybe |= (uint32_t)!out << u;
        }
        while (maybe) {
            const int u = (int)__builtin_ctz(maybe);
            maybe &= maybe - 1;
            const double* s = path + 5 * (j - u);
            if (way_point_reached(P, s[0], s[1], s[2], s[3], s[4], x, y, th)) return j - u;
        }
    }
    return -1;
}

template <int TRIP = 4, typename PathPtr>
__device__ __forceinline__ double reward_step(const DevParams& P, PathPtr path, PathWindow w, int m, double x, double y,
                                              double th, double& min_dist, int& target)
{
    if (target > m - 1) return 0.0;
    int last;
    if constexpr (std::is_same<PathPtr, const double*>::value) last = last_reached_from<TRIP>(P, path, w, m, target, x, y, th);
    else last = last_reached_from(P, path, w, m, target, x, y, th);
    if (last >= 0) {
        target = last + 1;
        if (!(target > m - 1)) {
            const PathPtr g = path + 5 * target;
            min_dist = hypot(g[0] - x, g[1] - y);
        } else {
            min_dist = 0.0;
        }
        return 1.0;
    }
    const PathPtr g = path + 5 * target;
    const double d = hypot(g[0] - x, g[1] - y);
    if (d < min_dist) {
        const double r = min_dist - d;
        min_dist = d;
        return r * P.progress_mult;
    }
    return 0.0;
}

// reward_step with the scan already done (`last` = last_reached_from's result for this pose and target): the rest of
// ContinuousRewardProvider.reward (envs/base/reward.py:234-259)
template <typename PathPtr>
__device__ __forceinline__ double reward_from_last(const DevParams& P, PathPtr path, int m, int last, double x, double y,
                                                   double& min_dist, int& target)
{
    if (target > m - 1) return 0.0;
    if (last >= 0) {
        target = last + 1;
        if (!(target > m - 1)) {
            const PathPtr g = path + 5 * target;
            min_dist = hypot(g[0] - x, g[1] - y);
        } else {
            min_dist = 0.0;
        }
        return 1.0;
    }
    const PathPtr g = path + 5 * target;
    const double d = hypot(g[0] - x, g[1] - y);
    if (d < min_dist) {
        const double r = min_dist - d;
        min_dist = d;
        return r * P.progress_mult;
    }
    return 0.0;
}

// ContinuousRewardPurePursuitProvider.reward (envs/base/reward.py:330-353) with update_goal (:125-139): the target is
// the first way point from target_idx on that is more than 2 m away (np.linalg.norm = sqrt of an fma-contracted
// 2-term dot product, like every 2-element np.dot in this code base), the goal is always the LAST way point.
template <typename PathPtr>
__device__ __forceinline__ double reward_pure_pursuit(PathPtr path, int m, double x, double y, bool collided,
                                                      double& min_dist, int& target)
{
    int found = m - 1;
    for (int i = target; i < m; ++i) {
        const double dx = path[5 * i] - x, dy = path[5 * i + 1] - y;
        if (sqrt(fma(dy, dy, dx * dx)) > 2.) {
            found = i;
            break;
        }
    }
    target = found;
    const PathPtr g = path + 5 * (m - 1);
    const double dist = hypot(g[0] - x, g[1] - y);
    double reward = -0.05;
    reward += min_dist - dist;
    min_dist = dist;
    if (collided) reward -= 100;
    return reward;
}

// _get_element_from_list_with_delay (envs/base/env.py:27-49) for the k-th push since the last reset: queue q is
// [delay][W][n]; element k lives in slot (k - 1) % delay.  `v` holds the new element on entry, the delayed one on exit.
template <int W>
__device__ __forceinline__ void fifo_delay(double* __restrict__ q, int delay, int64_t n, int64_t i, int k, double (&v)[W])
{
    if (delay <= 0) return;
    const int slot = (k - 1) % delay;
    double* cell = q + ((int64_t)slot * W) * n + i;
    if (k <= delay) {   // the list is not longer than `delay` yet: append, hand back the first element
#pragma unroll
        for (int c = 0; c < W; ++c) cell[c * n] = v[c];
        if (k > 1) {
#pragma unroll
            for (int c = 0; c < W; ++c) v[c] = q[c * n + i];
        }
    } else {            // pop(0): element k - delay, whose slot the new element takes
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const double first = cell[c * n];
            cell[c * n] = v[c];
            v[c] = first;
        }
    }
}

// The same in two halves: fifo_peek() reads, before anything is pushed, the element the k-th push will hand back --
// for k > delay the one it displaces, for 1 < k <= delay the list's first element (slot 0) -- and fifo_push() stores
// the new element and returns the peeked one (the new element itself for k = 1).  So what State exposes at a step
// (k > 1) is known before the robot model runs, and pushing twice (kernel 1 optimistically, kernel 2 again with the
// rolled-back pose after a collision) lands in the same slot and hands back the same element.
template <int W>
__device__ __forceinline__ void fifo_peek(const double* __restrict__ q, int delay, int64_t n, int64_t i, int k, double (&peeked)[W])
{
    if (delay <= 0 || k <= 1) return;
    const double* cell = q + ((int64_t)(k > delay ? (k - 1) % delay : 0) * W) * n + i;
#pragma unroll
    for (int c = 0; c < W; ++c) peeked[c] = cell[c * n];
}

template <int W>
__device__ __forceinline__ void fifo_push(double* __restrict__ q, int delay, int64_t n, int64_t i, int k, double (&v)[W],
                                          const double (&peeked)[W])
{
    if (delay <= 0) return;
    double* cell = q + ((int64_t)((k - 1) % delay) * W) * n + i;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        cell[c * n] = v[c];
        if (k > 1) v[c] = peeked[c];
    }
}

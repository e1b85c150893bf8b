// bcp_boxes_cell.h -- the box sampler's rule (bcp_scatter_boxes; include/bcplan.h): the argument checks, the draws of one
// attempt, its candidate box, the pixel runs of a four-vertex contour as cv2.fillPoly writes them, the verdict on a
// candidate, and one whole entry written out in attempt order.  Plain C++ with no HIP in it: scatter_boxes_kernel
// (bcp_boxes.h) calls these functions on the device, tests/c_abi/scatter_boxes_main.cpp calls the same ones on the host, and
// there is no other copy of them.  Everything is float64 + - *, rint and integers, each operation rounded on its own
// (-ffp-contract=off): tests/scatter_boxes_ref.py restates it in numpy and agrees bit for bit.
//
// The accepted boxes of an entry are the first n_boxes attempts of 0 .. max_attempts - 1, in attempt order, that are not
// rejected; a verdict depends on its attempt alone, so the order of evaluation does not matter.
#pragma once

#include <cstdint>

#include "bcp_outline.h"
#include "bcp_philox.h"

#ifndef BCP_HD
#if defined(__HIPCC__)
#define BCP_HD __host__ __device__
#else
#define BCP_HD
#endif
#endif

namespace bcp {

constexpr int32_t kBoxMaxBoxes = 64;
constexpr int32_t kBoxMaxAttempts = 4096;
constexpr int32_t kBoxMaxYaws = 4096;
constexpr int32_t kBoxMaxKeep = 16;
constexpr int32_t kBoxMaxSide = 2048;
constexpr int32_t kBoxChunk = 256;    // attempts judged at once: the workgroup's threads
constexpr int32_t kBoxWords = 9;      // a box on the way out: its attempt, then (x, y) of its four vertices
constexpr uint8_t kBoxLethal = 254;

// what a caller chooses (bcp_scatter_params, without the ABI's layout)
struct BoxRule {
    int32_t n_boxes, max_attempts, n_yaws;
    uint32_t seed_lo, seed_hi;
    double t_lo, t_hi, h_lo, h_hi;
};

// what bcp_scatter_boxes refuses with BCP_E_INVALID, in the order it looks
enum ScatterRefusal {
    kScatterOk = 0, kScatterHandle = 1, kScatterParams = 2, kScatterMaps = 3, kScatterShape = 4, kScatterResolution = 5,
    kScatterBoxes = 6, kScatterAttempts = 7, kScatterYaws = 8, kScatterKeep = 9, kScatterAlong = 10, kScatterHalf = 11,
    kScatterHalfFits = 12, kScatterValidPair = 13, kScatterPointers = 14
};

BCP_HD inline bool box_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

// have_arrays: data, origins, frame, yaw_cs, boxes and counts are all there.  The largest box must fit the map at any yaw:
// no corner lies farther than 2 h_hi from the centre along either axis, whatever the table holds up to a unit vector.
BCP_HD inline int scatter_check_args(bool have_handle, bool have_params, int64_t n_maps, int32_t rows, int32_t cols,
                                     double resolution, int32_t n_boxes, int32_t max_attempts, int32_t n_yaws, int32_t n_keep,
                                     double t_lo, double t_hi, double h_lo, double h_hi, bool have_valid_rows,
                                     bool have_valid_cols, bool have_arrays, bool have_keep)
{
    if (!have_handle) return kScatterHandle;
    if (!have_params) return kScatterParams;
    if (n_maps < 0) return kScatterMaps;
    if (rows < 1 || rows > kBoxMaxSide || cols < 1 || cols > kBoxMaxSide) return kScatterShape;
    if (!(resolution > 0.0) || !box_finite(resolution)) return kScatterResolution;
    if (n_boxes < 1 || n_boxes > kBoxMaxBoxes) return kScatterBoxes;
    if (max_attempts < 1 || max_attempts > kBoxMaxAttempts) return kScatterAttempts;
    if (n_yaws < 1 || n_yaws > kBoxMaxYaws) return kScatterYaws;
    if (n_keep < 0 || n_keep > kBoxMaxKeep) return kScatterKeep;
    if (!box_finite(t_lo) || !box_finite(t_hi) || !(t_lo <= t_hi)) return kScatterAlong;
    if (!box_finite(h_hi) || !(h_lo >= 0.0) || !(h_lo <= h_hi)) return kScatterHalf;
    if (!((4.0 * h_hi) * (1.0 / resolution) + 2.0 <= (double)(rows < cols ? rows : cols))) return kScatterHalfFits;
    if (have_valid_rows != have_valid_cols) return kScatterValidPair;
    if (n_maps > 0 && (!have_arrays || (n_keep > 0 && !have_keep))) return kScatterPointers;
    return kScatterOk;
}

BCP_HD inline double box_uniform(uint32_t w) { return ((double)w + 0.5) * 2.3283064365386963e-10; }   // 2^-32: in (0, 1)

// The candidate of attempt `a` on entry `m`: its four integer vertices V = (x0, y0, .. x3, y3), x a column and y a row, for
// the corner signs (+,+), (-,+), (-,-), (+,-).  frame = (ax, ay, dx, dy, nx, ny) of the entry, yaw_cs the caller's table
// [n_yaws][2] of (cos, sin), (ox, oy) the entry's origin, (vr, vc) its valid shape.  false -- V is then not to be read --
// when a vertex lies outside [0, vc) x [0, vr): the test is made on the rounded float64, before anything is converted, so
// 1e300 and NaN are merely "outside".
BCP_HD inline bool box_candidate(const BoxRule& R, uint64_t m, int32_t a, const double* frame, const double* yaw_cs, double ox,
                                 double oy, double inv_res, int32_t vr, int32_t vc, int32_t V[8])
{
    uint32_t w[4] = {(uint32_t)m, (uint32_t)(m >> 32), (uint32_t)a, 0u};
    philox4x32_10(w, R.seed_lo, R.seed_hi);
    uint32_t v[4] = {(uint32_t)m, (uint32_t)(m >> 32), (uint32_t)a, 1u};
    philox4x32_10(v, R.seed_lo, R.seed_hi);
    const double t = R.t_lo + box_uniform(w[0]) * (R.t_hi - R.t_lo);
    const double l = 2.0 * box_uniform(w[1]) - 1.0;
    const double hx = R.h_lo + box_uniform(w[2]) * (R.h_hi - R.h_lo);
    const double hy = R.h_lo + box_uniform(w[3]) * (R.h_hi - R.h_lo);
    const uint32_t k = (uint32_t)(((uint64_t)v[0] * (uint64_t)(uint32_t)R.n_yaws) >> 32);
    const double c = yaw_cs[2 * k], s = yaw_cs[2 * k + 1];
    const double cx = (frame[0] + t * frame[2]) + l * frame[4];
    const double cy = (frame[1] + t * frame[3]) + l * frame[5];
    bool inside = true;
    for (int q = 0; q < 4; ++q) {
        const double ex = (q == 0 || q == 3) ? hx : -hx, ey = q < 2 ? hy : -hy;
        const double wx = (cx + ex * c) - ey * s;
        const double wy = (cy + ex * s) + ey * c;
        const double px = __builtin_rint((wx - ox) * inv_res), py = __builtin_rint((wy - oy) * inv_res);   // half to even
        const bool in = px >= 0.0 && px < (double)vc && py >= 0.0 && py < (double)vr;
        V[2 * q] = in ? (int32_t)px : 0;
        V[2 * q + 1] = in ? (int32_t)py : 0;
        inside = inside && in;
    }
    return inside;
}

// ---- the pixel set of the contour V, as runs: sink.pixel(row, col) / sink.span(row, col_a, col_b) -> bool, true to stop.
// Runs may overlap; their union is exactly what cv2.fillPoly(img, [V], .) writes: the four edges by the LineIterator
// (bcp_outline.h), and per row the even-odd spans of the 16.16 crossings.  Nothing is assumed of V but coordinates within
// [0, kBoxMaxSide): no convexity (a row has up to four crossings), and vertices may coincide.

// edge k joins V[k - 1] and V[k], as CollectPolyEdges walks them
template <typename Sink>
BCP_HD inline bool box_outline(const int32_t V[8], int k, Sink& sink)
{
    const int j = (k + 3) & 3;
    return outline_edge(V[2 * j], V[2 * j + 1], V[2 * k], V[2 * k + 1], sink);
}

BCP_HD inline void box_rows(const int32_t V[8], int32_t& ymin, int32_t& ymax)
{
    ymin = ymax = V[1];
    for (int q = 1; q < 4; ++q) {
        ymin = V[2 * q + 1] < ymin ? V[2 * q + 1] : ymin;
        ymax = V[2 * q + 1] > ymax ? V[2 * q + 1] : ymax;
    }
}

// The spans of row y, ymin <= y < ymax: an edge is active on y0 <= y < y1, its crossing is (x of its upper end << 16) +
// (y - y0) * ((DX << 16) / DY) with C's truncation -- a multiple of the slope, so rows are independent -- and the x-sorted
// crossings are filled in pairs on [ceil(xa), floor(xb)].  (|(y - y0) * slope| <= |DX| << 16: nothing overflows.)
template <typename Sink>
BCP_HD inline bool box_span_row(const int32_t V[8], int32_t y, Sink& sink)
{
    int32_t xs[4];
    int n = 0;
    for (int k = 0; k < 4; ++k) {
        const int j = (k + 3) & 3;
        const int32_t x0 = V[2 * j], y0 = V[2 * j + 1], x1 = V[2 * k], y1 = V[2 * k + 1];
        if (y0 == y1) continue;
        const int32_t ey0 = y0 < y1 ? y0 : y1, ey1 = y0 < y1 ? y1 : y0;
        if (y < ey0 || y >= ey1) continue;
        const int32_t slope = ((x1 - x0) * 65536) / (y1 - y0);
        const int32_t xe = (y0 < y1 ? x0 : x1) * 65536 + (y - ey0) * slope;
        int i = n++;
        for (; i > 0 && xs[i - 1] > xe; --i) xs[i] = xs[i - 1];
        xs[i] = xe;
    }
    for (int i = 0; i + 1 < n; i += 2) {
        const int32_t a = (xs[i] + 65535) >> 16, b = xs[i + 1] >> 16;
        if (a <= b && sink.span(y, a, b)) return true;
    }
    return false;
}

template <typename Sink>
BCP_HD inline bool box_runs(const int32_t V[8], Sink& sink)
{
    for (int k = 0; k < 4; ++k)
        if (box_outline(V, k, sink)) return true;
    int32_t ymin, ymax;
    box_rows(V, ymin, ymax);
    for (int32_t y = ymin; y < ymax; ++y)
        if (box_span_row(V, y, sink)) return true;
    return false;
}

// Stops at the first run with a cell (r, c) for which (r - kr)^2 + (c - kc)^2 <= d2 for a keep-out (kr, kc, d2) of
// keep [n_keep][3]; d2 < 0 is an unused slot.  The nearest cell of a run to a keep-out is a clamp.
struct BoxKeepSink {
    const int32_t* keep;
    int32_t n_keep;
    BCP_HD bool span(int32_t r, int32_t ca, int32_t cb) const
    {
        for (int32_t i = 0; i < n_keep; ++i) {
            const int64_t kr = keep[3 * i], kc = keep[3 * i + 1], d2 = keep[3 * i + 2];
            if (d2 < 0) continue;
            const int64_t c = kc < ca ? ca : (kc > cb ? cb : kc);
            if ((r - kr) * (r - kr) + (c - kc) * (c - kc) <= d2) return true;
        }
        return false;
    }
    BCP_HD bool pixel(int32_t r, int32_t c) const { return span(r, c, c); }
};

// the verdict on attempt `a`: true = accepted, V its vertices
BCP_HD inline bool box_accepted(const BoxRule& R, uint64_t m, int32_t a, const double* frame, const double* yaw_cs, double ox,
                                double oy, double inv_res, int32_t vr, int32_t vc, const int32_t* keep, int32_t n_keep,
                                int32_t V[8])
{
    if (!box_candidate(R, m, a, frame, yaw_cs, ox, oy, inv_res, vr, vc, V)) return false;
    BoxKeepSink sink = {keep, n_keep};
    return !box_runs(V, sink);
}

BCP_HD inline int32_t box_clamp_valid(int32_t v, int32_t side) { return v < 0 ? 0 : (v > side ? side : v); }

// One entry in attempt order: its accepted boxes into boxes [n_boxes][kBoxWords] (zeros behind the count) and, through
// `fill` (a sink as above), every cell of theirs.  Returns the count.  What the kernel computes with a workgroup.
template <typename Fill>
BCP_HD inline int32_t scatter_entry(const BoxRule& R, uint64_t m, const double* frame, const double* yaw_cs, double ox, double oy,
                                    double inv_res, int32_t vr, int32_t vc, const int32_t* keep, int32_t n_keep, Fill& fill,
                                    int32_t* boxes)
{
    int32_t count = 0;
    for (int32_t a = 0; a < R.max_attempts && count < R.n_boxes; ++a) {
        int32_t V[8];
        if (!box_accepted(R, m, a, frame, yaw_cs, ox, oy, inv_res, vr, vc, keep, n_keep, V)) continue;
        boxes[kBoxWords * count] = a;
        for (int q = 0; q < 8; ++q) boxes[kBoxWords * count + 1 + q] = V[q];
        ++count;
        (void)box_runs(V, fill);
    }
    for (int32_t j = kBoxWords * count; j < kBoxWords * R.n_boxes; ++j) boxes[j] = 0;
    return count;
}

}  // namespace bcp

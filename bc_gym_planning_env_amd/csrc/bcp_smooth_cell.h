// bcp_smooth_cell.h -- the arithmetic of bcp_smooth_route (include/bcplan.h): the argument checks, the exact line-of-sight
// test between two cells (smooth_clear), the pull of a cell chain taut (smooth_pull_next), the blend of one corner
// (smooth_blend_level, smooth_corner), the pieces a smoothed path is written from (smooth_piece, smooth_piece_point), and
// the row as a sequential program (smooth_row).  Plain C++ with no HIP in it.  Who calls this, on the device: smooth_kernel
// (bcp_smooth.h), which spreads smooth_row's loops over a wave and calls the same functions per candidate, corner and piece.
// On the host, under sanitizers and through bounds-checked accessors: tests/c_abi/smooth_route_main.cpp calls smooth_row and
// smooth_clear, and there is no other copy of them.  The float64 arithmetic rounds every product, quotient, root and sum on
// its own (-ffp-contract=off); it uses + - * /, the square root, ceil and rint, and nothing else ahead of the headings.
#pragma once

#include <cmath>
#include <cstdint>

#include "bcp_goal_cell.h"   // goal_seed_of_path: a way point's cell; the status bits of a route; path_initial_reward

namespace bcp {

constexpr int32_t kSmoothMaxLen = 4096;      // way points of a row, in and out
constexpr int32_t kSmoothMaxLook = 4096;
constexpr int32_t kSmoothMaxHalvings = 8;
constexpr int32_t kSmoothBlocked = 16;       // beside kGoalRouteLong / TooClose / NoRoute
constexpr int32_t kSmoothSharp = 15;         // the level of a corner that is not blended
constexpr int32_t kSmoothTooMany = kSmoothMaxLen + 1;   // a piece count that no row can hold

struct SmoothParams {   // bcp_smooth_params, field for field
    int32_t look, halvings;
    double blend, delta;
};

// what bcp_smooth_route refuses, in the order it looks: 1 .. 12 with BCP_E_INVALID, 13 .. 16 with BCP_E_STATE.  n_entries:
// the entries of the binding, 0 while no costmaps are bound (the comparisons with the binding are then skipped and the call
// ends in kSmoothUnbound).  overlap: `paths` or `lens` shares a byte with `paths_in` or `lens_in` (smooth_overlap);
// bound_arrays: `paths` or `lens` is an array given to bcp_set_paths.
enum SmoothRefusal {
    kSmoothOk = 0, kSmoothNull = 1, kSmoothLook = 2, kSmoothHalvings = 3, kSmoothBlend = 4, kSmoothDelta = 5,
    kSmoothMaxLenIn = 6, kSmoothMaxLenOut = 7, kSmoothRows = 8, kSmoothRowEnv = 9, kSmoothShape = 10, kSmoothFields = 11,
    kSmoothEntries = 12, kSmoothUnbound = 13, kSmoothShared = 14, kSmoothOverlap = 15, kSmoothBoundArrays = 16
};

BCP_HD inline bool smooth_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    return a < b + b_bytes && b < a + a_bytes;
}

BCP_HD inline int smooth_check_args(bool have_pointers, bool have_params, int32_t look, int32_t halvings, double blend,
                                    double delta, int32_t max_len_in, int32_t max_len, int64_t n, bool have_row_env,
                                    bool rows_are_entries, int32_t rows, int32_t cols, int32_t map_rows, int32_t map_cols,
                                    int64_t n_fields, int64_t n_entries, bool shared_map, bool overlap, bool bound_arrays)
{
    const double lim = 1.7976931348623157e308;
    if (!have_pointers || !have_params) return kSmoothNull;
    if (look < 1 || look > kSmoothMaxLook) return kSmoothLook;
    if (halvings < 0 || halvings > kSmoothMaxHalvings) return kSmoothHalvings;
    if (!(blend >= 0.0 && blend <= lim)) return kSmoothBlend;     // (a NaN fails the comparison)
    if (!(delta > 0.0 && delta <= lim)) return kSmoothDelta;
    if (max_len_in < 2 || max_len_in > kSmoothMaxLen) return kSmoothMaxLenIn;
    if (max_len < 2 || max_len > kSmoothMaxLen) return kSmoothMaxLenOut;
    if (n <= 0) return kSmoothRows;
    if (rows_are_entries && have_row_env) return kSmoothRowEnv;
    if (n_entries > 0 && (rows != map_rows || cols != map_cols)) return kSmoothShape;
    if (n_entries > 0 && n_fields != n_entries && (rows_are_entries || n_fields != 1)) return kSmoothFields;
    if (n_entries > 0 && rows_are_entries && n != n_entries) return kSmoothEntries;
    if (n_entries <= 0) return kSmoothUnbound;
    if (rows_are_entries && shared_map) return kSmoothShared;
    if (overlap) return kSmoothOverlap;
    if (bound_arrays) return kSmoothBoundArrays;
    return kSmoothOk;
}

// The entry a row stands on, as far as the arithmetic needs it, and `passable`: inside the valid shape with a value.
template <typename Get>
struct SmoothMap {
    Get get;            // get(row, col) of the field, only ever called inside the valid shape
    int32_t vr, vc;
    double ox, oy, inv_res;
    BCP_HD bool passable(int32_t r, int32_t c) const
    {
        return (uint32_t)r < (uint32_t)vr && (uint32_t)c < (uint32_t)vc && (int32_t)get(r, c) != kGoalNone;
    }
    // the cell of a point by goal_value_at's rule; false: it has none
    BCP_HD bool cell_of(double x, double y, int32_t& r, int32_t& c) const { return goal_seed_of_path(x, y, ox, oy, inv_res, vr, vc, r, c); }
};

// clear(a, b) between the centres of cells a = (r0, c0) and b = (r1, c1); a negative row: the end has no cell.  Exact in
// integers: the products stay below 2^24 for maps up to 2048 x 2048.  At most |dc| + |dr| trips.
template <typename Map>
BCP_HD inline bool smooth_clear(const Map& map, int32_t r0, int32_t c0, int32_t r1, int32_t c1)
{
    if (r0 < 0 || r1 < 0) return false;
    if (!map.passable(r0, c0)) return false;
    const int32_t dc = c1 - c0, dr = r1 - r0;
    const int32_t ax = dc < 0 ? -dc : dc, ay = dr < 0 ? -dr : dr, sx = dc < 0 ? -1 : 1, sy = dr < 0 ? -1 : 1;
    int32_t i = 0, j = 0, r = r0, c = c0;
    while (i < ax || j < ay) {
        int32_t side = 0;   // < 0: the column, > 0: the row, 0: through the corner
        if (j == ay) side = -1;
        else if (i == ax) side = 1;
        else side = (2 * i + 1) * ay - (2 * j + 1) * ax;
        if (side == 0 && (!map.passable(r, c + sx) || !map.passable(r + sy, c))) return false;
        if (side <= 0) {
            c += sx;
            ++i;
        }
        if (side >= 0) {
            r += sy;
            ++j;
        }
        if (!map.passable(r, c)) return false;
    }
    return true;
}

// The pull's test of one candidate: way points k < j of a row whose cells cell(k, r, c) gives (false: no cell).
template <typename Map, typename Cell>
BCP_HD inline bool smooth_sees(const Map& map, const Cell& cell, int32_t k, int32_t j)
{
    int32_t r0 = -1, c0 = -1, r1 = -1, c1 = -1;
    if (!cell(k, r0, c0) || !cell(j, r1, c1)) return false;
    return smooth_clear(map, r0, c0, r1, c1);
}

// The anchor behind k among m way points: the largest j in (k, min(k + look, m - 1)] that k sees, or -1.
template <typename Map, typename Cell>
BCP_HD inline int32_t smooth_pull_next(const Map& map, const Cell& cell, int32_t k, int32_t m, int32_t look)
{
    const int32_t hi = k + look < m - 1 ? k + look : m - 1;
    for (int32_t j = hi; j > k; --j)
        if (smooth_sees(map, cell, k, j)) return j;
    return -1;
}

// ceil(len / step) as a piece count: at least 1 (a NaN too), and kSmoothTooMany for everything above kSmoothMaxLen
BCP_HD inline int32_t smooth_pieces(double len, double step)
{
    const double c = __builtin_ceil(len / step);
    if (!(c >= 1.0)) return 1;
    return c > (double)kSmoothMaxLen ? kSmoothTooMany : (int32_t)c;
}

struct SmoothCorner {
    double a[2], v[2], b[2];   // A, V, B
    int32_t q;                 // pieces of the blend, 0: sharp
};

// The corner at V between P and N for a blend length that has been halved `level` times: A, B and q.  A sharp corner
// (level == kSmoothSharp) has A = B = V and q = 0.
BCP_HD inline void smooth_legs(const double p[2], const double v[2], const double n[2], double& lp, double& ln)
{
    const double px = p[0] - v[0], py = p[1] - v[1], nx = n[0] - v[0], ny = n[1] - v[1];
    lp = __builtin_sqrt(px * px + py * py);
    ln = __builtin_sqrt(nx * nx + ny * ny);
}

BCP_HD inline double smooth_full_size(double blend, double lp, double ln)
{
    double d = blend;
    if (lp / 3.0 < d) d = lp / 3.0;
    if (ln / 3.0 < d) d = ln / 3.0;
    return d;
}

BCP_HD inline SmoothCorner smooth_corner_of_size(const double p[2], const double v[2], const double n[2], double lp, double ln,
                                                 double d, double delta)
{
    SmoothCorner k;
    const double fp = d / lp, fn = d / ln;
    for (int e = 0; e < 2; ++e) {
        k.v[e] = v[e];
        k.a[e] = v[e] + (p[e] - v[e]) * fp;
        k.b[e] = v[e] + (n[e] - v[e]) * fn;
    }
    k.q = smooth_pieces(2.0 * d, delta);
    return k;
}

BCP_HD inline SmoothCorner smooth_corner(const double p[2], const double v[2], const double n[2], double blend, double delta,
                                         int32_t level)
{
    if (level == kSmoothSharp) {
        SmoothCorner k;
        for (int e = 0; e < 2; ++e) k.a[e] = k.v[e] = k.b[e] = v[e];
        k.q = 0;
        return k;
    }
    double lp, ln;
    smooth_legs(p, v, n, lp, ln);
    double d = smooth_full_size(blend, lp, ln);
    for (int32_t h = 0; h < level; ++h) d = d / 2.0;
    return smooth_corner_of_size(p, v, n, lp, ln, d, delta);
}

// Q_k of a corner, k = 0 .. q: ((A * ((1-t)*(1-t))) + (V * ((2*t)*(1-t)))) + (B * (t*t)), t = (double)k / (double)q
BCP_HD inline void smooth_blend_point(const SmoothCorner& k, int32_t i, double xy[2])
{
    const double t = (double)i / (double)k.q, u = 1.0 - t;
    const double wa = u * u, wv = (2.0 * t) * u, wb = t * t;
    for (int e = 0; e < 2; ++e) xy[e] = ((k.a[e] * wa) + (k.v[e] * wv)) + (k.b[e] * wb);
}

// The blend of the corner at V: the number of halvings at which it is accepted (0: at full size), or kSmoothSharp.  A size
// with more than kSmoothMaxLen pieces is refused untested: no row could hold it.  At most 9 sizes of at most 4097 points.
template <typename Map>
BCP_HD inline int32_t smooth_blend_level(const Map& map, const double p[2], const double v[2], const double n[2], double blend,
                                         double delta, int32_t halvings)
{
    double lp, ln;
    smooth_legs(p, v, n, lp, ln);
    if (!(blend > 0.0) || lp == 0.0 || ln == 0.0) return kSmoothSharp;
    double d = smooth_full_size(blend, lp, ln);
    for (int32_t level = 0; level <= halvings; ++level, d = d / 2.0) {
        const SmoothCorner k = smooth_corner_of_size(p, v, n, lp, ln, d, delta);
        if (k.q == kSmoothTooMany) continue;
        double xy[2];
        int32_t r0 = -1, c0 = -1;
        smooth_blend_point(k, 0, xy);
        bool ok = map.cell_of(xy[0], xy[1], r0, c0);
        for (int32_t i = 1; ok && i <= k.q; ++i) {
            int32_t r1 = -1, c1 = -1;
            smooth_blend_point(k, i, xy);
            ok = map.cell_of(xy[0], xy[1], r1, c1) && smooth_clear(map, r0, c0, r1, c1);
            r0 = r1;
            c0 = c1;
        }
        if (ok) return level;
    }
    return kSmoothSharp;
}

// ---- the pieces of a row ----------------------------------------------------------------------------------------------
// A row with vertices V_0 .. V_M (M >= 1) is written as way point 0 = V_0 and then the points of pieces 0 .. 2 M - 2 in
// order: piece 2 s is the straight stretch from corner s's B (V_0 for s = 0) to corner s + 1's A (V_M for s = M - 1), piece
// 2 s + 1 the blend of corner s + 1, whose points Q_1 .. Q_q follow that A (none for a sharp corner).  in(k, e): coordinate
// e of input way point k; vertex(t): anchor index | level << 12 of vertex t.
struct SmoothPiece {
    SmoothCorner k;     // a blend: the corner
    double s[2], e[2];  // a stretch: its ends
    int32_t count;      // the points it writes
    int32_t blend;      // 1: a blend
};

template <typename In, typename Vertex>
BCP_HD inline SmoothCorner smooth_corner_at(const In& in, const Vertex& vertex, int32_t t, double blend, double delta)
{
    const int32_t w = (int32_t)vertex(t), kp = (int32_t)vertex(t - 1) & 4095, kn = (int32_t)vertex(t + 1) & 4095, kv = w & 4095;
    const double p[2] = {in(kp, 0), in(kp, 1)}, v[2] = {in(kv, 0), in(kv, 1)}, n[2] = {in(kn, 0), in(kn, 1)};
    return smooth_corner(p, v, n, blend, delta, w >> 12);
}

template <typename In, typename Vertex>
BCP_HD inline SmoothPiece smooth_piece(const In& in, const Vertex& vertex, int32_t M, int32_t piece, double blend, double delta)
{
    SmoothPiece o;
    const int32_t s = piece >> 1;
    o.blend = piece & 1;
    if (o.blend) {
        o.k = smooth_corner_at(in, vertex, s + 1, blend, delta);
        for (int e = 0; e < 2; ++e) o.s[e] = o.e[e] = 0.0;
        o.count = o.k.q;
        return o;
    }
    for (int e = 0; e < 2; ++e) {
        o.s[e] = in((int32_t)vertex(s) & 4095, e);
        o.e[e] = in((int32_t)vertex(s + 1) & 4095, e);
        o.k.a[e] = o.k.v[e] = o.k.b[e] = 0.0;
    }
    o.k.q = 0;
    if (s > 0) {
        const SmoothCorner k = smooth_corner_at(in, vertex, s, blend, delta);
        o.s[0] = k.b[0];
        o.s[1] = k.b[1];
    }
    if (s + 1 < M) {
        const SmoothCorner k = smooth_corner_at(in, vertex, s + 1, blend, delta);
        o.e[0] = k.a[0];
        o.e[1] = k.a[1];
    }
    const double dx = o.e[0] - o.s[0], dy = o.e[1] - o.s[1];
    o.count = smooth_pieces(__builtin_sqrt(dx * dx + dy * dy), delta);
    return o;
}

// point i = 1 .. count of a piece; a stretch's last point is E itself
BCP_HD inline void smooth_piece_point(const SmoothPiece& o, int32_t i, double xy[2])
{
    if (o.blend) {
        smooth_blend_point(o.k, i, xy);
    } else if (i == o.count) {
        xy[0] = o.e[0];
        xy[1] = o.e[1];
    } else {
        const double t = (double)i / (double)o.count;
        for (int e = 0; e < 2; ++e) xy[e] = o.s[e] + (o.e[e] - o.s[e]) * t;
    }
}

// the heading of way point j of wp[0 .. len), 0 < j < len - 1: bcp_goal_route's rule
BCP_HD inline double smooth_heading(const double* wp, int32_t j, double goal_heading)
{
    const double dx = wp[3 * (j + 1)] - wp[3 * j], dy = wp[3 * (j + 1) + 1] - wp[3 * j + 1];
    return dx == 0.0 && dy == 0.0 ? goal_heading : atan2(dy, dx);
}

BCP_HD inline bool smooth_finite(double v)
{
    const double lim = 1.7976931348623157e308;
    return v >= -lim && v <= lim;   // (a NaN fails every comparison)
}

// One row of bcp_smooth_route as a sequential program: in(k, e), e = 0 .. 2, are the row's m = min(lens_in, max_len_in) way
// points (m < 2, or valid == false for a row whose env or entry is out of range: NO_ROUTE).  cells: [2 m] int16 and
// vertices: [m] uint16 of scratch.  wp: [max_len][3], every slot is written.  Returns the status bits.
template <typename Map, typename In, typename Normalize>
BCP_HD inline int32_t smooth_row(const Map& map, const In& in, int32_t m, bool valid, const SmoothParams& prm, int32_t max_len,
                                 double sp, double ap, int pure_pursuit, const Normalize& normalize, int16_t* cells,
                                 uint16_t* vertices, double* wp, int32_t& len, double init[2], int32_t info[4])
{
    len = 0;
    init[0] = init[1] = 0.0;
    info[0] = info[1] = info[2] = info[3] = 0;
    for (int32_t j = 0; j < 3 * max_len; ++j) wp[j] = 0.0;
    bool finite = valid && m >= 2;
    for (int32_t k = 0; finite && k < m; ++k) finite = smooth_finite(in(k, 0)) && smooth_finite(in(k, 1)) && smooth_finite(in(k, 2));
    if (!finite) return kGoalRouteNoRoute;
    for (int32_t k = 0; k < m; ++k) {
        int32_t r = -1, c = -1;
        if (!map.cell_of(in(k, 0), in(k, 1), r, c)) r = c = -1;
        cells[2 * k] = (int16_t)r;
        cells[2 * k + 1] = (int16_t)c;
    }
    const auto cell = [cells](int32_t k, int32_t& r, int32_t& c) {
        r = cells[2 * k];
        c = cells[2 * k + 1];
        return r >= 0;
    };
    int32_t status = 0, M = 0;
    vertices[0] = (uint16_t)(kSmoothSharp << 12);
    for (int32_t k = 0; k < m - 1;) {   // every trip moves k on: at most m - 1
        int32_t next = smooth_pull_next(map, cell, k, m, prm.look);
        if (next < 0) {
            next = k + 1;
            status |= kSmoothBlocked;
        }
        vertices[++M] = (uint16_t)(next | (kSmoothSharp << 12));
        k = next;
    }
    const auto vertex = [vertices](int32_t t) { return vertices[t]; };
    info[0] = M + 1;
    for (int32_t t = 1; t < M; ++t) {
        const int32_t kp = vertices[t - 1] & 4095, kv = vertices[t] & 4095, kn = vertices[t + 1] & 4095;
        const double p[2] = {in(kp, 0), in(kp, 1)}, v[2] = {in(kv, 0), in(kv, 1)}, n[2] = {in(kn, 0), in(kn, 1)};
        const int32_t level = smooth_blend_level(map, p, v, n, prm.blend, prm.delta, prm.halvings);
        vertices[t] = (uint16_t)(kv | (level << 12));
        ++info[level == 0 ? 1 : (level == kSmoothSharp ? 3 : 2)];
    }
    int32_t total = 1;   // counted before anything is written: at most 8191 pieces of at most 4097 points
    for (int32_t piece = 0; piece < 2 * M - 1; ++piece) total += smooth_piece(in, vertex, M, piece, prm.blend, prm.delta).count;
    if (total > max_len) return status | kGoalRouteLong;
    wp[0] = in(0, 0);
    wp[1] = in(0, 1);
    wp[2] = in(0, 2);
    int32_t at = 1;
    for (int32_t piece = 0; piece < 2 * M - 1; ++piece) {
        const SmoothPiece o = smooth_piece(in, vertex, M, piece, prm.blend, prm.delta);
        for (int32_t i = 1; i <= o.count; ++i, ++at) smooth_piece_point(o, i, wp + 3 * at);
    }
    wp[3 * (total - 1) + 2] = in(m - 1, 2);
    for (int32_t j = 1; j + 1 < total; ++j) wp[3 * j + 2] = smooth_heading(wp, j, in(m - 1, 2));
    len = total;
    double min_dist = 0.0;
    int target = 0, rc = 0;
    path_initial_reward(wp, total, sp, ap, pure_pursuit, min_dist, target, rc, normalize);
    if (rc == 2) status |= kGoalRouteTooClose;
    init[0] = min_dist;
    init[1] = (double)target;
    return status;
}

}  // namespace bcp

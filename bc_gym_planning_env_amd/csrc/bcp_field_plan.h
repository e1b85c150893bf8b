// bcp_field_plan.h -- everything bcp_set_costmaps decides before it touches the device: the footprint geometry behind the
// distance-field classification (sample points, the thresholds t_out / t_in[] the bit-exact verdicts of classify() rest on,
// bcp_coop.h), the scaled footprint, and the shape of all that is derived from a map binding -- padding, clamp, tiles, the
// coarse copy, the strides, the element count of every buffer.  Pure arithmetic, no HIP in here: bcplan.hip and bcp_field.h
// include it, and so does a stand-alone host program (tests/c_abi/field_plan_main.cpp) that checks the geometric claims and a
// table of plans without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "bcp_desc.h"

namespace bcp {

// ---- sample points of the distance-field classification (see bcp_coop.h) -----------------------------------
static inline double seg_dist(double px, double py, double ax, double ay, double bx, double by)
{
    const double vx = bx - ax, vy = by - ay, wx = px - ax, wy = py - ay;
    const double vv = vx * vx + vy * vy;
    double t = vv > 0 ? (wx * vx + wy * vy) / vv : 0.0;
    t = t < 0 ? 0 : (t > 1 ? 1 : t);
    const double cx = ax + t * vx, cy = ay + t * vy;
    return std::sqrt((px - cx) * (px - cx) + (py - cy) * (py - cy));
}

static inline bool point_in_polygon(double px, double py, const double (*v)[2], int k)
{
    bool in = false;
    for (int i = 0, j = k - 1; i < k; j = i++) {
        if (((v[i][1] > py) != (v[j][1] > py)) &&
            (px < (v[j][0] - v[i][0]) * (py - v[i][1]) / (v[j][1] - v[i][1]) + v[i][0]))
            in = !in;
    }
    return in;
}

// Worst-case slack, in pixels, between the real rotated footprint and the pixel set cv2.fillPoly produces from it:
// vertex rounding moves the contour by <= sqrt(.5), Bresenham strays <= .5 from the rounded contour, 16.16 slopes
// add < .01; a sample centre is itself rounded to a pixel (<= sqrt(.5)).
static const double kSlackOuter = 0.7072 + 0.5 + 0.01 + 0.7072;
static const double kSlackInner = 0.7072 + 0.7072 + 0.05;

static inline void build_cull_geometry(const bcp_params& p, double res, CullDesc* C)
{
    const int K = p.n_verts;
    double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300, rmax = 0;
    for (int k = 0; k < K; ++k) {
        xmin = std::min(xmin, p.verts[k][0]);
        xmax = std::max(xmax, p.verts[k][0]);
        ymin = std::min(ymin, p.verts[k][1]);
        ymax = std::max(ymax, p.verts[k][1]);
        rmax = std::max(rmax, std::sqrt(p.verts[k][0] * p.verts[k][0] + p.verts[k][1] * p.verts[k][1]));
    }
    C->reach = (int)std::ceil(rmax / res) + 2;
    C->pad = 2 * C->reach + 4;
    const double ay = 0.5 * (ymin + ymax), half_w = 0.5 * (ymax - ymin);
    // axis segment: pulled in from the ends by a quarter of the half width, so that the round caps of the capsule
    // still cover the corners of a box-like footprint without inflating the radius (corner distance hypot(w/4, w))
    double a0 = xmin + 0.25 * half_w, a1 = xmax - 0.25 * half_w;
    if (a0 > a1) a0 = a1 = 0.5 * (xmin + xmax);
    // OUTER: capsule around the axis segment [a0,a1] x {ay} that contains every vertex (hence the polygon), covered
    // by n_out discs: a disc row of spacing h covers the capsule of radius rho when its radius is sqrt(rho^2+(h/2)^2)
    double rho = 0;
    for (int k = 0; k < K; ++k) rho = std::max(rho, seg_dist(p.verts[k][0], p.verts[k][1], a0, ay, a1, ay));
    // (compared as doubles: a footprint that lies ON its axis has rho == 0, and an infinite quotient must not reach an int)
    const double want_out = a1 > a0 ? std::ceil((a1 - a0) / (0.5 * rho)) + 1 : 1;
    const int n_out = a1 > a0 ? (want_out >= kMaxSamples ? kMaxSamples : std::max(2, (int)want_out)) : 1;
    const double h = n_out > 1 ? (a1 - a0) / (n_out - 1) : 0.0;
    const double r_out = std::sqrt(rho * rho + 0.25 * h * h) / res + kSlackOuter;
    C->n_out = n_out;
    for (int i = 0; i < n_out; ++i) C->out_x[i] = (a0 + i * h) / res;
    C->t_out = (int)std::floor(r_out) + 1;  // floor(d) >= t_out  =>  d > r_out
    // INNER: discs centred on the same axis that lie inside the polygon
    C->n_in = 0;
    for (int j = 0; j < kMaxSamples; ++j) {
        const double bx = kMaxSamples > 1 ? a0 + (a1 - a0) * j / (kMaxSamples - 1) : a0;
        if (!point_in_polygon(bx, ay, p.verts, K)) continue;
        double rin = 1e300;
        for (int k = 0; k < K; ++k) {
            const int kn = (k + 1) % K;
            rin = std::min(rin, seg_dist(bx, ay, p.verts[k][0], p.verts[k][1], p.verts[kn][0], p.verts[kn][1]));
        }
        const double r = rin / res - kSlackInner;   // lethal cell within r of the sample pixel => inside the mask
        const int t = (int)std::floor(r) - 1;       // floor(d) <= t  =>  d < t + 1 <= r
        if (t < 0) continue;
        C->in_x[C->n_in] = bx / res;
        C->t_in[C->n_in] = t;
        ++C->n_in;
        if (a1 <= a0) break;
    }
    C->axis_y = ay / res;
}

static inline int footprint_is_wide(const bcp_params& p, double res)
{
    double d2 = 0;
    for (int i = 0; i < p.n_verts; ++i)
        for (int j = 0; j < i; ++j) {
            const double dx = p.verts[i][0] - p.verts[j][0], dy = p.verts[i][1] - p.verts[j][1];
            d2 = std::max(d2, dx * dx + dy * dy);
        }
    return std::sqrt(d2) / res + 3.0 > 96.0;  // row masks of the cooperative path: 3 words unless wider
}

// robot_footprint / map_resolution (path_tools.py:145), divided on the host in fp64, and its bounding box
static inline void scale_footprint(DevParams& d, const bcp_params& p, double res)
{
    d.qbox[0] = d.qbox[2] = 1e30f;
    d.qbox[1] = d.qbox[3] = -1e30f;
    for (int k = 0; k < p.n_verts; ++k) {
        d.qverts[k][0] = p.verts[k][0] / res;
        d.qverts[k][1] = p.verts[k][1] / res;
        d.qbox[0] = std::min(d.qbox[0], (float)d.qverts[k][0]);
        d.qbox[1] = std::max(d.qbox[1], (float)d.qverts[k][0]);
        d.qbox[2] = std::min(d.qbox[2], (float)d.qverts[k][1]);
        d.qbox[3] = std::max(d.qbox[3], (float)d.qverts[k][1]);
    }
}

static inline int check_kernel_size(const bcp_params& p, double res)
{
    double r2 = 0;
    for (int k = 0; k < p.n_verts; ++k) {
        double d2 = p.verts[k][0] * p.verts[k][0] + p.verts[k][1] * p.verts[k][1];
        if (d2 > r2) r2 = d2;
    }
    return std::sqrt(r2) / res + 2.0 <= BCP_MAX_KERNEL_HALF;
}

// ---- the plan of a map binding ---------------------------------------------------------------------------------
// CullDesc::step_near of private maps unless BCP_TUNE_NEAR_SHIFT says otherwise: a quarter of the resolution (measured on one
// box, shift 0 / 1 / 2: one private 64 x 64 world per env 821 / 751 / 719 bytes of memory traffic per env-step and 21.1 / 20.6 /
// 20.6 us per step; 65 536 private 256 x 141 aisle maps 2.58 / 2.53 / 2.60e9 env-steps/s -- profiles/r04_near_shift.txt;
// shift 3, an eighth: 687 bytes, but 19.6 against 19.1 us and the aisle maps 2.24e9 -- more poses go to the exact test)
constexpr int kNearShiftPrivate = 2;

static inline int map_wpr(int cols) { return (cols + 31) / 32; }   // 32-bit words of a bitmap row

// What bcp_set_costmaps is asked for, as far as the shapes depend on it.  The two sizes that belong to the kernels are
// worked out where the kernels are (bcp_step.h) and passed in as numbers.
struct MapBinding {
    int32_t rows, cols;
    bool shared;
    int64_t entries;          // maps of a private binding (pool entries or envs); a shared binding has one
    double resolution;
    int32_t near_shift;       // BCP_TUNE_NEAR_SHIFT in force (-1: kNearShiftPrivate)
    bool cull;                // BCP_TUNE_CULL
    size_t staged_lds;        // collision_lds_bytes(n_verts, 1, rows, map_wpr(cols)): the collision scratch with the bitmap staged
    int64_t map_tile_words;   // map_tile_words(rows, map_wpr(cols)): an entry of MapDesc::tiles
};

// Every number derived from a binding, each held once.  `cull` is the descriptor as the kernels will get it but for its four
// pointers (edt, near, step_near stay null: whoever owns the buffers sets them); it carries pad, clamp, width, height, the
// strides, tiles_x (near_tx), near_words, the coarse shift and ctx (step_near_tx), and `on`.
struct FieldPlan {
    int64_t n_maps;
    int32_t wpr;
    int32_t in_lds;           // MapDesc::in_lds: the shared bitmap is staged in LDS (the whole scratch stays within 64 KiB)
    int32_t wide;             // kernel image may exceed 96 px: 8-word row masks in the cooperative path
    bool field;               // culling is enabled: a field is planned (its `on` may still be 0: t_out beyond the clamp)
    CullDesc cull;
    int32_t tiles_y, cty;     // tile rows of the tiles and of the coarse copy (cty = 0 without one)
    // elements to reserve, 0 = the buffer is not used by this binding
    size_t n_bitmap, n_map_tiles, n_edt, n_edt_col, n_near, n_near_coarse, n_stale, n_stale_list;
};

static inline FieldPlan plan_field(const bcp_params& p, const MapBinding& b)
{
    FieldPlan f;
    memset(&f, 0, sizeof(f));
    const int rows = b.rows, cols = b.cols;
    const bool shared = b.shared;
    f.n_maps = shared ? 1 : b.entries;
    f.wpr = map_wpr(cols);
    // stage the shared bitmap in LDS when the whole collision scratch then stays within 64 KiB per workgroup
    f.in_lds = (shared && b.staged_lds <= 64 * 1024) ? 1 : 0;
    f.wide = footprint_is_wide(p, b.resolution);
    f.n_bitmap = (size_t)f.n_maps * rows * f.wpr;
    f.n_map_tiles = (size_t)f.n_maps * b.map_tile_words;
    // distance field for the O(1) pre-classification
    CullDesc& C = f.cull;
    build_cull_geometry(p, b.resolution, &C);
    f.field = b.cull;
    if (!f.field) return f;
    // shared map: padding wide enough that every sample of a pose whose image touches the map is stored;
    // private maps: just enough that a sample outside the stored rectangle (more than `pad` px away from every
    // cell of the map) is known to clear the outer test
    if (!shared) C.pad = std::max(8, C.t_out);
    const int clamp = std::min(255, std::max(C.t_out + 1, 2));
    const int W = cols + 2 * C.pad, H = rows + 2 * C.pad;
    f.n_edt = f.n_edt_col = (size_t)f.n_maps * W * H;
    // the 1-bit form for the outer test (near_tiles_kernel)
    const int tiles_x = (W + 31) / 32, tiles_y = (H + 31) / 32;
    f.tiles_y = tiles_y;
    f.n_near = (size_t)f.n_maps * tiles_x * tiles_y * 32;
    C.near_tx = tiles_x;
    C.near_words = tiles_x * tiles_y * 32;
    C.near_stride = shared ? 0 : (int64_t)C.near_words;
    // what the single-launch step reads: the tiles themselves for a shared map (it stays in cache), a coarser copy for
    // private maps -- see CullDesc::step_near
    const int shift = shared ? 0 : (b.near_shift >= 0 ? b.near_shift : kNearShiftPrivate);
    C.step_near_stride = C.near_stride;
    C.step_near_tx = tiles_x;
    C.step_near_shift = 0;
    if (shift > 0) {
        const int cw = (W + (1 << shift) - 1) >> shift, ch = (H + (1 << shift) - 1) >> shift;
        const int ctx = (cw + 31) / 32, cty = (ch + 31) / 32;
        f.cty = cty;
        f.n_near_coarse = (size_t)f.n_maps * ctx * cty * 32;
        C.step_near_stride = (int64_t)ctx * cty * 32;
        C.step_near_tx = ctx;
        C.step_near_shift = shift;
    }
    C.width = W;
    C.height = H;
    C.clamp = clamp;
    C.env_stride = shared ? 0 : (int64_t)W * H;
    C.on = C.t_out <= clamp ? 1 : 0;
    // the stale marks of tiles-only refreshes and their list (private maps): an entry each, and the list's count
    if (!shared) {
        f.n_stale = (size_t)f.n_maps;
        f.n_stale_list = (size_t)f.n_maps + 1;
    }
    return f;
}

}  // namespace bcp

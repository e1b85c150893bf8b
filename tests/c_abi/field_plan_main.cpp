// The plan of a map binding (csrc/bcp_field_plan.h) on the host alone: the footprint geometry behind the distance-field
// classification and every shape and size bcp_set_costmaps derives from a binding.  The header has no HIP in it; this program
// includes nothing else of the library and is built with -fsanitize=address,undefined.
//
// Three kinds of checks over a small zoo of footprints at two or three resolutions each:
//   * geometric claims restated here, independent of the header's code: the outer discs cover the footprint, the inner
//     discs lie inside it (this program's own inside test and segment distance), the reach covers every vertex, the tiles
//     cover the padded field, the buffer counts are entries x per-entry sizes, `on` is exactly t_out <= clamp;
//   * a table of full plans whose numbers were printed by the code as it stood before the plan was split off
//     (bcp_set_costmaps and the geometry functions of bcplan.hip, compiled into a scratch program);
//   * the refusal of a footprint just over BCP_MAX_KERNEL_HALF.
#include <cmath>
#include <cstdio>
#include <vector>

#include "bcp_field_plan.h"
#include "host_io.h"

using namespace bcp;


// ---- the zoo ---------------------------------------------------------------------------------------------------
struct Footprint {
    const char* name;
    std::vector<std::pair<double, double>> verts;
    std::vector<double> resolutions;   // accepted by the size check
};

static const double kOversizeHalf = 125.01 * 0.05 / 1.4142135623730951;   // radius / 0.05 + 2 = 127.01

static std::vector<Footprint> zoo()
{
    std::vector<Footprint> z;
    z.push_back({"tricycle",
                 {{1.34835, 0.}, {1.33856, 0.13975}, {1.30671, 0.28012}, {1.22436, 0.33862}, {1.09381, 0.37464}, {-0.21437, 0.37464},
                  {-0.31362, 0.30856}, {-0.36636, 0.11744}, {-0.37401, -0.13575}, {-0.22796, -0.45913}, {-0.15672, -0.45878},
                  {0.7598, -0.44296}, {0.84969, -0.4264}, {1.17105, -0.35374}, {1.30315, -0.28654}, {1.34134, -0.11837}},
                 {0.05, 0.03, 0.1}});
    z.push_back({"square", {{-0.4, -0.4}, {0.4, -0.4}, {0.4, 0.4}, {-0.4, 0.4}}, {0.05, 0.03, 0.1}});
    z.push_back({"L", {{-0.5, -0.4}, {1.0, -0.4}, {1.0, 0.0}, {0.1, 0.0}, {0.1, 0.6}, {-0.5, 0.6}}, {0.05, 0.03, 0.1}});
    // every vertex on the sample axis: rho == 0, the quotient that sizes the disc row is infinite
    z.push_back({"on_axis", {{-0.8, 0.0}, {0.1, 0.0}, {0.9, 0.0}}, {0.05, 0.03, 0.1}});
    // 4.8 m x 0.6 m: more than 96 px across at 0.05 and 0.03 (wide row masks), not at 0.1
    z.push_back({"bar", {{-2.4, -0.3}, {2.4, -0.3}, {2.4, 0.3}, {-2.4, 0.3}}, {0.05, 0.03, 0.1}});
    // radius / 0.05 + 2 = 127.01: refused at 0.05, fine at coarser resolutions
    z.push_back({"oversize",
                 {{-kOversizeHalf, -kOversizeHalf}, {kOversizeHalf, -kOversizeHalf}, {kOversizeHalf, kOversizeHalf}, {-kOversizeHalf, kOversizeHalf}},
                 {0.1, 0.2}});
    return z;
}

static bcp_params params_of(const Footprint& f)
{
    bcp_params p;
    memset(&p, 0, sizeof(p));
    p.n_verts = (int32_t)f.verts.size();
    for (size_t k = 0; k < f.verts.size(); ++k) {
        p.verts[k][0] = f.verts[k].first;
        p.verts[k][1] = f.verts[k].second;
    }
    return p;
}

// ---- this program's own geometry ----------------------------------------------------------------------------
// distance from p to the segment a-b, by the sign of the two end projections (no clamped parameter)
static double own_segment_distance(double px, double py, double ax, double ay, double bx, double by)
{
    const double ex = bx - ax, ey = by - ay;
    if ((px - ax) * ex + (py - ay) * ey <= 0) return std::hypot(px - ax, py - ay);
    if ((px - bx) * ex + (py - by) * ey >= 0) return std::hypot(px - bx, py - by);
    return std::fabs((px - ax) * ey - (py - ay) * ex) / std::hypot(ex, ey);
}

// winding number by summed signed angles: non-zero = inside (the zoo has no self-intersecting member)
static bool own_inside(double px, double py, const std::vector<std::pair<double, double>>& q)
{
    double turn = 0;
    for (size_t i = 0; i < q.size(); ++i) {
        const size_t j = (i + 1) % q.size();
        const double ax = q[i].first - px, ay = q[i].second - py, bx = q[j].first - px, by = q[j].second - py;
        turn += std::atan2(ax * by - ay * bx, ax * bx + ay * by);
    }
    return std::fabs(turn) > 3.0;   // (+-2 pi inside, 0 outside)
}

// ---- claims ------------------------------------------------------------------------------------------------------
static size_t tile_words_of(int rows, int wpr) { return (size_t)((rows + 31) & ~31) * wpr; }

static MapBinding binding_of(int rows, int cols, bool shared, int64_t entries, double res, int near_shift, bool cull,
                             size_t staged_lds = 40000)
{
    const MapBinding b = {rows, cols, shared, entries, res, near_shift, cull, staged_lds, (int64_t)tile_words_of(rows, map_wpr(cols))};
    return b;
}

static void check_geometry(const Footprint& f, double res)
{
    const bcp_params p = params_of(f);
    CullDesc C;
    memset(&C, 0, sizeof(C));
    build_cull_geometry(p, res, &C);
    std::vector<std::pair<double, double>> q;   // the footprint in pixels
    for (const auto& v : f.verts) q.push_back({v.first / res, v.second / res});
    CHECK(C.n_out >= 1 && C.n_out <= kMaxSamples);
    CHECK(C.n_in >= 0 && C.n_in <= kMaxSamples);
    // every point of the outline lies closer than t_out - kSlackOuter to an outer sample centre (then so does every point
    // inside: the discs' union covers the capsule around the axis, which is convex and contains the outline)
    double worst = 0;
    for (size_t i = 0; i < q.size(); ++i) {
        const size_t j = (i + 1) % q.size();
        const double len = std::hypot(q[j].first - q[i].first, q[j].second - q[i].second);
        const int steps = (int)std::ceil(len / 0.05) + 1;   // a point every 0.05 px or closer
        for (int s = 0; s <= steps; ++s) {
            const double t = (double)s / steps;
            const double x = q[i].first + t * (q[j].first - q[i].first), y = q[i].second + t * (q[j].second - q[i].second);
            double nearest = 1e300;
            for (int k = 0; k < C.n_out; ++k) nearest = std::min(nearest, std::hypot(x - C.out_x[k], y - C.axis_y));
            worst = std::max(worst, nearest);
        }
    }
    CHECK(worst < (double)C.t_out - kSlackOuter);
    // around every inner sample the circle of radius t_in + 1 + kSlackInner lies inside the polygon: its centre is inside,
    // no edge comes closer than the radius, and (the same once more, point by point) 360 points of it are inside.
    // 1e-9 px: (rin / res - slack) + slack is rin / res to a few units in the last place, not exactly.
    for (int j = 0; j < C.n_in; ++j) {
        const double r = C.t_in[j] + 1 + kSlackInner - 1e-9;
        CHECK(C.t_in[j] >= 0);
        CHECK(own_inside(C.in_x[j], C.axis_y, q));
        double edge = 1e300;
        for (size_t i = 0; i < q.size(); ++i) {
            const size_t n = (i + 1) % q.size();
            edge = std::min(edge, own_segment_distance(C.in_x[j], C.axis_y, q[i].first, q[i].second, q[n].first, q[n].second));
        }
        CHECK(edge >= r);
        bool all_inside = true;
        for (int a = 0; a < 360; ++a) {
            const double th = a * 3.14159265358979323846 / 180.0;
            all_inside = all_inside && own_inside(C.in_x[j] + (r - 1e-6) * std::cos(th), C.axis_y + (r - 1e-6) * std::sin(th), q);
        }
        CHECK(all_inside);
    }
    for (const auto& v : q) CHECK(std::hypot(v.first, v.second) <= C.reach - 2);
    CHECK(C.pad == 2 * C.reach + 4);
}

static void check_plan(const Footprint& f, double res, const MapBinding& b)
{
    const bcp_params p = params_of(f);
    const FieldPlan plan = plan_field(p, b);
    const CullDesc& C = plan.cull;
    const int64_t n_maps = b.shared ? 1 : b.entries;
    CHECK(plan.n_maps == n_maps);
    CHECK(plan.wpr * 32 >= b.cols && (plan.wpr - 1) * 32 < b.cols);
    CHECK(plan.n_bitmap == (size_t)n_maps * b.rows * plan.wpr);
    CHECK(plan.n_map_tiles == (size_t)n_maps * tile_words_of(b.rows, plan.wpr));
    CHECK(plan.in_lds == ((b.shared && b.staged_lds <= 64 * 1024) ? 1 : 0));
    CHECK(C.edt == nullptr && C.near == nullptr && C.step_near == nullptr);
    CHECK(plan.field == b.cull);
    if (!b.cull) {   // the geometry alone: no field, nothing to reserve for one
        CHECK(C.on == 0 && C.width == 0 && C.height == 0 && C.near_words == 0);
        CHECK(plan.n_edt + plan.n_edt_col + plan.n_near + plan.n_near_coarse + plan.n_stale + plan.n_stale_list == 0);
        return;
    }
    const int W = C.width, H = C.height;
    CHECK(W == b.cols + 2 * C.pad && H == b.rows + 2 * C.pad);
    CHECK(C.on == (C.t_out <= C.clamp ? 1 : 0));
    CHECK(C.clamp <= 255 && C.clamp >= 2);
    // a private field is padded just far enough that a sample outside it clears the outer test
    if (!b.shared) CHECK(C.pad >= C.t_out);
    // the tiles cover the padded field, with no spare tile
    CHECK(C.near_tx * 32 >= W && (C.near_tx - 1) * 32 < W);
    CHECK(plan.tiles_y * 32 >= H && (plan.tiles_y - 1) * 32 < H);
    CHECK(C.near_words == C.near_tx * plan.tiles_y * 32);
    // ... and so does the coarse copy, a bit of which stands for 2^shift x 2^shift cells
    const int shift = C.step_near_shift;
    CHECK(shift == (b.shared ? 0 : (b.near_shift >= 0 ? b.near_shift : kNearShiftPrivate)));
    if (shift > 0) {
        CHECK(((int64_t)C.step_near_tx * 32 << shift) >= W && ((int64_t)plan.cty * 32 << shift) >= H);
        CHECK(((int64_t)(C.step_near_tx - 1) * 32 << shift) < W && ((int64_t)(plan.cty - 1) * 32 << shift) < H);
        CHECK(C.step_near_stride == (int64_t)C.step_near_tx * plan.cty * 32);
        CHECK(plan.n_near_coarse == (size_t)n_maps * C.step_near_stride);
    } else {
        CHECK(C.step_near_tx == C.near_tx && C.step_near_stride == C.near_stride && plan.cty == 0 && plan.n_near_coarse == 0);
    }
    // strides: an entry's size for private maps, 0 for the shared one
    CHECK(C.env_stride == (b.shared ? 0 : (int64_t)W * H));
    CHECK(C.near_stride == (b.shared ? 0 : (int64_t)C.near_words));
    // counts: entries x per-entry size
    CHECK(plan.n_edt == (size_t)n_maps * W * H && plan.n_edt_col == plan.n_edt);
    CHECK(plan.n_near == (size_t)n_maps * C.near_words);
    CHECK(plan.n_stale == (b.shared ? 0 : (size_t)n_maps));
    CHECK(plan.n_stale_list == (b.shared ? 0 : (size_t)n_maps + 1));
    CHECK(plan.wide == footprint_is_wide(p, res));
}

// ---- the table ----------------------------------------------------------------------------------------------------
struct PlanRow {
    const char* footprint;
    double res;
    int rows, cols;
    bool shared;
    int64_t entries;
    int near_shift;
    size_t staged_lds;
    // expected
    int wpr, in_lds, wide, on, pad, clamp, W, H, tiles_x, tiles_y, near_words, shift, ctx, cty;
    long long near_stride, step_near_stride, env_stride;
    int reach, t_out, n_out, n_in;
    size_t n_bitmap, n_map_tiles, n_edt, n_near, n_near_coarse, n_stale, n_stale_list;
};

// (inputs, then: wpr in_lds wide on pad clamp W H tiles_x tiles_y near_words shift ctx cty, the three strides, reach t_out
//  n_out n_in, then the counts)
static const PlanRow kTable[] = {
    {"tricycle", 0.05, 24, 40, true, 64, -1, 40000,
     2, 1, 0, 1, 62, 12, 164, 148, 6, 5, 960, 0, 6, 0, 0LL, 0LL, 0LL, 29, 11, 8, 6,
     48, 64, 24272, 960, 0, 0, 0},
    {"tricycle", 0.05, 17, 33, false, 3, -1, 40000,
     2, 0, 0, 1, 11, 12, 55, 39, 2, 2, 128, 2, 1, 1, 128LL, 32LL, 2145LL, 29, 11, 8, 6,
     102, 192, 6435, 384, 96, 3, 4},
    {"square", 0.03, 17, 33, false, 3, 0, 40000,
     2, 0, 0, 1, 17, 18, 67, 51, 3, 2, 192, 0, 3, 0, 192LL, 192LL, 3417LL, 21, 17, 4, 8,
     102, 192, 10251, 576, 0, 3, 4},
    {"L", 0.05, 256, 141, false, 4096, 3, 70000,
     5, 0, 0, 1, 13, 14, 167, 282, 6, 9, 1728, 3, 1, 2, 1728LL, 64LL, 47094LL, 24, 13, 6, 2,
     5242880, 5242880, 192897024, 7077888, 262144, 4096, 4097},
    {"bar", 0.05, 200, 320, true, 1, -1, 70000,
     10, 0, 1, 1, 106, 13, 532, 412, 17, 13, 7072, 0, 17, 0, 0LL, 0LL, 0LL, 51, 12, 8, 6,
     2000, 2240, 219184, 7072, 0, 0, 0},
    {"on_axis", 0.1, 64, 64, false, 64, -1, 40000,
     2, 0, 0, 1, 8, 5, 80, 80, 3, 3, 288, 2, 1, 1, 288LL, 32LL, 6400LL, 11, 4, 8, 0,
     8192, 8192, 409600, 18432, 2048, 64, 65},
    {"oversize", 0.1, 24, 40, false, 5, 0, 40000,
     2, 0, 1, 1, 49, 50, 138, 122, 5, 4, 640, 0, 5, 0, 640LL, 640LL, 16836LL, 65, 49, 4, 8,
     240, 320, 84180, 3200, 0, 5, 6},
};

static void check_table(const std::vector<Footprint>& z)
{
    for (const PlanRow& r : kTable) {
        const Footprint* f = nullptr;
        for (const Footprint& c : z)
            if (!strcmp(c.name, r.footprint)) f = &c;
        snprintf(g_where, sizeof(g_where), "table %s res %g %dx%d shared %d shift %d", r.footprint, r.res, r.rows, r.cols, (int)r.shared, r.near_shift);
        CHECK(f != nullptr);
        if (!f) continue;
        const FieldPlan plan = plan_field(params_of(*f), binding_of(r.rows, r.cols, r.shared, r.entries, r.res, r.near_shift, true, r.staged_lds));
        const CullDesc& C = plan.cull;
        CHECK(plan.wpr == r.wpr && plan.in_lds == r.in_lds && plan.wide == r.wide && C.on == r.on);
        CHECK(C.pad == r.pad && C.clamp == r.clamp && C.width == r.W && C.height == r.H);
        CHECK(C.near_tx == r.tiles_x && plan.tiles_y == r.tiles_y && C.near_words == r.near_words);
        CHECK(C.step_near_shift == r.shift && C.step_near_tx == r.ctx && plan.cty == r.cty);
        CHECK(C.near_stride == r.near_stride && C.step_near_stride == r.step_near_stride && C.env_stride == r.env_stride);
        CHECK(C.reach == r.reach && C.t_out == r.t_out && C.n_out == r.n_out && C.n_in == r.n_in);
        CHECK(plan.n_bitmap == r.n_bitmap && plan.n_map_tiles == r.n_map_tiles && plan.n_edt == r.n_edt && plan.n_edt_col == r.n_edt);
        CHECK(plan.n_near == r.n_near && plan.n_near_coarse == r.n_near_coarse && plan.n_stale == r.n_stale && plan.n_stale_list == r.n_stale_list);
    }
}

int main()
{
    const std::vector<Footprint> z = zoo();
    for (const Footprint& f : z) {
        for (double res : f.resolutions) {
            snprintf(g_where, sizeof(g_where), "%s res %g", f.name, res);
            CHECK(check_kernel_size(params_of(f), res));
            check_geometry(f, res);
            // shared and private bindings, a column count that is no multiple of 32, every near_shift, culling on and off
            for (int shift = -1; shift <= 3; ++shift)
                for (int cull = 0; cull < 2; ++cull) {
                    snprintf(g_where, sizeof(g_where), "%s res %g shift %d cull %d", f.name, res, shift, cull);
                    check_plan(f, res, binding_of(24, 40, true, 64, res, shift, cull != 0));
                    check_plan(f, res, binding_of(17, 33, false, 3, res, shift, cull != 0));
                    check_plan(f, res, binding_of(256, 141, false, 4096, res, shift, cull != 0, 70000));
                    check_plan(f, res, binding_of(200, 320, true, 1, res, shift, cull != 0, 70000));
                }
        }
    }
    snprintf(g_where, sizeof(g_where), "widths");
    CHECK(footprint_is_wide(params_of(z[4]), 0.05) && footprint_is_wide(params_of(z[4]), 0.03) && !footprint_is_wide(params_of(z[4]), 0.1));
    CHECK(!footprint_is_wide(params_of(z[0]), 0.05));
    // the oversized footprint is refused at the resolution that makes it so, and just inside the limit it is not
    snprintf(g_where, sizeof(g_where), "refusal");
    CHECK(!check_kernel_size(params_of(z[5]), 0.05));
    CHECK(check_kernel_size(params_of(z[5]), 0.05 * 127.02 / 127.0));
    check_table(z);
    if (g_failed) {
        fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    printf("field plan ok\n");
    return 0;
}

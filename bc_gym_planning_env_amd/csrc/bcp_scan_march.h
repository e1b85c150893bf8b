// bcp_scan_march.h -- the range scan's arithmetic (bcp_range_scan, include/bcplan.h): the argument checks, the test of a
// row's pose, and the walk of one ray over the grid.  Plain C++ with no HIP in it: range_scan_kernel (bcp_scan.h) calls these
// functions on the device, tests/c_abi/range_scan_main.cpp calls the same ones on the host, and there is no other copy of
// the loop.  Everything is float64 with every product, quotient and sum rounded on its own (-ffp-contract=off).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define BCP_HD __host__ __device__
#else
#define BCP_HD
#endif

namespace bcp {

constexpr int32_t kScanMaxBeams = 1024;
constexpr double kScanMaxCells = 4096.0;        // max_range * inv_res may not exceed this
constexpr double kScanMaxCoord = 1073741824.0;  // 2^30: |u|, |v| at or beyond it give a row of misses

// what bcp_range_scan refuses with BCP_E_INVALID, in the order it looks
enum ScanRefusal { kScanOk = 0, kScanNull = 1, kScanBeams = 2, kScanRows = 3, kScanRange = 4 };

// inv_res: MapDesc::inv_res, or 0 while no costmaps are bound (that refusal is the caller's)
// n_envs: what n must be without poses; final_form: the rows are the record's, n is not the caller's to choose
BCP_HD inline int scan_check_args(bool have_handle, bool have_beams, bool have_ranges, int32_t n_beams, int64_t n,
                                  int64_t n_envs, bool have_poses, bool final_form, double max_range, double inv_res)
{
    if (!have_handle || !have_beams || !have_ranges) return kScanNull;
    if (n_beams < 1 || n_beams > kScanMaxBeams) return kScanBeams;
    if (!final_form && (n <= 0 || (!have_poses && n != n_envs))) return kScanRows;
    // (written so that a NaN fails every comparison it meets)
    if (!(max_range > 0.0) || !(max_range <= 1.7976931348623157e308) || !(max_range * inv_res <= kScanMaxCells)) return kScanRange;
    return kScanOk;
}

// trips after which the walk has certainly ended: it crosses one grid line per trip, and R cells of ray cross at most
// ceil(R) + 1 lines of either family
BCP_HD inline int32_t scan_trip_bound(double R)
{
    const int32_t whole = (int32_t)R;   // (R <= 4096)
    return 2 * (whole + ((double)whole < R ? 1 : 0)) + 4;
}

// a row is walked only if its pose is finite and its grid coordinates are within +- 2^30 (the cell indices then fit an
// int32 with room for every step of the walk); every beam of another row is a miss
BCP_HD inline bool scan_row_ok(double x, double y, double th, double u, double v)
{
    const double lim = 1.7976931348623157e308;
    const bool finite = x >= -lim && x <= lim && y >= -lim && y <= lim && th >= -lim && th <= lim;
    return finite && u > -kScanMaxCoord && u < kScanMaxCoord && v > -kScanMaxCoord && v < kScanMaxCoord;
}

// A row's start in cell units, cell (row, col) covering [col, col + 1) x [row, row + 1), and how far its rays go: R cells,
// or 0 for a row that is not walked (u = v = 0 then)
BCP_HD inline void scan_row_start(double x, double y, double th, double ox, double oy, double inv_res, double R, double* u,
                                  double* v, double* row_R)
{
    *u = (x - ox) * inv_res + 0.5;
    *v = (y - oy) * inv_res + 0.5;
    const bool ok = scan_row_ok(x, y, th, *u, *v);
    if (!ok) *u = *v = 0.0;
    *row_R = ok ? R : 0.0;
}

// beam (cb, sb) of a robot heading along (c, s), in the map's frame
BCP_HD inline void scan_direction(double c, double s, double cb, double sb, double* dx, double* dy)
{
    *dx = c * cb - s * sb;
    *dy = s * cb + c * sb;
}

BCP_HD inline int32_t scan_floor(double a)   // floor of |a| < 2^30 as an integer
{
    const int32_t i = (int32_t)a;
    return (double)i > a ? i - 1 : i;
}

struct ScanResult {
    float range;
    int32_t hit;      // row * cols + col of the lethal cell, -1 for a miss
    int32_t trips;    // trips of the loop (tests: the bound is never reached)
};

// One ray of the contract in include/bcplan.h: from (u, v) in cell units -- cell (row, col) covers [col, col + 1) x
// [row, row + 1) -- along (dx, dy), until a lethal cell inside the valid shape (range = t * resolution) or t >= R (range =
// max_range).  words(k): word k of the entry's row-major lethal mask, `wpr` words per row, bit (col & 31) of word
// row * wpr + (col >> 5); `cols` is the allocated width that `hit` counts in.  A tie between the next vertical and the next
// horizontal grid line steps in y: a ray through the shared corner of two diagonally adjacent cells visits only the cell
// across the corner and the one above or below it, so it can slip between two wall cells that touch at that corner alone.
// Every other ray visits every cell it touches.
template <typename Words>
BCP_HD inline ScanResult scan_march(const Words& words, int32_t wpr, int32_t cols, int32_t valid_rows, int32_t valid_cols,
                                    double u, double v, double dx, double dy, double R, double resolution, double max_range,
                                    int32_t trip_bound)
{
    const double inf = __builtin_huge_val();
    int32_t col = scan_floor(u), row = scan_floor(v);
    const int32_t sx = dx > 0.0 ? 1 : -1, sy = dy > 0.0 ? 1 : -1;
    const double tdx = dx != 0.0 ? __builtin_fabs(1.0 / dx) : inf;
    const double tdy = dy != 0.0 ? __builtin_fabs(1.0 / dy) : inf;
    double tmx = dx > 0.0 ? ((double)(col + 1) - u) / dx : (dx < 0.0 ? ((double)col - u) / dx : inf);
    double tmy = dy > 0.0 ? ((double)(row + 1) - v) / dy : (dy < 0.0 ? ((double)row - v) / dy : inf);
    double t = 0.0;
    ScanResult r;
    r.range = (float)max_range;
    r.hit = -1;
    r.trips = 0;
    for (int32_t trip = 0; trip < trip_bound && t < R; ++trip) {
        r.trips = trip + 1;
        if ((uint32_t)row < (uint32_t)valid_rows && (uint32_t)col < (uint32_t)valid_cols &&
            ((words(row * wpr + (col >> 5)) >> (col & 31)) & 1u)) {
            r.range = (float)(t * resolution);
            r.hit = row * cols + col;
            return r;
        }
        if (tmx < tmy) {
            t = tmx;
            tmx += tdx;
            col += sx;
        } else {
            t = tmy;
            tmy += tdy;
            row += sy;
        }
    }
    return r;
}

}  // namespace bcp

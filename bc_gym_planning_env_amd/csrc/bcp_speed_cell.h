// bcp_speed_cell.h -- the arithmetic of bcp_path_speed (include/bcplan.h): the argument checks, a way point's curvature
// (speed_curvature), the limit it sets on the squared speed (speed_limit), the two passes that make a speed profile of the
// limits -- as the sequential recurrence that DEFINES the value (speed_row) and as the combine of the scan the device runs
// (speed_combine) --, and the plan of the kernel's LDS (speed_lds_plan).  Plain C++ with no HIP in it.  Who calls this, on
// the device: speed_kernel (bcp_speed.h), a lane per way point.  On the host, under sanitizers and through bounds-checked
// accessors: tests/c_abi/speed_profile_main.cpp, and there is no other copy.  Everything is float64 and every product,
// quotient, root and sum is rounded on its own (-ffp-contract=off); it uses + - * /, the square root and comparisons.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BCP_HD __host__ __device__
#else
#define BCP_HD
#endif

namespace bcp {

constexpr int32_t kSpeedMaxLen = 4096;      // way points of a row
constexpr int32_t kSpeedMaxSpan = 64;
constexpr int32_t kSpeedNoPath = 4;         // BCP_SPEED_NO_PATH
constexpr double kSpeedMinDen = 1e-18;      // a triple whose side lengths multiply to less has no curvature
constexpr double kSpeedInf = INFINITY;

struct SpeedParams {   // bcp_speed_params, field for field
    int32_t span, reserved;
    double v_max, v_min, a_lat, w_max, a_dec, a_acc, v_start, v_end;
};

// what bcp_path_speed refuses with BCP_E_INVALID, in the order it looks.  overlap: `speed`, `kappa` or `v_limit` shares a
// byte with `paths` (speed_overlap)
enum SpeedRefusal {
    kSpeedOk = 0, kSpeedNull = 1, kSpeedMaxLenRange = 2, kSpeedRows = 3, kSpeedSpan = 4, kSpeedPositive = 5,
    kSpeedNonNegative = 6, kSpeedOrder = 7, kSpeedOverlap = 8
};

BCP_HD inline bool speed_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    return a < b + b_bytes && b < a + a_bytes;
}

BCP_HD inline bool speed_finite(double v)
{
    const double lim = 1.7976931348623157e308;
    return v >= -lim && v <= lim;   // (a NaN fails both)
}

// which: the field a kSpeedPositive / kSpeedNonNegative names -- 0 .. 4 = v_max, a_lat, w_max, a_dec, a_acc; 0 .. 2 = v_min,
// v_start, v_end
BCP_HD inline int speed_check_args(bool have_pointers, bool have_params, int32_t max_len, int64_t n, const SpeedParams& p,
                                   bool overlap, int* which)
{
    *which = 0;
    if (!have_pointers || !have_params) return kSpeedNull;
    if (max_len < 1 || max_len > kSpeedMaxLen) return kSpeedMaxLenRange;
    if (n <= 0 || n > 0x7FFFFFFFll) return kSpeedRows;
    if (p.span < 1 || p.span > kSpeedMaxSpan) return kSpeedSpan;
    const double positive[5] = {p.v_max, p.a_lat, p.w_max, p.a_dec, p.a_acc};
    for (int k = 0; k < 5; ++k) {
        *which = k;
        if (!(positive[k] > 0.0 && speed_finite(positive[k]))) return kSpeedPositive;
    }
    const double non_negative[3] = {p.v_min, p.v_start, p.v_end};
    for (int k = 0; k < 3; ++k) {
        *which = k;
        if (!(non_negative[k] >= 0.0 && speed_finite(non_negative[k]))) return kSpeedNonNegative;
    }
    *which = 0;
    if (p.v_min > p.v_max) return kSpeedOrder;
    if (overlap) return kSpeedOverlap;
    return kSpeedOk;
}

// The kernel's dynamic LDS: one plane of max_len doubles.  It holds u_lim until the backward pass overwrites slot after slot
// with ub (u_lim[j] is read once more by nobody), which the forward pass reads.  32 KB at max_len = 4096.
struct SpeedLdsPlan {
    int32_t u_doubles;   // doubles of the plane, from offset 0
    uint32_t bytes;
};

BCP_HD inline SpeedLdsPlan speed_lds_plan(int32_t max_len)
{
    SpeedLdsPlan plan;
    plan.u_doubles = max_len;
    plan.bytes = (uint32_t)max_len * 8u;
    return plan;
}

// the row's way points as the call counts them
BCP_HD inline int32_t speed_row_len(int32_t len, int32_t max_len)
{
    const int32_t m = len < max_len ? len : max_len;
    return m < 0 ? 0 : m;
}

// ---- a way point's own numbers.  Points: P(k, e) = way point k's x (e = 0) / y (e = 1)
// The Menger curvature of (P_a, P_j, P_b), a = max(j - span, 0), b = min(j + span, m - 1); 0 at the row's ends and for a
// triple with (almost) coinciding points.
template <typename Points>
BCP_HD inline double speed_curvature(const Points& P, int32_t m, int32_t j, int32_t span)
{
    const int32_t a = j - span > 0 ? j - span : 0;
    const int32_t b = j + span < m - 1 ? j + span : m - 1;
    if (a == j || b == j) return 0.0;
    const double ax = P(j, 0) - P(a, 0), ay = P(j, 1) - P(a, 1);
    const double bx = P(b, 0) - P(j, 0), by = P(b, 1) - P(j, 1);
    const double cx = P(b, 0) - P(a, 0), cy = P(b, 1) - P(a, 1);
    const double la = std::sqrt(ax * ax + ay * ay), lb = std::sqrt(bx * bx + by * by), lc = std::sqrt(cx * cx + cy * cy);
    const double den = (la * lb) * lc;
    const double cr = std::fabs(ax * by - ay * bx);
    return den < kSpeedMinDen ? 0.0 : (2.0 * cr) / den;
}

// u_lim[j]: the largest squared speed way point j allows on its own
BCP_HD inline double speed_limit(double kappa, int32_t j, int32_t m, const SpeedParams& p)
{
    double u = p.v_max * p.v_max;
    if (kappa > 0.0) {
        const double t = p.a_lat / kappa;
        if (t < u) u = t;
        const double s = p.w_max / kappa;
        const double s2 = s * s;
        if (s2 < u) u = s2;
    }
    const double f = p.v_min * p.v_min;
    if (u < f) u = f;
    if (j == 0) {
        const double e = p.v_start * p.v_start;
        if (e < u) u = e;
    }
    if (j == m - 1) {
        const double e = p.v_end * p.v_end;
        if (e < u) u = e;
    }
    return u;
}

// ds_j: from way point j to j + 1 (j + 1 < m)
template <typename Points>
BCP_HD inline double speed_ds(const Points& P, int32_t j)
{
    const double dx = P(j + 1, 0) - P(j, 0), dy = P(j + 1, 1) - P(j, 1);
    return std::sqrt(dx * dx + dy * dy);
}

// c_j of a pass: the squared speed a stretch ds allows to gain (or shed) at acceleration acc
BCP_HD inline double speed_gain(double acc, double ds) { return (2.0 * acc) * ds; }

// ---- the passes as a scan.  A step of either pass is f(u) = min(A, u + c); first `second`, then `first`:
// (A1, c1) o (A2, c2) = (min(A1, A2 + c1), c1 + c2).  The identity is (inf, 0).  Every c is >= 0 and every A >= 0.
struct SpeedStep {
    double A, c;
};

BCP_HD inline SpeedStep speed_combine(const SpeedStep& first, const SpeedStep& second)
{
    SpeedStep out;
    const double through = second.A + first.c;
    out.A = through < first.A ? through : first.A;
    out.c = first.c + second.c;
    return out;
}

BCP_HD inline double speed_apply(const SpeedStep& f, double u)
{
    const double through = u + f.c;
    return through < f.A ? through : f.A;
}

// ---- the row as a sequential program: the recurrence that defines the value.  u: a scratch plane of m doubles (u_lim, then
// ub, then uf); speed [max_len], kappa / v_limit [max_len] or nullptr.  -> the row's status.
template <typename Points>
BCP_HD inline int32_t speed_row(const Points& P, int32_t len, int32_t max_len, const SpeedParams& p, double* u, double* speed,
                                double* kappa, double* v_limit)
{
    const int32_t m = speed_row_len(len, max_len);
    bool ok = len >= 1;
    for (int32_t j = 0; ok && j < m; ++j) ok = speed_finite(P(j, 0)) && speed_finite(P(j, 1));
    const int32_t written = ok ? m : 0;
    for (int32_t j = written; j < max_len; ++j) {
        speed[j] = 0.0;
        if (kappa) kappa[j] = 0.0;
        if (v_limit) v_limit[j] = 0.0;
    }
    if (!ok) return kSpeedNoPath;
    for (int32_t j = 0; j < m; ++j) {
        const double k = speed_curvature(P, m, j, p.span);
        u[j] = speed_limit(k, j, m, p);
        if (kappa) kappa[j] = k;
        if (v_limit) v_limit[j] = std::sqrt(u[j]);
    }
    for (int32_t j = m - 2; j >= 0; --j) {   // backward: brake in time
        const double through = u[j + 1] + speed_gain(p.a_dec, speed_ds(P, j));
        if (through < u[j]) u[j] = through;
    }
    for (int32_t j = 1; j < m; ++j) {        // forward: accelerate no harder than a_acc
        const double through = u[j - 1] + speed_gain(p.a_acc, speed_ds(P, j - 1));
        if (through < u[j]) u[j] = through;
    }
    for (int32_t j = 0; j < m; ++j) speed[j] = std::sqrt(u[j]);
    return 0;
}

}  // namespace bcp

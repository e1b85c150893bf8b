// bcp_speed.h -- speed_kernel: bcp_path_speed (include/bcplan.h), a speed per way point that slows for curvature, brakes in
// time and accelerates no harder than allowed.  The arithmetic -- a way point's curvature and limit, a step of a pass and
// the combine of two -- is bcp_speed_cell.h, which has no HIP in it and whose speed_row is the row as a sequential program;
// this file decides which lane owns which way point and in which order the steps of a pass are combined.
//
// One wave per row, one wave per workgroup (smooth_kernel's layout).  Way point j belongs to lane j % 64 in every phase, in
// trips of 64 aligned at multiples of 64, so the LDS plane is only ever read by the lane that wrote the slot and no barrier
// stands between the phases.
//   0  a lane per way point votes on "finite"; a row without a path is zeros and BCP_SPEED_NO_PATH
//   1  limits: kappa and u_lim per way point; u_lim goes to LDS, kappa and sqrt(u_lim) to the optional outputs
//   2  backward: the trips from the row's end to its start.  A trip is an inclusive suffix scan of the steps
//      (u_lim[j], cd_j) -- six __shfl_down on the two doubles of a step -- applied to the carry, ub of the first way point
//      of the trip behind (+inf behind the row's end); ub overwrites u_lim in LDS
//   3  forward: the trips from the start to the end, an inclusive prefix scan of (ub[j], ca_{j-1}) applied to the carry, uf
//      of the last way point of the trip before; speed = sqrt(uf), a lane per consecutive double
// The scans associate the sums of the c's in a tree where speed_row adds them one by one: include/bcplan.h bounds the
// difference.  LDS: speed_lds_plan -- 8 bytes per slot, 32 KB at max_len = 4096.
#pragma once

#include "bcp_device.h"
#include "bcp_speed_cell.h"

namespace bcp {

struct SpeedArgs {
    const double* paths;     // [n][max_len][3]
    const int32_t* lens;     // [n]
    int32_t max_len, pad;
    SpeedParams prm;
    double* speed;           // [n][max_len]
    double* kappa;           // [n][max_len], or nullptr
    double* v_limit;         // [n][max_len], or nullptr
    int32_t* status;         // [n]
};

typedef __attribute__((address_space(3))) double* SpeedLdsF64;

struct SpeedIn {
    const double* p;
    __device__ __forceinline__ double operator()(int32_t k, int32_t e) const { return p[3 * k + e]; }
};

__global__ void __launch_bounds__(64) speed_kernel(const SpeedArgs a)
{
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const SpeedLdsF64 u = (SpeedLdsF64)lds_dyn;   // [max_len]: u_lim, then ub
    const int32_t max_len = a.max_len;
    const int32_t len = a.lens[row];
    const int32_t m = speed_row_len(len, max_len);
    const SpeedIn in = {a.paths + row * (int64_t)max_len * 3};
    const SpeedParams prm = a.prm;
    double* const sp = a.speed + row * (int64_t)max_len;
    double* const kp = a.kappa ? a.kappa + row * (int64_t)max_len : nullptr;
    double* const vl = a.v_limit ? a.v_limit + row * (int64_t)max_len : nullptr;

    // ---- 0: is there a path
    bool finite = true;
    for (int32_t k = lane; k < m; k += 64) finite = finite && speed_finite(in(k, 0)) && speed_finite(in(k, 1));
    const bool ok = len >= 1 && __ballot(!finite) == 0;   // (wave-uniform)
    for (int32_t j = (ok ? m : 0) + lane; j < max_len; j += 64) {
        sp[j] = 0.0;
        if (kp) kp[j] = 0.0;
        if (vl) vl[j] = 0.0;
    }
    if (lane == 0) a.status[row] = ok ? 0 : kSpeedNoPath;
    if (!ok) return;
    // ---- 1: limits
    for (int32_t j = lane; j < m; j += 64) {
        const double k = speed_curvature(in, m, j, prm.span);
        const double ul = speed_limit(k, j, m, prm);
        u[j] = ul;
        if (kp) kp[j] = k;
        if (vl) vl[j] = sqrt(ul);
    }
    // ---- 2: backward.  Lanes past m hold the identity; every lane takes part in the shuffles.
    double carry = kSpeedInf;
    for (int32_t base = ((m - 1) >> 6) << 6; base >= 0; base -= 64) {
        const int32_t j = base + lane;
        SpeedStep f = {kSpeedInf, 0.0};
        if (j < m) {
            f.A = u[j];
            f.c = j + 1 < m ? speed_gain(prm.a_dec, speed_ds(in, j)) : 0.0;
        }
        for (int off = 1; off < 64; off <<= 1) {
            SpeedStep behind;
            behind.A = __shfl_down(f.A, off);
            behind.c = __shfl_down(f.c, off);
            if (lane + off < 64) f = speed_combine(f, behind);
        }
        const double ub = speed_apply(f, carry);
        if (j < m) u[j] = ub;
        carry = __shfl(ub, 0);
    }
    // ---- 3: forward
    carry = kSpeedInf;
    for (int32_t base = 0; base < m; base += 64) {
        const int32_t j = base + lane;
        SpeedStep f = {kSpeedInf, 0.0};
        if (j < m) {
            f.A = u[j];
            f.c = j > 0 ? speed_gain(prm.a_acc, speed_ds(in, j - 1)) : 0.0;
        }
        for (int off = 1; off < 64; off <<= 1) {
            SpeedStep before;
            before.A = __shfl_up(f.A, off);
            before.c = __shfl_up(f.c, off);
            if (lane >= off) f = speed_combine(f, before);
        }
        const double uf = speed_apply(f, carry);
        if (j < m) sp[j] = sqrt(uf);
        carry = __shfl(uf, 63);
    }
}

}  // namespace bcp

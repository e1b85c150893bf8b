// bcp_desc.h -- the two kernel-argument structs that host arithmetic fills without a device in sight: the device copy of the
// parameters and the description of the distance field.  Plain data, no HIP in here: bcp_device.h and bcp_coop.h include it for
// the kernels, bcp_field_plan.h for the host code that plans a map binding (and, through it, a stand-alone host program).
#pragma once

#include <stdint.h>

#include "../../include/bcplan.h"

namespace bcp {

// Device copy of the parameters (kernel argument, lives in SGPRs / scalar cache).
struct DevParams {
    int32_t model, n_verts, dynamic_model, model_front_column_pid, noise_on, iteration_timeout;
    double dt, L, max_wheel_angle, max_wheel_speed, max_lin_acc, max_ang_acc, p_gain;
    double inv_dt, inv_L;    // 1 / dt, 1 / L, correctly rounded (host): div_by_const; directly behind p_gain (step_local_kernel
                             // fetches dt .. inv_L as nine adjacent values)
    double alpha[6];
    double sp, ap, progress_mult;
    double par_thr;          // -sp / 9, utilities/path_tools.py:423
    double sp2_lo, sp2_hi;   // sp^2 (1 -+ 1e-13): dx^2+dy^2 outside this band decides hypot(dx,dy) < sp on its own
    double sp_prune;         // sp nudged up two ulps: |dx| > sp_prune  =>  hypot(dx,dy) >= sp for any faithful hypot
    double qverts[BCP_MAX_VERTS][2];  // footprint / resolution (path_tools.py:145), divided on the host in fp64
    float qbox[4];                    // bounding box of qverts in the robot frame: xmin, xmax, ymin, ymax (pixels)
    int32_t reward_provider;          // BCP_REWARD_*
    int32_t control_delay, pose_delay, state_delay;   // EnvParams delays (envs/base/params.py:28-30)
    float ap_cos_min;                 // cos(ap) - 1e-4 (-2 when ap >= pi): the heading test of the quantised prefilter records
};

constexpr int kMaxSamples = 8;

// distance-field description (kernel argument)
struct CullDesc {
    const uint8_t* edt;   // [(rows + 2 pad) * (cols + 2 pad)] floor(min(clamp, distance to nearest lethal cell))
    int64_t env_stride;   // bytes per env (0: one field shared by all envs)
    int32_t on;           // 0: no distance field -> every in-map pose is AMBIGUOUS
    int32_t pad, width, height;  // padding on each side, padded row width / row count
    int32_t clamp;        // the field saturates at this distance
    int32_t reach;        // any footprint pixel is within `reach` px of the robot pixel (off-map test)
    int32_t n_out, n_in;
    int32_t t_out;        // free  <=>  edt >= t_out at every outer sample
    int32_t t_in[kMaxSamples];   // hit <=  edt <= t_in[j] at inner sample j
    double out_x[kMaxSamples], in_x[kMaxSamples];  // sample abscissae on the robot axis, in pixels
    double axis_y;        // ordinate of the sample axis in the robot frame, in pixels
    // The outer test only asks "is a lethal cell closer than t_out": the field as ONE BIT per cell, in tiles of
    // 32 x 32 cells (32 row words = one 128-byte line each; the samples of a pose lie on a line of <= 2 reach px, so
    // they meet three to five lines instead of one each).  word = near[((y >> 5) * near_tx + (x >> 5)) * 32 + (y & 31)]
    const uint32_t* near;
    int64_t near_stride;  // words per env (0: shared)
    int32_t near_tx, near_words;   // tiles per tile row; words of one entry
    // What step_local_kernel's outer test reads: `near` itself (shift 0), or a copy at 1/2 or 1/4 of the resolution -- a bit
    // of it is the OR of the 2 x 2 / 4 x 4 cells it stands for (near_coarsen_kernel), so "not near" still holds for every
    // one of them.  A 128-byte line then covers 64 x 64 / 128 x 128 cells: the samples of a pose meet fewer lines (each a
    // full line of memory traffic for maps that do not stay in cache), at the price of a few more undecided poses.
    const uint32_t* step_near;
    int64_t step_near_stride;
    int32_t step_near_tx, step_near_shift;
};

}  // namespace bcp

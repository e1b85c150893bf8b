// bcp_track.h -- bcp_track(): K gain settings of a pure-pursuit path tracker per env, each rolled out over up to H trips of
// the noise-free forward model.  The roll-out is bcp_lookahead.h's core (plan_load, plan_trip<true>) and the lane layout is
// lookahead_kernel's; what is new is that the command of a trip is not read from memory but computed from the state the
// previous trip left (bcp_track_law.h).  Nothing of the handle is written; the only global stores are the outputs.
// Included by bcplan.hip after bcp_lookahead.h.
#pragma once

#include "bcp_lookahead.h"
#include "bcp_track_law.h"

// Launch arguments: the handle's parameter block, the caller's pointers (bcp_track_io) and *p by value, nothing that changes
// from call to call -- a captured call replays.
struct TrackArgs {
    const StepStatic* S;
    const double* gains;       // [K][2] or [N][K][2]
    const uint8_t* mask;       // nullptr or [N]
    double* actions;           // [N][K][H][2]
    double* ret;               // [N][K]
    int32_t* steps;
    uint8_t* reason;
    double* final_pose;        // optional [N][K][3]
    int32_t* final_target;     // optional
    int32_t* err;              // optional
    double* trace;             // optional [N][K][H][6]
    int32_t* best;             // optional [N]
    double* best_plan;         // optional [N][H][2]
    void* best_action;         // optional [N][2]
    int64_t n, total;          // N, N * K
    int32_t horizon, k;
    uint32_t flags;            // BCP_STEP_ACTIONS_F32 | BCP_LOOKAHEAD_PER_ENV
    double low[2], high[2], max_curvature;
    const double* profile;     // bcp_track_profile: [max_len] or [entries][max_len] speeds laid out as the bound paths; else nullptr
};

// the device's side of the law's Math parameter (bcp_track_law.h)
struct DeviceTrackMath {
    __device__ __forceinline__ void cos_sin(double a, double& c, double& s) const { bcp::cos_sin(a, c, s); }
    __device__ __forceinline__ double atan(double x) const { return ::atan(x); }
    __device__ __forceinline__ double normalize(double z) const { return normalize_angle(z); }
};

__device__ __forceinline__ void track_gains_of(const TrackArgs& a, int64_t c, int k, double& speed, double& reach)
{
    const GlobalPtr<const double> p = as_global(a.gains) + 2 * ((a.flags & BCP_LOOKAHEAD_PER_ENV) ? c : (int64_t)k);
    speed = p[0];
    reach = p[1];
}

// One lane per (env, setting), settings of an env adjacent, one wavefront per workgroup (collides_wave is a wave-wide call
// and owns the workgroup's dynamic LDS), lanes past N * K shadow the last row and never store: lookahead_kernel's layout.
// Every lane stays in the trip loop until the whole wave is through.  The carrot scan is the one data-dependent loop: a
// lane runs it only while it is active, over the way-point records of its env (the lanes of an env read the same lines);
// the wave rejoins before plan_trip, which every lane calls.
// PROFILE: step 4 of the law reads a.profile, the row of the slot g that plan_load resolves for the env (bcp_track_profile);
// without it the kernel is bcp_track's, a.profile not read.
template <bool PROFILE>
__global__ void __launch_bounds__(kBlock) track_kernel(const TrackArgs a)
{
    const StepStatic* S = a.S;
    const DevParams& P = S->P;
    const int tid = threadIdx.x;
    const int64_t gc = (int64_t)blockIdx.x * kBlock + tid;
    const bool in_range = gc < a.total;
    const int64_t c = in_range ? gc : a.total - 1;
    const int64_t i = c / a.k;
    const int k = (int)(c - i * a.k);
    const bool live = in_range && (!a.mask || as_global(a.mask)[i] != 0);

    const CollisionLds L = collision_lds_setup(P, S->map, tid);

    PlanState st;
    int64_t g;
    const double* pts;
    int m;
    plan_load(S, i, st, g, pts, m);
    double speed, reach;
    track_gains_of(a, c, k, speed, reach);
    const bool tricycle = P.model == BCP_MODEL_TRICYCLE;
    const DeviceTrackMath math;
    GlobalPtr<const double> profile(nullptr);
    if constexpr (PROFILE) profile = as_global(a.profile) + (S->path.shared ? 0 : g * (int64_t)S->path.max_len);

    double ret = 0.0, cmd0 = 0.0, cmd1 = 0.0;
    int steps = 0, reason = 0, errs = 0;
    int carrot = st.target;   // c_prev of the first trip
    // a lane with bad gains is finished before its first trip: steps = 0, reason = 0, ret = 0, zeros in actions and trace
    bool finished = !live || !bcp::track_gains_ok(speed, reach);
    const GlobalPtr<double> act_row = as_global(a.actions) + 2 * c * a.horizon;
    const GlobalPtr<double> trace_row = a.trace ? as_global(a.trace) + 6 * c * a.horizon : GlobalPtr<double>(nullptr);
    const double z[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < a.horizon; ++t) {
        if (__ballot(!finished) == 0) break;   // wave-uniform
        const bool active = !finished;
        if (active) {
            bcp::TrackCommand cmd;
            if constexpr (PROFILE)
                cmd = bcp::track_law_profile(as_global(pts), profile, m, st.r.p.x, st.r.p.y, st.r.p.th, st.r.wheel, st.target, carrot,
                                             speed, reach, a.max_curvature, tricycle, P.max_wheel_angle, P.L, a.low, a.high, math);
            else
                cmd = bcp::track_law(as_global(pts), m, st.r.p.x, st.r.p.y, st.r.p.th, st.r.wheel, st.target, carrot, speed, reach,
                                     a.max_curvature, tricycle, P.max_wheel_angle, P.L, a.low, a.high, math);
            if (a.trace) {   // the state as the law read it
                const GlobalPtr<double> q = trace_row + 6 * t;
                q[0] = st.r.p.x;
                q[1] = st.r.p.y;
                q[2] = st.r.p.th;
                q[3] = st.r.wheel;
                q[4] = (double)st.target;
                q[5] = (double)cmd.carrot;
            }
            carrot = cmd.carrot;
            cmd0 = cmd.cmd0;
            cmd1 = cmd.cmd1;
            act_row[2 * t + 0] = cmd0;
            act_row[2 * t + 1] = cmd1;
        }
        plan_trip<true>(S, L, g, pts, m, cmd0, cmd1, z, false, active, st, ret, errs, reason, finished);
        if (active) steps = t + 1;
    }
    if (!live) return;
    // after the done step: the last command repeated (the plan lies inside the box everywhere), the trace zeros
    for (int t = steps; t < a.horizon; ++t) {
        act_row[2 * t + 0] = cmd0;
        act_row[2 * t + 1] = cmd1;
        if (a.trace) {
#pragma unroll
            for (int f = 0; f < 6; ++f) trace_row[6 * t + f] = 0.0;
        }
    }
    as_global(a.ret)[c] = ret;
    as_global(a.steps)[c] = steps;
    as_global(a.reason)[c] = (uint8_t)reason;
    if (a.final_pose) {
        as_global(a.final_pose)[3 * c + 0] = st.r.p.x;
        as_global(a.final_pose)[3 * c + 1] = st.r.p.y;
        as_global(a.final_pose)[3 * c + 2] = st.r.p.th;
    }
    if (a.final_target) as_global(a.final_target)[c] = st.target;
    if (a.err) as_global(a.err)[c] = errs;
}

// best / best_plan / best_action: lookahead_best_kernel's reduction with the same key order (best_key_before: free before
// collided, then ret, lowest k on ties); a setting whose gains the law refuses takes free_ = -1, behind every collided one.
// After the butterfly every lane of the group holds the winner, and the group copies its plan.
__global__ void __launch_bounds__(256) track_best_kernel(const TrackArgs a, int group)
{
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = gid / group;
    const int sub = (int)(gid - i * group);
    const bool live = i < a.n && (!a.mask || as_global(a.mask)[i] != 0);
    BestKey b = {-1, 0, 0.0};
    if (live) {
        for (int k = sub; k < a.k; k += group) {
            const int64_t c = i * a.k + k;
            double speed, reach;
            track_gains_of(a, c, k, speed, reach);
            const int free_ = !bcp::track_gains_ok(speed, reach) ? -1 : (as_global(a.reason)[c] & BCP_DONE_COLLIDED) ? 0 : 1;
            const BestKey x = {k, free_, as_global(a.ret)[c]};
            if (best_key_before(x, b)) b = x;
        }
    }
    for (int off = group >> 1; off > 0; off >>= 1) {
        BestKey o;
        o.k = __shfl_xor(b.k, off);
        o.free_ = __shfl_xor(b.free_, off);
        o.ret = __shfl_xor(b.ret, off);
        if (best_key_before(o, b)) b = o;
    }
    if (!live) return;
    const GlobalPtr<const double> plan = as_global(const_cast<const double*>(a.actions)) + 2 * (i * a.k + b.k) * a.horizon;
    if (a.best_plan) {
        for (int e = sub; e < 2 * a.horizon; e += group) as_global(a.best_plan)[2 * i * a.horizon + e] = plan[e];
    }
    if (sub != 0) return;
    as_global(a.best)[i] = b.k;
    if (a.best_action) {
        if (a.flags & BCP_STEP_ACTIONS_F32) {
            as_global(reinterpret_cast<float*>(a.best_action))[2 * i + 0] = (float)plan[0];
            as_global(reinterpret_cast<float*>(a.best_action))[2 * i + 1] = (float)plan[1];
        } else {
            as_global(reinterpret_cast<double*>(a.best_action))[2 * i + 0] = plan[0];
            as_global(reinterpret_cast<double*>(a.best_action))[2 * i + 1] = plan[1];
        }
    }
}

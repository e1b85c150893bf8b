// bcp_lookahead.h -- the roll-out core of the planning kernels (PlanState, plan_load, plan_trip: one PlanEnv.step on a
// private copy of an env's state that lives in registers), and bcp_lookahead(): K candidate action sequences per env, each
// taking up to H such trips.  Nothing of the handle is written; the only global stores are the outputs.
// Included by bcplan.hip after bcp_step.h, whose device functions (robot model, collides_wave, reward providers) it is
// built from -- none of the step kernels' hand-off machinery (tickets, parking, alternating counters) is involved.
// bcp_mppi.h rolls its candidates out with the same core.
#pragma once

#include "bcp_step.h"

// ---- the roll-out core -----------------------------------------------------------------------------------------------
// What a trip advances: the part of an env's state that PlanEnv.step changes when no delay queue exists.
struct PlanState {
    Robot r;
    double min_dist;
    int target, iter;
    bool collided;
};

// Env i's state as it is bound to the handle, its slot g (map / path / pool entry), its way points and their count.  The
// lanes of one env read the same addresses: a broadcast load each.
__device__ __forceinline__ void plan_load(const StepStatic* S, int64_t i, PlanState& st, int64_t& g, const double*& pts, int& m)
{
    const bool tri = S->P.model == BCP_MODEL_TRICYCLE;
    st.r.p.x = as_global(S->st.x)[i];
    st.r.p.y = as_global(S->st.y)[i];
    st.r.p.th = as_global(S->st.angle)[i];
    st.r.v = as_global(S->st.v)[i];
    st.r.w = as_global(S->st.w)[i];
    st.r.steer = tri ? as_global(S->st.steer)[i] : 0.0;
    st.r.wheel = tri ? as_global(S->st.wheel)[i] : 0.0;
    st.min_dist = as_global(S->st.min_dist)[i];
    st.target = as_global(S->st.target_idx)[i];
    st.iter = as_global(S->st.cur_iter)[i];
    st.collided = as_global(S->st.collided)[i] != 0;
    g = S->geom_of_env ? (int64_t)as_global(S->geom_of_env)[i] : i;   // slot_of
    pts = S->path.pts + (S->path.shared ? 0 : g * (int64_t)S->path.max_len * 5);
    m = S->path.shared ? S->path.max_len : S->path.lens[g];
}

// One trip: PlanEnv.step without the stores -- _env_step (envs/base/env.py:442-461: robot, collision, roll-back), iter + 1,
// reward (:352), done (:400-419) -- in the order and by the laws of finalize_env_from, minus delay queues (refused by the
// host), reset and record.  This is the one statement of that sequence outside the step kernels, which stay as they are
// (bcp_step.h); test_bitwise_equal_to_the_step_on_a_twin_handle holds it to them bit for bit.
// Wave-uniform: every lane of the wave calls it, because collides_wave settles ambiguous poses with the whole wave; a lane
// with active = false (finished, masked out, past the end of the grid) keeps st, ret, errs, reason and finished as they are.
// PLAIN: continuous reward provider and no noise_z -- the pure-pursuit branch and kinematic_step_noise are compiled out.
// noisy_model false is the noise-free forward model, whatever the handle's noise_on; z is then not read.
template <bool PLAIN>
__device__ __forceinline__ void plan_trip(const StepStatic* S, const CollisionLds& L, int64_t g, const double* pts, int m,
                                          double cmd0, double cmd1, const double z[3], bool noisy_model, bool active,
                                          PlanState& st, double& ret, int& errs, int& reason, bool& finished)
{
    const DevParams& P = S->P;
    const bool pure_pursuit = !PLAIN && P.reward_provider == BCP_REWARD_PURE_PURSUIT;
    Robot nr = st.r;
    int drawn = 0;
    RobotDrive d = robot_step_begin(P, nr, cmd0, cmd1);
    if (!noisy_model) d.noisy = false;   // kinematic_step, not kinematic_step_noise fed with zeros
    const int e = robot_step_end(P, nr, d, z, drawn);
    const bool hit = collides_wave(P, S->map, S->cull, L, S->exact_mode, S->dense_threshold, S->wide != 0, active, g,
                                   nr.p.x, nr.p.y, nr.p.th);
    if (!active) return;
    if (hit) {   // robot.set_pose(*old_position): pose restored, v = w = 0 (tricycle_model.py:471-476)
        nr.p = st.r.p;
        nr.v = 0.0;
        nr.w = 0.0;
    }
    st.r = nr;
    st.iter += 1;
    st.collided = st.collided || hit;
    double rew;
    bool goal;
    if (pure_pursuit) {
        rew = reward_pure_pursuit(pts, m, nr.p.x, nr.p.y, st.collided, st.min_dist, st.target);
        goal = hypot(pts[5 * (m - 1)] - nr.p.x, pts[5 * (m - 1) + 1] - nr.p.y) < 1.0;   // done(), reward.py:141-150
    } else {
        const PathWindow w = path_window_of(P, S->path.shared != 0, S->path.bbox, S->path.index, g, nr.p.x, nr.p.y);
        rew = reward_step<4>(P, pts, w, m, nr.p.x, nr.p.y, nr.p.th, st.min_dist, st.target);
        goal = st.target > m - 1;
    }
    const bool timeout = st.iter >= P.iteration_timeout;
    ret += rew;
    errs |= e;
    if (goal || timeout || st.collided) {
        reason = (goal ? BCP_DONE_GOAL : 0) | (timeout ? BCP_DONE_TIMEOUT : 0) | (st.collided ? BCP_DONE_COLLIDED : 0);
        finished = true;
    }
}

// ---- bcp_lookahead ---------------------------------------------------------------------------------------------------

// Launch arguments: the handle's parameter block and the caller's pointers (bcp_lookahead_io), nothing that changes from
// call to call -- a captured call replays.
struct LookaheadArgs {
    const StepStatic* S;
    const void* actions;       // [H][K][2] or [H][N][K][2]
    const double* noise_z;     // nullptr or [H][N][K][3]
    const uint8_t* mask;       // nullptr or [N]
    double* ret;               // [N][K]
    int32_t* steps;
    uint8_t* reason;
    double* final_pose;        // optional [N][K][3]
    int32_t* final_target;     // optional
    int32_t* err;              // optional
    int32_t* best;             // optional [N]
    void* best_action;         // optional [N][2]
    int64_t n, total;          // N, N * K
    int32_t horizon, k;
    uint32_t flags;            // BCP_STEP_ACTIONS_F32 | BCP_LOOKAHEAD_PER_ENV
};

// step t of candidate k of env i, float32 or float64, widened like load_env does
__device__ __forceinline__ void lookahead_action(const LookaheadArgs& a, int64_t row, double& cmd0, double& cmd1)
{
    if (a.flags & BCP_STEP_ACTIONS_F32) {
        const GlobalPtr<const float> p = as_global(reinterpret_cast<const float*>(a.actions)) + 2 * row;
        cmd0 = (double)p[0];
        cmd1 = (double)p[1];
    } else {
        const GlobalPtr<const double> p = as_global(reinterpret_cast<const double*>(a.actions)) + 2 * row;
        cmd0 = p[0];
        cmd1 = p[1];
    }
}

// One lane per (env, candidate), candidates of an env adjacent: lane c of the grid holds candidate c % K of env c / K, so
// with K >= 64 a wave is 64 candidates of ONE env (its state is one broadcast load; map tiles, path window and footprint
// are the same lines for the whole wave) and with K < 64 a wave holds 64 / K envs.  One wavefront per workgroup, like
// step_kernel: collides_wave settles ambiguous poses with the whole wave and owns the workgroup's dynamic LDS.
// PLAIN: plan_trip's -- the host picks it when the provider is the continuous one and no noise_z is given.
template <bool PLAIN>
__global__ void __launch_bounds__(kBlock) lookahead_kernel(const LookaheadArgs a)
{
    const StepStatic* S = a.S;
    const DevParams& P = S->P;
    const int tid = threadIdx.x;
    const int64_t gc = (int64_t)blockIdx.x * kBlock + tid;
    const bool in_range = gc < a.total;
    const int64_t c = in_range ? gc : a.total - 1;   // lanes past N * K shadow the last candidate and never store
    const int64_t i = c / a.k;
    const int k = (int)(c - i * a.k);
    const bool live = in_range && (!a.mask || as_global(a.mask)[i] != 0);

    const CollisionLds L = collision_lds_setup(P, S->map, tid);

    const bool noisy_model = !PLAIN && a.noise_z != nullptr;
    const bool per_env = (a.flags & BCP_LOOKAHEAD_PER_ENV) != 0;
    PlanState st;   // the env's state, once
    int64_t g;
    const double* pts;
    int m;
    plan_load(S, i, st, g, pts, m);

    double ret = 0.0;
    int steps = 0, reason = 0, errs = 0;
    bool finished = !live;
    // Every lane stays in the loop until the whole wave is through (plan_trip is a wave-wide call); a lane that is
    // finished, masked out or past N * K passes active = false and keeps its results as they are.
    for (int t = 0; t < a.horizon; ++t) {
        if (__ballot(!finished) == 0) break;   // wave-uniform
        const bool active = !finished;
        const int64_t wide_row = ((int64_t)t * a.n + i) * a.k + k;
        double cmd0, cmd1;
        lookahead_action(a, per_env ? wide_row : (int64_t)t * a.k + k, cmd0, cmd1);
        double z[3] = {0.0, 0.0, 0.0};
        if (noisy_model) {
            z[0] = as_global(a.noise_z)[3 * wide_row + 0];
            z[1] = as_global(a.noise_z)[3 * wide_row + 1];
            z[2] = as_global(a.noise_z)[3 * wide_row + 2];
        }
        plan_trip<PLAIN>(S, L, g, pts, m, cmd0, cmd1, z, noisy_model, active, st, ret, errs, reason, finished);
        if (active) steps = t + 1;
    }
    if (!live) return;
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

// best / best_action: the candidate of each env with the largest key (free before collided, then ret), lowest k on ties.
// `group` lanes (a power of two <= 64, chosen by the host from K) share an env: each scans k = lane, lane + group, .. in
// ascending order, then the group reduces with shuffles.  Keys are compared, never added: the result does not depend on
// the order of the reduction.  Every lane takes part in every shuffle (an env past N or masked out holds "none").
struct BestKey {
    int k, free_;
    double ret;
};

__device__ __forceinline__ bool best_key_before(const BestKey& x, const BestKey& y)   // x wins over y
{
    if (x.k < 0) return false;
    if (y.k < 0) return true;
    if (x.free_ != y.free_) return x.free_ > y.free_;
    if (x.ret != y.ret) return x.ret > y.ret;
    return x.k < y.k;
}

__global__ void __launch_bounds__(256) lookahead_best_kernel(const LookaheadArgs a, int group)
{
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = gid / group;
    const int sub = (int)(gid - i * group);
    const bool live = i < a.n && (!a.mask || as_global(a.mask)[i] != 0);
    BestKey b = {-1, 0, 0.0};
    if (live) {
        for (int k = sub; k < a.k; k += group) {
            const int64_t c = i * a.k + k;
            const BestKey x = {k, (as_global(a.reason)[c] & BCP_DONE_COLLIDED) ? 0 : 1, as_global(a.ret)[c]};
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
    if (!live || sub != 0) return;
    as_global(a.best)[i] = b.k;
    if (a.best_action) {   // step 0 of the winner, in the dtype of `actions`
        const int64_t row = (a.flags & BCP_LOOKAHEAD_PER_ENV) ? i * a.k + b.k : (int64_t)b.k;
        if (a.flags & BCP_STEP_ACTIONS_F32) {
            const GlobalPtr<const float> p = as_global(reinterpret_cast<const float*>(a.actions)) + 2 * row;
            as_global(reinterpret_cast<float*>(a.best_action))[2 * i + 0] = p[0];
            as_global(reinterpret_cast<float*>(a.best_action))[2 * i + 1] = p[1];
        } else {
            const GlobalPtr<const double> p = as_global(reinterpret_cast<const double*>(a.actions)) + 2 * row;
            as_global(reinterpret_cast<double*>(a.best_action))[2 * i + 0] = p[0];
            as_global(reinterpret_cast<double*>(a.best_action))[2 * i + 1] = p[1];
        }
    }
}

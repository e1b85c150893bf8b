// bcp_mppi.h -- bcp_mppi(): sampling-based refinement of one plan per env (MPPI), I iterations of sample -> roll out ->
// weight -> update inside ONE launch.  Included by bcplan.hip after bcp_lookahead.h, whose roll-out core (plan_load,
// plan_trip) takes the trips: a candidate is rolled out by the very code lookahead_kernel runs.  Candidate actions are not
// read from memory but made in registers: mean + sigma * eps, clipped to the action box.
// Nothing of the handle is written; the only global stores are the caller's outputs (bcp_mppi_io).
// bcp_mppi_field() is the same launch with one read more per candidate: the goal field (bcp_goal_field) at the pose the
// candidate ended on, taken off its score as a distance to go (mppi_kernel<.., FIELD>; the cell rule is bcp_goal_cell.h's).
// bcp_mppi_adapt() is the same launch again with a width per (env, step, component) in the caller's `sigma` array in place
// of the two of bcp_mppi_params, each moved towards the weighted spread of its commands after every iteration
// (mppi_kernel<.., ADAPT>; the clamp and the move are bcp_mppi_widths.h's).
#pragma once

#include "bcp_goal_cell.h"
#include "bcp_lookahead.h"
#include "bcp_mppi_widths.h"

// Launch arguments: the handle's parameter block, the caller's pointers and bcp_mppi_params by value -- nothing that the
// library changes from call to call, so a captured call replays (fresh perturbations come from *draw_index).
struct MppiArgs {
    const StepStatic* S;
    bcp_mppi_params p;
    double* mean;                // [N][H][2], in / out
    void* action;                // [N][2]
    const uint8_t* mask;         // nullptr or [N]
    const float* eps_in;         // nullptr or [I][N][K][H][2]
    float* eps_out;              // nullptr or same
    const uint64_t* draw_index;  // nullptr or one device word
    double* iter_mean;           // nullptr or [I][N][H][2]
    double* iter_ret;            // nullptr or [I][N][K]
    uint8_t* iter_reason;        // nullptr or [I][N][K]
    int32_t* err;                // nullptr or [N]
    int64_t n;
    int32_t score_word;          // where the score area starts in the dynamic LDS (32-bit words, even), behind collides_wave's
    uint32_t flags;              // BCP_STEP_ACTIONS_F32
};

// What bcp_mppi_field adds to a launch: a finished goal field (bcp_goal_field) and the map binding's frame as
// goal_sample_kernel takes it (bcp_goal.h), so that a candidate's final pose reads the cell bcp_goal_field_sample would read.
struct MppiTerminal {
    const uint16_t* field;       // [n_fields][rows][cols]
    int64_t field_stride;        // rows * cols, or 0 when n_fields == 1: every env reads field 0
    int64_t n_entries;           // pool entries, or n_envs without a pool: a slot outside [0, n_entries) reads nothing
    const int32_t* valid_rows;   // per entry, or nullptr: the allocated shape
    const int32_t* valid_cols;
    const double* origins;       // per entry, or nullptr: (ox, oy)
    double ox, oy, inv_res, resolution;
    double weight;               // reward per metre of distance to go
    int32_t* iter_value;         // nullptr or [I][N][K]
    double* iter_score;          // nullptr or [I][N][K]
    int32_t rows, cols, shared;
};

// What bcp_mppi_adapt adds to a launch: the widths, their clamps and the rate.
struct MppiWidths {
    double* sigma;               // [N][H][2], in / out
    double* iter_sigma;          // nullptr or [I][N][H][2]
    double lo[2], hi[2];         // sigma_min, sigma_max
    double rate;
};

// The kernel's argument: MppiArgs as it is, and behind it the terminal part for the FIELD kernels and the widths for the
// ADAPT kernels only -- the plain ones take what they always took.
template <bool FIELD, bool ADAPT> struct MppiKernelArgs;
template <> struct MppiKernelArgs<false, false> {
    MppiArgs m;
};
template <> struct MppiKernelArgs<true, false> {
    MppiArgs m;
    MppiTerminal t;
};
template <> struct MppiKernelArgs<false, true> {
    MppiArgs m;
    MppiWidths w;
};
template <> struct MppiKernelArgs<true, true> {
    MppiArgs m;
    MppiTerminal t;
    MppiWidths w;
};

struct MppiFieldGet {
    GlobalPtr<const uint16_t> p;
    int32_t cols;
    __device__ __forceinline__ uint16_t operator()(int32_t r, int32_t c) const { return p[r * cols + c]; }
};

// The field value at a candidate's final pose (x, y) of an env on slot g: the rule of goal_sample_kernel -- the map frame is
// entry 0's when the map is shared, the field is the slot's unless there is only one -- through goal_value_at.  One global
// 2-byte load at most.
__device__ __forceinline__ int32_t mppi_terminal_value(const MppiTerminal& t, int64_t g, double x, double y)
{
    if (g < 0 || g >= t.n_entries) return kGoalNone;
    const int64_t e = t.shared ? 0 : g;
    const double ox = t.origins ? as_global(t.origins)[2 * e] : t.ox, oy = t.origins ? as_global(t.origins)[2 * e + 1] : t.oy;
    const int32_t vr = t.valid_rows ? max(0, min(as_global(t.valid_rows)[e], t.rows)) : t.rows;
    const int32_t vc = t.valid_cols ? max(0, min(as_global(t.valid_cols)[e], t.cols)) : t.cols;
    const double lim = 1.7976931348623157e308;
    const bool finite = x >= -lim && x <= lim && y >= -lim && y <= lim;
    const MppiFieldGet get = {as_global(t.field) + g * t.field_stride, t.cols};
    return goal_value_at(get, vr, vc, x, y, finite, ox, oy, t.inv_res);
}

// The two perturbations of (env, draw, iteration j, candidate k, step t): Philox4x32-10 keyed by the seed on the counter
//   c0 = env (low word), c1 = k | env (high bits) << 10 | draw (bits 32..51) << 12, c2 = j * H + t, c3 = draw (low word)
// (distinct for draws below 2^52 and I * H <= 2^32), then ONE float32 Box-Muller pair on the top 24 bits of two words:
// u = (m + 1/2) 2^-24 in (0, 1], r = sqrt(-2 ln u) <= 5.89, angle 2 pi m' 2^-24 through sincospi.  A function of its
// arguments alone: the update pass calls it again for the values the roll-out pass used instead of keeping K * H of them.
__device__ __forceinline__ void mppi_draw(uint64_t seed, uint64_t env, uint64_t draw, uint32_t jt, int k, float& e0, float& e1)
{
    uint32_t c[4] = {(uint32_t)env, (uint32_t)k | ((uint32_t)(env >> 32) << 10) | ((uint32_t)(draw >> 32) << 12), jt,
                     (uint32_t)draw};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u = ((float)(c[0] >> 8) + 0.5f) * 5.9604644775390625e-08f;   // 2^-24
    const float r = sqrtf(-2.0f * logf(u));
    float sn, cs;
    sincospif(2.0f * ((float)(c[1] >> 8) * 5.9604644775390625e-08f), &sn, &cs);
    e0 = r * cs;
    e1 = r * sn;
}

// u = min(max(mean + sigma * eps, low), high): one product, one sum, two comparisons, each rounded on its own
__device__ __forceinline__ double mppi_command(double mean, double sigma, float eps, double low, double high)
{
    double u = mean + sigma * (double)eps;
    u = u < low ? low : u;
    return u > high ? high : u;
}

// The width of component d at element `row` = env * H + t of the caller's array, clamped as it is read (ADAPT).
__device__ __forceinline__ double mppi_width(const MppiWidths& w, int64_t row, int d)
{
    return mppi_clamp_width(as_global(w.sigma)[row * 2 + d], w.lo[d], w.hi[d]);
}

// The two perturbations of candidate k at step t of iteration j (c = (j * N + env) * K + k): read from eps_in or drawn;
// candidate 0 has none.  What the update's second walk (ADAPT) makes again.
__device__ __forceinline__ void mppi_eps(const MppiArgs& a, int64_t env, uint64_t draw, int j, int t, int k, float& e0, float& e1)
{
    const int H = a.p.horizon;
    e0 = e1 = 0.0f;
    if (k == 0) return;
    if (a.eps_in) {
        const int64_t c = ((int64_t)j * a.n + env) * a.p.n_candidates + k;
        e0 = as_global(a.eps_in)[(c * H + t) * 2 + 0];
        e1 = as_global(a.eps_in)[(c * H + t) * 2 + 1];
    } else {
        mppi_draw(a.p.seed, (uint64_t)env, draw, (uint32_t)j * (uint32_t)H + (uint32_t)t, k, e0, e1);
    }
}

// One wavefront per workgroup (collides_wave is wave-wide and owns the dynamic LDS up to score_word).  With K >= 64 the
// workgroup is ONE env: its K / 64 chunks of candidates are rolled out one after another by the same lanes (lane l holds
// k = chunk * 64 + l), so the env's state is loaded once and everything the update needs stays in the wave.  With K < 64
// the wave holds 64 / K envs, and the reductions run over groups of K adjacent lanes (xor shuffles: every lane of a group
// ends with the same bits, whatever its position).
// The mean lives in the caller's `mean` array, not in LDS: the rows of an env are read and written by the one wave that
// owns the env, a lane's row is one broadcast load per trip (all lanes of an env read the same 16 bytes, L1-resident:
// H * 16 bytes per env), and an LDS copy of 64 / K envs x H rows would sit on top of the ~14 KB collision area that already
// bounds the waves per CU.  Row t is replaced in place as soon as its weighted sum is known (nothing reads the old row t
// afterwards); a workgroup barrier -- one wave: a fence -- orders an iteration's stores before the next one's loads.
// Scores: one double per (lane, chunk) in LDS behind the collision area (K >= 64: K * 8 bytes; K < 64: 512), written
// and read by the same lane; they turn into the weights in place.  The update needs every u[t] again after the weights
// are known: the perturbation is drawn again from its counter (or read again from eps_in).
// FIELD (bcp_mppi_field): after its last trip a live lane reads the goal field at the pose it ended on -- the rolled-back
// pose where it collided, bcp_lookahead's final_pose -- and its score loses weight * metres to go, a pose without a route
// counting as kGoalFar cells.  Nothing else differs: iter_ret and iter_reason stay the pure return and reason.
// ADAPT (bcp_mppi_adapt): the widths live in the caller's `sigma` array as the mean lives in `mean` -- row t is one broadcast
// load per trip, clamped as it is read (a row the kernel wrote is inside the clamps already, so only what the caller passed
// in changes under it).  The variance of row t needs the new mean of row t, so the update walks the lane's chunks a second
// time for that row: the commands of every chunk but the last are made again from their counters (or read again from
// eps_in), the last chunk's are still in registers -- the same bits either way, mppi_command is a function of its arguments.
// The same butterflies reduce the two sums, the lane with kl == 0 replaces the row in place, and the barrier that ends the
// iteration orders it like the mean's.  No LDS beyond the scores, no atomics.
// The second walk fetches through mppi_eps; the roll-out and the first walk carry the same fetch inline, and the choice of
// s0, s1 is written out in both.  That is measured, not taste (profiles/mppi_one_path.txt): with all three fetches through
// mppi_eps and one mppi_widths_at, bcp_mppi at N = 4096, K = 64, H = 16, I = 4 took 3.97 ms against 3.93 ms and
// bcp_mppi_adapt 4.21 against 4.13; with only the roll-out's block back 4.04, with only the first walk's 4.08; with both
// back and only the widths in a function 4.05.  These ~14 k-instruction kernels change their schedule with any edit of the
// body, so a change to the [I][N][K][H][2] layout has three places to find: here (mppi_eps) and the two blocks below.
// Loops are bounded by I, H and K / 64; no atomics, no waits on other workgroups.
template <bool PLAIN, bool FIELD, bool ADAPT>
__global__ void __launch_bounds__(kBlock) mppi_kernel(const MppiKernelArgs<FIELD, ADAPT> ka)
{
    const MppiArgs& a = ka.m;
    typedef __attribute__((address_space(3))) double* LdsScore;
    const StepStatic* S = a.S;
    const DevParams& P = S->P;
    const int tid = threadIdx.x;
    const int K = a.p.n_candidates, H = a.p.horizon;
    const int group = K < kBlock ? K : kBlock;    // lanes that share an env (a power of two, the host checked K)
    const int chunks = K / group;
    const int64_t i_raw = (int64_t)blockIdx.x * (kBlock / group) + tid / group;
    const bool in_range = i_raw < a.n;
    const int64_t i = in_range ? i_raw : a.n - 1;   // lanes past N shadow the last env and never store
    const int kl = tid & (group - 1);
    const bool live = in_range && (!a.mask || as_global(a.mask)[i] != 0);

    const CollisionLds L = collision_lds_setup(P, S->map, tid);
    const LdsScore score = (LdsScore)(lds_dyn + a.score_word) + tid;   // chunk ch at score[ch * kBlock]

    PlanState st0;   // the env's state, once for all iterations and chunks
    int64_t g;
    const double* pts;
    int m;
    plan_load(S, i, st0, g, pts, m);

    const uint64_t draw = a.draw_index ? *as_global(a.draw_index) : a.p.draw_index;
    const GlobalPtr<double> mean = as_global(a.mean) + i * H * 2;
    const double zero3[3] = {0.0, 0.0, 0.0};
    int errs = 0;
    double first0 = 0.0, first1 = 0.0;   // row 0 of the newest mean

    for (int j = 0; j < a.p.iterations; ++j) {
        if (a.iter_mean && live)
            for (int e = kl; e < 2 * H; e += group) as_global(a.iter_mean)[((int64_t)j * a.n + i) * H * 2 + e] = mean[e];
        if constexpr (ADAPT) {
            if (ka.w.iter_sigma && live)
                for (int e = kl; e < 2 * H; e += group)
                    as_global(ka.w.iter_sigma)[((int64_t)j * a.n + i) * H * 2 + e] = mppi_width(ka.w, i * H + (e >> 1), e & 1);
        }
        // ---- roll-outs: plan_trip on a copy of the state, one chunk of candidates at a time
        double best = -INFINITY;
        for (int ch = 0; ch < chunks; ++ch) {
            const int k = ch * kBlock + kl;
            const int64_t c = ((int64_t)j * a.n + i) * K + k;   // [I][N][K]
            PlanState st = st0;
            double ret = 0.0;
            int reason = 0;
            bool finished = !live;
            for (int t = 0; t < H; ++t) {
                // the perturbations are made (and written to eps_out) for every step, taken or not: the update uses them all
                float e0 = 0.0f, e1 = 0.0f;
                if (a.eps_in) {
                    if (k != 0) {
                        e0 = as_global(a.eps_in)[(c * H + t) * 2 + 0];
                        e1 = as_global(a.eps_in)[(c * H + t) * 2 + 1];
                    }
                } else if (k != 0) {
                    mppi_draw(a.p.seed, (uint64_t)i, draw, (uint32_t)j * (uint32_t)H + (uint32_t)t, k, e0, e1);
                }
                if (a.eps_out && live) {
                    as_global(a.eps_out)[(c * H + t) * 2 + 0] = e0;
                    as_global(a.eps_out)[(c * H + t) * 2 + 1] = e1;
                }
                if (__ballot(!finished) == 0) {   // wave-uniform
                    if (a.eps_out) continue;
                    break;
                }
                const bool active = !finished;
                double s0 = a.p.sigma[0], s1 = a.p.sigma[1];
                if constexpr (ADAPT) {
                    s0 = mppi_width(ka.w, i * H + t, 0);
                    s1 = mppi_width(ka.w, i * H + t, 1);
                }
                const double cmd0 = mppi_command(mean[2 * t + 0], s0, e0, a.p.low[0], a.p.high[0]);
                const double cmd1 = mppi_command(mean[2 * t + 1], s1, e1, a.p.low[1], a.p.high[1]);
                plan_trip<PLAIN>(S, L, g, pts, m, cmd0, cmd1, zero3, false, active, st, ret, errs, reason, finished);
            }
            if (live) {
                if (a.iter_ret) as_global(a.iter_ret)[c] = ret;
                if (a.iter_reason) as_global(a.iter_reason)[c] = (uint8_t)reason;
            }
            double s = (reason & BCP_DONE_COLLIDED) ? ret - a.p.collision_penalty : ret;
            if constexpr (FIELD) {
                const MppiTerminal& T = ka.t;
                const int32_t v = live ? mppi_terminal_value(T, g, st.r.p.x, st.r.p.y) : kGoalNone;
                s = s - T.weight * goal_metres(v == kGoalNone ? kGoalFar : v, T.resolution);
                if (live) {
                    if (T.iter_value) as_global(T.iter_value)[c] = v;
                    if (T.iter_score) as_global(T.iter_score)[c] = s;
                }
            }
            score[ch * kBlock] = s;
            best = s > best ? s : best;
        }
        // ---- weights: w_k = exp((s_k - max s) / lambda) / sum, over the lane's chunks and then the group's lanes
        for (int off = group >> 1; off > 0; off >>= 1) {
            const double o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        double total = 0.0;
        for (int ch = 0; ch < chunks; ++ch) {
            const double w = exp((score[ch * kBlock] - best) / a.p.lambda_);
            score[ch * kBlock] = w;
            total += w;
        }
        for (int off = group >> 1; off > 0; off >>= 1) total += __shfl_xor(total, off);
        for (int ch = 0; ch < chunks; ++ch) score[ch * kBlock] = score[ch * kBlock] / total;
        // ---- update: mean[t] = sum_k w_k u_k[t], the commands made again from their counters
        for (int t = 0; t < H; ++t) {
            const double m0 = mean[2 * t + 0], m1 = mean[2 * t + 1];
            double s0 = a.p.sigma[0], s1 = a.p.sigma[1];
            if constexpr (ADAPT) {
                s0 = mppi_width(ka.w, i * H + t, 0);
                s1 = mppi_width(ka.w, i * H + t, 1);
            }
            double acc0 = 0.0, acc1 = 0.0;
            double u0 = 0.0, u1 = 0.0;   // (after the loop: the last chunk's commands)
            for (int ch = 0; ch < chunks; ++ch) {
                const int k = ch * kBlock + kl;
                float e0 = 0.0f, e1 = 0.0f;   // (mppi_eps written out, as in the roll-out: see above the kernel)
                if (a.eps_in) {
                    if (k != 0) {
                        const int64_t c = ((int64_t)j * a.n + i) * K + k;
                        e0 = as_global(a.eps_in)[(c * H + t) * 2 + 0];
                        e1 = as_global(a.eps_in)[(c * H + t) * 2 + 1];
                    }
                } else if (k != 0) {
                    mppi_draw(a.p.seed, (uint64_t)i, draw, (uint32_t)j * (uint32_t)H + (uint32_t)t, k, e0, e1);
                }
                const double w = score[ch * kBlock];
                u0 = mppi_command(m0, s0, e0, a.p.low[0], a.p.high[0]);
                u1 = mppi_command(m1, s1, e1, a.p.low[1], a.p.high[1]);
                acc0 += w * u0;
                acc1 += w * u1;
            }
            for (int off = group >> 1; off > 0; off >>= 1) {
                acc0 += __shfl_xor(acc0, off);
                acc1 += __shfl_xor(acc1, off);
            }
            if (live && kl == 0) {
                mean[2 * t + 0] = acc0;
                mean[2 * t + 1] = acc1;
            }
            if constexpr (ADAPT) {
                // ---- widths: sd = sqrt(sum_k w_k (u_k - m')^2) about the row's new mean, then the move towards it.  The
                // last chunk's commands are still in u0, u1; the others are made again
                double v0 = 0.0, v1 = 0.0;
                for (int ch = 0; ch < chunks; ++ch) {
                    double x0 = u0, x1 = u1;
                    if (ch != chunks - 1) {
                        float e0, e1;
                        mppi_eps(a, i, draw, j, t, ch * kBlock + kl, e0, e1);
                        x0 = mppi_command(m0, s0, e0, a.p.low[0], a.p.high[0]);
                        x1 = mppi_command(m1, s1, e1, a.p.low[1], a.p.high[1]);
                    }
                    const double w = score[ch * kBlock];
                    const double d0 = x0 - acc0, d1 = x1 - acc1;
                    v0 += w * (d0 * d0);
                    v1 += w * (d1 * d1);
                }
                for (int off = group >> 1; off > 0; off >>= 1) {
                    v0 += __shfl_xor(v0, off);
                    v1 += __shfl_xor(v1, off);
                }
                if (live && kl == 0) {
                    const GlobalPtr<double> sg = as_global(ka.w.sigma) + (i * H + t) * 2;
                    sg[0] = mppi_next_width(s0, sqrt(v0), ka.w.rate, ka.w.lo[0], ka.w.hi[0]);
                    sg[1] = mppi_next_width(s1, sqrt(v1), ka.w.rate, ka.w.lo[1], ka.w.hi[1]);
                }
            }
            if (t == 0) {
                first0 = acc0;
                first1 = acc1;
            }
        }
        __syncthreads();   // this iteration's rows before the next one's loads (one wave per workgroup)
    }
    for (int off = group >> 1; off > 0; off >>= 1) errs |= __shfl_xor(errs, off);
    if (!live || kl != 0) return;
    if (a.flags & BCP_STEP_ACTIONS_F32) {
        as_global(reinterpret_cast<float*>(a.action))[2 * i + 0] = (float)first0;
        as_global(reinterpret_cast<float*>(a.action))[2 * i + 1] = (float)first1;
    } else {
        as_global(reinterpret_cast<double*>(a.action))[2 * i + 0] = first0;
        as_global(reinterpret_cast<double*>(a.action))[2 * i + 1] = first1;
    }
    if (a.err) as_global(a.err)[i] = errs;
}

// bcp_step_env.h -- one env inside a step kernel: the LDS of the in-place collision test (collides_wave), the env's state
// between robot model and verdict (Pending), its loads (load_env) and everything that follows the verdict (finalize_env).
#pragma once

#include "bcp_path_window.h"
#include "bcp_diag.h"

// dynamic LDS of the collision kernels:
//   [lethal bitmap words (when the shared map is staged)] [qverts: n_verts * 2 doubles] [vertex scratch of the
//   per-thread rasteriser: n_verts * 2 * kBlock words]
extern __shared__ uint32_t lds_dyn[];

struct CollisionLds {
    bool staged;      // the shared lethal bitmap sits at LDS offset 0
    LdsWords bits;
    LdsF64 qverts;
    VertLds scratch;
    LdsU32 cells;     // kSparseCap words: the cell list of coop_collides_sparse (exact mode 3)
};

__device__ __forceinline__ CollisionLds collision_lds_setup(const DevParams& P, const MapDesc& map, int tid)
{
    CollisionLds L;
    const int map_words = map.in_lds ? map.rows * map.wpr : 0;
    const LdsU32 lds = (LdsU32)lds_dyn;
    for (int k = tid; k < map_words; k += kBlock) lds[k] = map.bits[k];
    const CollisionLdsPlan lo = collision_lds_plan(P.n_verts, map_words);
    __attribute__((address_space(3))) double* q = (__attribute__((address_space(3))) double*)(lds + lo.map);
    for (int k = tid; k < 2 * P.n_verts; k += kBlock) q[k] = P.qverts[k >> 1][k & 1];
    L.staged = map.in_lds != 0;
    L.bits = lds;
    L.qverts = q;
    L.scratch.base = lds + lo.map + lo.qverts + tid;
    L.scratch.stride = kBlock;
    L.cells = lds + lo.map + lo.qverts + lo.scratch;   // kSparseLdsWords
    __syncthreads();
    return L;
}

// pose_collides (envs/base/env.py:464-489) for the pose held by each lane.  EVERY lane of the wave must call this
// (inactive lanes pass active = false): ambiguous poses are settled one at a time by the whole wave.
__device__ __forceinline__ bool collides_wave(const DevParams& P, const MapDesc& map, const CullDesc& cull,
                                              const CollisionLds& L, int exact_mode, int dense_threshold, bool wide,
                                              bool active, int64_t env, double x, double y, double th)
{
    double ox = map.ox, oy = map.oy;
    if (map.origins) {
        ox = map.origins[2 * env + 0];
        oy = map.origins[2 * env + 1];
    }
    const int px = (int)rint((x - ox) * map.inv_res);   // world_to_pixel, coordinate_transformations.py:185-205
    const int py = (int)rint((y - oy) * map.inv_res);
    double c, s;
    cos_sin(th, c, s);
    int cls = active ? classify(cull, map.shared ? 0 : env, map.rows, map.cols, px, py, c, s) : kFree;
    bool hit = cls == kHit;
    uint64_t amb = __ballot(cls == kAmbiguous);
    if (amb == 0) return hit;
    const bool dense = exact_mode == 2 || (exact_mode == 0 && (int)__popcll(amb) > dense_threshold);   // (modes 1 and 3: cooperative)
    if (dense) {
        // many undecided lanes: one per-thread rasteriser pass settles them all at once
        if (cls == kAmbiguous) {
            if (L.staged) {
                CollisionSink<LdsWords> sink{L.bits, map.rows, map.cols, map.wpr, px, py};
                hit = raster_runs(P, c, s, L.scratch, sink);
            } else {
                const uint32_t* words = map.bits + (map.shared ? 0 : env * map.env_stride);
                CollisionSink<const uint32_t*> sink{words, map.rows, map.cols, map.wpr, px, py};
                hit = raster_runs(P, c, s, L.scratch, sink);
            }
        }
        return hit;
    }
    // few undecided lanes: the wave rasterises them cooperatively, one pose at a time
    const int ln = lane_id();
    const double vqx = ln < P.n_verts ? L.qverts[2 * ln] : 0.0, vqy = ln < P.n_verts ? L.qverts[2 * ln + 1] : 0.0;
    while (amb) {
        const int src = __ffsll((unsigned long long)amb) - 1;
        amb &= amb - 1;
        const double c_ = bcast_d(c, src), s_ = bcast_d(s, src);
        const int px_ = bcast_i(px, src), py_ = bcast_i(py, src);
        bool h;
        const int64_t env_ = ((int64_t)bcast_i((int)(env >> 32), src) << 32) | (uint32_t)bcast_i((int)env, src);
        const uint32_t* words = map.bits + (map.shared ? 0 : env_ * map.env_stride);
        int verdict = kSparseTooMany;
        if (exact_mode == 3) {   // the cell-by-cell form of the exact test (what step_local_kernel uses)
            if (L.staged)
                verdict = wide ? coop_collides_sparse<true>(P, L.qverts, c_, s_, px_, py_, L.bits, map.rows, map.cols, map.wpr, L.cells)
                               : coop_collides_sparse<false>(P, L.qverts, c_, s_, px_, py_, L.bits, map.rows, map.cols, map.wpr, L.cells);
            else
                verdict = wide ? coop_collides_sparse<true>(P, L.qverts, c_, s_, px_, py_, words, map.rows, map.cols, map.wpr, L.cells)
                               : coop_collides_sparse<false>(P, L.qverts, c_, s_, px_, py_, words, map.rows, map.cols, map.wpr, L.cells);
        }
        if (verdict != kSparseTooMany) {
            h = verdict == kSparseHit;
        } else if (L.staged) {
            h = coop_collides(P, vqx, vqy, c_, s_, px_, py_, L.bits, map.rows, map.cols, map.wpr, wide);
        } else {
            h = coop_collides(P, vqx, vqy, c_, s_, px_, py_, words, map.rows, map.cols, map.wpr, wide);
        }
        if (lane_id() == src) hit = h;
    }
    return hit;
}

// One env's state after the robot model ran, before the collision verdict is known.
struct Pending {
    double c, s;        // cos / sin of the new heading (as used by the classification)
    int32_t px, py;     // world_to_pixel of the new position
    Robot r;            // after robot.step()
    Pose old;           // pose before the step (rollback target)
    double min_dist;
    double z[3];
    int32_t target, iter, err, drawn;
    int32_t collided;   // sticky flag before this step
    int32_t env_lo, env_hi;
    int32_t geom;       // geometry-pool entry of the env during this step (pool mode only)
    // delays > 0: the elements this step's pushes into the pose / robot-state FIFOs will hand back (fifo_peek: read with
    // the state, before anything is pushed), so that kernel 2 can redo the pushes of an env kernel 1 finished optimistically
    double popped_pose[3], popped_state[7];
};

// An env's initial state (entry k of the initial-state arrays), all loads in flight together
struct InitAhead {
    double x, y, th, v, w, steer, wheel, min_dist;
    int32_t target, iter, collided;
};

template <typename SP>
__device__ __forceinline__ InitAhead fetch_init_ahead(SP S, int64_t k, bool tri)
{
    InitAhead p;
    p.x = as_global(S->init.x)[k];
    p.y = as_global(S->init.y)[k];
    p.th = as_global(S->init.angle)[k];
    p.v = as_global(S->init.v)[k];
    p.w = as_global(S->init.w)[k];
    p.steer = tri ? as_global(S->init.steer)[k] : 0.0;
    p.wheel = tri ? as_global(S->init.wheel)[k] : 0.0;
    p.min_dist = as_global(S->init.min_dist)[k];
    p.target = as_global(S->init.target_idx)[k];
    p.iter = as_global(S->init.cur_iter)[k];
    p.collided = (int32_t)as_global(S->init.collided)[k];
    return p;
}

// The same from a declared uniform initial state: the block of the LDS copy of *S (step_local_kernel's shared-geometry variant
// behind kStepInitUniform) -- a few wide LDS reads in place of eleven loads from memory at the very end of a workgroup.
template <typename SP>
__device__ __forceinline__ InitAhead init_ahead_uniform(SP S, bool tri)
{
    InitAhead p;
    p.x = S->init_uniform.x;
    p.y = S->init_uniform.y;
    p.th = S->init_uniform.th;
    p.v = S->init_uniform.v;
    p.w = S->init_uniform.w;
    p.steer = tri ? S->init_uniform.steer : 0.0;
    p.wheel = tri ? S->init_uniform.wheel : 0.0;
    p.min_dist = S->init_uniform.min_dist;
    p.target = S->init_uniform.target;
    p.iter = S->init_uniform.iter;
    p.collided = S->init_uniform.collided;
    return p;
}

// reward-provider outcome for the pose as it is when nothing collides, computed ahead of the collision verdict
struct ScoredFree {
    double rew, min_dist;
    int target;
};

// A parked pose of the single-launch step (LDS): what the exact test needs, and its verdict.  The env's state stays in
// the registers of the mover lane that parked it; that lane finishes the env once the verdict is in.
struct ParkedPose {
    double c, s;             // cos / sin of the new heading
    int32_t px, py;          // world_to_pixel of the new position
    int32_t env_lo, env_hi;  // env index (private maps: the map entry)
    int32_t geom;            // geometry-pool entry
    int32_t verdict;         // 0 = pending, 1 = free, 2 = collides
    // private paths: what the reward provider returns for the rolled-back pose, should the verdict be "collides" -- worked
    // out by the env's mover while the scanners are still busy (step_local_kernel), valid when spec_ok != 0
    double spec_rew, spec_min;
    int32_t spec_target, spec_ok;
};

// entry of the non-shared map / path arrays that env i uses
template <typename SP>   // const StepStatic* in global memory, or step_local_kernel's copy of the block in LDS
__device__ __forceinline__ int64_t slot_of(SP S, int64_t i, const Pending& q)
{
    return S->geom_of_env ? (int64_t)q.geom : i;
}

// Everything of PlanEnv.step() that follows pose_collides(): rollback (env.py:458-459), bookkeeping and delay queues
// (:377-396), reward (:352), done (:407-419), outputs, optional reset, state write-back.  Runs on one lane for env i.
// PLAIN = true (no delays, continuous reward provider -- see step_is_plain) compiles the delay queues and the
// pure-pursuit branch out.
// (A: StepArgs by value, or by reference into the kernel-argument segment, or FinishArgs -- only the global block, the output
//  pointers, a.hot.st and a.flags are used)
// Returns the episode-record slot the env took (-1: none, or no record bound).
// SHARED (step_local_kernel's variant for one map, one path and no geometry pool, see step_local_body): the branches on
// those properties are compiled out.
template <bool PLAIN, bool SHARED = false, typename A, typename SP>
__device__ __forceinline__ int finalize_env_from(const A& a, SP S, int64_t i, Pending& q, bool hit, LdsF64 lds_path = nullptr,
                                             const PathWindow* free_window = nullptr, bool have_score = false,
                                             ScoredFree score = ScoredFree(), int known_len = -1, bool score_fits_hit = false,
                                             int64_t out_base = 0, RecRedo redo = RecRedo{0.0, -1, false})
{   // (redo.on: step_pending_kernel finishes again an env that step_fast_pair_kernel finished optimistically as free -- the
    //  record keeps the slot kernel 1 gave it, redo.slot, and the return starts from redo.ret_before;
    //  the score travels by value: a pointer to a local made the compiler keep it in scratch memory;
    //  out_base: element offset of this step's rows in the output arrays -- step k of a rollout writes row k, bcp_rollout --;
    //  known_len >= 0: the caller already holds the length of this env's path;
    //  score_fits_hit: `score` was computed for the rolled-back pose of a colliding env -- continuous provider only)
    const DevParams& P = *(const DevParams*)&S->P;   // (S may point into LDS: step_local_kernel)
    const int pose_delay = PLAIN ? 0 : P.pose_delay, state_delay = PLAIN ? 0 : P.state_delay;
    const bool pure_pursuit = !PLAIN && P.reward_provider == BCP_REWARD_PURE_PURSUIT;
    const bool tri = P.model == BCP_MODEL_TRICYCLE;
    const int64_t n = S->n;
    Robot& r = q.r;
    if (hit) {  // robot.set_pose(*old_position): pose restored, v = w = 0 (tricycle_model.py:471-476)
        r.p = q.old;
        r.v = 0.0;
        r.w = 0.0;
    }
    int iter = q.iter + 1;
    bool collided = q.collided != 0 || hit;
    double min_dist = q.min_dist;
    int target = q.target;
    // State.pose / State.robot_state: what the reward provider and the observation see (env.py:377-394)
    double seen[3] = {r.p.x, r.p.y, r.p.th};
    double seen_rs[7] = {r.p.x, r.p.y, r.p.th, r.v, r.w, r.steer, r.wheel};
    if (pose_delay) fifo_push<3>(S->st.pose_q, pose_delay, n, i, iter, seen, q.popped_pose);
    if (state_delay) fifo_push<7>(S->st.state_q, state_delay, n, i, iter, seen_rs, q.popped_state);

    // shared path: uniform pointers (scalar cache); private paths: per-lane pointers
    double rew = 0.0;
    int m;
    bool goal;
    const int64_t g = SHARED ? i : slot_of(S, i, q);
    const double* pts = S->path.pts + ((SHARED || S->path.shared) ? 0 : g * (int64_t)S->path.max_len * 5);
    m = known_len >= 0 ? known_len : ((SHARED || S->path.shared) ? S->path.max_len : S->path.lens[g]);
    if (pure_pursuit) {
        if (have_score && !hit) {   // the scorer wave has already done it (no collision: the flag it assumed stands)
            rew = score.rew;
            min_dist = score.min_dist;
            target = score.target;
        } else if (!ABLATED(a, kAblateNoReward)) {
            rew = reward_pure_pursuit(pts, m, seen[0], seen[1], collided, min_dist, target);
        }
        goal = hypot(pts[5 * (m - 1)] - seen[0], pts[5 * (m - 1) + 1] - seen[1]) < 1.0;   // done(), reward.py:141-150
    } else {
        // the scorer wave has already done it (step_fast_pair_kernel) for the pose State exposes if nothing collides --
        // which, with a pose delay, is an earlier pose whatever this step's verdict (from the second step of an episode on)
        if (have_score && (!hit || score_fits_hit || (pose_delay && iter > 1))) {
            rew = score.rew;
            min_dist = score.min_dist;
            target = score.target;
        } else if (!ABLATED(a, kAblateNoReward)) {
            // way-point window of the pose: the caller may have looked it up already for the un-rolled-back pose
            const PathWindow w =
                (free_window && !hit && !pose_delay) ? *free_window : path_window_of(P, SHARED || S->path.shared != 0, S->path.bbox, S->path.index, g, seen[0], seen[1]);
            if ((SHARED || lds_path) && (SHARED || S->path.shared))  // way points staged in LDS by the step kernel
                rew = reward_step(P, lds_path, w, m, seen[0], seen[1], seen[2], min_dist, target);
            else
                rew = reward_step<PLAIN ? 4 : 2>(P, pts, w, m, seen[0], seen[1], seen[2], min_dist, target);
        }
        goal = target > m - 1;
    }
    const bool timeout = iter >= P.iteration_timeout;
    const bool done = goal || timeout || collided;   // env.py:400-419

    const int64_t o = out_base + i;
    DIAG_WAIT_LGKM();
    DIAG_STAMP_FIN(0);   // arguments in hand (the shared-geometry variant: read from LDS ahead of the verdicts)
    as_global(a.reward)[o] = rew;
    as_global(a.done)[o] = (uint8_t)done;
    if (a.collided_now) as_global(a.collided_now)[o] = (uint8_t)hit;
    if (a.err) as_global(a.err)[o] = q.err;
    if (a.noise_z_out) {
        const double nan = __builtin_nan("");
        as_global(a.noise_z_out)[3 * o + 0] = (q.drawn & 1) ? q.z[0] : nan;
        as_global(a.noise_z_out)[3 * o + 1] = (q.drawn & 2) ? q.z[1] : nan;
        as_global(a.noise_z_out)[3 * o + 2] = (q.drawn & 4) ? q.z[2] : nan;
    }

    DIAG_STAMP_FIN(1);   // outputs stored
    const bool reset = done && (a.flags & BCP_STEP_AUTO_RESET);
    InitAhead ahead = InitAhead();   // (initialised: left undefined outside the branch, it was kept in scratch memory)
    if (reset) {  // PlanEnv.reset(): set_state(initial_state) (env.py:293-303)
        int64_t k = i;
        if (!SHARED && S->geom_of_env) {  // RandomMiniEnv.reset(): the env moves on to its next geometry (mini_env.py:469-481).
            // Computed from the entry the step started with, so kernel 2 redoing an env that kernel 1 already reset
            // lands on the same geometry (a hit always ends the episode, so both reset or neither does).
            k = S->next_geom ? as_global(S->next_geom)[g] : g;
            as_global(S->geom_of_env)[i] = (int32_t)k;
        }
        // (SHARED: a declared uniform initial state is in the LDS copy of *S -- one wave-uniform test of the launch flags, which
        //  the generic variants never see set)
        if (SHARED && (a.flags & kStepInitUniform)) ahead = init_ahead_uniform(S, tri);
        else ahead = fetch_init_ahead(S, k, tri);
    }
    // Episode record (bcp_bind_episode_record), one wave-uniform test of the launch flags when none is bound.  The state the
    // env holds after its last step goes to a slot while the initial-state loads above are in flight.
    int rec_slot = -1;
    if (a.flags & kStepRecord) {
        const EpisodeRec& R = global_block(a)->rec;   // (the global block: step_local_kernel's LDS copy ends before the record)
        double ret_sum = 0.0;             // the episode's return, summed in step order (reward.py:66-69, :144-153)
        if (R.ret) ret_sum = (redo.on ? redo.ret_before : as_global(R.ret)[i]) + rew;
        as_global(R.reason)[i] = done ? (uint8_t)((goal ? BCP_DONE_GOAL : 0) | (timeout ? BCP_DONE_TIMEOUT : 0) |
                                                  (collided ? BCP_DONE_COLLIDED : 0))
                                      : (uint8_t)0;
        // one ballot and one atomic per wave hand out the slots (kernel 2's redo keeps the slot kernel 1 gave the env)
        const bool keeps = redo.on && redo.slot >= 0;
        const bool take = done && !keeps;
        const uint64_t takers = __ballot(take);
        if (takers) {
            const int first = (int)__ffsll((unsigned long long)takers) - 1;
            const int lane = lane_id();
            int base = 0;
            if (lane == first) base = (int)atomicAdd(R.work, (uint32_t)__popcll(takers));
            base = bcast_i(base, first);
            if (take) rec_slot = base + (int)__popcll(takers & ((1ull << lane) - 1ull));
        }
        if (keeps) rec_slot = redo.slot;
        if (done && rec_slot < R.capacity) {   // (beyond: overflow, only counted)
            const int64_t j = rec_slot, c = R.capacity;
            as_global(R.env_id)[j] = (int32_t)i;
            as_global(R.geom)[j] = (!SHARED && S->geom_of_env) ? (int32_t)g : -1;
            if (R.ret) as_global(R.final_ret)[j] = ret_sum;
            as_global(R.fin.x)[j] = r.p.x;
            as_global(R.fin.y)[j] = r.p.y;
            as_global(R.fin.angle)[j] = r.p.th;
            as_global(R.fin.v)[j] = r.v;
            as_global(R.fin.w)[j] = r.w;
            if (tri) {
                as_global(R.fin.steer)[j] = r.steer;
                as_global(R.fin.wheel)[j] = r.wheel;
            }
            as_global(R.fin.min_dist)[j] = min_dist;
            as_global(R.fin.target_idx)[j] = target;
            as_global(R.fin.cur_iter)[j] = iter;
            as_global(R.fin.collided)[j] = (uint8_t)collided;
            if (pose_delay) {
#pragma unroll
                for (int k = 0; k < 3; ++k) R.fin.pose_seen[k * c + j] = seen[k];
            }
            if (state_delay) {
#pragma unroll
                for (int k = 0; k < 7; ++k) R.fin.state_seen[k * c + j] = seen_rs[k];
            }
        }
        if (!done) rec_slot = -1;
        if (R.ret) as_global(R.ret)[i] = reset ? 0.0 : ret_sum;
    }
    if (reset) {
        r.p.x = ahead.x;
        r.p.y = ahead.y;
        r.p.th = ahead.th;
        r.v = ahead.v;
        r.w = ahead.w;
        if (tri) {
            r.steer = ahead.steer;
            r.wheel = ahead.wheel;
        }
        min_dist = ahead.min_dist;
        target = ahead.target;
        iter = ahead.iter;
        collided = ahead.collided != 0;
        // the restored State exposes the initial pose / robot state; its queues are empty (pushes restart at k = 1)
        seen[0] = r.p.x;
        seen[1] = r.p.y;
        seen[2] = r.p.th;
        seen_rs[0] = r.p.x;
        seen_rs[1] = r.p.y;
        seen_rs[2] = r.p.th;
        seen_rs[3] = r.v;
        seen_rs[4] = r.w;
        seen_rs[5] = r.steer;
        seen_rs[6] = r.wheel;
#ifdef BCP_DIAG
        DIAG_WAIT_VMEM();
        DIAG_STAMP_FIN(2);   // reset values in hand (diagnostic build only: the wait is not in the shipping kernel)
#endif
    }
    // (the state pointers come with the kernel arguments -- StepHot -- not through *S: one dependent load less per array;
    //  step_local_kernel's shared-geometry variant: with the rest of FinishArgs, from the LDS copy of *S)
    as_global(a.hot.st.x)[i] = r.p.x;
    as_global(a.hot.st.y)[i] = r.p.y;
    as_global(a.hot.st.angle)[i] = r.p.th;
    as_global(a.hot.st.v)[i] = r.v;
    as_global(a.hot.st.w)[i] = r.w;
    if (tri) {
        as_global(a.hot.st.steer)[i] = r.steer;
        as_global(a.hot.st.wheel)[i] = r.wheel;
    }
    as_global(a.hot.st.min_dist)[i] = min_dist;
    as_global(a.hot.st.target_idx)[i] = target;
    as_global(a.hot.st.cur_iter)[i] = iter;
    as_global(a.hot.st.collided)[i] = (uint8_t)collided;
    if (pose_delay) {
#pragma unroll
        for (int c = 0; c < 3; ++c) S->st.pose_seen[c * n + i] = seen[c];
    }
    if (state_delay) {
#pragma unroll
        for (int c = 0; c < 7; ++c) S->st.state_seen[c * n + i] = seen_rs[c];
    }
    DIAG_STAMP_FIN(3);   // state stored
    return rec_slot;
}

// (the parameter block where the launch arguments point to: the two-launch and the general step kernels)
template <bool PLAIN, typename A>
__device__ __forceinline__ int finalize_env(const A& a, int64_t i, Pending& q, bool hit, LdsF64 lds_path = nullptr,
                                            const PathWindow* free_window = nullptr, bool have_score = false,
                                            ScoredFree score = ScoredFree(), int known_len = -1, bool score_fits_hit = false,
                                            RecRedo redo = RecRedo{0.0, -1, false})
{
    return finalize_env_from<PLAIN>(a, a.S, i, q, hit, lds_path, free_window, have_score, score, known_len, score_fits_hit, 0,
                                    redo);
}

// ---- loads shared by the step kernels ------------------------------------------------------------------------
template <bool PLAIN, typename A>
__device__ __forceinline__ void load_env(const A& a, uint64_t seed, uint64_t step_counter, int64_t i, bool active,
                                         Pending& q, double& cmd0, double& cmd1, bool draw_noise = true)
{
    // (no branch in here: the pointers are adjacent launch arguments, fetched by a few wide scalar loads in one go; an
    //  array a configuration does not have -- the tricycle's two values, the pool entry -- is read from a stand-in)
    Robot& r = q.r;
    const bool tri = a.hot.model == BCP_MODEL_TRICYCLE;
    const double* const p_steer = tri ? a.hot.st.steer : a.hot.st.x;
    const double* const p_wheel = tri ? a.hot.st.wheel : a.hot.st.x;
    const int32_t* const p_geom = a.hot.geom_of_env ? a.hot.geom_of_env : a.hot.st.target_idx;
    r.p.x = as_global(a.hot.st.x)[i];
    r.p.y = as_global(a.hot.st.y)[i];
    r.p.th = as_global(a.hot.st.angle)[i];
    r.v = as_global(a.hot.st.v)[i];
    r.w = as_global(a.hot.st.w)[i];
    const double v_steer = as_global(p_steer)[i], v_wheel = as_global(p_wheel)[i];
    q.min_dist = as_global(a.hot.st.min_dist)[i];
    q.target = as_global(a.hot.st.target_idx)[i];
    q.iter = as_global(a.hot.st.cur_iter)[i];
    q.collided = as_global(a.hot.st.collided)[i] != 0;
    const int32_t v_geom = as_global(p_geom)[i];
    r.steer = tri ? v_steer : 0.0;
    r.wheel = tri ? v_wheel : 0.0;
    q.geom = a.hot.geom_of_env ? v_geom : 0;
    // the action, float32 [N,2] or float64 [N,2], as two 8-byte words read without a branch (float32: the same word twice);
    // they are only looked at below, so the loads above and the caller's next ones are all in flight together
    const bool f32 = (a.flags & BCP_STEP_ACTIONS_F32) != 0;
    const GlobalPtr<const uint64_t> aw = as_global(reinterpret_cast<const uint64_t*>(a.actions)) + (f32 ? i : 2 * i);
    const uint64_t a_lo = aw[0], a_hi = aw[f32 ? 0 : 1];
    cmd0 = f32 ? (double)__uint_as_float((uint32_t)a_lo) : __longlong_as_double((long long)a_lo);
    cmd1 = f32 ? (double)__uint_as_float((uint32_t)(a_lo >> 32)) : __longlong_as_double((long long)a_hi);
    if (!PLAIN && a.hot.control_delay && active) {   // the robot executes the command given control_delay steps ago (env.py:371-373)
        double cmd[2] = {cmd0, cmd1};
        fifo_delay<2>(a.hot.st.control_q, a.hot.control_delay, a.hot.n, i, q.iter + 1, cmd);
        cmd0 = cmd[0];
        cmd1 = cmd[1];
    }
    if (!PLAIN) {   // what this step's pushes will displace (k = iter + 1)
        fifo_peek<3>(a.hot.st.pose_q, a.hot.pose_delay, a.hot.n, i, q.iter + 1, q.popped_pose);
        fifo_peek<7>(a.hot.st.state_q, a.hot.state_delay, a.hot.n, i, q.iter + 1, q.popped_state);
    }
    q.z[0] = q.z[1] = q.z[2] = 0.0;
    if (a.hot.noise_on) {
        if (a.noise_z) {
            q.z[0] = as_global(a.noise_z)[3 * i + 0];
            q.z[1] = as_global(a.noise_z)[3 * i + 1];
            q.z[2] = as_global(a.noise_z)[3 * i + 2];
        } else if (draw_noise) {
            device_normals(seed, (uint64_t)(a.hot.env_id_base + i), step_counter, q.z);
        }
    }
}

template <bool PLAIN>
__device__ __forceinline__ void load_env(const StepArgs& a, int64_t i, bool active, Pending& q, double& cmd0, double& cmd1)
{
    load_env<PLAIN>(a, a.seed, a.step_counter, i, active, q, cmd0, cmd1);
}

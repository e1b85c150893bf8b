// bcp_step.h -- device code of the batched PlanEnv.step(): the step kernels (general / fast / pending; local), behind what they
// are built from, each part in a header of its own and included here in order -- staging limits and LDS layouts, the parameter
// blocks shared with the host, the one-time path kernels, the reward providers and the delay queues, the diagnostic stamps, and
// one env inside a kernel.  Included by
// bcplan.hip; the handle is in bcp_host.h, the step's launcher and C entry points in bcp_step_host.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "bcp_device.h"
#include "bcp_raster.h"
#include "bcp_coop.h"
#include "bcp_init_uniform.h"
#include "bcp_step_layout.h"
#include "bcp_step_args.h"
#include "bcp_bind_kernels.h"
#include "bcp_path_window.h"
#include "bcp_diag.h"
#include "bcp_step_env.h"

using namespace bcp;

constexpr int kWavePerPoseFrom = 1;   // step_pending_kernel: more than this many rounds of parked poses per team -> a pose per wave

// General step kernel: robot model, collision settled in place by collides_wave (distance-field classification when
// there is one, then the cooperative / per-thread exact rasterisers), reward, done, write-back.  Used when there
// is no distance field, when the batch is too small to need load balancing, or when a mode is forced.
__global__ void __launch_bounds__(kBlock) step_kernel(const StepArgs launch_args)
{
    const StepArgs a = resolve_step(launch_args, 0);
    const DevParams& P = a.S->P;
    const int tid = threadIdx.x;
    const int64_t gi = (int64_t)blockIdx.x * kBlock + tid;
    const bool active = gi < a.hot.n;
    const int64_t i = active ? gi : a.hot.n - 1;  // inactive lanes of the last wave shadow env n-1 and never store

    const CollisionLds L = collision_lds_setup(P, a.S->map, tid);
    Pending q;
    double cmd0, cmd1;
    load_env<false>(a, i, active, q, cmd0, cmd1);

    // ---- _env_step (envs/base/env.py:442-461)
    q.old = q.r.p;
    q.drawn = 0;
    q.err = robot_step(P, q.r, cmd0, cmd1, q.z, q.drawn);
    bool hit = false;
    if (!ABLATED(a, kAblateNoCollision))
        hit = collides_wave(P, a.S->map, a.S->cull, L, a.S->exact_mode, a.S->dense_threshold, a.S->wide != 0, active,
                            slot_of(a.S, i, q), q.r.p.x, q.r.p.y, q.r.p.th);
    if (active) finalize_env<false>(a, i, q, hit);
    advance_step_by_ticket(a);
}


// Kernel 1 of the two-kernel step (needs a distance field).  A pose is cleared in O(1) by the outer test; the few
// envs it cannot clear are finished optimistically ("free") AND parked in `pending`, and kernel 2 redoes those that
// really collide.  Waves with many undecided lanes (robots hugging walls) settle them in place.  Memory operations are
// grouped so that independent round trips overlap: a wave has at most one partner on its SIMD, so an exposed L2 / HBM
// latency is nearly pure stall.
//
// It runs with TWO wavefronts per 64 envs.  A wave that runs alone on its SIMD is bound by the latency of its
// own dependent chain, and the two longest stretches after the robot model -- collision classification + parking on
// one side, the reward scan on the other -- only share the new pose.  So the "mover" wave (loads, robot model,
// classification, parking / in-place settling, write-back) hands the pose to the "scorer" wave through LDS, the
// scorer runs the reward provider for the free pose meanwhile, and the mover picks the result up for every env that
// did not collide in place (those redo the reward themselves for the rolled-back pose).
// LDS: pair_lds_plan (bcp_step_layout.h)
// PLAIN = false: delay queues and / or the pure-pursuit provider (finalize_env's general form; the scorer wave's
// result is then only used where it applies: continuous reward, no pose delay).
template <bool WIDE, bool PLAIN>
__global__ void __launch_bounds__(2 * kBlock) step_fast_pair_kernel(const StepArgs launch_args)
{
    const StepArgs a = resolve_step(launch_args, 0);
    const DevParams& P = a.S->P;
    const int tid = threadIdx.x, lane = tid & 63;
    const bool mover = tid < kBlock;
    const int64_t gi = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gi < a.hot.n;
    const int64_t i = active ? gi : a.hot.n - 1;

    // (1) staging loads (both waves), then the mover's state / action / noise and the scorer's two reward-state words
    __attribute__((address_space(3))) double* qv = (__attribute__((address_space(3))) double*)lds_dyn;
    const PairLds lo = pair_lds_plan(P.n_verts, a.hot.lds_path_doubles);
    const int nq = lo.path;
    const double my_q = tid < nq ? P.qverts[tid >> 1][tid & 1] : 0.0;
    double t[kPairStageRegs];
#pragma unroll
    for (int u = 0; u < kPairStageRegs; ++u) {
        const int k = u * 2 * kBlock + tid;
        t[u] = k < a.hot.lds_path_doubles ? a.hot.path_pts[k] : 0.0;
    }
    Pending q;
    double cmd0 = 0.0, cmd1 = 0.0;
    if (mover) {
        load_env<PLAIN>(a, i, active, q, cmd0, cmd1);
        if (gi < kShards) a.pending_next[gi] = 0;  // arm the counters of the NEXT step (the two sets alternate)
        if (gi < kShards && a.inplace_next) a.inplace_next[gi] = 0;
    } else {
        q.min_dist = a.hot.st.min_dist[i];
        q.target = a.hot.st.target_idx[i];
        q.geom = a.hot.geom_of_env ? a.hot.geom_of_env[i] : 0;
        q.collided = PLAIN ? 0 : (int32_t)(a.hot.st.collided[i] != 0);   // (the pure-pursuit reward depends on it)
    }
    // the scorer also brings the bounding box and the bucket index of a shared path into LDS while the mover is busy
    // with the robot model (its window look-up then needs no global round trip); a private path's box is fetched now
    // as well -- it does not depend on the pose
    float box[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t index_words[2] = {0, 0};
    if (!mover) {
        if (a.hot.path_shared) {
            if (lane < 8) box[0] = reinterpret_cast<const float*>(a.hot.path_bbox)[lane];
            const uint32_t* iw = reinterpret_cast<const uint32_t*>(a.hot.path_index);   // [2][kPathBuckets][2] int16
            index_words[0] = iw[lane];
            index_words[1] = iw[kBlock + lane];
        } else {
            const int64_t g = a.hot.geom_of_env ? (int64_t)q.geom : i;
#pragma unroll
            for (int k = 0; k < 8; ++k) box[k] = reinterpret_cast<const float*>(a.hot.path_bbox + g * kBoxDoubles)[k];
        }
    }
    if (tid < nq) qv[tid] = my_q;
#pragma unroll
    for (int u = 0; u < kPairStageRegs; ++u) {
        const int k = u * 2 * kBlock + tid;
        if (k < a.hot.lds_path_doubles) qv[nq + k] = t[u];
    }
    for (int k = kPairStageDoubles + tid; k < a.hot.lds_path_doubles; k += 2 * kBlock) qv[nq + k] = a.hot.path_pts[k];  // long paths
    const LdsF64 lds_path = a.hot.lds_path_doubles ? (LdsF64)(qv + lo.path) : (LdsF64) nullptr;
    __attribute__((address_space(3))) double* hand_pose = qv + lo.hand_pose;
    __attribute__((address_space(3))) double* hand_score = qv + lo.hand_score;
    __attribute__((address_space(3))) double* lds_box = qv + lo.box;                    // [8]
    __attribute__((address_space(3))) uint32_t* lds_index = (__attribute__((address_space(3))) uint32_t*)(qv + lo.index);  // [128]
    if (!mover && a.hot.path_shared) {
        if (lane < 8) lds_box[lane] = (double)box[0];
        lds_index[lane] = index_words[0];
        lds_index[kBlock + lane] = index_words[1];
    }

    // (2) mover: _env_step's robot model (envs/base/env.py:442-461); the new pose goes to the scorer
    Robot& r = q.r;
    if (mover) {
        q.old = r.p;
        q.drawn = 0;
        q.err = robot_step(P, r, cmd0, cmd1, q.z, q.drawn);
        // the pose the reward provider will see: the new one, or -- with a pose delay -- the one fifo_peek fetched
        const bool delayed = !PLAIN && P.pose_delay > 0 && q.iter + 1 > 1;
        hand_pose[lane] = delayed ? q.popped_pose[0] : r.p.x;
        hand_pose[kBlock + lane] = delayed ? q.popped_pose[1] : r.p.y;
        hand_pose[2 * kBlock + lane] = delayed ? q.popped_pose[2] : r.p.th;
    }
    __syncthreads();

    bool hit = false;
    int64_t parked_at = -1;   // the env's parking slot (episode record: kernel 1 leaves the env's record slot there)
    double park_ret = 0.0;
    if (mover) {
        // (3a) collision: distance-field classification, then parking or in-place settling
        const int64_t g = slot_of(a.S, i, q);
        double ox = a.S->map.ox, oy = a.S->map.oy;
        if (a.S->map.origins) {
            ox = a.S->map.origins[2 * g + 0];
            oy = a.S->map.origins[2 * g + 1];
        }
        const int px = (int)rint((r.p.x - ox) * a.S->map.inv_res);  // world_to_pixel, coordinate_transformations.py:185-205
        const int py = (int)rint((r.p.y - oy) * a.S->map.inv_res);
        double c, s;
        cos_sin(r.p.th, c, s);
        const int64_t map_env = a.S->map.shared ? 0 : g;
        OuterLookups look;
        look.off_map = true;
        if (!ABLATED(a, kAblateNoCollision | kAblateNoClassify))
            look = outer_lookups_issue(a.S->cull, map_env, a.S->map.rows, a.S->map.cols, px, py, c, s);
        const int cls = active ? outer_lookups_verdict(a.S->cull, look) : kFree;
        const uint64_t amb = __ballot(cls == kAmbiguous);
        const int n_amb = (int)__popcll(amb);
        const int threshold = a.threshold_now ? *a.threshold_now : a.S->dense_threshold;
        if (n_amb > threshold) {
            if (lane == 0 && a.inplace_count) atomicAdd(a.inplace_count + (int)(blockIdx.x % kShards), n_amb);
            const bool inner = cls == kAmbiguous && classify_inner_hit(a.S->cull, map_env, px, py, c, s);
            hit = inner;
            uint64_t todo = __ballot(cls == kAmbiguous && !inner);
            const double vqx = lane < P.n_verts ? qv[2 * lane] : 0.0, vqy = lane < P.n_verts ? qv[2 * lane + 1] : 0.0;
            while (todo) {
                const int src = __ffsll((unsigned long long)todo) - 1;
                todo &= todo - 1;
                const int64_t env_ = ((int64_t)bcast_i((int)(g >> 32), src) << 32) | (uint32_t)bcast_i((int)g, src);
                const uint32_t* words = a.S->map.bits + (a.S->map.shared ? 0 : env_ * a.S->map.env_stride);
                const bool h = coop_collides<WIDE>(P, vqx, vqy, bcast_d(c, src), bcast_d(s, src), bcast_i(px, src),
                                                   bcast_i(py, src), words, a.S->map.rows, a.S->map.cols, a.S->map.wpr);
                if (lane == src) hit = h;
            }
        } else if (cls == kAmbiguous && !ABLATED(a, kAblateNoPark)) {
            const int shard = (int)(blockIdx.x % kShards);
            const int slot = atomicAdd(a.pending_count + shard, 1);
            q.c = c;
            q.s = s;
            q.px = px;
            q.py = py;
            q.env_lo = (int32_t)(uint32_t)i;
            q.env_hi = (int32_t)(i >> 32);
            parked_at = (int64_t)slot * kShards + shard;
            a.S->pending[parked_at] = q;  // interleaved: the used slots stay in a few pages
            // (episode record: kernel 2's redo starts the return from where this step found it)
            if ((a.flags & kStepRecord) && a.S->rec.ret) park_ret = a.S->rec.ret[i];
        }
    } else if (!ABLATED(a, kAblateNoReward)) {
        // (3b) scorer: ContinuousRewardProvider.reward for the pose as it stands if nothing collides
        const double x = hand_pose[lane], y = hand_pose[kBlock + lane], th = hand_pose[2 * kBlock + lane];
        const int64_t g = slot_of(a.S, i, q);
        PathWindow win;
        if (a.S->path.shared)
            win = path_window(P, (LdsF64)lds_box, (const __attribute__((address_space(3))) int16_t*)lds_index, x, y);
        else
            win = path_window_compact(P, box, reinterpret_cast<const uint16_t*>(a.hot.path_bbox + g * kBoxDoubles) + kBoxIndexU16,
                                      reinterpret_cast<const int32_t*>(a.hot.path_bbox + g * kBoxDoubles)[kBoxLenWord + 1], x, y);
        const int m = a.S->path.shared ? a.S->path.max_len : a.S->path.lens[g];
        double min_dist = q.min_dist;
        int target = q.target;
        double rew;
        const double* gpath = a.S->path.pts + (a.S->path.shared ? 0 : g * (int64_t)a.S->path.max_len * 5);
        if (!PLAIN && P.reward_provider == BCP_REWARD_PURE_PURSUIT) {   // (no collision this step: the sticky flag as it is)
            if (lds_path) rew = reward_pure_pursuit(lds_path, m, x, y, q.collided != 0, min_dist, target);
            else rew = reward_pure_pursuit(gpath, m, x, y, q.collided != 0, min_dist, target);
        } else if (lds_path) {
            rew = reward_step(P, lds_path, win, m, x, y, th, min_dist, target);
        } else {
            rew = reward_step(P, gpath, win, m, x, y, th, min_dist, target);
        }
        hand_score[lane] = rew;
        hand_score[kBlock + lane] = min_dist;
        hand_score[2 * kBlock + lane] = (double)target;
    }
    __syncthreads();
    if (mover && active) {
        ScoredFree sc;
        sc.rew = hand_score[lane];
        sc.min_dist = hand_score[kBlock + lane];
        sc.target = (int)hand_score[2 * kBlock + lane];
        const int rec_slot = finalize_env<PLAIN>(a, i, q, hit, lds_path, nullptr, !ABLATED(a, kAblateNoReward), sc);
        if ((a.flags & kStepRecord) && parked_at >= 0) {
            RecPark p;
            p.ret_before = park_ret;
            p.slot = rec_slot;
            p.pad = 0;
            a.S->rec.park[parked_at] = p;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tick[1] = a.step_counter;   // for kernel 2 (see StepArgs::tick)
    advance_step_by_ticket(a);   // (only when no kernel 2 follows)
}

// Kernel 2 of a step: kPendingWaves wavefronts per parked env: the lanes rasterise
// the footprint together (coop_collides, wave w takes the row chunks w, w+2, ...); on a collision thread 0 redoes
// the env's finalisation from the parked state.  The first entry is fetched speculatively, together with the
// counter that says whether it exists, so the two round trips overlap.
// Undecided poses per step up to which kernel 1 parks them all.  With a pose per wave (below) kernel 2 takes 8192 poses
// per round and spreads them evenly, which beat settling them inside kernel 1's waves in every workload measured (the
// aisle config, tens of thousands of undecided poses per step: 0.076 ms parked, 0.086 ms in place, 0.102 ms with the
// former limit of 8192); the in-place path remains for far denser cases and as BCP_TUNE_DENSE_THRESHOLD.
constexpr int kParkCapacity = 1 << 20;

// kernel 2's redo of the env in parking slot `at`: with a record, the return and slot kernel 1 left for it
__device__ __forceinline__ RecRedo redo_of(const StepArgs& a, int64_t at)
{
    RecRedo r{0.0, -1, true};
    if (a.flags & kStepRecord) {
        const RecPark p = a.S->rec.park[at];
        r.ret_before = p.ret_before;
        r.slot = p.slot;
    }
    return r;
}

template <bool WIDE, bool PLAIN>
__global__ void __launch_bounds__(kBlock * kPendingWaves) step_pending_kernel(const StepArgs launch_args)
{
    const StepArgs a = resolve_step(launch_args, 1);
    DIAG_STAMP(0);
    const DevParams& P = a.S->P;
    const int lane = threadIdx.x % kBlock, wave = threadIdx.x / kBlock;
    const int shard = (int)(blockIdx.x % kShards);
    const int stride = gridDim.x / kShards;
    const Pending* slots = a.hot.pending + shard;
    const double vqx = lane < P.n_verts ? P.qverts[lane][0] : 0.0, vqy = lane < P.n_verts ? P.qverts[lane][1] : 0.0;
    const int count = a.pending_count[shard];
    if (blockIdx.x == 0 && a.threshold_next && threadIdx.x < kShards) {
        // Undecided poses of this step, parked + settled in place.  Up to kParkCapacity the next step parks everything
        // (no wave is held up by its own unlucky lanes); beyond that every wave settles its own.
        int total = a.pending_count[threadIdx.x] + a.inplace_count[threadIdx.x];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
        if (threadIdx.x == 0) *a.threshold_next = total <= kParkCapacity ? 64 : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tick[0] = a.step_counter + 1;   // the next step's kernel 1 reads this
    if (count > kWavePerPoseFrom * stride) {
        // Many parked poses in this shard (private worlds with the robots near their walls: several rounds for every
        // team): throughput matters more than the latency of one pose, so every WAVE takes poses of its own -- four
        // times as many in flight, each about twice as long in the single-wave rasteriser.
        for (int idx = (blockIdx.x / kShards) * kPendingWaves + wave; idx < count; idx += stride * kPendingWaves) {
            const Pending* e = slots + (int64_t)idx * kShards;
            const int64_t i = ((int64_t)e->env_hi << 32) | (uint32_t)e->env_lo;
            const int64_t g = a.hot.geom_of_env ? (int64_t)e->geom : i;
            const uint32_t* words = a.hot.map_bits + (a.hot.map_shared ? 0 : g * a.hot.map_env_stride);
            bool hit = false;
            if (!ABLATED(a, kAblateNoCoop))
                hit = coop_collides<WIDE>(P, vqx, vqy, e->c, e->s, e->px, e->py, words, a.hot.map_rows, a.hot.map_cols,
                                          a.hot.map_wpr);
            if (hit && lane == 0) {
                Pending q = *e;
                finalize_env<PLAIN>(a, i, q, true, nullptr, nullptr, false, ScoredFree(), -1, false,
                                    redo_of(a, (int64_t)idx * kShards + shard));
            }
        }
        if (a.flags & kStepRecord) {   // (the last workgroup publishes the step's count of ended envs)
            __syncthreads();
            if (threadIdx.x == 0) record_publish(a.S, gridDim.x);
        }
        return;
    }
    for (int idx = blockIdx.x / kShards; idx < a.hot.pending_cap; idx += stride) {
        const Pending* e = slots + (int64_t)idx * kShards;   // in bounds whatever `count` says
        const double c = e->c, s = e->s;
        const int px = e->px, py = e->py;
        const int64_t i = ((int64_t)e->env_hi << 32) | (uint32_t)e->env_lo;
        const int64_t g = a.hot.geom_of_env ? (int64_t)e->geom : i;
        if (idx >= count) break;
        DIAG_STAMP(1);
        const uint32_t* words = a.hot.map_bits + (a.hot.map_shared ? 0 : g * a.hot.map_env_stride);
        // (no inner distance-field test here: nearly every parked pose is free, so the test would cost a dependent
        //  round trip per pose and almost never spare the rasteriser)
        bool hit = false;
        DIAG_STAMP(2);
        if (!ABLATED(a, kAblateNoCoop))
            hit = coop_collides_quad<WIDE>(P, vqx, vqy, c, s, px, py, words, a.hot.map_rows, a.hot.map_cols, a.hot.map_wpr, wave,
                                           (LdsU32)lds_dyn);
        DIAG_STAMP(3);
        hit = __syncthreads_or(hit);  // wave-uniform verdicts of the block's waves
        DIAG_STAMP(4);
        // kernel 1 already finished this env as "free"; only a collision changes anything
        if (hit && threadIdx.x == 0) {
            Pending q = *e;
            finalize_env<PLAIN>(a, i, q, true, nullptr, nullptr, false, ScoredFree(), -1, false,
                                redo_of(a, (int64_t)idx * kShards + shard));
        }
    }
    if (a.flags & kStepRecord) {
        __syncthreads();
        if (threadIdx.x == 0) record_publish(a.S, gridDim.x);
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The step as ONE launch: step_local_kernel.  The hand-off of undecided poses stays inside the workgroup.
//
// Round 1 settled them in a second launch (step_pending_kernel: 13 of the step's 30 us on the metric workload -- kernel
// boundary, cold caches, ramp-up -- for ~1000 poses).  A global hand-off inside one launch (queues in HBM, write-through
// stores, sc1 polls, no fences) was built and measured in round 2: 13 - 25 x SLOWER, every parked pose costs device-scope
// atomics and polls on a few hot lines that the memory side serves one after the other (profiles/r02_queue_handoff_attempt.txt).
// So nothing leaves the CU here:
//   * a workgroup = 256 envs = 4 (mover, scorer) wave pairs as in step_fast_pair_kernel + 8 helper waves: 16 waves, one
//     workgroup per CU, four waves per SIMD;
//   * the waves that idle until the new pose exists do what needs no pose: the scorers draw the step's odometry noise, a
//     helper computes cos / sin of the old heading (barrier 0 hands both to the movers);
//   * movers park the POSES of their undecided envs in LDS (40 bytes each; the env's state stays in the mover lane's
//     registers); "barrier 2" is a pair of LDS counters: a mover waits for the three scan results of its pair, everybody
//     for all four movers' parked poses;
//   * then ALL 16 waves draw tickets (an LDS counter) and settle one parked pose each -- the exact test, cell by cell
//     (coop_collides_sparse) -- and post the verdict in the record, while the movers first finish their decided envs;
//   * a mover lane that parked an env waits for its verdict (a few hundred cycles, LDS) and finishes the env itself:
//     rollback on a hit, reward, done, in-kernel reset, stores -- in SIMD with the wave's other parked lanes.
//     With ~4 parked poses per 256 envs and 16 waves the exact tests of a workgroup run side by side, right after the
//     classification, on a warm CU.
// No queue, no atomic in global memory, no poll, no second launch; load balance comes from the workgroup being large
// (the sum of 256 envs' luck) and from the helper waves.
// The workgroup comes in three sizes (template parameter PAIRS, BCP_TUNE_LOCAL_PAIRS): 4 pairs = 16 waves = 256 envs (one
// workgroup per CU: rounds 2-3), 2 pairs = 8 waves = 128 envs (two co-resident per CU) and 1 pair = 4 waves = 64 envs (four).
// Every form has the same four waves per 64 envs and the same four waves per SIMD when the chip is full; what changes is the
// granule in which the CU's registers are handed out: a 16-wave workgroup shares a CU with NOTHING (112 VGPRs x 1024 threads),
// so one workgroup more than the chip holds, a sampler or an RCCL kernel resident on some CUs, costs a whole further round
// (profiles/r03_n_sweep.txt: 65 536 envs 11.8 us, 65 792 envs 17.8 us); an 8-wave one can start beside a leaving neighbour.
constexpr int kLocalPairsDefault = 4;   // (bcp_step_host.h: local_pairs)

typedef const __attribute__((address_space(4))) StepArgs& KernArgs;   // the launch arguments where they lie: scalar loads on
                                                                      // demand instead of ~500 bytes pinned in SGPRs

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kStaticChunks = (int)((offsetof(StepStatic, rec) + 15) / 16);   // *S in 16-byte pieces, up to the record

static_assert(kStepLds.parked_pose_bytes == sizeof(ParkedPose) && kStepLds.sparse_lds_words == kSparseLdsWords &&
              kStepLds.static_chunks == kStaticChunks && kStepLds.finish_slot_bytes == kFinishSlotBytes && kFinishSlotBytes % 16 == 0,
              "bcp_step_layout.h restates these: the LDS plans are computed from its copies");

// A launch-argument value fetched NOW: the empty asm makes every 32-bit word of `v` an opaque scalar register at this
// point, so the compiler can neither sink the fetch into a later basic block nor fetch the field again.  At a kernel start
// every first touch of an argument line is a scalar-cache miss of ~450 cycles (measured: tools/diag_local.py), and hipcc
// fetches an argument where it is first used, block by block, each fetch with its own wait -- nine dependent round trips
// = 4.3 k cycles before the mover's last load was issued.  Fetched together (fetch_words: plain loads of adjacent words,
// merged into wide fetches) and then pinned (pin_words), the prologue's arguments arrive in ONE round trip.
template <int NW>
__device__ __forceinline__ void fetch_words(const __attribute__((address_space(4))) void* p, uint32_t (&w)[NW])
{
    const __attribute__((address_space(4))) uint32_t* src = (const __attribute__((address_space(4))) uint32_t*)p;
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = src[k];
}

template <int NW>
__device__ __forceinline__ void pin_words(uint32_t (&w)[NW])
{
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        asm("" : "+s"(w[k]));   // (not volatile: a volatile asm counts as a store, and every later fetch of a uniform
                                //  address -- the parameter block *S -- would turn into a vector load)
        w[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[k]);   // (tells the compiler the word is wave-uniform; folds away)
    }
}

// what the prologue of step_local_kernel needs from the launch arguments (same member names as StepArgs: load_env takes either)
struct PrologueArgs {
    StepHot hot;
    const StepStatic* S;
    const void* actions;
    const double* noise_z;
    uint64_t* tick;
    uint32_t flags;
};

// a wave-uniform 64-bit value that arrived through a vector load
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

static_assert(kStaticChunks <= 128, "*S is staged by the last two waves of a workgroup");
// A spin on an LDS word another wave of the workgroup will set (`cond` true = keep waiting, wave-uniform).  Bounded: a wait
// that the hand-off protocol guarantees to end within ~20 k cycles gives up after kPollLimit trips (~10^7 cycles) and sets
// `expired`; the wave carries on with what it has and reports BCP_ERR_INTERNAL at the end.  (hipcc 7.2 has turned two
// shapes of exactly these loops into endless spins, DESIGN.md "Compiler notes": a miscompile must fail a test, not wedge the GPU.)
constexpr int kPollLimit = 1 << 16;
#define BOUNDED_POLL(cond, expired) do { int trips_ = 0; while (cond) { __builtin_amdgcn_s_sleep(1); if (++trips_ > kPollLimit) { (expired) = true; break; } } } while (0)
constexpr uint32_t kDiagWithholdVerdicts = 1u << 23;   // -DBCP_DIAG builds: parked poses are tested but their verdicts never posted

// ROLL (bcp_rollout): the workgroup takes its envs through StepArgs::rollout_steps steps inside ONE launch -- actions,
// optional normals and the outputs are [steps][N] arrays, the state goes through its usual arrays between steps.  The launch
// and the staging of footprint / path / lethal map / parameter block happen once, and -- the larger part -- a workgroup
// starts its next step when IT is done, not when the slowest workgroup of the chip is (envs are independent,
// envs/base/env.py:334-361: there is nothing to wait for).  Every trip fetches its launch arguments again (scalar-cache hits
// from the second on): carried across the loop the ~60 pinned words did not fit the scalar registers (600 spills).  Bit for
// bit the same states and outputs as that many launches of the one-step form (tests/test_gpu_rollout.py).  The one-step
// form is this code with the loop folded away.
typedef const __attribute__((address_space(4))) StepArgs* KernArgPtr;

// SHARED: the variant for handles whose geometry is one map and one path, both staged in LDS, with no geometry pool, no
// per-env origins and the 1-bit `near` tiles (local_step_shared, bcp_step_host.h: C2, C3, the sharded C5, every replica
// batch).  What the generic variant asks at run time is then known when the kernel is compiled, and the variant holds ONE
// exact test (on the LDS map), the LDS list scan, classify_near and coop_last_reached for hits -- not both copies of the
// exact test, the private-path scans and their speculative reward, and the branches between them.  SHARED = false is the
// code as it was.
//
// one step of the workgroup's envs: the whole of the one-step kernel, and one trip (`rs`) of a rollout
template <bool WIDE, bool PLAIN, int PAIRS, bool ROLL, bool SHARED = false>
__device__ __forceinline__ void step_local_body(KernArgPtr kernarg, const int rs)
{
    static_assert(!SHARED || (PAIRS == 4 && !ROLL), "the shared-geometry variant exists for the 16-wave one-step kernel");
    static_assert(PAIRS == 1 || PAIRS == 2 || PAIRS == 4, "a workgroup holds 1, 2 or 4 (mover, scorer, helper, helper) quartets");
    constexpr int kLocalPairs = PAIRS, kLocalWaves = 4 * PAIRS, kLocalEnvs = PAIRS * kBlock;
    constexpr int kPairShift = PAIRS == 4 ? 2 : (PAIRS == 2 ? 1 : 0);
    constexpr int kStaticFrom = (kLocalWaves - 2) * kBlock;   // *S is staged by the last two waves
    constexpr int kCtlFrom = (kLocalWaves - 1) * kBlock;      // the control words are zeroed by the last wave
    [[maybe_unused]] constexpr int kWScorer = PAIRS, kWHelper1 = 2 * PAIRS, kWHelper2 = 3 * PAIRS;   // pair 0's waves (stamps)
    DIAG_STAMP_WAVES(512);    // every wave: first instruction
    DIAG_REAL_ENTRY();
    // (static issue priorities by role, s_setprio -- the movers above everybody else, or everybody else above the movers
    //  until barrier 0, or behind barrier 1 -- change nothing: +-0.5 % in every form tried)
    // The prologue is ONE memory round trip.  Everything a wave asks for first -- the mover's state, action and robot
    // constants, a scanner's target index, the old heading of the helper that takes its cos / sin, every wave's share of the
    // staging data (footprint, shared path + index, lethal bitmap, the parameter block *S) -- is addressed from the launch
    // arguments alone (StepHot, fetched together: fetch_words / pin_words) and issued back to back before anything is waited
    // for; what was loaded is stored to LDS only after the wave has done what it can do without it.  Nothing before barrier 0
    // reads *S through the scalar cache: those fetches take 1.3 - 2.2 k cycles at a kernel start, and a wave that waits for
    // one waits for all of them.  (Round 2 staged array by array -- load, wait, LDS store -- fetched each launch argument
    // where it was first used (~450 cycles per first touch, nine in a row) and only then issued the state loads: 4.1 k
    // cycles until a mover's state had landed, 5.1 k to barrier 0; tools/diag_local.py.)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool mover = wave < kLocalPairs, scorer = wave >= kLocalPairs && wave < 2 * kLocalPairs;
    const int pair = wave & (kLocalPairs - 1);
    KernArgs a = *kernarg;
    // (the launch arguments the prologue uses, fetched together before the first branch: pin_sgpr)
    PrologueArgs L;
    {
        constexpr int kStateWords = PLAIN ? kHotStateWords : (int)(sizeof(DevState) / 4);
        uint32_t w_st[kStateWords], w_hot[kHotPrologueWords];
        fetch_words(&a.hot.st, w_st);
        fetch_words(&a.hot.n, w_hot);
        pin_words(w_st);
        pin_words(w_hot);
        __builtin_memset(&L.hot, 0, sizeof(L.hot));
        __builtin_memcpy(&L.hot.st, w_st, sizeof(w_st));
        __builtin_memcpy(&L.hot.n, w_hot, sizeof(w_hot));
        L.actions = L.hot.io_actions;
        L.noise_z = L.hot.io_noise_z;
        L.tick = L.hot.io_tick;
        L.flags = L.hot.io_flags;
        L.S = a.S;   // (not pinned: a pointer that went through the asm is no longer known to be uniform, nor global)
        if (ROLL) {   // this step's rows of the [steps][N].. inputs
            const int64_t row = (int64_t)rs * L.hot.n;
            L.actions = (const char*)L.actions + row * ((L.flags & BCP_STEP_ACTIONS_F32) ? 8 : 16);
            L.noise_z = L.noise_z ? L.noise_z + 3 * row : nullptr;
        }
    }
    const int64_t out_base = ROLL ? (int64_t)rs * L.hot.n : 0;
    const int hot_n_verts = L.hot.n_verts, hot_npath = L.hot.lds_path_doubles, hot_path_shared = SHARED ? 1 : L.hot.path_shared;
    const int hot_map_rows = L.hot.map_rows, hot_map_cols = L.hot.map_cols, hot_map_wpr = L.hot.map_wpr;
    const int hot_map_shared = SHARED ? 1 : L.hot.map_shared, hot_noise_on = L.hot.noise_on, hot_max_len = L.hot.path_max_len;
    // (SHARED: no pool and no origins of their own -- the launcher has looked)
    const int32_t* const hot_geom_of_env = SHARED ? nullptr : L.hot.geom_of_env;
    const double* const hot_map_origins = SHARED ? nullptr : L.hot.map_origins;
    const int64_t hot_n = L.hot.n;
    // PLAIN (continuous reward, no delays): the backward scan for the last reached way point -- the longest stretch of
    // the reward provider -- is split three ways between the pair's scorer and its two helper waves (every third
    // candidate of the window each; contiguous thirds for paths in global memory); the mover takes the maximum and does
    // the rest of the provider itself.
    const bool scanner = PLAIN ? !mover : scorer;
    const int member = (wave >> kPairShift) - 1;   // 0 = scorer, 1 / 2 = helpers (PLAIN only)

    // ---- LDS
    typedef __attribute__((address_space(3))) char* LdsBytes;
    const int npath = hot_npath;
    const LocalLds lf = local_lds_front(hot_n_verts, npath, PAIRS);
    const int nq = lf.path;
    const LdsBytes lds0 = (LdsBytes)lds_dyn;
    __attribute__((address_space(3))) double* qv = (__attribute__((address_space(3))) double*)lds_dyn;
    const LdsF64 lds_path = (SHARED || npath) ? (LdsF64)(qv + lf.path) : (LdsF64) nullptr;
    __attribute__((address_space(3))) double* hand_pose = qv + lf.hand + pair * kHandDoubles * kBlock;
    __attribute__((address_space(3))) double* hand_score = hand_pose + 3 * kBlock;
    __attribute__((address_space(3))) double* hand_heading = hand_pose + 6 * kBlock;
    __attribute__((address_space(3))) double* lds_box = qv + lf.box;   // [8]
    __attribute__((address_space(3))) uint32_t* lds_index = (__attribute__((address_space(3))) uint32_t*)(qv + lf.index);  // [128]
    __attribute__((address_space(3))) int32_t* ctl = (__attribute__((address_space(3))) int32_t*)(qv + lf.ctl);   // [kCtlWords]
    __attribute__((address_space(3))) ParkedPose* rec = (__attribute__((address_space(3))) ParkedPose*)(lds0 + lf.rec);
    const LdsU32 cell_list = (LdsU32)(lds0 + lf.cells) + wave * kSparseLdsWords;
    const LdsU32 lds_map = (LdsU32)(lds0 + lf.map);
    const int map_words = SHARED ? hot_map_rows * hot_map_wpr : staged_map_words(hot_map_shared != 0, hot_map_rows, hot_map_wpr);
    const LocalLds lo = local_lds_rear(lf, map_words, PLAIN, PAIRS);
    // the parameter block *S, copied into LDS by the prologue: behind barrier 0 every wave reads its parameters from there.
    // (Scalar fetches of *S take 1.3 - 2.2 k cycles at a kernel start, and a wave that holds the ~60 words it needs of the
    //  block in scalar registers from the start has none left for the launch arguments.)
    __attribute__((address_space(3))) u32x4* lds_static = (__attribute__((address_space(3))) u32x4*)(lds0 + lo.stat);
    const __attribute__((address_space(3))) StepStatic* SL = (const __attribute__((address_space(3))) StepStatic*)lds_static;
    // delay queues (PLAIN = false): the ten values this step's pushes into the pose / robot-state queues will hand back are
    // fetched with the state (fifo_peek) and needed when the env is finished; in between they wait in LDS, not in 20 vector
    // registers of a wave that has none to spare
    __attribute__((address_space(3))) double* fifo_stash = (__attribute__((address_space(3))) double*)(lds0 + lo.stash) + pair * kBlock + lane;
    // this launch's FinishWords, behind the parameter block (SHARED: written by the last wave ahead of barrier 0)
    __attribute__((address_space(3))) uint32_t* const lds_finish_words = (__attribute__((address_space(3))) uint32_t*)(lds0 + lo.finish);

    DIAG_STAMP(0);
    DIAG_STAMP_WAVES(768);    // every wave: launch arguments fetched
    const int64_t gi = (int64_t)blockIdx.x * kLocalEnvs + pair * kBlock + lane;
    const bool active = gi < hot_n;
    const int64_t i = active ? gi : hot_n - 1;   // (inactive lanes of the last workgroup shadow env n-1 and never store)
    const bool noise_by_waves = (hot_noise_on != 0) & (L.noise_z == nullptr);   // the step's odometry noise is drawn here, by idle waves

    // (0) the step counter and the noise seed live on the device (StepArgs::tick): two dependent scalar fetches, first in
    //     line for the waves that draw the noise (the last wave also moves the counter on at the end); movers never read them
    //     (vector loads of a uniform address: a scalar fetch would share its counter with the fetches of *S below, and a
    //      wave waiting for the one waits for all of them)
    uint64_t tick_counter = 0, tick_seed = 0;
    if (!mover) {
        int zero;
        asm("v_mov_b32 %0, 0" : "=v"(zero));   // (opaque: keeps these loads on the vector side)
        const GlobalPtr<const uint64_t> t = as_global((const uint64_t*)L.tick) + zero;
        tick_counter = t[0];
        tick_seed = t[2];
    }
    // (1) every wave's own loads: the mover's state / action, a scanner's reward-state words, the old heading for the
    //     helper that takes its cos / sin
    Pending q;
    double cmd0 = 0.0, cmd1 = 0.0;
    float box[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // (a private path's box and bucket grid: the f32 words of its record)
    float quant_inv = 0.0f;                    // (... and the reciprocal step of its prefilter records)
    double old_angle = 0.0;
    double own_org_x = 0.0, own_org_y = 0.0;                  // (only ever written by the loads below: a later assignment
    uint64_t own_len_shift = 0;                                // (private path: way points | index shift << 32)
                                                               //  to a register a load is in flight to would wait for it)
    const bool own_origin = !hot_path_shared || hot_map_origins != nullptr;
    if (mover) {
        load_env<PLAIN>(L, 0, 0, i, active, q, cmd0, cmd1, false);
        if (!hot_path_shared) {   // private paths: origin and length of the entry share a line
            const int64_t g = hot_geom_of_env ? (int64_t)q.geom : i;
            own_org_x = as_global(L.hot.path_bbox)[g * kBoxDoubles + kBoxOrigin];
            own_org_y = as_global(L.hot.path_bbox)[g * kBoxDoubles + kBoxOrigin + 1];
            own_len_shift = as_global(reinterpret_cast<const uint64_t*>(L.hot.path_bbox))[g * kBoxDoubles + kBoxLenWord / 2];
        } else if (hot_map_origins) {   // (private maps with a shared path)
            const int64_t g = hot_geom_of_env ? (int64_t)q.geom : i;
            own_org_x = as_global(hot_map_origins)[2 * g + 0];
            own_org_y = as_global(hot_map_origins)[2 * g + 1];
        }
    } else {
        if (scanner) {
            if (!PLAIN) q.min_dist = as_global(L.hot.st.min_dist)[i];   // (PLAIN: the scan only needs the target index)
            q.target = as_global(L.hot.st.target_idx)[i];
            q.geom = hot_geom_of_env ? as_global(hot_geom_of_env)[i] : 0;
            q.collided = PLAIN ? 0 : (int32_t)(as_global(L.hot.st.collided)[i] != 0);
            if (!hot_path_shared) {
                const int64_t g = hot_geom_of_env ? (int64_t)q.geom : i;
#pragma unroll
                for (int k = 0; k < 8; ++k) box[k] = as_global(reinterpret_cast<const float*>(L.hot.path_bbox + g * kBoxDoubles))[k];
                quant_inv = as_global(reinterpret_cast<const float*>(L.hot.path_bbox + g * kBoxDoubles))[kBoxQuantStep + 1];
                own_len_shift = as_global(reinterpret_cast<const uint64_t*>(L.hot.path_bbox))[g * kBoxDoubles + kBoxLenWord / 2];
            }
        }
        if (member == 1) old_angle = as_global(L.hot.st.angle)[i];
    }
    //     ... and the mover the seven robot constants of the model's first half (dt .. p_gain, adjacent in DevParams), by
    //     vector loads of a uniform address: they arrive with the state, in vector registers, and scalar registers stay free
    //     (PLAIN only: with delay queues the first half runs behind barrier 0, on the constants in LDS)
    double rc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // (+ 1 / dt, 1 / L: div_by_const)
    if (PLAIN && mover) {   // (a rollout fetches them in every trip: seven loads, nothing to carry across the loop)
        int zero;
        asm("v_mov_b32 %0, 0" : "=v"(zero));   // (opaque: keeps these loads on the vector side)
        const GlobalPtr<const double> pc = as_global(&a.S->P.dt) + zero;
#pragma unroll
        for (int u = 0; u < 9; ++u) rc[u] = pc[u];
    }
    // (2) the parameter block *S (16 bytes per thread of the last two waves) is the only staging data anybody needs before
    //     barrier 1: the mover's second half reads its parameters from the LDS copy.  Footprint vertices, the shared path with
    //     its bounding box and bucket index and the shared lethal bitmap are first read behind barrier 1, so the waves that
    //     idle between the barriers fetch and store them there (below) -- a prologue that also addressed and issued ~8 staging
    //     loads per thread kept the SIMDs busy for 1 - 2 k cycles before the movers' own loads were even issued.
    //     (issued FIRST by those two waves it was measured slower, 11.75 against 11.70 us: it then competes with the movers' loads)
    u32x4 st_static = {0u, 0u, 0u, 0u};
    const bool first_trip = !ROLL || rs == 0;   // the staging data is copied into LDS once per launch
    if (first_trip && tid >= kStaticFrom && tid < kStaticFrom + kStaticChunks) st_static = as_global(reinterpret_cast<const u32x4*>(a.S))[tid - kStaticFrom];
    // (2a) SHARED: the per-launch words of the finishing pass -- output pointers, flags -- go to LDS too.  They belong to this
    //     launch (a caller may hand a different `done` row every step), so they are fetched from the launch arguments every
    //     time, by the last wave, whose chain is not the movers': a word per lane, by a VECTOR load of the argument segment
    //     that is in flight beside the wave's share of *S and stored with it, in front of barrier 0.  (As a scalar fetch the
    //     two or three cold argument lines cost the wave a wait of ~1.2 k cycles of its own: without noise to draw it was then
    //     the last to reach barrier 0, C2 +0.6 %.)  The flags are in the prologue's hands already.  The movers read the slot
    //     back ahead of their verdict polls (FinishArgs).
    uint32_t st_finish = 0;
    const bool finish_stager = SHARED && tid >= kCtlFrom && tid < kCtlFrom + kFinishPtrWords;
    if (finish_stager)
        st_finish = as_global(reinterpret_cast<const uint32_t*>((uintptr_t)kernarg + offsetof(StepArgs, noise_z_out)))[tid - kCtlFrom];
    if (SHARED && tid == kCtlFrom + kFinishPtrWords) lds_finish_words[kFinishPtrWords] = L.flags;
    DIAG_STAMP_U(0, 10);   // mover: own + staging loads issued
    DIAG_STAMP_U(kWScorer, 11);   // scorer: the same
    DIAG_STAMP_WAVES(1280);   // every wave: prologue loads issued
    __builtin_amdgcn_sched_barrier(0);
    // (a rollout: the counter in memory stands still until the launch's last trip has drawn its ticket)
    const uint64_t step_counter = mover ? 0 : uniform_u64(tick_counter) + (ROLL ? (uint64_t)rs : 0ull), seed = mover ? 0 : uniform_u64(tick_seed);
    // (5) what needs no pose.  The odometry noise of this step needs nothing but seed, env id and step counter: Philox +
    //     float64 Box-Muller.  Slots 1 and 2 -- the ones PlanEnv's noise model draws -- are the two halves of one pair
    //     (device_normals): the scorer draws them; slot 0, when the model can consume it at all, the pair's second helper;
    //     (Splitting the pair -- radius on the scorer, direction on a helper, both running the Philox block -- was measured
    //      in round 3: the second copy of the generator costs the SIMD more issue slots than the shorter chain wins,
    //      11.87 - 12.0 against 11.72 us per step.)
    //     (So was drawing the NEXT step's pair at the end of a step, when the scorers idle, and fetching it here with a key
    //      {seed, step, env base}: the noise is then ready 0.9 k cycles earlier, but the ten extra loads in the scorers'
    //      prologue hold up everybody's own loads -- the movers reached barrier 0 0.4 k cycles LATER; 11.7 against 11.56 us.
    //      And fetching the scanners' target index / path box and the helper's old heading behind barrier 0 instead of
    //      here: 11.63 against 11.51 us.)
    if (noise_by_waves && scorer) {
        double z1, z2;
        device_normals_12(seed, (uint64_t)(L.hot.env_id_base + i), step_counter, z1, z2);
        hand_score[kBlock + lane] = z1;
        hand_score[2 * kBlock + lane] = z2;
        DIAG_STAMP_U(kWScorer, 1);   // scorer: noise drawn
    }
    if (noise_by_waves && member == 2) hand_score[lane] = L.hot.noise_slot0 ? device_normal_0(seed, (uint64_t)(L.hot.env_id_base + i), step_counter) : 0.0;
    //     (the first helper's cos / sin of the OLD heading is needed behind barrier 1 only: it follows barrier 0)
    //     the mover the first half of the robot model (_env_step, envs/base/env.py:442-461): front-wheel column, cos / sin
    //     of the new wheel angle, velocity model
    Robot& r = q.r;
    RobotDrive drive;
    drive.v = drive.w = 0.0;
    drive.noisy = false;
    if (mover) {
        q.old = r.p;
        q.drawn = 0;
#ifdef BCP_DIAG
        DIAG_WAIT_VMEM();
        DIAG_STAMP_U(0, 3);    // mover: state loads landed (diagnostic build only: the wait is not in the shipping kernel)
#endif
      if (PLAIN) {
        RobotConsts robot;
        robot.model = L.hot.model;
        robot.dynamic_model = L.hot.dynamic_model;
        robot.model_front_column_pid = L.hot.model_front_column_pid;
        robot.noise_on = hot_noise_on;
        robot.dt = rc[0];
        robot.L = rc[1];
        robot.max_wheel_angle = rc[2];
        robot.max_wheel_speed = rc[3];
        robot.max_lin_acc = rc[4];
        robot.max_ang_acc = rc[5];
        robot.p_gain = rc[6];
        robot.inv_dt = rc[7];
        robot.inv_L = rc[8];
        drive = robot_step_begin(robot, r, cmd0, cmd1);
        DIAG_STAMP_U(0, 12);   // mover: first half of the robot model done
      }
        if (!PLAIN) {
#pragma unroll
            for (int k = 0; k < 3; ++k) fifo_stash[k * kLocalEnvs] = q.popped_pose[k];
#pragma unroll
            for (int k = 0; k < 7; ++k) fifo_stash[(3 + k) * kLocalEnvs] = q.popped_state[k];
        }
    }
    // (6) the parameter block into LDS
    if (tid >= kCtlFrom && tid < kCtlFrom + kCtlWords) ctl[tid - kCtlFrom] = 0;
    if (first_trip && tid >= kStaticFrom && tid < kStaticFrom + kStaticChunks) lds_static[tid - kStaticFrom] = st_static;
    if (finish_stager) lds_finish_words[tid - kCtlFrom] = st_finish;
    DIAG_STAMP_WAVES(1024);
    __syncthreads();   // barrier 0: noise, old heading and the parameter block are in LDS
    const DevParams& P = *(const DevParams*)&SL->P;
    const int map_rows = hot_map_rows, map_cols = hot_map_cols;
    const int my_len = hot_path_shared ? hot_max_len : (int)(uint32_t)own_len_shift;   // way points of this env's path
    // (7) mover: the second half of the robot model; the pose the reward provider will see goes to the scanning waves
    Pose new_pose;
    new_pose.x = new_pose.y = new_pose.th = 0.0;
    if (mover) {
        if (noise_by_waves) {
            q.z[0] = hand_score[lane];
            q.z[1] = hand_score[kBlock + lane];
            q.z[2] = hand_score[2 * kBlock + lane];
        }
        DIAG_STAMP(1);   // (the compiler may move loads across this: indicative only)
        if (!PLAIN) drive = robot_step_begin(P, r, cmd0, cmd1);
        // the new pose goes out as soon as it exists; the measured velocities (path_velocity: a square root, two divisions)
        // are the mover's own business, behind barrier 1
        new_pose = robot_step_pose(P, r, drive, q.z, q.drawn);
        const bool delayed = !PLAIN && P.pose_delay > 0 && q.iter + 1 > 1;
        hand_pose[lane] = delayed ? fifo_stash[0] : new_pose.x;
        hand_pose[kBlock + lane] = delayed ? fifo_stash[kLocalEnvs] : new_pose.y;
        hand_pose[2 * kBlock + lane] = delayed ? fifo_stash[2 * kLocalEnvs] : new_pose.th;
        DIAG_STAMP(2);
    }
    // (7a) the first helper: cos / sin of the OLD heading, which the robot model needs at its very end (path_velocity, behind
    //      barrier 1) -- before barrier 0 it made its wave the last one to arrive there
    if (!mover && member == 1) {
        double c0, s0;
        cos_sin(old_angle, c0, s0);
        hand_heading[lane] = c0;
        hand_heading[kBlock + lane] = s0;
        DIAG_STAMP_U(kWHelper1, 2);   // helper: cos / sin of the old heading
    }
    // (7b) everybody else stages what is read behind barrier 1: loads first, all of them in flight together, then the stores
    if (!mover && first_trip) {
        constexpr int kStagers = local_stagers(PAIRS);            // 768 / 384 / 192 threads
        constexpr int kMapPerStager = local_map_per_stager(PAIRS);   // 6 / 11 / 22 words each
        constexpr int kBoxAt = kStagers >= 448 ? 256 : kStagers - 8;              // who fetches the path's box (8 doubles) ...
        constexpr int kIndexAt = kStagers >= 448 ? 320 : kStagers - 136;          // ... and its bucket index (128 words)
        const int nm = tid - kLocalPairs * kBlock;
        double st_q = 0.0, st_path = 0.0;
        float st_box = 0.0f;
        uint32_t st_index = 0;
        uint32_t st_map[kMapPerStager] = {};
        if (nm < nq) st_q = as_global(L.hot.qverts)[nm];
        if (nm < npath) st_path = as_global(L.hot.path_pts)[nm];
        if (hot_path_shared) {
            if (nm >= kBoxAt && nm < kBoxAt + 8) st_box = as_global(reinterpret_cast<const float*>(L.hot.path_bbox))[nm - kBoxAt];
            if (nm >= kIndexAt && nm < kIndexAt + 128) st_index = as_global(reinterpret_cast<const uint32_t*>(L.hot.path_index))[nm - kIndexAt];
        }
#pragma unroll
        for (int u = 0; u < kMapPerStager; ++u) {
            const int k = u * kStagers + nm;
            if (k < map_words) st_map[u] = as_global(L.hot.map_bits)[k];
        }
        if (nm < nq) qv[nm] = st_q;
        if (nm < npath) qv[nq + nm] = st_path;
        for (int k = kStagers + nm; k < npath; k += kStagers) qv[nq + k] = as_global(L.hot.path_pts)[k];   // (long paths)
        if (hot_path_shared) {
            if (nm >= kBoxAt && nm < kBoxAt + 8) lds_box[nm - kBoxAt] = (double)st_box;
            if (nm >= kIndexAt && nm < kIndexAt + 128) lds_index[nm - kIndexAt] = st_index;
        }
#pragma unroll
        for (int u = 0; u < kMapPerStager; ++u) {
            const int k = u * kStagers + nm;
            if (k < map_words) lds_map[k] = st_map[u];
        }
    }
    DIAG_STAMP_WAVES(1536);
    __syncthreads();
    DIAG_STAMP(3);
    if (mover) {
        KnownHeading old_heading;   // (from the first helper wave, barrier 1)
        old_heading.c0 = hand_heading[lane];
        old_heading.s0 = hand_heading[kBlock + lane];
        old_heading.known = true;
        q.err = robot_step_measure(P, r, new_pose, old_heading);
    }
    bool park = false;
    bool poll_expired = false;   // (wave-uniform) one of the bounded waits below gave up
    if (mover) {
        // (3a) collision: distance-field classification; an undecided env is parked below
        // (its parameters are read from the LDS copy of *S here, where they are used: held from barrier 0 on they cost
        //  25 vector registers across the robot model)
        OuterParams outer = outer_params(*(const CullDesc*)&SL->cull);
        outer.near_tx = SL->cull.step_near_tx;
        outer.near_shift = SL->cull.step_near_shift;
        const double map_inv_res = SL->map.inv_res;
        const int64_t near_stride = SL->cull.step_near_stride;
        const double org_x = own_origin ? own_org_x : SL->map.ox, org_y = own_origin ? own_org_y : SL->map.oy;
        const int64_t g = SHARED ? i : slot_of(SL, i, q);
        const int px = (int)rint((r.p.x - org_x) * map_inv_res);  // world_to_pixel, coordinate_transformations.py:185-205
        const int py = (int)rint((r.p.y - org_y) * map_inv_res);
        double c, s;
        cos_sin(r.p.th, c, s);
        DIAG_STAMP_U(0, 4);    // mover: cos / sin of the new heading
        const int64_t map_env = (SHARED || a.hot.map_shared) ? 0 : g;
        int cls = kFree;
#ifdef BCP_DIAG
        if (!ABLATED(a, kAblateNoCollision | kAblateNoClassify))
#endif
        {
            // (a shared field is 18 KB for the 183 x 183 map and stays in the CU's L1: a copy in LDS measured no faster)
            if (SHARED || a.hot.near) {
                // (SHARED: `near` from the LDS copy of *S instead, SL->cull.step_near, one scalar fetch less in front of the
                //  classification: measured, no difference -- profiles/step_finish_pass.txt)
                cls = classify_near(outer, as_global(a.hot.near) + map_env * near_stride, map_rows, map_cols, px, py, c, s);
            } else {
                const OuterLookups look = outer_lookups_issue(*(const CullDesc*)&SL->cull, map_env, map_rows, map_cols, px, py, c, s);
                cls = outer_lookups_verdict(*(const CullDesc*)&SL->cull, look);
            }
        }
        if (!active) cls = kFree;
        DIAG_STAMP_U(0, 5);    // mover: classified
        if (cls == kAmbiguous && !ABLATED(a, kAblateNoPark)) {
            park = true;
            q.c = c;
            q.s = s;
            q.px = px;
            q.py = py;
            q.env_lo = (int32_t)(uint32_t)i;
            q.env_hi = (int32_t)(i >> 32);
        }
    } else if (scanner && !ABLATED(a, kAblateNoReward)) {
        // (3b) the reward provider for the pose as it stands if nothing collides
        const double x = hand_pose[lane], y = hand_pose[kBlock + lane], th = hand_pose[2 * kBlock + lane];
        const int64_t g = SHARED ? i : slot_of(SL, i, q);
        const int m = my_len;
        const double* gpath = a.hot.path_pts + ((SHARED || a.hot.path_shared) ? 0 : g * (int64_t)a.hot.path_max_len * 5);
        if (PLAIN && (SHARED || lds_path)) {
            // Shared path in LDS: the candidates of the pair's 64 envs as ONE list, shared out evenly between the three
            // scanning waves.  More than half of the envs of a rollout are nowhere near the path (no candidate at all) while
            // a few have ten: with a lane per env the waves ran as many trips as their unluckiest lane (four) for an average
            // of less than one useful candidate per lane and trip.  The scorer looks up every env's window, numbers the
            // candidates (prefix sum over the wave), writes the list -- item k -> env -- and releases it; then every wave
            // takes its share of the items (64 per wave and round), tests way point lo(env) + (k - first(env)) against the env's
            // pose and keeps the largest reached index per env with an LDS maximum.  (`hand_score` is free by now: the noise
            // it carried was read behind barrier 0.)
            __attribute__((address_space(3))) int32_t* res = (__attribute__((address_space(3))) int32_t*)hand_score;        // [64]
            __attribute__((address_space(3))) uint32_t* lo_first = (__attribute__((address_space(3))) uint32_t*)(res + kBlock);   // [64]: lo | first << 16
            __attribute__((address_space(3))) uint8_t* items = (__attribute__((address_space(3))) uint8_t*)(res + 2 * kBlock);   // [kScanItems]
            int total;
            if (member == 0) {
                const PathWindow win = path_window(P, (LdsF64)lds_box, (const __attribute__((address_space(3))) int16_t*)lds_index, x, y);
                DIAG_STAMP_U(kWScorer, 6);    // scorer: candidate window known
                const int lo = max(win.lo, q.target), hi = min(win.hi, m - 1);
                const int cnt = max(hi - lo + 1, 0);
                // inclusive prefix sum over the wave: four DPP row shifts inside every 16-lane row (lanes shifted in from
                // outside a row read 0), then the totals of the rows below (three v_readlane) -- no LDS round trip
                int incl = cnt;
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);   // row_shr:1
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);   // row_shr:2
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);   // row_shr:4
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);   // row_shr:8
                const int t0 = bcast_i(incl, 15), t1 = bcast_i(incl, 31), t2 = bcast_i(incl, 47);
                incl += (lane >= 16 ? t0 : 0) + (lane >= 32 ? t1 : 0) + (lane >= 48 ? t2 : 0);
                total = bcast_i(incl, 63);
                const int first = incl - cnt;
                res[lane] = -1;
                if (total <= kScanItems) {
                    lo_first[lane] = (uint32_t)lo | ((uint32_t)first << 16);
                    for (int t = 0; t < cnt; ++t) items[first + t] = (uint8_t)lane;
                }
                DIAG_MAX(9, cnt);   // longest candidate window among the lanes 0 of the workgroup's waves
                if (lane == 0) __hip_atomic_store(&ctl[kCtlListReady + pair], total + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                int ready;
                BOUNDED_POLL((ready = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&ctl[kCtlListReady + pair], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP))) == 0, poll_expired);
                total = ready > 0 ? ready - 1 : 0;
            }
            if (total <= kScanItems) {
                // (the scorer, who has just made the list, takes the LAST share of every round: 64 * (3 r + 2) ...)
                // (the scorer taking the FIRST share -- on the metric workload the only one that is not empty -- straight after
                //  building the list: 11.64 against 11.54 us, round 3)
                for (int base = 64 * ((member + 2) % 3); base < total; base += 64 * 3) {
                    const int k = base + lane;
                    if (k < total) {
                        const int e = (int)items[k];
                        const uint32_t lf = lo_first[e];
                        const int j = (int)(lf & 0xFFFFu) + (k - (int)(lf >> 16));
                        const LdsF64 wp = lds_path + 5 * j;
                        if (way_point_reached(P, wp[0], wp[1], wp[2], wp[3], wp[4], hand_pose[e], hand_pose[kBlock + e], hand_pose[2 * kBlock + e]))
                            __hip_atomic_fetch_max(&res[e], j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            } else {
                // (a path so dense that the pair's windows hold more than kScanItems way points: a lane per env, every third
                //  candidate per wave, as for paths in global memory)
                const PathWindow win = path_window(P, (LdsF64)lds_box, (const __attribute__((address_space(3))) int16_t*)lds_index, x, y);
                PathWindow part;
                part.hi = min(win.hi, m - 1) - member;
                part.lo = max(win.lo, q.target);
                const int last = last_reached_from(P, lds_path, part, m, q.target, x, y, th, 3);
                if (last >= 0) __hip_atomic_fetch_max(&res[lane], last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            DIAG_STAMP_U(kWScorer, 14);    // scorer of pair 0: scanned
            DIAG_STAMP_U(kWHelper1, 7);     // helper 1 of pair 0: scanned
            DIAG_STAMP_U(kWHelper2, 8);    // helper 2 of pair 0: scanned
        } else {
        PathWindow win;
        if (SHARED || SL->path.shared)
            win = path_window(P, (LdsF64)lds_box, (const __attribute__((address_space(3))) int16_t*)lds_index, x, y);
        else
            win = path_window_compact(P, box, as_global(reinterpret_cast<const uint16_t*>(L.hot.path_bbox + g * kBoxDoubles)) + kBoxIndexU16,
                                      (int)(own_len_shift >> 32), x, y);
        DIAG_STAMP_U(kWScorer, 6);    // scorer: candidate window known
        if (PLAIN) {
            // way points in memory: this member's share of the candidate window [max(lo, target), min(hi, m - 1)] is a
            // contiguous third, counted from the top (four neighbours per round trip)
            const int lo = max(win.lo, q.target), hi = min(win.hi, m - 1);
            int last;
            {
                const int third = (max(hi - lo + 1, 0) + 2) / 3;
                PathWindow part;
                part.hi = hi - member * third;
                part.lo = max(lo, part.hi - third + 1);
                if (a.hot.path_pre) {
                    // (private paths: quantised prefilter records, in steps from the corner of this path's box)
                    last = last_reached_prefiltered(P, gpath, a.hot.path_pre + g * (int64_t)a.hot.path_max_len * 2, part, m,
                                                    q.target, x, y, th, (double)box[0], (double)box[2], quant_inv);
                } else {
                    last = last_reached_from(P, gpath, part, m, q.target, x, y, th);
                }
            }
            ((__attribute__((address_space(3))) int32_t*)hand_score)[member * kBlock + lane] = last;
            DIAG_STAMP_U(kWHelper1, 7);     // helper 1 of pair 0: scanned
            DIAG_STAMP_U(kWHelper2, 8);    // helper 2 of pair 0: scanned
            DIAG_MAX(9, max(hi - lo + 1, 0));   // longest candidate window among the lanes 0 of the workgroup's waves
        } else {
            double min_dist = q.min_dist;
            int target = q.target;
            double rew;
            if (P.reward_provider == BCP_REWARD_PURE_PURSUIT) {
                if (SHARED || lds_path) rew = reward_pure_pursuit(lds_path, m, x, y, q.collided != 0, min_dist, target);
                else rew = reward_pure_pursuit(gpath, m, x, y, q.collided != 0, min_dist, target);
            } else if (SHARED || lds_path) {
                rew = reward_step(P, lds_path, win, m, x, y, th, min_dist, target);
            } else {
                rew = reward_step(P, gpath, win, m, x, y, th, min_dist, target);
            }
            hand_score[lane] = rew;
            hand_score[kBlock + lane] = min_dist;
            hand_score[2 * kBlock + lane] = (double)target;
        }
        }
    }
    // (An env that ends its episode this step reloads its initial state in finalize_env_from, a dependent round trip at
    //  the end of the step.  Fetching it ahead for the lanes that may end -- time-out reached, pose not cleared -- was
    //  measured in round 3: the ~60 instructions it adds to every mover cost more than the round trip they hide,
    //  12.24 against 12.00 us per step.)
    // (4) movers park the undecided poses in LDS right away (one LDS atomic per wave hands out the slots)
    __attribute__((address_space(3))) ParkedPose* my_rec = rec;
    if (mover) {
        const uint64_t parking = __ballot(park);
        if (parking) {
            const int first = (int)__ffsll((unsigned long long)parking) - 1;
            int base = 0;
            if (lane == first) base = atomicAdd((int*)&ctl[kCtlParked], (int)__popcll(parking));
            base = bcast_i(base, first);
            if (park) {
                my_rec = rec + base + (int)__popcll(parking & ((1ull << lane) - 1ull));
                my_rec->c = q.c;
                my_rec->s = q.s;
                my_rec->px = q.px;
                my_rec->py = q.py;
                my_rec->env_lo = q.env_lo;
                my_rec->env_hi = q.env_hi;
                my_rec->geom = q.geom;
                my_rec->verdict = 0;
                my_rec->spec_ok = 0;
            }
        }
    }
    DIAG_STAMP(4);        // mover: classified and parked
    DIAG_STAMP_W(kWScorer, 8);   // scorer of pair 0: scanned
    // "Barrier 2" is two counters in LDS instead of an s_barrier: a mover only needs the scan results of ITS pair, and the
    // other waves only need every mover's poses parked -- the waves that finish their scan first start on the parked
    // poses while the slowest scan of the workgroup is still running (release adds / acquire polls, workgroup scope).
    if (mover) {
        if (lane == 0) __hip_atomic_fetch_add(&ctl[kCtlMoversParked], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        // Private paths: a parked pose that turns out to collide is rolled back, and the reward provider then runs for
        // the OLD pose -- window lookup, way-point scan, distance to the target: five to ten dependent round trips to
        // memory by one lane at the very end of the step, with the rest of the workgroup idle (C4: the workgroups that
        // end last all hold such an env).  The mover has nothing to do until its pair's scans are in, so it works that
        // reward out now for every pose it parked; the verdict then only picks between two finished results.
        if (PLAIN && !(SHARED || lds_path) && !hot_path_shared && a.hot.path_pre && park && !ABLATED(a, kAblateNoReward)) {
            const int64_t g = slot_of(SL, i, q);
            const GlobalPtr<const float> bx = as_global(reinterpret_cast<const float*>(L.hot.path_bbox + g * kBoxDoubles));
            float obox[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) obox[k] = bx[k];
            const PathWindow ow = path_window_compact(P, obox, as_global(reinterpret_cast<const uint16_t*>(L.hot.path_bbox + g * kBoxDoubles)) + kBoxIndexU16,
                                                      (int)(own_len_shift >> 32), q.old.x, q.old.y);
            const double* opath = SL->path.pts + g * (int64_t)SL->path.max_len * 5;
            const int olast = last_reached_prefiltered(P, opath, a.hot.path_pre + g * (int64_t)a.hot.path_max_len * 2, ow, my_len,
                                                       q.target, q.old.x, q.old.y, q.old.th, (double)obox[0], (double)obox[2],
                                                       bx[kBoxQuantStep + 1]);
            double omin = q.min_dist;
            int otarget = q.target;
            my_rec->spec_rew = reward_from_last(P, opath, my_len, olast, q.old.x, q.old.y, omin, otarget);
            my_rec->spec_min = omin;
            my_rec->spec_target = otarget;
            my_rec->spec_ok = 1;
        }
        const int scans = PLAIN ? 3 : 1;
        BOUNDED_POLL(__builtin_amdgcn_readfirstlane(__hip_atomic_load(&ctl[kCtlScansDone + pair], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < scans, poll_expired);
    } else if (scanner && lane == 0) {
        __hip_atomic_fetch_add(&ctl[kCtlScansDone + pair], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // (everybody: the number of parked poses must be final before a wave draws tickets -- a ticket is consumed by the
    //  draw, so a wave that compared it with a stale count would drop a pose, and its owner would wait for ever)
    BOUNDED_POLL(__builtin_amdgcn_readfirstlane(__hip_atomic_load(&ctl[kCtlMoversParked], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < kLocalPairs, poll_expired);
    DIAG_STAMP(5);
    // (scalar: the ticket loop below must stay wave-uniform)
    const int n_parked = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&ctl[kCtlParked], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    // (5) movers: the rest of the reward provider, handed to the parked records, then the decided envs are finished;
    //     everybody else goes straight to the parked poses
    ScoredFree sc;
    sc.rew = 0.0;
    sc.min_dist = 0.0;
    sc.target = 0;
    if (mover) {
        if (PLAIN) {
            const __attribute__((address_space(3))) int32_t* found = (__attribute__((address_space(3))) int32_t*)hand_score;
            const int last = (SHARED || lds_path) ? found[lane] : max(max(found[lane], found[kBlock + lane]), found[2 * kBlock + lane]);
            const int64_t g = SHARED ? i : slot_of(SL, i, q);
            const int m = my_len;
            sc.min_dist = q.min_dist;
            sc.target = q.target;
            if (SHARED || lds_path)
                sc.rew = reward_from_last(P, lds_path, m, last, r.p.x, r.p.y, sc.min_dist, sc.target);
            else
                sc.rew = reward_from_last(P, SL->path.pts + (SL->path.shared ? 0 : g * (int64_t)SL->path.max_len * 5), m,
                                          last, r.p.x, r.p.y, sc.min_dist, sc.target);
        } else {
            sc.rew = hand_score[lane];
            sc.min_dist = hand_score[kBlock + lane];
            sc.target = (int)hand_score[2 * kBlock + lane];
        }
        DIAG_STAMP(6);    // mover: reward provider done
        // (Round 4: the envs are finished in ONE pass at the end, the decided ones together with the parked ones.  Rounds 2-3
        //  finished the decided lanes here and the parked ones behind their verdicts: two passes of the same ~2.5 k-cycle
        //  latency chain -- stores, the reset loads of lanes whose episode ends -- in the waves that end the step, and two
        //  inlined copies of finalize_env_from in a kernel larger than the instruction cache.)
    }
    DIAG_STAMP_W(kWHelper1, 9);   // helper: past the second barrier
    const double vqx = lane < P.n_verts ? qv[2 * lane] : 0.0, vqy = lane < P.n_verts ? qv[2 * lane + 1] : 0.0;   // (row-by-row fallback)
    // (6) every wave settles parked poses, a ticket at a time: exact test, verdict into the record.
    // (Control flow: a scalar loop condition and NO single-lane region around the draw.  With two `if (lane == 0)` regions
    //  per trip hipcc 7.2 threaded lane 0's path across the back edge and split the loop in two; lanes 1..63 then span in
    //  the inner one on ticket 0 for ever while lane 0 waited outside it.  Round 2 kept one such region per trip; round 3
    //  draws with every lane, so no edit or compiler update can bring that shape back.)
    DIAG_STAMP(7);        // mover: decided envs finished
    // (One pose tested by two or three waves -- every n-th row of the footprint's image each, the verdicts meeting in one LDS
    //  add -- when few poses are parked and most waves would find no ticket: measured in round 3, 11.78 against 11.55 us.  The
    //  edge set-up and the cell list are repeated by every share, and a test is not long because of its cells: with three
    //  shares the longest tests still took 6.5 k cycles.)
    // (the draw has no single-lane region: every lane issues an LDS add -- lane 0 adds 1 to the ticket counter, the others add
    //  0 to a word of their own in the wave's cell list, which changes nothing: 64 lanes on ONE word are 64 serialised
    //  atomics, and 16 waves drawing at once cost the step 4 us that way -- and lane 0's returned value is the ticket)
    __attribute__((address_space(3))) int* const ticket_word =
        lane == 0 ? (__attribute__((address_space(3))) int*)&ctl[kCtlTicket] : (__attribute__((address_space(3))) int*)(cell_list + lane);
    int ticket = __builtin_amdgcn_readfirstlane(__hip_atomic_fetch_add(ticket_word, lane == 0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    while (ticket < n_parked) {
        DIAG_STAMP_W(kWHelper1, 10);   // helper: has a ticket
        __attribute__((address_space(3))) ParkedPose* e = rec + ticket;
        const double c = e->c, s = e->s;
        const int px = e->px, py = e->py;
        const int64_t env = ((int64_t)e->env_hi << 32) | (uint32_t)e->env_lo;
        const int64_t g = (SHARED || a.hot.map_shared) ? 0 : (a.hot.geom_of_env ? (int64_t)e->geom : env);
        const uint32_t* words = a.hot.map_bits + g * a.hot.map_env_stride;
        const uint32_t* tiles = a.map_tiles + g * map_tile_words(a.hot.map_rows, a.hot.map_wpr);
        bool h = false;
        [[maybe_unused]] const unsigned long long test_from = DIAG_NOW();
        [[maybe_unused]] int how = 0;
        if (!ABLATED(a, kAblateNoCoop)) {
            // the lethal cells under the image tested one by one; a map too dense for that is rasterised row by row
#ifdef BCP_DIAG
            unsigned long long phase[3] = {test_from, test_from, 0};
            unsigned long long* const phases = phase;
#else
            unsigned long long* const phases = nullptr;
#endif
            const int verdict = (SHARED || map_words)
                ? coop_collides_sparse<WIDE>(P, (LdsF64)qv, c, s, px, py, (LdsWords)lds_map, a.hot.map_rows, a.hot.map_cols,
                                             a.hot.map_wpr, cell_list, phases)
                : coop_collides_sparse<WIDE, true>(P, (LdsF64)qv, c, s, px, py, as_global(tiles), a.hot.map_rows, a.hot.map_cols,
                                                   a.hot.map_wpr, cell_list, phases);
#ifdef BCP_DIAG
            // wave 8's test: cycles for the edge set-up, for listing the cells, for the rest, and the list's length
            if (threadIdx.x == kWHelper1 * 64 && blockIdx.x < 2048) {
                const unsigned long long now = DIAG_NOW();
                g_diag[(2048 + blockIdx.x) * 16 + 13] = ((phase[0] - test_from) << 40) | ((phase[1] - phase[0]) << 20) | (now - phase[1]);
                g_diag[(2048 + blockIdx.x) * 16 + 15] = phase[2];
            }
#endif
            h = verdict == kSparseHit;
            if (verdict == kSparseTooMany)
                h = coop_collides<WIDE>(P, vqx, vqy, c, s, px, py, words, a.hot.map_rows, a.hot.map_cols, a.hot.map_wpr);
            how = verdict;
        }
        DIAG_MAX(0, ((DIAG_NOW() - test_from) << 4) | (unsigned)how);   // the longest exact test of the workgroup, and its kind
        DIAG_STAMP_W(kWHelper1, 11);   // helper: verdict
        bool post = lane == 0;
#ifdef BCP_DIAG
        post = post && !(a.flags & kDiagWithholdVerdicts);
#endif
        if (post) __hip_atomic_store(&e->verdict, h ? 2 : 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        ticket = __builtin_amdgcn_readfirstlane(__hip_atomic_fetch_add(ticket_word, lane == 0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        DIAG_STAMP_W(kWHelper1, 12);   // helper: verdict posted
    }
    // (7) movers: the envs they parked are finished by the lane that holds their state, as soon as the verdicts are in
    //     (every parked pose has been claimed by now -- by this wave or by one that is working on it)
    if (mover) {
        // SHARED: everything the finishing pass takes from the launch, read from LDS in one batch and issued HERE, ahead of
        // the verdict polls, so that it has landed when the verdicts are in: this launch's FinishWords and the state arrays of
        // the LDS copy of *S (the same pointers as StepHot's).  The generic variants fetch them from the launch arguments.
        FinishArgs fin = FinishArgs();
        uint32_t fin_flags = 0;
        if (SHARED) {
            const __attribute__((address_space(3))) FinishWords* fw = (const __attribute__((address_space(3))) FinishWords*)lds_finish_words;
            fin.launch = kernarg;
            fin.noise_z_out = fw->noise_z_out;
            fin.reward = fw->reward;
            fin.done = fw->done;
            fin.collided_now = fw->collided_now;
            fin.err = fw->err;
            fin_flags = fw->flags;
            fin.hot.st.x = SL->st.x;
            fin.hot.st.y = SL->st.y;
            fin.hot.st.angle = SL->st.angle;
            fin.hot.st.v = SL->st.v;
            fin.hot.st.w = SL->st.w;
            fin.hot.st.steer = SL->st.steer;
            fin.hot.st.wheel = SL->st.wheel;
            fin.hot.st.min_dist = SL->st.min_dist;
            fin.hot.st.target_idx = SL->st.target_idx;
            fin.hot.st.cur_iter = SL->st.cur_iter;
            fin.hot.st.collided = SL->st.collided;
        }
        int verdict = park ? 0 : 1;
        {
            int trips = 0;
            while (__ballot(verdict == 0)) {
                if (verdict == 0) verdict = __hip_atomic_load(&my_rec->verdict, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_s_sleep(1);
                if (++trips > kPollLimit) {   // (a verdict that never comes: the env is finished as free, and the step says so)
                    poll_expired = true;
                    if (verdict == 0) {
                        verdict = 1;
                        q.err |= BCP_ERR_INTERNAL;
                    }
                    break;
                }
            }
        }
        // A pose that really collides is rolled back, and the reward provider runs for the OLD pose: the scan for its last
        // reached way point by the whole wave, a candidate per lane (one lane walking the window alone took ~5 k cycles, and
        // the step ends with the workgroups that hold such an env).  Shared path in LDS, continuous provider without delays;
        // otherwise finalize_env_from computes it itself.
        const bool hit_score = PLAIN && (SHARED || lds_path) && (SHARED || a.hot.path_shared) && !ABLATED(a, kAblateNoReward);
        fin.flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)fin_flags);   // (one value for the pass's tests of the flags)
        int last_hit = -1;
        if (hit_score) {
            uint64_t hits = __ballot(park && verdict == 2);
            while (hits) {
                const int src = (int)__ffsll((unsigned long long)hits) - 1;
                hits &= hits - 1;
                const double ox = bcast_d(q.old.x, src), oy = bcast_d(q.old.y, src), oth = bcast_d(q.old.th, src);
                const int tg = bcast_i(q.target, src);
                const PathWindow w = path_window(P, (LdsF64)lds_box, (const __attribute__((address_space(3))) int16_t*)lds_index, ox, oy);
                const int found = coop_last_reached(P, lds_path, w, my_len, tg, ox, oy, oth);
                if (lane == src) last_hit = found;
            }
        }
        if (active) {
            const bool hit_now = park && verdict == 2;
            bool fits = hit_score && hit_now;
            if (fits) {
                sc.min_dist = q.min_dist;
                sc.target = q.target;
                sc.rew = reward_from_last(P, lds_path, my_len, last_hit, q.old.x, q.old.y, sc.min_dist, sc.target);
            } else if (!SHARED && PLAIN && hit_now && my_rec->spec_ok) {   // (private path: worked out ahead, see above)
                sc.rew = my_rec->spec_rew;
                sc.min_dist = my_rec->spec_min;
                sc.target = my_rec->spec_target;
                fits = true;
            }
            if (!PLAIN) {
#pragma unroll
                for (int k = 0; k < 3; ++k) q.popped_pose[k] = fifo_stash[k * kLocalEnvs];
#pragma unroll
                for (int k = 0; k < 7; ++k) q.popped_state[k] = fifo_stash[(3 + k) * kLocalEnvs];
            }
            if constexpr (SHARED)
                finalize_env_from<PLAIN, SHARED>(fin, SL, i, q, hit_now, lds_path, nullptr, !ABLATED(a, kAblateNoReward), sc, my_len, fits, out_base);
            else
                finalize_env_from<PLAIN, SHARED>(a, SL, i, q, hit_now, lds_path, nullptr, !ABLATED(a, kAblateNoReward), sc, my_len, fits, out_base);
        }
        // Episode record: the step's count can only be published once every mover has taken its slots, so with a record the
        // last mover of the workgroup (ctl[kCtlMoversDone], an LDS count) draws the step's ticket in place of the wave below -- one
        // global atomic per workgroup, as without a record; the last workgroup moves the counter on and publishes the count.
        if (((SHARED ? fin.flags : a.flags) & kStepRecord) && lane == 0 &&
            __hip_atomic_fetch_add(&ctl[kCtlMoversDone], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == kLocalPairs - 1) {
            __threadfence();
            unsigned int* ticket = reinterpret_cast<unsigned int*>(a.tick + kTickLocalTicket);
            if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
                *ticket = 0u;
                a.tick[0] = a.tick[0] + 1;   // (every workgroup read the counter before it drew; movers never hold it)
                record_store_count(a.S->rec);
            }
        }
    }
    DIAG_STAMP(13);            // mover: out of tickets
    DIAG_STAMP_W(kWHelper1, 14);       // helper: out of tickets
#ifdef BCP_DIAG
    if (tid == 0 && blockIdx.x < kDiagBlocks) g_diag[blockIdx.x * 16 + 15] = (unsigned long long)n_parked;
#endif
    if (poll_expired && lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.tick + 4), 1ull);   // (bcp_expired_waits)
    DIAG_REAL_EXIT();
    // The last workgroup to get here moves the step counter on (every workgroup has read it long before it draws).  The ticket
    // has a cache line of its own, and it is drawn HERE, in the last instructions of a wave that is done before the movers are:
    // measured in round 4 (tools/step_time.py, builds side by side on one box) -- no ticket at all, workgroup 0 moving the
    // counter on: 11.7 us against 11.8 with the ticket, i.e. it hides behind the movers; the ticket drawn early (behind barrier
    // 0 or barrier 1, looked at here): 13.3 - 13.8 us -- 256 workgroups draw at the same moment, the returning atomics queue
    // at the memory side (~10 ns each on one address), and the drawing wave waits for its ticket at its next wait of any kind,
    // which holds up its share of the way-point scan and with it its pair's mover; a second atomic per workgroup on the
    // ticket's line (the parked-pose count, first form): 14.3 us.  The parked poses are counted in a word per workgroup instead.
    if ((a.flags & kStepAdvances) && tid == (kLocalWaves - 1) * kBlock) {
        if (n_parked) a.parked_slots[blockIdx.x] += (uint64_t)n_parked;   // (this workgroup's word: no atomic; bcp_parked_poses adds them up)
        if ((!ROLL || rs == a.rollout_steps - 1) && !(a.flags & kStepRecord)) {   // (with a record: the movers draw, above)
            const unsigned int ticket_drawn =
                __hip_atomic_fetch_add((GlobalPtr<unsigned int>)(a.tick + kTickLocalTicket), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ticket_drawn == gridDim.x - 1) {
                *reinterpret_cast<unsigned int*>(a.tick + kTickLocalTicket) = 0u;
                a.tick[0] = step_counter + 1;
            }
        }
    }
}

// A rollout's trips are CALLS of one out-of-line copy of the step: written as a loop around the inlined body the compiler
// hoisted the body's loop-invariant values -- launch arguments, addresses, the few hundred float64 constants of its
// transcendental functions -- in front of the loop and carried them across it (300 - 500 scalar and ~100 vector spills,
// 300 bytes of scratch per lane); a call boundary keeps every trip's code what the one-step kernel's is.
template <bool WIDE, bool PLAIN, int PAIRS>
__device__ __attribute__((noinline)) void step_local_trip(uint64_t kernarg_bits, int rs)
{
    // (arguments of a device function arrive in vector registers: the address of the launch arguments and the trip number are
    //  made scalar again.  The kernarg-segment builtin is no way to the arguments from inside a callee: the first form of
    //  this function used it and read address 0.)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)kernarg_bits);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(kernarg_bits >> 32));
    step_local_body<WIDE, PLAIN, PAIRS, true>((KernArgPtr)(uintptr_t)(((uint64_t)hi << 32) | lo), __builtin_amdgcn_readfirstlane(rs));
}

template <bool WIDE, bool PLAIN, int PAIRS, bool ROLL = false, bool SHARED = false>
__global__ void __attribute__((amdgpu_flat_work_group_size(4 * PAIRS * kBlock, 4 * PAIRS * kBlock), amdgpu_waves_per_eu(4)))
step_local_kernel(const StepArgs launch_args)
{
    KernArgPtr kernarg = (KernArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    if constexpr (!ROLL) {
        step_local_body<WIDE, PLAIN, PAIRS, false, SHARED>(kernarg, 0);
    } else {
        const int n_steps = kernarg->rollout_steps;
        for (int rs = 0; rs < n_steps; ++rs) {
            step_local_trip<WIDE, PLAIN, PAIRS>((uint64_t)(uintptr_t)kernarg, rs);
            // the next step: the control words, the hand-over buffers and the parked records are rewritten from here on, and the
            // scanners read what this step's movers have just stored (workgroup scope: the waves share the compute unit's L1)
            __syncthreads();
        }
    }
}

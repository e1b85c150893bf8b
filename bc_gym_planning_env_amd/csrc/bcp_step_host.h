// bcp_step_host.h -- the host side of the step: which form a step takes, the device-resident parameter block, the launcher,
// the methods of Parking and WaitWatchdog, and the entry points built on them (bcp_step, bcp_rollout, the timing calls).
// The kernels are in bcp_step.h (behind the bcp_step_*.h it includes), the LDS they get in bcp_step_layout.h.  Included by bcplan.hip after bcp_field.h; the planners, which step nothing, are in
// bcp_plan_host.h behind it.
#pragma once

// no delay queues and the continuous reward provider: the step kernels compile both out (their PLAIN variants)
static bool step_is_plain(const bcp_handle* h)
{
    const bcp_params& p = h->params;
    return p.control_delay == 0 && p.pose_delay == 0 && p.state_delay == 0 && p.reward_provider == BCP_REWARD_CONTINUOUS;
}

static bool step_uses_deferral(const bcp_handle* h)
{
    return h->tune.defer && h->cull.on && h->tune.exact_mode == 0 && h->parking.slots() != nullptr;
}

// Which kernels a step of this handle launches as it is configured now -- the numbers bcp_step_form documents: 0 step_kernel,
// 1 step_fast_pair_kernel alone, 2 that + step_pending_kernel, 3 step_local_kernel (the single-launch form).  Once
// upload_step_static has run, S.pending != nullptr says the same as step_uses_deferral.
// (an explicit BCP_TUNE_DENSE_THRESHOLD asks for poses to be settled inside the stepping wave: the two-launch form has that
// path, and bcp_set_tuning clears `adaptive` with it -- form 3 never meets a negative threshold)
static int step_form(const bcp_handle* h)
{
    if (!step_uses_deferral(h)) return 0;
    if (h->tune.dense_threshold < 0) return 1;
    return (h->tune.fused && h->tune.adaptive) ? 3 : 2;
}

// (re)builds the device-resident StepStatic block and, from it, the StepHot image that every launch copies
static int upload_step_static(bcp_handle* h, hipStream_t s)
{
    StepStatic& S = h->host_static;
    S.P = h->dev;
    S.map = h->map;
    S.cull = h->cull;
    S.path = h->path;
    S.st = h->st;
    S.init = h->init;
    S.n = h->n;
    S.env_id_base = h->env_id_base;
    S.exact_mode = h->tune.exact_mode;
    S.dense_threshold = h->tune.dense_threshold;   // (a negative value settles every undecided pose inside kernel 1)
    S.wide = h->wide;
    S.pending_cap = h->parking.slots_per_shard();
    const bool defer = step_uses_deferral(h);
    S.pending = defer ? h->parking.slots() : nullptr;
    S.geom_of_env = h->n_geoms > 0 ? h->geom_of_env : nullptr;
    S.next_geom = h->n_geoms > 0 ? h->next_geom : nullptr;
    S.lds_path_doubles =
        (defer && h->path.shared && h->path.max_len * kWayPointDoubles * sizeof(double) <= kPathLdsBytes) ? h->path.max_len * kWayPointDoubles : 0;
    if (h->have_rec) {
        BCP_TRY(h->parking.record_slots(defer, &h->rec.park));
        S.rec = h->rec;
    } else {
        memset(&S.rec, 0, sizeof(S.rec));
    }
    // a declared uniform initial state: the handle's snapshot (the kernels read it behind kStepInitUniform only)
    memset(&S.init_uniform, 0, sizeof(S.init_uniform));
    if (h->init_declared) S.init_uniform = h->init_snapshot;
    HIP_TRY(h->dev_static.reserve(1));
    // pageable source: the copy is staged before the call returns, so host_static may change afterwards
    HIP_TRY(hipMemcpyAsync(h->dev_static.get(), &S, sizeof(StepStatic), hipMemcpyHostToDevice, s));
    StepHot& hot = h->host_hot;   // (io_flags, io_actions, io_noise_z and io_tick belong to a launch: launch_step)
    hot.st = S.st;
    hot.n = S.n;
    hot.geom_of_env = S.geom_of_env;
    hot.path_pts = S.path.pts;
    hot.path_pre = S.path.pre;
    hot.path_bbox = S.path.bbox;
    hot.path_index = S.path.index;
    hot.pending = S.pending;
    hot.map_bits = S.map.bits;
    hot.map_env_stride = S.map.env_stride;
    hot.model = S.P.model;
    hot.lds_path_doubles = S.lds_path_doubles;
    hot.path_shared = S.path.shared;
    hot.pending_cap = S.pending_cap;
    hot.map_rows = S.map.rows;
    hot.map_cols = S.map.cols;
    hot.map_wpr = S.map.wpr;
    hot.map_shared = S.map.shared;
    hot.path_max_len = S.path.max_len;
    hot.near = S.cull.on ? S.cull.step_near : nullptr;
    hot.noise_on = S.P.noise_on;
    hot.n_verts = S.P.n_verts;
    hot.control_delay = S.P.control_delay;
    hot.pose_delay = S.P.pose_delay;
    hot.state_delay = S.P.state_delay;
    hot.dynamic_model = S.P.dynamic_model;
    hot.noise_slot0 = (S.P.alpha[0] > 0.0 || S.P.alpha[1] > 0.0) ? 1 : 0;
    hot.model_front_column_pid = S.P.model_front_column_pid;
    hot.env_id_base = S.env_id_base;
    hot.qverts = &h->dev_static.get()->P.qverts[0][0];
    hot.map_origins = S.map.origins;
    h->static_dirty = false;
    return BCP_OK;
}

// ---- Parking (declared in bcp_host.h) ---------------------------------------------------------------------------
// The parity-keyed parking / adaptation counters are only maintained by the two-kernel step (kernel 1 zeroes the NEXT
// step's set), so whoever restarts the count of steps (bcp_seed) or resumes that form after another re-arms both sets.
inline int Parking::arm(int32_t threshold, hipStream_t s)
{
    if (pending_count.get()) HIP_TRY(hipMemsetAsync(pending_count.get(), 0, 2 * kShards * sizeof(int32_t), s));
    if (adapt.get()) {
        HIP_TRY(hipMemsetAsync(adapt.get() + 2, 0, 2 * kShards * sizeof(int32_t), s));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)adapt.get(), threshold, 2, s));
    }
    return BCP_OK;
}

inline int Parking::bind(int64_t n_envs, int32_t threshold, hipStream_t s)
{
    if (pending.get()) return BCP_OK;
    const int64_t blocks = (n_envs + kBlock - 1) / kBlock;
    cap = (int32_t)(((blocks + kShards - 1) / kShards) * kBlock);  // every env of a shard's blocks
    HIP_TRY(pending_count.reserve(2 * kShards));
    HIP_TRY(adapt.reserve(2 + 2 * kShards));
    BCP_TRY(arm(threshold, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the first bind has always returned with the counters in place)
    // (last: the slots mark this block as done, so a failure above is met again by the next call)
    HIP_TRY(pending.reserve((size_t)kShards * cap));
    return BCP_OK;
}

// Whenever the step form changes (bcp_set_tuning between steps, a costmap without distance field, ...) both sets are
// re-armed on the stream of the steps, so the two-kernel step never resumes on stale counts.
inline int Parking::step_takes_form(int form, int32_t threshold, hipStream_t s)
{
    if ((form == 1 || form == 2) && (last_form == 0 || last_form == 3)) BCP_TRY(arm(threshold, s));
    last_form = form;
    return BCP_OK;
}

inline int Parking::record_slots(bool defer, RecPark** out)
{
    if (defer) HIP_TRY(rec_park.reserve((size_t)kShards * cap));   // (cap never changes)
    *out = defer ? rec_park.get() : nullptr;
    return BCP_OK;
}

// The two launches of step form 2, <WIDE, PLAIN>, indexed by variant = WIDE << 1 | PLAIN like local_step_fn below
static const void* const kFastPairFn[4] = {(const void*)step_fast_pair_kernel<false, false>, (const void*)step_fast_pair_kernel<false, true>,
                                           (const void*)step_fast_pair_kernel<true, false>, (const void*)step_fast_pair_kernel<true, true>};
static const void* const kPendingFn[4] = {(const void*)step_pending_kernel<false, false>, (const void*)step_pending_kernel<false, true>,
                                          (const void*)step_pending_kernel<true, false>, (const void*)step_pending_kernel<true, true>};

// The shared-geometry variant of step_local_kernel (SHARED, bcp_step.h) takes for granted what this asks: one map for all
// envs, staged in LDS; one path, staged in LDS; no geometry pool, no per-env origins; the 1-bit `near` tiles.  (C2, C3, the
// sharded C5, every replica batch.)  BCP_TUNE_LOCAL_SHARED = 0 keeps a handle on the generic variant.
static bool local_step_shared(const bcp_handle* h, const StepStatic& S)
{
    return h->tune.local_shared != 0 && staged_map_words(S.map.shared != 0, S.map.rows, S.map.wpr) > 0 && S.path.shared &&
           S.lds_path_doubles > 0 && S.geom_of_env == nullptr && S.map.origins == nullptr && S.cull.on && S.cull.step_near != nullptr;
}

// step_local_kernel<WIDE, PLAIN, PAIRS, ROLL, SHARED>: variant = WIDE << 1 | PLAIN; the rollout form and the shared-geometry
// variant exist for the 16-wave workgroup
static const void* local_step_fn(int variant, int pairs, bool roll = false, bool shared = false)
{
    if (shared) {   // (the caller has looked: 16-wave workgroups, one step per launch)
        switch (variant) {
            case 3: return (const void*)step_local_kernel<true, true, 4, false, true>;
            case 2: return (const void*)step_local_kernel<true, false, 4, false, true>;
            case 1: return (const void*)step_local_kernel<false, true, 4, false, true>;
            default: return (const void*)step_local_kernel<false, false, 4, false, true>;
        }
    }
    if (roll) {
        switch (variant) {
            case 3: return (const void*)step_local_kernel<true, true, 4, true>;
            case 2: return (const void*)step_local_kernel<true, false, 4, true>;
            case 1: return (const void*)step_local_kernel<false, true, 4, true>;
            default: return (const void*)step_local_kernel<false, false, 4, true>;
        }
    }
#define BCP_LOCAL_FN(W, P) (pairs == 4 ? (const void*)step_local_kernel<W, P, 4> : pairs == 2 ? (const void*)step_local_kernel<W, P, 2> \
                                                                                              : (const void*)step_local_kernel<W, P, 1>)
    switch (variant) {
        case 3: return BCP_LOCAL_FN(true, true);
        case 2: return BCP_LOCAL_FN(true, false);
        case 1: return BCP_LOCAL_FN(false, true);
        default: return BCP_LOCAL_FN(false, false);
    }
#undef BCP_LOCAL_FN
}

// Size of step_local_kernel's workgroups for this handle: BCP_TUNE_LOCAL_PAIRS, or (0) the default of the configuration.
static int local_pairs(const bcp_handle* h)
{
    const int32_t pairs = h->tune.local_pairs;
    if (pairs == 1 || pairs == 2 || pairs == 4) return pairs;
    return kLocalPairsDefault;
}

// rollout_steps > 1: only the single-launch form (step_local_kernel<.., ROLL = true>) takes several steps per launch; the
// caller (bcp_rollout) steps the other forms one launch at a time.
static int launch_step(bcp_handle* h, const bcp_step_io* io, uint32_t flags, hipStream_t s, bool first_only = false,
                       int32_t rollout_steps = 1)
{
    if (h->static_dirty) BCP_TRY(upload_step_static(h, s));
    const StepStatic& S = h->host_static;
    const int form = step_form(h);
    const bool fused = form == 3;
    if (!fused && h->field.has_stale_fields()) BCP_TRY(h->field.ensure_fields(h, s));   // these forms read the uint8 field
    BCP_TRY(h->parking.step_takes_form(form, h->tune.dense_threshold, s));
    StepArgs a;
    a.S = h->dev_static.get();
    a.hot = h->host_hot;
    a.actions = io->actions;
    a.noise_z = io->noise_z;
    a.noise_z_out = io->noise_z_out;
    a.reward = io->reward;
    a.done = io->done;
    a.collided_now = io->collided_now;
    a.err = io->err;
    a.flags = flags;
    if (h->have_rec) a.flags |= kStepRecord;   // (the kernels look at the record only with this flag)
    // the step counter and the noise seed are read on the device (StepArgs::tick); the kernels resolve these themselves
    a.seed = a.step_counter = 0;
    a.pending_count = a.pending_next = nullptr;
    a.threshold_now = nullptr;
    a.threshold_next = a.inplace_count = a.inplace_next = nullptr;
    const bool adapt = h->tune.adaptive && h->parking.thresholds() && S.pending && S.dense_threshold >= 0;
    a.tick = h->tick.get();
    a.parked_slots = nullptr;
    a.map_tiles = S.map.tiles;
    a.rollout_steps = 1;
    a.pending_base = h->parking.counters();
    a.adapt_base = adapt ? h->parking.thresholds() : nullptr;
    const int blocks = (int)((h->n + kBlock - 1) / kBlock);
    const int variant = (S.wide ? 2 : 0) | (step_is_plain(h) ? 1 : 0);
    if (fused) {
        // the whole step as one launch: 256 envs per workgroup of 16 waves; undecided poses are handed over in LDS and
        // settled by all the workgroup's waves (step_local_kernel)
        const bool roll = rollout_steps > 1;
        const int pairs = roll ? 4 : local_pairs(h);
        a.rollout_steps = rollout_steps;
        const size_t lds = local_lds_plan(h->params.n_verts, S.lds_path_doubles, staged_map_words(S.map.shared != 0, S.map.rows, S.map.wpr),
                                          step_is_plain(h), pairs).bytes;
        a.flags |= kStepAdvances;
        const bool shared = pairs == 4 && !roll && local_step_shared(h, S);
        // resets from the declared uniform initial state in the LDS copy of *S: the shared-geometry variant alone
        const bool uniform_reset = shared && h->init_declared && (flags & BCP_STEP_AUTO_RESET);
        if (uniform_reset) a.flags |= kStepInitUniform;
        a.hot.io_flags = a.flags;   // (the prologue's copies, next to the rest of what it fetches)
        a.hot.io_actions = a.actions;
        a.hot.io_noise_z = a.noise_z;
        a.hot.io_tick = a.tick;
        const int envs_per_group = pairs * kBlock;
        const dim3 grid((unsigned)((h->n + envs_per_group - 1) / envs_per_group)), block(4 * pairs * kBlock);
        if (!h->parked_slots.get()) {   // (sized for the smallest workgroup: the size may change between steps)
            HIP_TRY(h->parked_slots.reserve((size_t)((h->n + kBlock - 1) / kBlock)));
            HIP_TRY(hipMemsetAsync(h->parked_slots.get(), 0, h->parked_slots.capacity() * sizeof(uint64_t), s));
        }
        a.parked_slots = h->parked_slots.get();
        h->last_local_shared = shared ? 1 : 0;
        h->last_uniform_reset = uniform_reset ? 1 : 0;
        return launch_variant(h, local_step_fn(variant, pairs, roll, shared), grid, block, lds, s, a);
    }
    h->last_local_shared = 0;
    h->last_uniform_reset = 0;
    if (rollout_steps > 1) return fail(BCP_E_STATE, "launch_step: only the single-launch step form takes several steps per launch");
    if (form == 0) {
        const size_t lds = collision_lds_bytes(h->params.n_verts, h->map.in_lds, h->map.rows, h->map.wpr);
        a.flags |= kStepAdvances;
        hipLaunchKernelGGL(step_kernel, dim3(blocks), dim3(kBlock), lds, s, a);
        return BCP_OK;
    }
    // kernel 1 settles every env the distance field decides; kernel 2 rasterises the parked rest
    const int waves = 2048;  // a multiple of kShards: 32 teams per shard, so that a shard rarely needs a second round
    const bool second = !first_only && S.dense_threshold >= 0;  // (threshold < 0: everything settled in place)
    if (!second) a.flags |= kStepAdvances;   // kernel 1 is the whole step
    // kernel 1 runs with two wavefronts per 64 envs (mover + scorer, step_fast_pair_kernel)
    const int rc = launch_variant(h, kFastPairFn[variant], dim3(blocks), dim3(2 * kBlock), pair_lds_plan(h->params.n_verts, S.lds_path_doubles).bytes, s, a);
    if (rc != BCP_OK || !second) return rc;
    return launch_variant(h, kPendingFn[variant], dim3(waves), dim3(kBlock * kPendingWaves), pending_lds_bytes(S.wide != 0), s, a);
}

// Flags a caller may pass.  The ablation switches of bcp_diag.h (timing experiments, results wrong by construction)
// exist only in a -DBCP_DIAG build (tools/); kStepAdvances is internal and never accepted.
#ifdef BCP_DIAG
constexpr uint32_t kCallerFlags = BCP_STEP_AUTO_RESET | BCP_STEP_ACTIONS_F32 | kAblateNoCollision | kAblateNoReward |
                                  kAblateNoCoop | kAblateNoPark | kAblateNoClassify | kDiagWithholdVerdicts;
#else
constexpr uint32_t kCallerFlags = BCP_STEP_AUTO_RESET | BCP_STEP_ACTIONS_F32;
#endif

static int check_step(bcp_handle* h, const bcp_step_io* io, uint32_t flags, const char* who)
{
    if (!h || !io) return fail(BCP_E_INVALID, "%s: null argument", who);
    if (flags & ~kCallerFlags) return fail(BCP_E_INVALID, "%s: undefined flag bits 0x%x", who, flags & ~kCallerFlags);
    if (!h->have_map || !h->have_path || !h->have_state)
        return fail(BCP_E_STATE, "%s: costmaps, paths and state must be set first", who);
    if ((flags & BCP_STEP_AUTO_RESET) && !h->have_init)
        return fail(BCP_E_STATE, "%s: BCP_STEP_AUTO_RESET needs bcp_bind_initial_state", who);
    if (!io->actions || !io->reward || !io->done) return fail(BCP_E_INVALID, "%s: actions/reward/done are required", who);
    return BCP_OK;
}

// A wait of step_local_kernel that gives up lets its envs finish as free (bcp_step.h: BCP_ERR_INTERNAL): a training loop
// that never calls bcp_expired_waits would not notice.  So bcp_step itself looks, without ever waiting for the GPU: every
// kWatchdogSteps calls the counter is copied to pinned host memory behind the step just launched, and a later call, once
// that copy has landed, compares it with what was seen before.
constexpr uint32_t kWatchdogSteps = 256;

inline int WaitWatchdog::after_step(bcp_handle* h, hipStream_t s)
{
    if (step_form(h) != 3) return BCP_OK;   // (only step_local_kernel has such waits)
    if (in_flight) {
        const hipError_t q = hipEventQuery(event.get());
        if (q == hipSuccess) {
            in_flight = false;
            const uint64_t now = *host.get();
            if (now > seen) {
                const uint64_t fresh = now - seen;
                seen = now;
                return fail(BCP_E_INTERNAL, "bcp_step: %llu bounded wait(s) of the step kernel gave up during earlier steps "
                                            "(BCP_ERR_INTERNAL in err[] marks the envs; their verdicts are unreliable)",
                            (unsigned long long)fresh);
            }
        } else {
            (void)hipGetLastError();   // hipErrorNotReady is not an error here
        }
        return BCP_OK;
    }
    if (++steps_since_probe < kWatchdogSteps) return BCP_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return BCP_OK;   // (a captured step is replayed without this function: the caller asks bcp_expired_waits)
    }
    if (!host) {
        HIP_TRY(hipHostMalloc((void**)host.put(), sizeof(uint64_t), hipHostMallocDefault));
        *host.get() = 0;
        HIP_TRY(hipEventCreateWithFlags(event.put(), hipEventDisableTiming));
    }
    HIP_TRY(hipMemcpyAsync(host.get(), h->tick.get() + 4, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(event.get(), s));
    in_flight = true;
    steps_since_probe = 0;
    return BCP_OK;
}

extern "C" int bcp_step(bcp_handle* h, const bcp_step_io* io, uint32_t flags, void* stream)
{
    BCP_TRY(check_step(h, io, flags, "bcp_step"));
    HIP_TRY(hipSetDevice(h->device));
    BCP_TRY(launch_step(h, io, flags, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return h->watchdog.after_step(h, (hipStream_t)stream);
}

// K steps per call for callers that hold the actions of a whole rollout (Monte-Carlo rollouts from one state, the use the
// reference documents: /root/reference/README.md "many rollouts from one state"; StepEnvRoller's 128-step rollouts once the
// policy is open-loop).  With the single-launch step form the K steps are ONE launch of step_local_kernel<.., ROLL = true>;
// otherwise K launches.  Either way: the states and outputs of K calls of bcp_step with row k of the arrays, bit for bit.
extern "C" int bcp_rollout(bcp_handle* h, const bcp_step_io* io, int32_t n_steps, uint32_t flags, void* stream)
{
    BCP_TRY(check_step(h, io, flags, "bcp_rollout"));
    if (n_steps <= 0) return fail(BCP_E_INVALID, "bcp_rollout: n_steps must be positive");
    if (h->have_rec) return fail(BCP_E_STATE, "bcp_rollout: an episode record is bound (rows over K steps are not kept)");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (step_form(h) == 3 && n_steps > 1) {
        BCP_TRY(launch_step(h, io, flags, s, false, n_steps));
        HIP_TRY(hipGetLastError());
        return BCP_OK;
    }
    const int64_t n = h->n;
    const size_t act = (flags & BCP_STEP_ACTIONS_F32) ? 8 : 16;
    for (int32_t k = 0; k < n_steps; ++k) {
        bcp_step_io row = *io;
        row.actions = (const char*)io->actions + (size_t)k * n * act;
        if (io->noise_z) row.noise_z = io->noise_z + (size_t)k * n * 3;
        if (io->noise_z_out) row.noise_z_out = io->noise_z_out + (size_t)k * n * 3;
        row.reward = io->reward + (size_t)k * n;
        row.done = io->done + (size_t)k * n;
        if (io->collided_now) row.collided_now = io->collided_now + (size_t)k * n;
        if (io->err) row.err = io->err + (size_t)k * n;
        BCP_TRY(launch_step(h, &row, flags, s));
    }
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_expired_waits(bcp_handle* h, int64_t* count, void* stream)
{
    if (!h || !count) return fail(BCP_E_INVALID, "bcp_expired_waits: null argument");
    HIP_TRY(hipSetDevice(h->device));
    uint64_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->tick.get() + 4, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *count = (int64_t)v;
    return BCP_OK;
}

extern "C" int bcp_parked_poses(bcp_handle* h, int64_t* count, void* stream)
{
    if (!h || !count) return fail(BCP_E_INVALID, "bcp_parked_poses: null argument");
    HIP_TRY(hipSetDevice(h->device));
    *count = 0;
    if (!h->parked_slots.get()) return BCP_OK;
    std::vector<uint64_t> slots(h->parked_slots.capacity());
    HIP_TRY(hipMemcpyAsync(slots.data(), h->parked_slots.get(), slots.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    uint64_t sum = 0;
    for (uint64_t v : slots) sum += v;
    *count = (int64_t)sum;
    return BCP_OK;
}

extern "C" int bcp_step_shared_variant(bcp_handle* h)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_step_shared_variant: null handle");
    return h->last_local_shared;
}

extern "C" int bcp_step_uniform_reset(bcp_handle* h)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_step_uniform_reset: null handle");
    return h->last_uniform_reset;
}

extern "C" int bcp_step_form(bcp_handle* h)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_step_form: null handle");
    if (!h->have_map || !h->have_path || !h->have_state) return fail(BCP_E_STATE, "bcp_step_form: costmaps, paths and state must be set first");
    return step_form(h);
}

// average device time of `steps` back-to-back step launches on `s` (first_only: of kernel 1 of the two-launch form alone)
static int time_loop(bcp_handle* h, const bcp_step_io* io, uint32_t flags, int steps, hipStream_t s, bool first_only,
                     float* avg_ms)
{
    OwnedEvent e0, e1;   // (destroyed on every way out)
    HIP_TRY(hipEventCreate(e0.put()));
    HIP_TRY(hipEventCreate(e1.put()));
    HIP_TRY(hipEventRecord(e0.get(), s));
    int rc = BCP_OK;
    for (int k = 0; k < steps && rc == BCP_OK; ++k) rc = launch_step(h, io, flags, s, first_only);
    HIP_TRY(hipEventRecord(e1.get(), s));
    HIP_TRY(hipEventSynchronize(e1.get()));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0.get(), e1.get()));
    HIP_TRY(hipGetLastError());
    if (rc != BCP_OK) return rc;
    *avg_ms = ms / (float)steps;
    return BCP_OK;
}

extern "C" int bcp_time_steps(bcp_handle* h, const bcp_step_io* io, uint32_t flags, int32_t steps, void* stream,
                              float* avg_ms)
{
    BCP_TRY(check_step(h, io, flags, "bcp_time_steps"));
    if (steps <= 0 || !avg_ms) return fail(BCP_E_INVALID, "bcp_time_steps: steps must be positive");
    HIP_TRY(hipSetDevice(h->device));
    return time_loop(h, io, flags, steps, (hipStream_t)stream, false, avg_ms);
}

extern "C" int bcp_time_step_kernels(bcp_handle* h, const bcp_step_io* io, uint32_t flags, int32_t steps, void* stream,
                                     float* kernel_ms)
{
    BCP_TRY(check_step(h, io, flags, "bcp_time_step_kernels"));
    if (steps <= 0 || !kernel_ms) return fail(BCP_E_INVALID, "bcp_time_step_kernels: bad steps / output");
    if (h->have_rec)   // (its kernel-1-only loop would take record slots that no launch publishes)
        return fail(BCP_E_STATE, "bcp_time_step_kernels: an episode record is bound");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    // full steps first (the state advances), then the same number of kernel-1-only launches on the reached state:
    // envs parked by a lone step_kernel are never finished, so every launch of that loop sees the same batch.
    float full = 0, first = 0;
    BCP_TRY(time_loop(h, io, flags, steps, s, false, &full));
    if (bcp_step_form(h) != 2) {   // the step is ONE launch (step_local_kernel, step_kernel): nothing to split, and no second loop
        kernel_ms[0] = full;
        kernel_ms[1] = 0.0f;
        return BCP_OK;
    }
    BCP_TRY(time_loop(h, io, flags, steps, s, true, &first));
    kernel_ms[0] = first;
    kernel_ms[1] = full > first ? full - first : 0.0f;
    return BCP_OK;
}

// bcp_track_host.h -- the host side of bcp_track and bcp_track_profile: the checks and the two launches (kernels in
// bcp_track.h, the argument rules in bcp_track_law.h: track_check_args).  Included by bcplan.hip after bcp_plan_host.h
// (plan_ready).
#pragma once

// K gain settings of the path tracker per env, rolled out on private copies of the env's state.  Like bcp_lookahead it reads
// the handle and writes only the caller's outputs.  profile: nullptr (bcp_track), or the speeds bcp_track_profile checked.
static int track_launch(bcp_handle* h, const bcp_track_params* p, const bcp_track_io* io, const double* profile, uint32_t flags,
                        void* stream, const char* who)
{
    if (!h || !p || !io) return fail(BCP_E_INVALID, "%s: null argument", who);
    constexpr uint32_t allowed = BCP_STEP_ACTIONS_F32 | BCP_LOOKAHEAD_PER_ENV;
    if (flags & ~allowed) return fail(BCP_E_INVALID, "%s: undefined flag bits 0x%x", who, flags & ~allowed);
    hipStream_t s = (hipStream_t)stream;
    BCP_TRY(plan_ready(h, who, s));
    if (h->params.reward_provider != BCP_REWARD_CONTINUOUS)
        return fail(BCP_E_INVALID, "%s: the pure-pursuit reward provider is not supported (the tracker reads target_idx as "
                                   "the next way point to reach, which only the continuous provider keeps)", who);
    int d = 0;
    switch (track_check_args(p->horizon, p->n_candidates, p->max_curvature, p->low, p->high,
                             io->gains && io->actions && io->ret && io->steps && io->reason, io->best != nullptr,
                             io->best_plan || io->best_action, h->n, &d)) {
    case kTrackOk: break;
    case kTrackShape: return fail(BCP_E_INVALID, "%s: horizon and n_candidates must be at least 1", who);
    case kTrackCurvature: return fail(BCP_E_INVALID, "%s: max_curvature must be positive and finite", who);
    case kTrackBoxFinite: return fail(BCP_E_INVALID, "%s: the action box must be finite", who);
    case kTrackBoxOrder: return fail(BCP_E_INVALID, "%s: low[%d] > high[%d]", who, d, d);
    case kTrackNull: return fail(BCP_E_INVALID, "%s: gains / actions / ret / steps / reason are required", who);
    case kTrackBest: return fail(BCP_E_INVALID, "%s: best_plan and best_action need best", who);
    default: return fail(BCP_E_INVALID, "%s: n_envs * n_candidates * horizon is too large for 64-bit element offsets", who);
    }
    const int64_t total = h->n * p->n_candidates;
    const int64_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFF) return fail(BCP_E_INVALID, "%s: n_envs * n_candidates exceeds the largest grid (2^37 lanes)", who);
    TrackArgs a;
    a.S = h->dev_static.get();
    a.gains = io->gains;
    a.mask = io->mask;
    a.actions = io->actions;
    a.ret = io->ret;
    a.steps = io->steps;
    a.reason = io->reason;
    a.final_pose = io->final_pose;
    a.final_target = io->final_target_idx;
    a.err = io->err;
    a.trace = io->trace;
    a.best = io->best;
    a.best_plan = io->best_plan;
    a.best_action = io->best_action;
    a.n = h->n;
    a.total = total;
    a.horizon = p->horizon;
    a.k = p->n_candidates;
    a.flags = flags;
    for (int c = 0; c < 2; ++c) {
        a.low[c] = p->low[c];
        a.high[c] = p->high[c];
    }
    a.max_curvature = p->max_curvature;
    a.profile = profile;
    const size_t lds = collision_lds_bytes(h->params.n_verts, h->map.in_lds, h->map.rows, h->map.wpr);
    const void* fn = profile ? (const void*)track_kernel<true> : (const void*)track_kernel<false>;
    BCP_TRY(launch_variant(h, fn, dim3((unsigned)blocks), dim3(kBlock), lds, s, a));
    if (io->best) {
        int group = 1;
        while (group < 64 && group < p->n_candidates) group <<= 1;
        const int64_t lanes = h->n * group;
        hipLaunchKernelGGL(track_best_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a, group);
    }
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_track(bcp_handle* h, const bcp_track_params* p, const bcp_track_io* io, uint32_t flags, void* stream)
{
    return track_launch(h, p, io, nullptr, flags, stream, "bcp_track");
}

// bcp_track with step 4 of the law reading a speed per way point (bcp_path_speed's output, or anyone's), laid out as the
// bound paths.  The pointer travels in the launch arguments like the caller's other pointers.
extern "C" int bcp_track_profile(bcp_handle* h, const bcp_track_params* p, const bcp_track_io* io, const bcp_track_profile_io* prof,
                                 uint32_t flags, void* stream)
{
    const char* who = "bcp_track_profile";
    if (!prof || !prof->speed) return fail(BCP_E_INVALID, "%s: null profile", who);
    if (h && h->have_path && prof->max_len != h->path.max_len)
        return fail(BCP_E_INVALID, "%s: the profile's max_len %d is not the bound paths' %d", who, prof->max_len, h->path.max_len);
    return track_launch(h, p, io, prof->speed, flags, stream, who);
}

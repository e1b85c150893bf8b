// bcp_plan_host.h -- the host side of the planners, which read the handle and step nothing: what they need of the handle
// (plan_ready), bcp_lookahead, and the one launcher of bcp_mppi, bcp_mppi_field and bcp_mppi_adapt with their entry points.
// The kernels are in bcp_lookahead.h and bcp_mppi.h.  Included by bcplan.hip after bcp_step_host.h (upload_step_static).
#pragma once

// What bcp_lookahead and bcp_mppi (`who`) need of the handle before their kernels read it: complete, without delay queues,
// its parameter block on the device and no stale uint8 field (collides_wave classifies with it).
static int plan_ready(bcp_handle* h, const char* who, hipStream_t s)
{
    if (!h->have_map || !h->have_path || !h->have_state)
        return fail(BCP_E_STATE, "%s: costmaps, paths and state must be set first", who);
    const bcp_params& p = h->params;
    if (p.control_delay > 0 || p.pose_delay > 0 || p.state_delay > 0)
        return fail(BCP_E_INVALID, "%s: control_delay / pose_delay / state_delay > 0 are not supported (every "
                                   "candidate would need delay queues of its own)", who);
    HIP_TRY(hipSetDevice(h->device));
    if (h->static_dirty) BCP_TRY(upload_step_static(h, s));
    return h->field.has_stale_fields() ? h->field.ensure_fields(h, s) : BCP_OK;
}

// K candidate plans per env, scored on private copies of the env's state (bcp_lookahead.h).  Reads the handle, writes only
// the caller's outputs: no step counter, ticket, parking counter, record or watchdog word is touched, so the steps before
// and after the call are the steps of a handle that never looked ahead.
extern "C" int bcp_lookahead(bcp_handle* h, const bcp_lookahead_io* io, uint32_t flags, void* stream)
{
    if (!h || !io) return fail(BCP_E_INVALID, "bcp_lookahead: null argument");
    constexpr uint32_t allowed = BCP_STEP_ACTIONS_F32 | BCP_LOOKAHEAD_PER_ENV;
    if (flags & ~allowed) return fail(BCP_E_INVALID, "bcp_lookahead: undefined flag bits 0x%x", flags & ~allowed);
    hipStream_t s = (hipStream_t)stream;
    BCP_TRY(plan_ready(h, "bcp_lookahead", s));
    const bcp_params& p = h->params;
    if (io->horizon < 1 || io->n_candidates < 1)
        return fail(BCP_E_INVALID, "bcp_lookahead: horizon and n_candidates must be at least 1");
    if (!io->actions || !io->ret || !io->steps || !io->reason)
        return fail(BCP_E_INVALID, "bcp_lookahead: actions / ret / steps / reason are required");
    if (io->noise_z && !p.noise_on)
        return fail(BCP_E_INVALID, "bcp_lookahead: noise_z given, but the handle was created without noise (noise_on = 0)");
    if (io->best_action && !io->best) return fail(BCP_E_INVALID, "bcp_lookahead: best_action needs best");
    // element offsets are int64: the largest is 3 * H * N * K (noise_z); the grid has N * K / 64 workgroups
    const int64_t limit = (int64_t)1 << 62;
    const int64_t nk_max = limit / 3 / io->horizon;
    if (h->n > nk_max / io->n_candidates)
        return fail(BCP_E_INVALID, "bcp_lookahead: n_envs * n_candidates * horizon is too large for 64-bit element offsets");
    const int64_t total = h->n * io->n_candidates;
    const int64_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFF) return fail(BCP_E_INVALID, "bcp_lookahead: n_envs * n_candidates exceeds the largest grid (2^37 lanes)");
    LookaheadArgs a;
    a.S = h->dev_static.get();
    a.actions = io->actions;
    a.noise_z = io->noise_z;
    a.mask = io->mask;
    a.ret = io->ret;
    a.steps = io->steps;
    a.reason = io->reason;
    a.final_pose = io->final_pose;
    a.final_target = io->final_target_idx;
    a.err = io->err;
    a.best = io->best;
    a.best_action = io->best_action;
    a.n = h->n;
    a.total = total;
    a.horizon = io->horizon;
    a.k = io->n_candidates;
    a.flags = flags;
    const size_t lds = collision_lds_bytes(p.n_verts, h->map.in_lds, h->map.rows, h->map.wpr);
    const bool plain = p.reward_provider == BCP_REWARD_CONTINUOUS && !io->noise_z;
    const void* fn = plain ? (const void*)lookahead_kernel<true> : (const void*)lookahead_kernel<false>;
    BCP_TRY(launch_variant(h, fn, dim3((unsigned)blocks), dim3(kBlock), lds, s, a));
    if (io->best) {
        int group = 1;
        while (group < 64 && group < io->n_candidates) group <<= 1;
        const int64_t lanes = h->n * group;
        hipLaunchKernelGGL(lookahead_best_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a, group);
    }
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

// One of the eight mppi_kernel variants: the argument struct of <FIELD, ADAPT> cut from the filled <true, true> one, and the
// PLAIN kernel or the other.  (The LDS can pass 64 KiB: a staged map of nearly that plus the scores.)
template <bool FIELD, bool ADAPT>
static int launch_mppi_variant(const bcp_handle* h, const MppiKernelArgs<true, true>& full, bool plain, dim3 grid, size_t lds,
                               hipStream_t s)
{
    MppiKernelArgs<FIELD, ADAPT> ka;
    ka.m = full.m;
    if constexpr (FIELD) ka.t = full.t;
    if constexpr (ADAPT) ka.w = full.w;
    const void* fn = plain ? (const void*)mppi_kernel<true, FIELD, ADAPT> : (const void*)mppi_kernel<false, FIELD, ADAPT>;
    return launch_variant(h, fn, grid, dim3(kBlock), lds, s, ka);
}

// Sampling-based refinement of one plan per env (bcp_mppi.h): I iterations of sample, roll out, weight and update in one
// launch.  Like bcp_lookahead it reads the handle and writes only the caller's arrays.  The one launcher of bcp_mppi,
// bcp_mppi_field and bcp_mppi_adapt (`who`; term == nullptr: the kernels without the terminal read; ad == nullptr: the
// kernels with the two widths of *p): the checks of what the three have in common are written here, once.
static int launch_mppi(bcp_handle* h, const bcp_mppi_params* p, const bcp_mppi_io* io, const bcp_mppi_terminal* term,
                       const bcp_mppi_widths* ad, uint32_t flags, hipStream_t s, const char* who)
{
    if (flags & ~(uint32_t)BCP_STEP_ACTIONS_F32) return fail(BCP_E_INVALID, "%s: undefined flag bits 0x%x", who, flags & ~(uint32_t)BCP_STEP_ACTIONS_F32);
    BCP_TRY(plan_ready(h, who, s));
    const bcp_params& hp = h->params;
    if (p->horizon < 1 || p->iterations < 1) return fail(BCP_E_INVALID, "%s: horizon and iterations must be at least 1", who);
    const int32_t K = p->n_candidates;
    if (K < 8 || K > 1024 || (K & (K - 1)) != 0)
        return fail(BCP_E_INVALID, "%s: n_candidates must be a power of two in [8, 1024], got %d", who, K);
    if (!(p->lambda_ > 0.0) || !std::isfinite(p->lambda_)) return fail(BCP_E_INVALID, "%s: lambda_ must be positive and finite", who);
    if (!std::isfinite(p->collision_penalty)) return fail(BCP_E_INVALID, "%s: collision_penalty must be finite", who);
    for (int d = 0; d < 2; ++d) {
        if (!(p->sigma[d] >= 0.0) || !std::isfinite(p->sigma[d]))
            return fail(BCP_E_INVALID, "%s: sigma[%d] must be finite and not negative", who, d);
        if (!std::isfinite(p->low[d]) || !std::isfinite(p->high[d])) return fail(BCP_E_INVALID, "%s: the action box must be finite", who);
        if (p->low[d] > p->high[d]) return fail(BCP_E_INVALID, "%s: low[%d] > high[%d]", who, d, d);
    }
    if (!io->mean || !io->action) return fail(BCP_E_INVALID, "%s: mean and action are required", who);
    // element offsets are int64: the largest is 2 * I * N * K * H (eps); the bound leaves the room the header promises
    const int64_t limit = (int64_t)1 << 62;
    if (h->n > limit / 5 / p->iterations / K / p->horizon)
        return fail(BCP_E_INVALID, "%s: iterations * n_envs * n_candidates * horizon is too large for 64-bit element offsets", who);
    const int group = K < kBlock ? K : kBlock;
    const int64_t blocks = (h->n * group + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFF) return fail(BCP_E_INVALID, "%s: n_envs exceeds the largest grid", who);
    MppiKernelArgs<true, true> ka;   // (its head is all the plain kernels take)
    memset(&ka, 0, sizeof(ka));
    MppiArgs& a = ka.m;
    a.S = h->dev_static.get();
    a.p = *p;
    a.mean = io->mean;
    a.action = io->action;
    a.mask = io->mask;
    a.eps_in = io->eps_in;
    a.eps_out = io->eps_out;
    a.draw_index = io->draw_index;
    a.iter_mean = io->iter_mean;
    a.iter_ret = io->iter_ret;
    a.iter_reason = io->iter_reason;
    a.err = io->err;
    a.n = h->n;
    a.flags = flags;
    // the scores of a lane's chunks of candidates sit behind the collision area: 8 bytes per (lane, chunk)
    const size_t collision = (collision_lds_bytes(hp.n_verts, h->map.in_lds, h->map.rows, h->map.wpr) + 7) & ~(size_t)7;
    a.score_word = (int32_t)(collision / sizeof(uint32_t));
    const size_t lds = collision + (size_t)(K / group) * kBlock * sizeof(double);
    const bool plain = hp.reward_provider == BCP_REWARD_CONTINUOUS;
    if (ad) {   // (checked by bcp_mppi_adapt: mppi_adapt_check_args)
        MppiWidths& w = ka.w;
        w.sigma = ad->sigma;
        w.iter_sigma = ad->iter_sigma;
        for (int d = 0; d < 2; ++d) {
            w.lo[d] = ad->sigma_min[d];
            w.hi[d] = ad->sigma_max[d];
        }
        w.rate = ad->rate;
    }
    if (term) {
        if (!(term->weight >= 0.0) || !std::isfinite(term->weight))
            return fail(BCP_E_INVALID, "%s: weight must be finite and not negative", who);
        // the field's shape and count against the binding: bcp_goal_field_sample's rules (the other arguments are made to pass)
        const int64_t n_entries = n_slots(h);
        switch (goal_sample_check_args(true, true, true, 1, 1.0, h->n, h->n, false, false, false, term->rows, term->cols, h->map.rows,
                                       h->map.cols, term->n_fields, n_entries)) {
        case kGoalSampleOk: break;
        case kGoalSampleShape: return fail(BCP_E_INVALID, "%s: the field's shape %d x %d is not the bound maps' %d x %d", who, term->rows,
                                           term->cols, h->map.rows, h->map.cols);
        default: return fail(BCP_E_INVALID, "%s: n_fields %lld is neither 1 nor the %lld entries bound", who, (long long)term->n_fields,
                             (long long)n_entries);
        }
        MppiTerminal& t = ka.t;
        t.field = term->field;
        t.field_stride = term->n_fields == 1 ? 0 : (int64_t)term->rows * term->cols;
        t.n_entries = n_entries;
        t.valid_rows = h->map_valid_rows;
        t.valid_cols = h->map_valid_cols;
        t.origins = h->map.origins;
        t.ox = h->map.ox;
        t.oy = h->map.oy;
        t.inv_res = h->map.inv_res;
        t.resolution = h->resolution;
        t.weight = term->weight;
        t.iter_value = term->iter_value;
        t.iter_score = term->iter_score;
        t.rows = term->rows;
        t.cols = term->cols;
        t.shared = h->map.shared;
    }
    const dim3 grid((unsigned)blocks);
    if (!term) {
        if (ad) return launch_mppi_variant<false, true>(h, ka, plain, grid, lds, s);
        return launch_mppi_variant<false, false>(h, ka, plain, grid, lds, s);
    }
    if (ad) return launch_mppi_variant<true, true>(h, ka, plain, grid, lds, s);
    return launch_mppi_variant<true, false>(h, ka, plain, grid, lds, s);
}

extern "C" int bcp_mppi(bcp_handle* h, const bcp_mppi_params* p, const bcp_mppi_io* io, uint32_t flags, void* stream)
{
    if (!h || !p || !io) return fail(BCP_E_INVALID, "bcp_mppi: null argument");
    return launch_mppi(h, p, io, nullptr, nullptr, flags, (hipStream_t)stream, "bcp_mppi");
}

// bcp_mppi with a goal field as the terminal cost of a candidate (bcp_mppi.h, FIELD): the same launch, one 2-byte read more
// per candidate and iteration.
extern "C" int bcp_mppi_field(bcp_handle* h, const bcp_mppi_params* p, const bcp_mppi_io* io, const bcp_mppi_terminal* term,
                              uint32_t flags, void* stream)
{
    if (!h || !p || !io || !term || !term->field) return fail(BCP_E_INVALID, "bcp_mppi_field: null argument");
    return launch_mppi(h, p, io, term, nullptr, flags, (hipStream_t)stream, "bcp_mppi_field");
}

// bcp_mppi (or, with term, bcp_mppi_field) with a width per env, step and component that follows the weights (bcp_mppi.h,
// ADAPT): the same launch, a second walk over the candidates of a row for its variance.  The checks of `ad` are
// bcp_mppi_widths.h's, in its order; everything else is launch_mppi's.
extern "C" int bcp_mppi_adapt(bcp_handle* h, const bcp_mppi_params* p, const bcp_mppi_io* io, const bcp_mppi_widths* ad,
                              const bcp_mppi_terminal* term, uint32_t flags, void* stream)
{
    const char* who = "bcp_mppi_adapt";
    if (!h || !p || !io) return fail(BCP_E_INVALID, "%s: null argument", who);
    int d = 0;
    switch (mppi_adapt_check_args(ad != nullptr, ad && ad->sigma, ad ? ad->rate : 0.0, ad ? ad->sigma_min : nullptr,
                                  ad ? ad->sigma_max : nullptr, &d)) {
    case kMppiAdaptOk: break;
    case kMppiAdaptNull: return fail(BCP_E_INVALID, "%s: null argument (ad and ad->sigma are required)", who);
    case kMppiAdaptRate: return fail(BCP_E_INVALID, "%s: rate must lie in [0, 1]", who);
    case kMppiAdaptMin: return fail(BCP_E_INVALID, "%s: sigma_min[%d] must be finite and not negative", who, d);
    case kMppiAdaptMax: return fail(BCP_E_INVALID, "%s: sigma_max[%d] must be finite and not negative", who, d);
    default: return fail(BCP_E_INVALID, "%s: sigma_min[%d] > sigma_max[%d]", who, d, d);
    }
    if (term && !term->field) return fail(BCP_E_INVALID, "%s: null argument (term->field)", who);
    return launch_mppi(h, p, io, term, ad, flags, (hipStream_t)stream, who);
}

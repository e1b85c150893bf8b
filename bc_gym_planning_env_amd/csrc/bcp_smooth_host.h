// bcp_smooth_host.h -- the host side of bcp_smooth_route: the checks (smooth_check_args, bcp_smooth_cell.h, which the host
// tests run too), the rows as bcp_goal_route resolves them (goal_rows, bcp_goal_host.h) -- or, rows_are_entries, row m =
// entry m of the binding --, and one launch of smooth_kernel (bcp_smooth.h).  Nothing is uploaded or allocated, the
// parameters travel by value in the launch arguments, and the dynamic LDS stays below 64 KB (6 bytes per slot of paths_in,
// at most 4096 slots), so no attribute is raised: a call can be captured after one ordinary call.  Included by bcplan.hip
// after bcp_goal_host.h.
#pragma once

static_assert(sizeof(bcp_smooth_params) == sizeof(SmoothParams) && offsetof(bcp_smooth_params, blend) == offsetof(SmoothParams, blend) &&
                  offsetof(bcp_smooth_params, delta) == offsetof(SmoothParams, delta) &&
                  offsetof(bcp_smooth_params, halvings) == offsetof(SmoothParams, halvings),
              "bcp_smooth_params is SmoothParams, field for field");
static_assert(BCP_SMOOTH_BLOCKED == kSmoothBlocked, "one value for the status bit");

extern "C" int bcp_smooth_route(bcp_handle* h, const uint16_t* field, int64_t n_fields, int32_t rows, int32_t cols,
                                const double* paths_in, const int32_t* lens_in, int32_t max_len_in, int64_t n,
                                const int32_t* row_env, int32_t rows_are_entries, const bcp_smooth_params* p, int32_t max_len,
                                double* paths, int32_t* lens, double* init, int32_t* status, int32_t* info, void* stream)
{
    const char* who = "bcp_smooth_route";
    const bool bound = h && h->have_map;
    const int64_t n_entries = bound ? n_slots(h) : 0;
    const bool pointers = h && field && paths_in && lens_in && paths && lens && status;
    bool overlap = false;
    if (pointers && p && n > 0 && max_len_in >= 2 && max_len_in <= kSmoothMaxLen && max_len >= 2 && max_len <= kSmoothMaxLen) {
        const uint64_t in_p = (uint64_t)(uintptr_t)paths_in, in_l = (uint64_t)(uintptr_t)lens_in, out_p = (uint64_t)(uintptr_t)paths,
                       out_l = (uint64_t)(uintptr_t)lens;
        const uint64_t in_p_bytes = (uint64_t)n * max_len_in * 24, out_p_bytes = (uint64_t)n * max_len * 24, l_bytes = (uint64_t)n * 4;
        overlap = smooth_overlap(out_p, out_p_bytes, in_p, in_p_bytes) || smooth_overlap(out_p, out_p_bytes, in_l, l_bytes) ||
                  smooth_overlap(out_l, l_bytes, in_p, in_p_bytes) || smooth_overlap(out_l, l_bytes, in_l, l_bytes);
    }
    const bool bound_arrays = h && h->have_path && ((const void*)paths == (const void*)h->path_src ||
                                                    (h->path.lens && (const void*)lens == (const void*)h->path.lens));
    switch (smooth_check_args(pointers, p != nullptr, p ? p->look : 0, p ? p->halvings : 0, p ? p->blend : 0.0, p ? p->delta : 0.0,
                              max_len_in, max_len, n, row_env != nullptr, rows_are_entries != 0, rows, cols,
                              bound ? h->map.rows : 0, bound ? h->map.cols : 0, n_fields, n_entries, bound && h->map.shared, overlap,
                              bound_arrays)) {
    case kSmoothOk: break;
    case kSmoothNull: return fail(BCP_E_INVALID, "%s: null argument", who);
    case kSmoothLook: return fail(BCP_E_INVALID, "%s: look %d outside [1, %d]", who, p->look, kSmoothMaxLook);
    case kSmoothHalvings: return fail(BCP_E_INVALID, "%s: halvings %d outside [0, %d]", who, p->halvings, kSmoothMaxHalvings);
    case kSmoothBlend: return fail(BCP_E_INVALID, "%s: blend must be a finite number >= 0", who);
    case kSmoothDelta: return fail(BCP_E_INVALID, "%s: delta must be a finite number > 0", who);
    case kSmoothMaxLenIn: return fail(BCP_E_INVALID, "%s: max_len_in %d outside [2, %d]", who, max_len_in, kSmoothMaxLen);
    case kSmoothMaxLenOut: return fail(BCP_E_INVALID, "%s: max_len %d outside [2, %d]", who, max_len, kSmoothMaxLen);
    case kSmoothRows: return fail(BCP_E_INVALID, "%s: n must be positive", who);
    case kSmoothRowEnv: return fail(BCP_E_INVALID, "%s: row_env does not go with rows_are_entries", who);
    case kSmoothShape: return fail(BCP_E_INVALID, "%s: the field's shape %d x %d is not the bound maps' %d x %d", who, rows, cols,
                                   h->map.rows, h->map.cols);
    case kSmoothFields: return fail(BCP_E_INVALID, "%s: n_fields %lld is neither 1 nor the %lld entries bound (rows_are_entries: "
                                                   "not the entries bound)", who, (long long)n_fields, (long long)n_entries);
    case kSmoothEntries: return fail(BCP_E_INVALID, "%s: n %lld is not the %lld entries bound, which rows_are_entries needs", who,
                                     (long long)n, (long long)n_entries);
    case kSmoothUnbound: return fail(BCP_E_STATE, "%s: costmaps not set", who);
    case kSmoothShared: return fail(BCP_E_STATE, "%s: a shared map has no per-entry rows -- pass rows_are_entries = 0", who);
    case kSmoothOverlap: return fail(BCP_E_STATE, "%s: paths / lens overlap paths_in / lens_in, which the call reads", who);
    default: return fail(BCP_E_STATE, "%s: paths / lens are the bound paths' own arrays", who);
    }
    HIP_TRY(hipSetDevice(h->device));
    const ObsRows R = obs_rows(h, nullptr);
    SmoothArgs a;
    memset(&a, 0, sizeof(a));
    a.src = goal_rows(h, R, field, n_fields, rows, cols, nullptr, n, row_env);
    if (rows_are_entries) {   // row m is entry m: no env in between
        a.src.entry = nullptr;
        a.src.n_envs = n_entries;
    }
    a.paths_in = paths_in;
    a.lens_in = lens_in;
    a.max_len_in = max_len_in;
    a.max_len = max_len;
    a.pure_pursuit = h->params.reward_provider == BCP_REWARD_PURE_PURSUIT;
    a.prm.look = p->look;
    a.prm.halvings = p->halvings;
    a.prm.blend = p->blend;
    a.prm.delta = p->delta;
    a.sp = h->params.spatial_precision;
    a.ap = h->params.angular_precision;
    a.paths = paths;
    a.lens = lens;
    a.init = init;
    a.status = status;
    a.info = info;
    if (n > 0x7FFFFFFFll) return fail(BCP_E_INVALID, "%s: more than 2^31 - 1 rows", who);
    return launch_fn((const void*)smooth_kernel, dim3((unsigned)n), dim3(64), (size_t)max_len_in * 6, (hipStream_t)stream, a);
}

// bcp_goal_host.h -- the host side of the goal field: bcp_goal_field (checks, the choice of where masks and plane live, the
// launch), bcp_goal_field_bound / bcp_refresh_goal_fields (the same launch on the handle's own binding, for all entries or a
// device-side list of them), bcp_goal_field_cost / bcp_goal_field_cost_bound (the two again with a host table of extras per
// map byte, copied into the launch arguments), bcp_goal_field_sample / bcp_final_goal_field_sample over the rows of obs_rows() (bcp_ego_host.h),
// bcp_goal_route / bcp_goal_route_bound over the same rows or the binding's entries, and the value
// check of BCP_TUNE_GOAL_ROUTE.  The refusals are the checks of bcp_goal_cell.h and the shape of every field launch is
// plan_goal's (bcp_goal_plan.h), both of which the host tests run too; the kernels are in bcp_goal.h.  Included by
// bcplan.hip after bcp_ego_host.h.
// Capture: the launch arguments depend only on what the caller passes and nothing is uploaded, but a field kernel whose
// dynamic LDS passes 64 KB needs its limit raised on first use (raise_dynamic_lds: not a stream operation), and the global
// route may grow the scratch: one ordinary call with the same shapes must precede a capture.  The sample call uses no LDS.
#pragma once

static int goal_set_route(bcp_handle* h, int32_t value)
{
    if (value != 0 && value != 2) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_GOAL_ROUTE takes 0 or 2");
    h->tune.goal_route = value;
    return BCP_OK;
}

// The table of a cost call (bcp_goal_field_cost, bcp_goal_field_cost_bound), checked behind everything the plain call
// refuses (goal_cost_check_args) and copied by value into the launch arguments: no upload, no allocation, no
// synchronisation, and a captured launch keeps the table it was captured with.
static int goal_cost_table(const uint16_t* extra_of_cost, GoalCost& c, const char* who)
{
    int32_t bad = 0;
    switch (goal_cost_check_args(extra_of_cost, bad)) {
    case kGoalCostOk: break;
    case kGoalCostTable: return fail(BCP_E_INVALID, "%s: null extra_of_cost", who);
    default: return fail(BCP_E_INVALID, "%s: extra_of_cost[%d] = %d is above %d", who, bad, (int)extra_of_cost[bad], kGoalMaxExtra);
    }
    memcpy(c.extra, extra_of_cost, sizeof(c.extra));
    return BCP_OK;
}

// The one launch of goal_field_kernel, for every form: the arguments that only depend on the shape and the clearance, the
// plan (plan_goal, bcp_goal_plan.h: route, threads, grid, LDS, scratch), the scratch the caller hands in -- reserved here,
// on the global route alone -- and the launch.  trips >= 1: the maps, or the listed entries of the bound form.
static_assert(kGoalMaxLds == kMaxDynamicLds, "plan_goal decides the route by the library's limit on dynamic LDS");

template <bool kBound, bool kCost>
static int goal_launch(bcp_handle* h, GoalKernelArgs<kBound, kCost>& ka, int32_t rows, int32_t cols, int32_t clearance_d2,
                       int32_t max_passes, int64_t trips, DevBuf<uint32_t>& scratch, hipStream_t s, const char* who)
{
    GoalArgs& a = ka.g;
    a.rows = rows;
    a.cols = cols;
    a.wpr = (cols + 31) / 32;
    a.clearance_d2 = clearance_d2;
    a.reach = goal_isqrt(clearance_d2);
    a.max_passes = max_passes > 0 ? max_passes : rows * cols;
    const GoalPlan p = plan_goal(rows, cols, trips, kBound, kCost, h->tune.goal_route == 2);
    if (!p.in_lds) {
        if (scratch.reserve((size_t)p.scratch_words) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BCP_E_HIP, "%s: cannot allocate %lld bytes of scratch", who, (long long)(p.scratch_words * 4));
        }
        a.scratch = scratch.get();
    }
    const void* fn = p.in_lds ? reinterpret_cast<const void*>(goal_field_kernel<true, kBound, kCost>)
                              : reinterpret_cast<const void*>(goal_field_kernel<false, kBound, kCost>);
    return launch_variant(h, fn, dim3((unsigned)p.grid), dim3(p.threads), p.lds_bytes, s, ka);
}

// bcp_goal_field (cost = false: extra_of_cost is not looked at) and bcp_goal_field_cost
template <bool kCost>
static int goal_field_maps(bcp_handle* h, const uint8_t* data, int64_t n_maps, int32_t rows, int32_t cols, int32_t shared,
                           const int32_t* valid_rows, const int32_t* valid_cols, const int32_t* seeds, int32_t n_seeds,
                           int32_t clearance_d2, int32_t max_passes, const uint16_t* extra_of_cost, uint16_t* out, int32_t* info,
                           void* stream, const char* who)
{
    switch (goal_field_check_args(h != nullptr, n_maps, data != nullptr, seeds != nullptr, out != nullptr, rows, cols, n_seeds,
                                  clearance_d2, max_passes, valid_rows != nullptr, valid_cols != nullptr, shared != 0)) {
    case kGoalOk: break;
    case kGoalHandle: return fail(BCP_E_INVALID, "%s: null handle", who);
    case kGoalMaps: return fail(BCP_E_INVALID, "%s: n_maps %lld is negative", who, (long long)n_maps);
    case kGoalShape: return fail(BCP_E_INVALID, "%s: shape %d x %d outside [1, 2048] x [1, 2048]", who, rows, cols);
    case kGoalSeeds: return fail(BCP_E_INVALID, "%s: n_seeds %d outside [1, %d]", who, n_seeds, kGoalMaxSeeds);
    case kGoalClearance: return fail(BCP_E_INVALID, "%s: clearance_d2 %d outside [0, %d]", who, clearance_d2, kGoalMaxClearance);
    case kGoalPasses: return fail(BCP_E_INVALID, "%s: max_passes %d is negative", who, max_passes);
    case kGoalValidPair: return fail(BCP_E_INVALID, "%s: valid_rows and valid_cols go together, both or neither", who);
    case kGoalValidShared: return fail(BCP_E_INVALID, "%s: a shared map takes no valid shapes", who);
    default: return fail(BCP_E_INVALID, "%s: null data / seeds / out", who);
    }
    GoalKernelArgs<false, kCost> ka;
    memset(&ka, 0, sizeof(ka));
    if constexpr (kCost) {
        const int rc = goal_cost_table(extra_of_cost, ka.c, who);
        if (rc != BCP_OK) return rc;
    }
    if (n_maps == 0) return BCP_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;

    GoalArgs& a = ka.g;
    a.data = data;
    a.valid_rows = valid_rows;
    a.valid_cols = valid_cols;
    a.seeds = seeds;
    a.out = out;
    a.info = info;
    a.n_maps = n_maps;
    a.shared = shared ? 1 : 0;
    a.n_seeds = n_seeds;
    return goal_launch(h, ka, rows, cols, clearance_d2, max_passes, n_maps, h->goal_scratch, s, who);
}

extern "C" int bcp_goal_field(bcp_handle* h, const uint8_t* data, int64_t n_maps, int32_t rows, int32_t cols, int32_t shared,
                              const int32_t* valid_rows, const int32_t* valid_cols, const int32_t* seeds, int32_t n_seeds,
                              int32_t clearance_d2, int32_t max_passes, uint16_t* out, int32_t* info, void* stream)
{
    return goal_field_maps<false>(h, data, n_maps, rows, cols, shared, valid_rows, valid_cols, seeds, n_seeds, clearance_d2,
                                  max_passes, nullptr, out, info, stream, "bcp_goal_field");
}

extern "C" int bcp_goal_field_cost(bcp_handle* h, const uint8_t* data, int64_t n_maps, int32_t rows, int32_t cols, int32_t shared,
                                   const int32_t* valid_rows, const int32_t* valid_cols, const int32_t* seeds, int32_t n_seeds,
                                   int32_t clearance_d2, int32_t max_passes, const uint16_t* extra_of_cost, uint16_t* out,
                                   int32_t* info, void* stream)
{
    return goal_field_maps<true>(h, data, n_maps, rows, cols, shared, valid_rows, valid_cols, seeds, n_seeds, clearance_d2,
                                 max_passes, extra_of_cost, out, info, stream, "bcp_goal_field_cost");
}

// ---- fields of the handle's own binding ---------------------------------------------------------------------------
// bcp_goal_field_bound and bcp_refresh_goal_fields: the checks (goal_bound_check_args), the arguments from the binding, the
// route as bcp_goal_field chooses it, and a grid that never depends on the device-side count.  refresh_form: the list is the
// ring's `dirty` and the count its tally[0], as bcp_refresh_mini_worlds used them (bcp_worlds_host.h).
template <bool kCost>
static int goal_field_bound(bcp_handle* h, const int32_t* entries, const int32_t* count, int64_t n_list, int32_t clearance_d2,
                            int32_t max_passes, const uint16_t* extra_of_cost, uint16_t* field, int32_t* info, void* stream,
                            bool refresh_form, const char* who)
{
    const int64_t n_entries = h ? n_slots(h) : 0;
    switch (goal_bound_check_args(h != nullptr, field != nullptr, n_list, n_entries, entries != nullptr, count != nullptr,
                                  clearance_d2, max_passes, h && h->have_map, h && h->have_path, h && h->map.shared,
                                  h && h->path.shared, h ? h->map.rows : 0, h ? h->map.cols : 0, refresh_form,
                                  h && h->ring_refreshed && h->ring.get() && (int64_t)h->n_geoms == h->n * h->ring_episodes)) {
    case kGoalBoundOk: break;
    case kGoalBoundHandle: return fail(BCP_E_INVALID, "%s: null handle", who);
    case kGoalBoundField: return fail(BCP_E_INVALID, "%s: null field", who);
    case kGoalBoundList: return fail(BCP_E_INVALID, "%s: n_list %lld outside [0, %lld], the entries bound", who, (long long)n_list,
                                     (long long)n_entries);
    case kGoalBoundCount: return fail(BCP_E_INVALID, "%s: count needs entries", who);
    case kGoalBoundClearance: return fail(BCP_E_INVALID, "%s: clearance_d2 %d outside [0, %d]", who, clearance_d2, kGoalMaxClearance);
    case kGoalBoundPasses: return fail(BCP_E_INVALID, "%s: max_passes %d is negative", who, max_passes);
    case kGoalBoundUnbound: return fail(BCP_E_STATE, "%s: costmaps and paths must be bound first", who);
    case kGoalBoundShared: return fail(BCP_E_STATE, "%s: a shared map or a shared path has no per-entry goal here -- bcp_goal_field "
                                                    "serves those", who);
    case kGoalBoundShape: return fail(BCP_E_STATE, "%s: the bound maps' shape %d x %d is outside [1, 2048] x [1, 2048]", who,
                                      h->map.rows, h->map.cols);
    default: return fail(BCP_E_STATE, "%s: no refresh pending (between bcp_refresh_mini_worlds and bcp_release_mini_worlds)", who);
    }
    GoalKernelArgs<true, kCost> ka;
    memset(&ka, 0, sizeof(ka));
    if constexpr (kCost) {
        const int rc = goal_cost_table(extra_of_cost, ka.c, who);
        if (rc != BCP_OK) return rc;
    }
    if (refresh_form) {   // the ring's arrays as bcp_plan_mini_worlds laid them out
        const int64_t* first_world = (const int64_t*)h->ring.get();
        const int32_t* counts = (const int32_t*)(first_world + h->n);
        entries = counts + h->n;
        count = entries + n_entries;
        n_list = n_entries;
    }
    if (n_list == 0) return BCP_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;

    GoalArgs& a = ka.g;
    a.data = h->map_data;
    a.valid_rows = h->map_valid_rows && h->map_valid_cols ? h->map_valid_rows : nullptr;
    a.valid_cols = a.valid_rows ? h->map_valid_cols : nullptr;
    a.out = field;
    a.info = info;
    a.n_maps = n_entries;
    a.n_seeds = 1;
    GoalBound& b = ka.b;
    b.sel.list = entries;
    b.sel.count = entries ? count : nullptr;
    b.sel.n = n_list;
    b.paths = h->path_src;
    b.lens = h->path.lens;
    b.origins = h->map.origins;
    b.ox = h->map.ox;
    b.oy = h->map.oy;
    b.inv_res = h->map.inv_res;
    b.max_len = h->path.max_len;
    return goal_launch(h, ka, h->map.rows, h->map.cols, clearance_d2, max_passes, n_list, h->goal_bound_scratch, s, who);
}

extern "C" int bcp_goal_field_bound(bcp_handle* h, const int32_t* entries, const int32_t* count, int64_t n_list,
                                    int32_t clearance_d2, int32_t max_passes, uint16_t* field, int32_t* info, void* stream)
{
    return goal_field_bound<false>(h, entries, count, n_list, clearance_d2, max_passes, nullptr, field, info, stream, false,
                                   "bcp_goal_field_bound");
}

extern "C" int bcp_goal_field_cost_bound(bcp_handle* h, const int32_t* entries, const int32_t* count, int64_t n_list,
                                         int32_t clearance_d2, int32_t max_passes, const uint16_t* extra_of_cost,
                                         uint16_t* field, int32_t* info, void* stream)
{
    return goal_field_bound<true>(h, entries, count, n_list, clearance_d2, max_passes, extra_of_cost, field, info, stream, false,
                                  "bcp_goal_field_cost_bound");
}

extern "C" int bcp_refresh_goal_fields(bcp_handle* h, int32_t clearance_d2, int32_t max_passes, uint16_t* field, int32_t* info,
                                       void* stream)
{
    return goal_field_bound<false>(h, nullptr, nullptr, 0, clearance_d2, max_passes, nullptr, field, info, stream, true,
                                   "bcp_refresh_goal_fields");
}

// Whose row reads what (GoalRows, bcp_goal.h), from the handle's map binding and the rows of obs_rows(): the one statement
// for bcp_goal_field_sample and bcp_goal_route.
static GoalRows goal_rows(const bcp_handle* h, const ObsRows& R, const uint16_t* field, int64_t n_fields, int32_t rows,
                          int32_t cols, const double* poses, int64_t n, const int32_t* row_env)
{
    GoalRows a;
    memset(&a, 0, sizeof(a));
    a.field = field;
    a.n_fields = n_fields;
    a.n_entries = n_slots(h);   // (a shared map may go with private paths: a field per env)
    a.rows = rows;
    a.cols = cols;
    a.shared = h->map.shared;
    a.valid_rows = h->map_valid_rows;
    a.valid_cols = h->map_valid_cols;
    a.origins = h->map.origins;
    a.ox = h->map.ox;
    a.oy = h->map.oy;
    a.inv_res = h->map.inv_res;
    a.resolution = h->resolution;
    a.poses = poses;
    const bool delayed = h->params.pose_delay > 0 && R.st.pose_seen;   // the observation shows State.pose, i.e. the delayed pose
    a.sx = delayed ? R.st.pose_seen : R.st.x;
    a.sy = delayed ? R.st.pose_seen + R.n : R.st.y;
    a.sth = delayed ? R.st.pose_seen + 2 * R.n : R.st.angle;
    a.entry = h->n_geoms > 0 ? (R.entry ? R.entry : h->geom_of_env) : R.entry;
    a.row_env = row_env;
    a.n_envs = R.n;
    a.n = n;
    return a;
}

// rec != nullptr: the final states of the episode record, n = capacity, rows j < min(*count, capacity)
static int goal_field_sample(bcp_handle* h, const uint16_t* field, int64_t n_fields, int32_t rows, int32_t cols,
                             const double* poses, int64_t n, const int32_t* row_env, int32_t carrot_cells, double max_dist,
                             float* out3, int32_t* cell_value, int32_t* carrot, void* stream, const EpisodeRec* rec,
                             const char* who)
{
    const bool bound = h && h->have_map;
    const int64_t n_entries = bound ? n_slots(h) : 0;   // (a shared map may go with private paths: a field per env)
    switch (goal_sample_check_args(h != nullptr, field != nullptr, out3 != nullptr, carrot_cells, max_dist, n, h ? h->n : 0,
                                   poses != nullptr, row_env != nullptr, rec != nullptr, rows, cols, bound ? h->map.rows : 0,
                                   bound ? h->map.cols : 0, n_fields, n_entries)) {
    case kGoalSampleOk: break;
    case kGoalSampleNull: return fail(BCP_E_INVALID, "%s: null argument", who);
    case kGoalSampleCarrot: return fail(BCP_E_INVALID, "%s: carrot_cells %d outside [1, %d]", who, carrot_cells, kGoalMaxCarrot);
    case kGoalSampleDist: return fail(BCP_E_INVALID, "%s: max_dist must be > 0 (+inf is allowed)", who);
    case kGoalSampleRows: return fail(BCP_E_INVALID, "%s: n must be positive, and n_envs without poses", who);
    case kGoalSampleRowEnv: return fail(BCP_E_INVALID, "%s: row_env needs poses", who);
    case kGoalSampleShape: return fail(BCP_E_INVALID, "%s: the field's shape %d x %d is not the bound maps' %d x %d", who, rows, cols,
                                       h->map.rows, h->map.cols);
    default: return fail(BCP_E_INVALID, "%s: n_fields %lld is neither 1 nor the %lld entries bound", who, (long long)n_fields,
                         (long long)n_entries);
    }
    if (!h->have_map) return fail(BCP_E_STATE, "%s: costmaps not set", who);
    if (!poses && !rec && !h->have_state) return fail(BCP_E_STATE, "%s: no poses given and no state bound", who);
    HIP_TRY(hipSetDevice(h->device));
    const ObsRows R = obs_rows(h, rec);
    GoalSampleArgs a;
    memset(&a, 0, sizeof(a));
    a.src = goal_rows(h, R, field, n_fields, rows, cols, poses, n, row_env);
    a.carrot_cells = carrot_cells;
    a.max_dist = max_dist;
    a.live = R.live;
    a.out3 = out3;
    a.cell_value = cell_value;
    a.carrot = carrot;
    return launch_fn((const void*)goal_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

extern "C" int bcp_goal_field_sample(bcp_handle* h, const uint16_t* field, int64_t n_fields, int32_t rows, int32_t cols,
                                     const double* poses, int64_t n, const int32_t* row_env, int32_t carrot_cells,
                                     double max_dist, float* out3, int32_t* cell_value, int32_t* carrot, void* stream)
{
    return goal_field_sample(h, field, n_fields, rows, cols, poses, n, row_env, carrot_cells, max_dist, out3, cell_value, carrot,
                             stream, nullptr, "bcp_goal_field_sample");
}

extern "C" int bcp_final_goal_field_sample(bcp_handle* h, const uint16_t* field, int64_t n_fields, int32_t rows, int32_t cols,
                                           int32_t carrot_cells, double max_dist, float* out3, int32_t* cell_value,
                                           int32_t* carrot, void* stream)
{
    if (h && !h->have_rec) return fail(BCP_E_STATE, "bcp_final_goal_field_sample: no episode record bound");
    return goal_field_sample(h, field, n_fields, rows, cols, nullptr, h ? h->rec.capacity : 0, nullptr, carrot_cells, max_dist,
                             out3, cell_value, carrot, stream, h ? &h->rec : nullptr, "bcp_final_goal_field_sample");
}

// ---- routes -----------------------------------------------------------------------------------------------------------
// bcp_goal_route and bcp_goal_route_bound: the checks (goal_route_check_args), the rows as bcp_goal_field_sample resolves
// them -- or, bound_form, row m = entry m of the binding, from its bound path[0] to its last way point -- and one launch.
// Nothing is uploaded or allocated and the kernel uses no LDS: a call can be captured after one ordinary call.
static int goal_route(bcp_handle* h, const uint16_t* field, int64_t n_fields, int32_t rows, int32_t cols, const double* poses,
                      int64_t n, const int32_t* row_env, const double* goals, int32_t stride, int32_t max_len, double* paths,
                      int32_t* lens, double* init, int32_t* status, void* stream, bool bound_form, const char* who)
{
    const bool bound = h && h->have_map;
    const int64_t n_entries = bound ? n_slots(h) : 0;
    switch (goal_route_check_args(h != nullptr, field != nullptr, paths != nullptr, lens != nullptr, status != nullptr, stride,
                                  max_len, n, h ? h->n : 0, poses != nullptr, row_env != nullptr, bound_form, rows, cols,
                                  bound ? h->map.rows : 0, bound ? h->map.cols : 0, n_fields, n_entries)) {
    case kGoalRouteOk: break;
    case kGoalRouteNull: return fail(BCP_E_INVALID, "%s: null argument", who);
    case kGoalRouteStride: return fail(BCP_E_INVALID, "%s: stride %d outside [1, %d]", who, stride, kGoalRouteMaxStride);
    case kGoalRouteMaxLenRange: return fail(BCP_E_INVALID, "%s: max_len %d outside [2, %d]", who, max_len, kGoalRouteMaxLen);
    case kGoalRouteRows: return fail(BCP_E_INVALID, "%s: n must be positive, and n_envs without poses", who);
    case kGoalRouteRowEnv: return fail(BCP_E_INVALID, "%s: row_env needs poses", who);
    case kGoalRouteShape: return fail(BCP_E_INVALID, "%s: the field's shape %d x %d is not the bound maps' %d x %d", who, rows, cols,
                                      h->map.rows, h->map.cols);
    default: return fail(BCP_E_INVALID, "%s: n_fields %lld is neither 1 nor the %lld entries bound", who, (long long)n_fields,
                         (long long)n_entries);
    }
    if (!h->have_map) return fail(BCP_E_STATE, "%s: costmaps not set", who);
    const bool reads_path = bound_form || !goals;
    if (reads_path && !h->have_path) return fail(BCP_E_STATE, "%s: no goals given and no paths bound", who);
    if (bound_form && (h->map.shared || h->path.shared))
        return fail(BCP_E_STATE, "%s: a shared map or a shared path has no per-entry route here -- bcp_goal_route serves those", who);
    if (!bound_form && !poses && !h->have_state) return fail(BCP_E_STATE, "%s: no poses given and no state bound", who);
    if (reads_path && ((const void*)paths == (const void*)h->path_src || (const void*)lens == (const void*)h->path.lens))
        return fail(BCP_E_STATE, "%s: paths / lens are the bound paths' own arrays, which the call reads", who);
    HIP_TRY(hipSetDevice(h->device));
    const ObsRows R = obs_rows(h, nullptr);
    GoalRouteArgs a;
    memset(&a, 0, sizeof(a));
    a.src = goal_rows(h, R, field, n_fields, rows, cols, poses, bound_form ? n_entries : n, row_env);
    if (bound_form) {   // row m is entry m: no env in between
        a.src.entry = nullptr;
        a.src.n_envs = n_entries;
    }
    a.goals = goals;
    if (reads_path) {
        a.src_paths = h->path_src;
        a.src_lens = h->path.shared ? nullptr : h->path.lens;
        a.src_max_len = h->path.max_len;
    }
    a.bound = bound_form ? 1 : 0;
    a.stride = stride;
    a.max_len = max_len;
    a.pure_pursuit = h->params.reward_provider == BCP_REWARD_PURE_PURSUIT;
    a.sp = h->params.spatial_precision;
    a.ap = h->params.angular_precision;
    a.paths = paths;
    a.lens = lens;
    a.init = init;
    a.status = status;
    return launch_fn((const void*)goal_route_kernel, dim3((unsigned)((a.src.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

extern "C" int bcp_goal_route(bcp_handle* h, const uint16_t* field, int64_t n_fields, int32_t rows, int32_t cols,
                              const double* poses, int64_t n, const int32_t* row_env, const double* goals, int32_t stride,
                              int32_t max_len, double* paths, int32_t* lens, double* init, int32_t* status, void* stream)
{
    return goal_route(h, field, n_fields, rows, cols, poses, n, row_env, goals, stride, max_len, paths, lens, init, status, stream,
                      false, "bcp_goal_route");
}

extern "C" int bcp_goal_route_bound(bcp_handle* h, const uint16_t* field, int32_t rows, int32_t cols, int32_t stride,
                                    int32_t max_len, double* paths, int32_t* lens, double* init, int32_t* status, void* stream)
{
    return goal_route(h, field, h && h->have_map ? n_slots(h) : 0, rows, cols, nullptr, 0, nullptr, nullptr, stride, max_len, paths,
                      lens, init, status, stream, true, "bcp_goal_route_bound");
}

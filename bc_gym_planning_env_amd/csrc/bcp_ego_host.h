// bcp_ego_host.h -- the host side of the observations: egocentric costmaps (arguments, then the route of bcp_ego_route.h
// from the call's shape and the cell lists of bcp_host.h's EgoCells, then that route's launch), the goal-state vectors with
// their two small kernels, and the episode record with its final observations.  Included by bcplan.hip after bcp_step_host.h.
#pragma once

// The rows an observation kernel reads: the bound state (n = n_envs, env i on entry geom_of_env[i] or i), or the final
// states of an episode record (n = capacity, row j on entry `entry[j]`, only rows j < *live).
struct ObsRows {
    DevState st;
    int64_t n;
    const int32_t* entry;          // nullptr: the bound state's own entries, geom_of_env[i] or i
    const int32_t* live;
};

// the bound state's rows, or (rec) the record's final states -- the one place that chooses them, for the images and the
// goal vectors alike
static ObsRows obs_rows(const bcp_handle* h, const EpisodeRec* rec)
{
    ObsRows R;
    R.st = rec ? rec->fin : h->st;
    R.n = rec ? rec->capacity : h->n;
    R.entry = rec ? (h->n_geoms > 0 ? rec->geom : rec->env_id) : nullptr;   // (without a pool: the env's private map and path)
    R.live = rec ? rec->count : nullptr;
    return R;
}

// EgocentricCostmap.observation's goal_n_state (envs/egocentric.py:140-160), one thread per env
__global__ void goal_n_state_kernel(const StepStatic* __restrict__ S, ObsRows R, double wsx, double wsy, int n_state,
                                    float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n || (R.live && i >= *R.live)) return;
    const DevState& rs = R.st;
    const int64_t g = R.entry ? (int64_t)R.entry[i] : (S->geom_of_env ? (int64_t)S->geom_of_env[i] : i);
    const int m = S->path.shared ? S->path.max_len : S->path.lens[g];
    // Observation.path: the way points still ahead, path[target_idx:] (reward.py:59-64) -- or, for the pure-pursuit
    // provider, path[:target_idx + 1] (reward.py:118-123), whose first row is always way point 0
    const int target = S->P.reward_provider == BCP_REWARD_PURE_PURSUIT ? 0 : rs.target_idx[i];
    float* o = out + i * (3 + n_state);
    if (target > m - 1) {   // nothing left of the path: zeros (egocentric.py:142-150)
        for (int k = 0; k < 3 + n_state; ++k) o[k] = 0.0f;
        return;
    }
    const double* wp = S->path.pts + ((S->path.shared ? 0 : g * (int64_t)S->path.max_len) + target) * 5;
    const int64_t n = R.n;
    // Observation.pose / .robot_state are the delayed ones when delays are configured
    const bool dp = S->P.pose_delay > 0, ds = S->P.state_delay > 0;
    const double x = dp ? rs.pose_seen[i] : rs.x[i], y = dp ? rs.pose_seen[n + i] : rs.y[i];
    const double th = dp ? rs.pose_seen[2 * n + i] : rs.angle[i];
    // inverse_transform (coordinate_transformations.py:57-84), then project_poses (:310-328)
    const double c = cos(th), s = sin(th);
    const double tx = -x * c - y * s, ty = x * s - y * c, tt = normalize_angle(-th);
    const double ct = cos(tt), st = sin(tt);
    const double ex = ct * wp[0] + (-st) * wp[1] + tx;
    const double ey = st * wp[0] + ct * wp[1] + ty;
    const double eth = normalize_angle(wp[2] + tt);
    o[0] = (float)fmin(fmax(ex / wsx, -1.0), 1.0);
    o[1] = (float)fmin(fmax(ey / wsy, -1.0), 1.0);
    o[2] = (float)eth;
    // robot_state.to_numpy_array(): x, y, angle, v, w (, wheel_angle)
    o[3] = (float)(ds ? rs.state_seen[i] : rs.x[i]);
    o[4] = (float)(ds ? rs.state_seen[n + i] : rs.y[i]);
    o[5] = (float)(ds ? rs.state_seen[2 * n + i] : rs.angle[i]);
    o[6] = (float)(ds ? rs.state_seen[3 * n + i] : rs.v[i]);
    o[7] = (float)(ds ? rs.state_seen[4 * n + i] : rs.w[i]);
    if (n_state > 5) o[8] = (float)(ds ? rs.state_seen[6 * n + i] : rs.wheel[i]);
}

// ColoredEgoCostmapRandomAisleTurnEnv's `goal` vector (envs/synth_turn_env.py:412-420), one thread per env: the LAST way
// point in the robot frame over the window's world size, normalised to unit length, then (v, w, wheel_angle)
__global__ void goal_direction_state_kernel(const StepStatic* __restrict__ S, ObsRows R, double wsx, double wsy,
                                            double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n || (R.live && i >= *R.live)) return;
    const DevState& rs = R.st;
    const int64_t g = R.entry ? (int64_t)R.entry[i] : (S->geom_of_env ? (int64_t)S->geom_of_env[i] : i);
    const int m = S->path.shared ? S->path.max_len : S->path.lens[g];
    const double* wp = S->path.pts + ((S->path.shared ? 0 : g * (int64_t)S->path.max_len) + (m - 1)) * 5;
    const double x = rs.x[i], y = rs.y[i], th = rs.angle[i];   // the robot's own pose (not the delayed one)
    const double c = cos(th), s = sin(th);
    const double tx = -x * c - y * s, ty = x * s - y * c, tt = normalize_angle(-th);
    const double ct = cos(tt), st = sin(tt);
    const double gx = (ct * wp[0] + (-st) * wp[1] + tx) / wsx, gy = (st * wp[0] + ct * wp[1] + ty) / wsy;
    const double norm = sqrt(fma(gy, gy, gx * gx));   // np.linalg.norm: fma-contracted 2-term dot
    double* o = out + 5 * i;
    o[0] = gx / norm;
    o[1] = gy / norm;
    o[2] = rs.v[i];
    o[3] = rs.w[i];
    o[4] = S->P.model == BCP_MODEL_TRICYCLE ? rs.wheel[i] : 0.0;
}

// One of the two goal vectors for the rows of obs_rows(): `kernel` takes (S, R, world size x, y, tail...).
template <typename... Tail>
static int goal_vectors(const void* kernel, bcp_handle* h, const double* world_size, const void* out, void* stream,
                        const EpisodeRec* rec, const char* who, const Tail&... tail)
{
    if (!h || !world_size || !out) return fail(BCP_E_INVALID, "%s: null argument", who);
    if (!h->have_path || !h->have_state) return fail(BCP_E_STATE, "%s: paths and state must be set first", who);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->static_dirty) BCP_TRY(upload_step_static(h, s));
    const ObsRows R = obs_rows(h, rec);
    const StepStatic* S = h->dev_static.get();
    return launch_fn(kernel, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, s, S, R, world_size[0], world_size[1], tail...);
}

static int goal_n_state(bcp_handle* h, const double* world_size, float* out, void* stream, const EpisodeRec* rec, const char* who)
{
    const int n_state = h && h->params.model == BCP_MODEL_TRICYCLE ? 6 : 5;
    return goal_vectors((const void*)goal_n_state_kernel, h, world_size, out, stream, rec, who, n_state, out);
}

static int goal_direction_state(bcp_handle* h, const double* world_size, double* out, void* stream, const EpisodeRec* rec,
                                const char* who)
{
    return goal_vectors((const void*)goal_direction_state_kernel, h, world_size, out, stream, rec, who, out);
}

// ---- egocentric observation ----------------------------------------------------------------------------------
static int ego_shape(const bcp_handle* h, const double* window_size, int32_t* drows, int32_t* dcols)
{
    if (window_size) {
        const double inv = 1.0 / h->resolution;
        *dcols = (int32_t)std::nearbyint(window_size[0] * inv);  // world_to_pixel(resulting_size, (0, 0), resolution)
        *drows = (int32_t)std::nearbyint(window_size[1] * inv);
    } else {
        *drows = h->map.rows;
        *dcols = h->map.cols;
    }
    return *drows > 0 && *dcols > 0 && (int64_t)*drows * *dcols * *dcols < (int64_t)1 << 32 && *dcols <= 8192 && *drows <= 8192;
}

extern "C" int bcp_egocentric_shape(bcp_handle* h, const double* window_size, int32_t* shape_hw)
{
    if (!h || !shape_hw) return fail(BCP_E_INVALID, "bcp_egocentric_shape: null argument");
    if (!h->have_map) return fail(BCP_E_STATE, "bcp_egocentric_shape: costmaps not set");
    if (!ego_shape(h, window_size, &shape_hw[0], &shape_hw[1]))
        return fail(BCP_E_INVALID, "bcp_egocentric_shape: unsupported window size");
    return BCP_OK;
}

extern "C" int bcp_egocentric_route(bcp_handle* h, int32_t* info4)
{
    if (!h || !info4) return fail(BCP_E_INVALID, "bcp_egocentric_route: null argument");
    for (int k = 0; k < 4; ++k) info4[k] = h->ego_route[k];
    return BCP_OK;
}

// the kernels' arguments for images of the rows R (route-dependent fields: launch_ego)
static EgoArgs ego_args_of(const bcp_handle* h, const ObsRows& R, const double* poses, int64_t n, const double* window_origin,
                           int32_t drows, int32_t dcols, uint8_t border_value, uint8_t* out)
{
    EgoArgs a;
    memset(&a, 0, sizeof(a));
    a.drows = drows;
    a.dcols = dcols;
    a.data = h->map_data;
    a.shared = h->map.shared;
    a.rows = h->map.rows;
    a.cols = h->map.cols;
    a.map_stride = a.shared ? 0 : (int64_t)a.rows * a.cols;
    a.valid_rows = h->map_valid_rows;
    a.valid_cols = h->map_valid_cols;
    a.origins = h->map.origins;
    a.ox = h->map.ox;
    a.oy = h->map.oy;
    a.res = h->resolution;
    a.inv_res = h->map.inv_res;
    a.poses = poses;
    const bool delayed = h->params.pose_delay > 0 && R.st.pose_seen;   // the observation shows State.pose, i.e. the delayed pose
    a.sx = delayed ? R.st.pose_seen : R.st.x;
    a.sy = delayed ? R.st.pose_seen + R.n : R.st.y;
    a.sth = delayed ? R.st.pose_seen + 2 * R.n : R.st.angle;
    // (one map for all: the entry does not matter)
    a.geom_of_env = h->n_geoms > 0 ? (R.entry ? R.entry : h->geom_of_env) : (a.shared ? nullptr : R.entry);
    a.n_envs = R.n;
    a.live = R.live;
    a.has_window = window_origin != nullptr;
    if (window_origin) {
        a.win_ox = window_origin[0];
        a.win_oy = window_origin[1];
    }
    a.border = border_value;
    a.out = out;
    a.n_images = n;
    a.cols_magic = (uint32_t)(((uint64_t)1 << 32) / (uint64_t)a.cols) + 1;   // (staged maps are < 64 KB: exact)
    return a;
}

// A persistent kernel: as many workgroups as are resident at once, and no more than there is work.
template <typename... Args>
static int launch_persistent(const bcp_handle* h, const void* fn, int threads, size_t lds, int64_t work, hipStream_t s,
                             const Args&... args)
{
    BCP_TRY(variant_lds(h, fn, lds));
    int cus = 0, per_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds));
    const dim3 grid((unsigned)std::min<int64_t>(work, (int64_t)std::max(per_cu, 1) * std::max(cus, 1)));
    return launch_fn(fn, grid, dim3(threads), lds, s, args...);
}

// the launch of one route
static int launch_ego(bcp_handle* h, EgoArgs a, const EgoPlan& plan, int32_t pool, hipStream_t st)
{
    const int64_t n = a.n_images;
    const int threads = 64 * plan.waves;
    const dim3 per_wave((unsigned)((n + plan.waves - 1) / plan.waves));   // (the one-image-per-wave kernels)
    const EgoCells& cells = h->ego_cells;
    const EgoPool Q = {pool, (a.drows + pool - 1) / pool, (a.dcols + pool - 1) / pool, (uint32_t)(((uint64_t)1 << 32) / (uint64_t)pool) + 1};
    const bool px8 = plan.px == 8;
    a.stage_map = plan.stage_map;
    a.win_lds_bytes = plan.win_lds_bytes;
    switch (plan.route) {
    case BCP_EGO_POOLED_SPARSE:
        hipLaunchKernelGGL(ego_pooled_sparse_kernel, per_wave, dim3(threads), plan.lds_bytes, st, a, Q, cells.lists(), cells.list_counts(),
                           cells.stride());
        break;
    case BCP_EGO_SPARSE:
        // One image per wave, eight per workgroup: 8 192 short workgroups for 65 536 images.  (Round 3 first ran this kernel
        // persistently -- as many workgroups as the chip holds, 64 images per wave, the lanes sharing the transforms' float64
        // arithmetic: 11 % slower on the same box, 0.249 against 0.222 ms.  Stores from many short workgroups drain faster than
        // from a few long-lived ones, tools/fill_rate.hip; the arithmetic saved was never the bottleneck, VALU busy 17 %.
        // Also measured: an image split over 2 / 4 waves of a workgroup (+- 0 / 14 % slower), a plain one-image kernel with
        // 48 instead of 83 registers (3 - 8 % slower), fewer workgroups per CU by way of unused LDS (within the noise).)
        hipLaunchKernelGGL(ego_sparse_kernel, per_wave, dim3(threads), plan.lds_bytes, st, a, cells.lists(), cells.list_counts(),
                           cells.stride());
        break;
    case BCP_EGO_POOLED_SAMPLED:
        hipLaunchKernelGGL(ego_pooled_sampled_kernel, per_wave, dim3(threads), 0, st, a, Q);
        break;
    case BCP_EGO_BINNED: {
        const int64_t n_bins = n_slots(h);
        // (two arrays in each buffer; only ever reserved in pairs, so half the capacity is the second one's offset)
        HIP_TRY(h->ego_bins.reserve((size_t)2 * n_bins));
        HIP_TRY(h->ego_order.reserve((size_t)2 * n));
        int32_t* bin_count = h->ego_bins.get();
        int32_t* bin_start = h->ego_bins.get() + h->ego_bins.capacity() / 2;
        int32_t* rank = h->ego_order.get();
        int32_t* order = h->ego_order.get() + h->ego_order.capacity() / 2;
        HIP_TRY(hipMemsetAsync(bin_count, 0, (size_t)n_bins * sizeof(int32_t), st));
        const dim3 per_image((unsigned)((n + 255) / 256)), block(256);
        hipLaunchKernelGGL(ego_bin_count_kernel, per_image, block, 0, st, a.geom_of_env, a.n_envs, n, bin_count, rank, a.live);
        hipLaunchKernelGGL(ego_bin_scan_kernel, dim3(1), dim3(1024), 0, st, bin_count, n_bins, bin_start);
        hipLaunchKernelGGL(ego_bin_scatter_kernel, per_image, block, 0, st, a.geom_of_env, a.n_envs, n, bin_start, rank, order,
                           a.live);
        HIP_TRY(hipGetLastError());
        const void* fn = px8 ? (const void*)ego_costmap_binned_kernel<8> : (const void*)ego_costmap_binned_kernel<4>;
        return launch_persistent(h, fn, threads, plan.lds_bytes, n, st, a, bin_start, bin_count, order);
    }
    case BCP_EGO_WINDOW: {
        const void* fn = px8 ? (const void*)ego_costmap_window_kernel<8> : (const void*)ego_costmap_window_kernel<4>;
        return launch_persistent(h, fn, threads, plan.lds_bytes, n, st, a);
    }
    default: {   // BCP_EGO_STAGED, BCP_EGO_GLOBAL
        const void* fn = a.stage_map ? (px8 ? (const void*)ego_costmap_kernel<true, 8> : (const void*)ego_costmap_kernel<true, 4>)
                                     : (px8 ? (const void*)ego_costmap_kernel<false, 8> : (const void*)ego_costmap_kernel<false, 4>);
        return launch_persistent(h, fn, threads, plan.lds_bytes, (n + plan.waves - 1) / plan.waves, st, a);
    }
    }
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

// rec != nullptr: the final observations of an episode record (bcp_final_egocentric_costmaps) -- image j from final state j
// on entry rec->geom[j] (private maps without a pool: env rec->env_id[j]), n = capacity, only the first *count drawn
// pool > 1: the block maxima of those images (bcp_egocentric_costmaps_pooled), same arguments, same cell lists
static int egocentric_costmaps(bcp_handle* h, const double* poses, int64_t n, const double* window_origin,
                               const double* window_size, uint8_t border_value, uint8_t* out, void* stream,
                               const EpisodeRec* rec, int32_t pool = 1,
                               const char* who = "bcp_egocentric_costmaps")
{
    if (!h || !out) return fail(BCP_E_INVALID, "%s: null argument", who);
    if (!h->have_map) return fail(BCP_E_STATE, "%s: costmaps not set", who);
    if (!poses && !h->have_state) return fail(BCP_E_STATE, "%s: no poses given and no state bound", who);
    if (n <= 0 || (!poses && !rec && n != h->n)) return fail(BCP_E_INVALID, "%s: n must be n_envs without poses", who);
    if ((window_origin == nullptr) != (window_size == nullptr))
        return fail(BCP_E_INVALID, "%s: window origin and size go together", who);
    int32_t drows = 0, dcols = 0;
    if (!ego_shape(h, window_size, &drows, &dcols)) return fail(BCP_E_INVALID, "%s: unsupported window size", who);
    HIP_TRY(hipSetDevice(h->device));
    if (dcols < 4) return fail(BCP_E_INVALID, "%s: windows narrower than 4 px are not supported", who);
    const EgoArgs a = ego_args_of(h, obs_rows(h, rec), poses, n, window_origin, drows, dcols, border_value, out);
    const EgoCall call = {a.rows, a.cols, a.shared != 0, drows, dcols, border_value, pool, n};
    hipStream_t st = (hipStream_t)stream;
    // the cell lists, where the sparse route can serve the call: counted (and listed) on the first such call after the maps
    // were (re)bound
    h->ego_route[0] = h->ego_route[1] = h->ego_route[2] = h->ego_route[3] = 0;
    EgoCells& cells = h->ego_cells;
    int32_t limit = 0;
    if (ego_sparse_candidate(call, h->tune.ego_sparse, cells.refused())) {
        limit = ego_sparse_limit(h->tune.ego_sparse, (int64_t)drows * dcols, ego_fits_lds(a.rows, a.cols, drows));
        BCP_TRY(cells.ensure(h, a.shared ? 1 : n_slots(h), limit, st));
        h->ego_route[1] = cells.largest();
        h->ego_route[2] = cells.stride();
        h->ego_route[3] = limit;
    }
    const EgoPlan plan = ego_route_of(call, limit > 0 && cells.usable(limit), cells.largest(), limit);
    h->ego_route[0] = plan.route;
    return launch_ego(h, a, plan, pool, st);
}

extern "C" int bcp_egocentric_costmaps(bcp_handle* h, const double* poses, int64_t n, const double* window_origin,
                                       const double* window_size, uint8_t border_value, uint8_t* out, void* stream)
{
    return egocentric_costmaps(h, poses, n, window_origin, window_size, border_value, out, stream, nullptr);
}

extern "C" int bcp_egocentric_pooled_shape(bcp_handle* h, const double* window_size, int32_t pool, int32_t* shape_hw)
{
    if (pool < 1 || pool > 64) return fail(BCP_E_INVALID, "bcp_egocentric_pooled_shape: pool must be in [1, 64]");
    const int rc = bcp_egocentric_shape(h, window_size, shape_hw);
    if (rc != BCP_OK) return rc;
    shape_hw[0] = (shape_hw[0] + pool - 1) / pool;
    shape_hw[1] = (shape_hw[1] + pool - 1) / pool;
    return BCP_OK;
}

extern "C" int bcp_egocentric_costmaps_pooled(bcp_handle* h, const double* poses, int64_t n, const double* window_origin,
                                              const double* window_size, uint8_t border_value, int32_t pool, uint8_t* out,
                                              void* stream)
{
    if (pool < 1 || pool > 64) return fail(BCP_E_INVALID, "bcp_egocentric_costmaps_pooled: pool must be in [1, 64]");
    return egocentric_costmaps(h, poses, n, window_origin, window_size, border_value, out, stream, nullptr, pool,
                               "bcp_egocentric_costmaps_pooled");
}

extern "C" int bcp_goal_n_state(bcp_handle* h, const double* world_size, float* out, void* stream)
{
    return goal_n_state(h, world_size, out, stream, nullptr, "bcp_goal_n_state");
}

extern "C" int bcp_goal_direction_state(bcp_handle* h, const double* world_size, double* out, void* stream)
{
    return goal_direction_state(h, world_size, out, stream, nullptr, "bcp_goal_direction_state");
}

// ---- episode ends under auto-reset (bcp_episode_record) ----------------------------------------------------------
extern "C" int bcp_bind_episode_record(bcp_handle* h, const bcp_episode_record* rec)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_bind_episode_record: null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (!rec) {
        h->have_rec = false;
        memset(&h->rec, 0, sizeof(h->rec));
        h->static_dirty = true;
        return BCP_OK;
    }
    const bcp_params& p = h->params;
    const bcp_state& f = rec->final;
    if (rec->capacity <= 0 || rec->capacity > ((int64_t)1 << 31) - 1)
        return fail(BCP_E_INVALID, "bcp_bind_episode_record: capacity must be in [1, 2^31)");
    if (!rec->reason || !rec->count || !rec->env_id || !rec->geom || (rec->ret && !rec->final_ret))
        return fail(BCP_E_INVALID, "bcp_bind_episode_record: reason, count, env_id, geom (and final_ret with ret) are required");
    if (!f.x || !f.y || !f.angle || !f.v || !f.w || !f.min_spat_dist_so_far || !f.target_idx || !f.current_iter ||
        !f.robot_collided || (p.model == BCP_MODEL_TRICYCLE && (!f.steering_motor_command || !f.wheel_angle)))
        return fail(BCP_E_INVALID, "bcp_bind_episode_record: missing final-state array");
    if ((p.pose_delay > 0 && !f.pose_seen) || (p.state_delay > 0 && !f.robot_state_seen))
        return fail(BCP_E_INVALID, "bcp_bind_episode_record: delays > 0 need the final pose_seen / robot_state_seen");
    if (f.control_queue || f.poses_queue || f.robot_state_queue)
        return fail(BCP_E_INVALID, "bcp_bind_episode_record: the final state keeps no queues (their pointers must be NULL)");
    HIP_TRY(h->rec_work.reserve(3));
    // (no stream to order this on: every step still in flight on any stream finishes first)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(h->rec_work.get(), 0, 3 * sizeof(uint32_t)));
    EpisodeRec& R = h->rec;
    R.reason = rec->reason;
    R.ret = rec->ret;
    R.count = rec->count;
    R.env_id = rec->env_id;
    R.geom = rec->geom;
    R.final_ret = rec->final_ret;
    R.fin = to_dev_state(&f);
    R.fin.pose_seen = p.pose_delay > 0 ? f.pose_seen : nullptr;
    R.fin.state_seen = p.state_delay > 0 ? f.robot_state_seen : nullptr;
    R.capacity = rec->capacity;
    R.work = h->rec_work.get();
    h->have_rec = true;
    h->static_dirty = true;
    return BCP_OK;
}

extern "C" int bcp_episode_record_overflows(bcp_handle* h, int64_t* steps, void* stream)
{
    if (!h || !steps) return fail(BCP_E_INVALID, "bcp_episode_record_overflows: null argument");
    *steps = 0;
    if (!h->rec_work.get()) return BCP_OK;
    HIP_TRY(hipSetDevice(h->device));
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->rec_work.get() + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(h->rec_work.get() + 2, 0, sizeof(uint32_t), (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *steps = (int64_t)v;
    return BCP_OK;
}

extern "C" int bcp_final_egocentric_costmaps(bcp_handle* h, const double* window_origin, const double* window_size,
                                             int32_t border_value, uint8_t* out, void* stream)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_final_egocentric_costmaps: null handle");
    if (!h->have_rec) return fail(BCP_E_STATE, "bcp_final_egocentric_costmaps: no episode record bound");
    if (border_value < 0 || border_value > 255) return fail(BCP_E_INVALID, "bcp_final_egocentric_costmaps: border value");
    return egocentric_costmaps(h, nullptr, h->rec.capacity, window_origin, window_size, (uint8_t)border_value, out, stream,
                               &h->rec, 1, "bcp_final_egocentric_costmaps");
}

extern "C" int bcp_final_egocentric_costmaps_pooled(bcp_handle* h, const double* window_origin, const double* window_size,
                                                    int32_t border_value, int32_t pool, uint8_t* out, void* stream)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_final_egocentric_costmaps_pooled: null handle");
    if (!h->have_rec) return fail(BCP_E_STATE, "bcp_final_egocentric_costmaps_pooled: no episode record bound");
    if (border_value < 0 || border_value > 255) return fail(BCP_E_INVALID, "bcp_final_egocentric_costmaps_pooled: border value");
    if (pool < 1 || pool > 64) return fail(BCP_E_INVALID, "bcp_final_egocentric_costmaps_pooled: pool must be in [1, 64]");
    return egocentric_costmaps(h, nullptr, h->rec.capacity, window_origin, window_size, (uint8_t)border_value, out, stream,
                               &h->rec, pool, "bcp_final_egocentric_costmaps_pooled");
}

extern "C" int bcp_final_goal_n_state(bcp_handle* h, const double* world_size, float* out, void* stream)
{
    if (h && !h->have_rec) return fail(BCP_E_STATE, "bcp_final_goal_n_state: no episode record bound");
    return goal_n_state(h, world_size, out, stream, h ? &h->rec : nullptr, "bcp_final_goal_n_state");
}

extern "C" int bcp_final_goal_direction_state(bcp_handle* h, const double* world_size, double* out, void* stream)
{
    if (h && !h->have_rec) return fail(BCP_E_STATE, "bcp_final_goal_direction_state: no episode record bound");
    return goal_direction_state(h, world_size, out, stream, h ? &h->rec : nullptr, "bcp_final_goal_direction_state");
}

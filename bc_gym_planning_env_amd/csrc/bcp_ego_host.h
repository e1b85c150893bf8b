// bcp_ego_host.h -- the host side of the observations: egocentric costmaps (which of the kernels of bcp_ego.h draws them,
// and the cell lists of the sparse route), the goal-state vectors with their two small kernels, and the episode record
// with its final observations.  Included by bcplan.hip after bcp_step_host.h.
#pragma once

// The rows an observation kernel reads: the bound state (n = n_envs, env i on entry geom_of_env[i] or i), or the final
// states of an episode record (n = capacity, row j on entry `entry[j]`, only rows j < *live).
struct ObsRows {
    DevState st;
    int64_t n;
    const int32_t* entry;
    const int32_t* live;
};

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

// The cost model of the sparse route (tools/bench_ego_cells.py measures both sides on the box): per image the fill-and-patch
// kernel pays ~0.4 instructions per listed cell for the culling pass and ~2.5 per cell that meets the window, the sampling
// kernels ~0.1 per destination pixel when the map is staged in LDS whole and five times that when every workgroup stages the
// part of the map its window sees.  BCP_TUNE_EGO_SPARSE >= 2 is an explicit limit (tests, sweeps).
static int32_t ego_sparse_limit(int32_t tuning, int64_t pixels, bool fits_lds)
{
    if (tuning >= 2) return tuning;
    const int64_t lim = fits_lds ? pixels / 8 : pixels / 2;
    return (int32_t)std::max<int64_t>(kEgoCellCapMin, std::min<int64_t>(lim, 16384));
}

extern "C" int bcp_egocentric_route(bcp_handle* h, int32_t* info4)
{
    if (!h || !info4) return fail(BCP_E_INVALID, "bcp_egocentric_route: null argument");
    for (int k = 0; k < 4; ++k) info4[k] = h->ego_route[k];
    return BCP_OK;
}

// waves per workgroup of ego_pooled_sparse_kernel: as many of kEgoWaves as fit the 64 KB the sparse route budgets (a small
// `pool` on a large window leaves many words per image); 0 = not even one, the sampled route takes the call
static int ego_pooled_sparse_waves(int drows, int dcols, const EgoPool& Q)
{
    const size_t one = ego_pooled_lds_bytes(drows, dcols, Q.prows, Q.pcols, 1);
    return (int)std::min<size_t>(kEgoWaves, 64 * 1024 / one);
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
    EgoArgs a;
    memset(&a, 0, sizeof(a));
    if (!ego_shape(h, window_size, &a.drows, &a.dcols))
        return fail(BCP_E_INVALID, "%s: unsupported window size", who);
    HIP_TRY(hipSetDevice(h->device));
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
    a.sx = h->st.x;
    a.sy = h->st.y;
    a.sth = h->st.angle;
    if (h->params.pose_delay > 0 && h->st.pose_seen) {   // the observation shows State.pose, i.e. the delayed pose
        a.sx = h->st.pose_seen;
        a.sy = h->st.pose_seen + h->n;
        a.sth = h->st.pose_seen + 2 * h->n;
    }
    a.geom_of_env = h->n_geoms > 0 ? h->geom_of_env : nullptr;
    a.n_envs = h->n;
    if (rec) {   // the record's rows: its final poses (State.pose: the delayed one with a pose delay), entries, count
        const int64_t c = rec->capacity;
        a.sx = rec->fin.x;
        a.sy = rec->fin.y;
        a.sth = rec->fin.angle;
        if (h->params.pose_delay > 0 && rec->fin.pose_seen) {
            a.sx = rec->fin.pose_seen;
            a.sy = rec->fin.pose_seen + c;
            a.sth = rec->fin.pose_seen + 2 * c;
        }
        a.geom_of_env = h->n_geoms > 0 ? rec->geom : (h->map.shared ? nullptr : rec->env_id);
        a.n_envs = c;
        a.live = rec->count;
    }
    a.has_window = window_origin != nullptr;
    if (window_origin) {
        a.win_ox = window_origin[0];
        a.win_oy = window_origin[1];
    }
    const size_t map_bytes = ((size_t)(a.rows + 2) * (a.cols + 2) + 7) & ~(size_t)7;   // LDS copy with a border ring
    const size_t row_bytes = ((size_t)a.drows * 2 + kEgoBoundInts) * sizeof(int32_t);   // one table: row terms, row bounds
    a.border = border_value;
    a.out = out;
    a.n_images = n;
    a.cols_magic = (uint32_t)(((uint64_t)1 << 32) / (uint64_t)a.cols) + 1;   // (staged maps are < 64 KB: exact)
    if (a.dcols < 4) return fail(BCP_E_INVALID, "%s: windows narrower than 4 px are not supported", who);
    const bool px8 = a.dcols >= 8;   // 8 pixels (one 64-bit store) per lane; narrow windows fall back to 4
    hipStream_t st = (hipStream_t)stream;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    cus = std::max(cus, 1);
    const dim3 block(256);
    // Sparse maps and a zero border (extract_egocentric_costmap's default): zero fill + one patch per non-zero source cell
    // (ego_sparse_kernel).  Decided per call from the counts of non-zero cells: a counting pass over the maps on the first
    // such call after the maps were (re)bound, one read-back of the largest count, lists sized from it; a pool refresh keeps
    // counts and lists of the entries it re-samples up to date.  Maps with more cells than the cost model's limit (or a
    // non-zero border) keep the sampling kernels below.
    const bool fits_lds = map_bytes + 4 * row_bytes <= 150 * 1024;
    h->ego_route[0] = h->ego_route[1] = h->ego_route[2] = h->ego_route[3] = 0;
    EgoPool Q = {pool, (a.drows + pool - 1) / pool, (a.dcols + pool - 1) / pool, (uint32_t)(((uint64_t)1 << 32) / (uint64_t)pool) + 1};
    // (pooled: fewer waves per workgroup where the pooled words of eight images do not fit; none -> the sampled route)
    const int sparse_waves = pool > 1 ? ego_pooled_sparse_waves(a.drows, a.dcols, Q)
                                      : (ego_sparse_lds_bytes(a.drows, a.dcols, kEgoWaves) <= 64 * 1024 ? kEgoWaves : 0);
    if (border_value == 0 && a.rows <= 4095 && a.cols <= 4095 && !h->ego_cells_refused && h->ego_sparse && sparse_waves > 0) {
        const int64_t entries = a.shared ? 1 : n_slots(h);
        const int32_t limit = ego_sparse_limit(h->ego_sparse, (int64_t)a.drows * a.dcols, fits_lds);
        if (h->refresh_recorded && (!h->ego_cells_built || h->ego_cells_max < 0))
            HIP_TRY(hipStreamWaitEvent(st, h->refresh_done, 0));   // (a refresh on another stream may still be writing the maps / counts)
        if (h->ego_cells_entries != entries || !h->ego_cell_counts.get()) {
            (void)h->ego_cells.reset();
            h->ego_cells_entries = 0;
            h->ego_cell_cap = 0;
            h->ego_cells_built = false;
            if (h->ego_cell_counts.reserve((size_t)entries + 1) != hipSuccess) {
                (void)hipGetLastError();
                h->ego_cells_refused = true;   // (no room: not an error, the sampling kernels take over)
            } else {
                h->ego_cells_entries = entries;
            }
        }
        if (h->ego_cell_counts.get() && !h->ego_cells_built) {
            // counting pass -> largest count -> stride of the lists -> lists
            const EntrySelect all = {nullptr, nullptr, entries};
            (void)h->ego_cells.reset();   // (the counting pass is the one without lists; they are sized from its result)
            h->ego_cell_cap = 0;
            HIP_TRY(hipMemsetAsync(h->ego_cell_counts.get() + entries, 0, sizeof(int32_t), st));
            launch_ego_cells(h, all, entries, st);
            HIP_TRY(hipMemcpyAsync(&h->ego_cells_max, h->ego_cell_counts.get() + entries, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            h->ego_cells_built = true;
            if (h->ego_cells_max <= limit) {
                // pool entries change under a refresh: leave room for a world with more cells than today's largest
                int64_t cap = std::max<int64_t>(kEgoCellCapMin, ((int64_t)h->ego_cells_max + 63) & ~(int64_t)63);
                const int64_t budget = (int64_t)1 << 30;   // bytes of lists per handle
                if (entries * cap * 4 > budget) cap = ((int64_t)h->ego_cells_max + 63) & ~(int64_t)63;
                if (h->ego_stride > 0) cap = h->ego_stride;   // (tests: entries with more cells than this are drawn pixel by pixel)
                if (cap > 0 && entries * cap * 4 <= budget &&
                    h->ego_cells.reserve((size_t)entries * cap) == hipSuccess) {
                    h->ego_cell_cap = (int32_t)cap;
                    const int32_t counted = h->ego_cells_max;
                    launch_ego_cells(h, all, entries, st);   // (the same counts again, and the lists)
                    h->ego_cells_max = counted;
                } else {
                    (void)hipGetLastError();
                    if (cap > 0) h->ego_cells_refused = true;
                }
            }
        }
        if (h->ego_cell_counts.get() && h->ego_cells_built && h->ego_cells_max < 0) {   // (a refresh re-counted some entries)
            HIP_TRY(hipMemcpyAsync(&h->ego_cells_max, h->ego_cell_counts.get() + entries, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        h->ego_route[1] = h->ego_cells_max;
        h->ego_route[2] = h->ego_cell_cap;
        h->ego_route[3] = limit;
        if (pool > 1 && h->ego_cells.get() && h->ego_cells_built && h->ego_cells_max >= 0 && h->ego_cells_max <= limit) {
            // one image per wave as below; nothing but the pooled bytes goes to HBM
            const dim3 grid((unsigned)((n + sparse_waves - 1) / sparse_waves));
            const size_t lds = ego_pooled_lds_bytes(a.drows, a.dcols, Q.prows, Q.pcols, sparse_waves);   // (<= 64 KB)
            hipLaunchKernelGGL(ego_pooled_sparse_kernel, grid, dim3(64 * sparse_waves), lds, st, a, Q, h->ego_cells.get(),
                               h->ego_cell_counts.get(), h->ego_cell_cap);
            HIP_TRY(hipGetLastError());
            h->ego_route[0] = BCP_EGO_POOLED_SPARSE;
            return BCP_OK;
        }
        if (pool == 1 && h->ego_cells.get() && h->ego_cells_built && h->ego_cells_max >= 0 && h->ego_cells_max <= limit) {
            // One image per wave, eight per workgroup: 8 192 short workgroups for 65 536 images.  (Round 3 first ran this kernel
            // persistently -- as many workgroups as the chip holds, 64 images per wave, the lanes sharing the transforms' float64
            // arithmetic: 11 % slower on the same box, 0.249 against 0.222 ms.  Stores from many short workgroups drain faster than
            // from a few long-lived ones, tools/fill_rate.hip; the arithmetic saved was never the bottleneck, VALU busy 17 %.
            // Also measured: an image split over 2 / 4 waves of a workgroup (+- 0 / 14 % slower), a plain one-image kernel with
            // 48 instead of 83 registers (3 - 8 % slower), fewer workgroups per CU by way of unused LDS (within the noise).)
            const dim3 wide(64 * kEgoWaves);
            const dim3 grid((unsigned)((n + kEgoWaves - 1) / kEgoWaves));
            const size_t lds = ego_sparse_lds_bytes(a.drows, a.dcols, kEgoWaves);   // (<= 64 KB: checked above)
            hipLaunchKernelGGL(ego_sparse_kernel, grid, wide, lds, st, a, h->ego_cells.get(), h->ego_cell_counts.get(), h->ego_cell_cap);
            HIP_TRY(hipGetLastError());
            h->ego_route[0] = BCP_EGO_SPARSE;
            return BCP_OK;
        }
    }
    if (pool > 1) {
        // any map, any border value: every pooled cell samples its block from global memory
        const dim3 grid((unsigned)((n + kEgoWaves - 1) / kEgoWaves));
        hipLaunchKernelGGL(ego_pooled_sampled_kernel, grid, dim3(64 * kEgoWaves), 0, st, a, Q);
        HIP_TRY(hipGetLastError());
        h->ego_route[0] = BCP_EGO_POOLED_SAMPLED;
        return BCP_OK;
    }
    if (!a.shared && fits_lds && n < ((int64_t)1 << 31)) {
        h->ego_route[0] = BCP_EGO_BINNED;
        // private / pooled maps that fit LDS: group the images by map entry, then one workgroup per entry at a time
        const int64_t n_bins = n_slots(h);
        // (two arrays in each buffer; only ever reserved in pairs, so half the capacity is the second one's offset)
        HIP_TRY(h->ego_bins.reserve((size_t)2 * n_bins));
        HIP_TRY(h->ego_order.reserve((size_t)2 * n));
        int32_t* bin_count = h->ego_bins.get();
        int32_t* bin_start = h->ego_bins.get() + h->ego_bins.capacity() / 2;
        int32_t* rank = h->ego_order.get();
        int32_t* order = h->ego_order.get() + h->ego_order.capacity() / 2;
        HIP_TRY(hipMemsetAsync(bin_count, 0, (size_t)n_bins * sizeof(int32_t), st));
        const dim3 per_image((unsigned)((n + 255) / 256));
        hipLaunchKernelGGL(ego_bin_count_kernel, per_image, block, 0, st, a.geom_of_env, a.n_envs, n, bin_count, rank, a.live);
        hipLaunchKernelGGL(ego_bin_scan_kernel, dim3(1), dim3(1024), 0, st, bin_count, n_bins, bin_start);
        hipLaunchKernelGGL(ego_bin_scatter_kernel, per_image, block, 0, st, a.geom_of_env, a.n_envs, n, bin_start, rank, order,
                           a.live);
        HIP_TRY(hipGetLastError());
        const size_t lds = map_bytes + 4 * row_bytes;
        const void* fn = px8 ? (const void*)ego_costmap_binned_kernel<8> : (const void*)ego_costmap_binned_kernel<4>;
        BCP_TRY(variant_lds(h, fn, lds));
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds));
        const dim3 grid((unsigned)std::min<int64_t>(n, (int64_t)std::max(per_cu, 1) * cus));
        a.stage_map = 1;
        return launch_fn(fn, grid, block, lds, st, a, bin_start, bin_count, order);
    } else {
        // shared map (staged in LDS when it fits) or maps too large for LDS: persistent workgroups, as many as are
        // resident at once
        // (gfx950 gives a workgroup up to 160 KB of LDS; a big copy costs occupancy, but LDS sampling still wins)
        a.stage_map = (a.shared && fits_lds) ? 1 : 0;
        // too large: each workgroup stages just the part of the map its window can see -- at most the window's
        // diagonal (+ 2 px of rounding, + ring) squared
        const double diag = std::sqrt((double)a.drows * a.drows + (double)a.dcols * a.dcols);
        const size_t side = (size_t)std::ceil(diag) + 5;
        const size_t win_bytes = (side * side + 7) & ~(size_t)7;
        if (!a.stage_map && win_bytes + row_bytes <= 60 * 1024) {
            a.win_lds_bytes = (int32_t)win_bytes;
            const size_t lds = win_bytes + row_bytes;
            const void* fn = px8 ? (const void*)ego_costmap_window_kernel<8> : (const void*)ego_costmap_window_kernel<4>;
            int per_cu = 0;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds));
            const dim3 grid((unsigned)std::min<int64_t>(n, (int64_t)std::max(per_cu, 1) * cus));
            h->ego_route[0] = BCP_EGO_WINDOW;
            return launch_fn(fn, grid, block, lds, st, a);   // (lds <= 60 KiB)
        }
        const int waves = kEgoWaves;
        h->ego_route[0] = a.stage_map ? BCP_EGO_STAGED : BCP_EGO_GLOBAL;
        const size_t lds = waves * row_bytes + (a.stage_map ? map_bytes : 0);
        const void* fn = a.stage_map ? (px8 ? (const void*)ego_costmap_kernel<true, 8> : (const void*)ego_costmap_kernel<true, 4>)
                                     : (px8 ? (const void*)ego_costmap_kernel<false, 8> : (const void*)ego_costmap_kernel<false, 4>);
        BCP_TRY(variant_lds(h, fn, lds));
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * waves, lds));
        const dim3 grid((unsigned)std::min<int64_t>((n + waves - 1) / waves, (int64_t)std::max(per_cu, 1) * cus));
        return launch_fn(fn, grid, dim3(64 * waves), lds, st, a);
    }
}

// the bound state's rows, or (rec) the record's final states
static ObsRows obs_rows(const bcp_handle* h, const EpisodeRec* rec)
{
    ObsRows R;
    if (rec) {
        R.st = rec->fin;
        R.n = rec->capacity;
        R.entry = h->n_geoms > 0 ? rec->geom : rec->env_id;
        R.live = rec->count;
    } else {
        R.st = h->st;
        R.n = h->n;
        R.entry = nullptr;
        R.live = nullptr;
    }
    return R;
}

static int goal_n_state(bcp_handle* h, const double* world_size, float* out, void* stream, const EpisodeRec* rec, const char* who)
{
    if (!h || !world_size || !out) return fail(BCP_E_INVALID, "%s: null argument", who);
    if (!h->have_path || !h->have_state) return fail(BCP_E_STATE, "%s: paths and state must be set first", who);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->static_dirty) BCP_TRY(upload_step_static(h, s));
    const int n_state = h->params.model == BCP_MODEL_TRICYCLE ? 6 : 5;
    const ObsRows R = obs_rows(h, rec);
    hipLaunchKernelGGL(goal_n_state_kernel, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, s, h->dev_static.get(), R,
                       world_size[0], world_size[1], n_state, out);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

static int goal_direction_state(bcp_handle* h, const double* world_size, double* out, void* stream, const EpisodeRec* rec,
                                const char* who)
{
    if (!h || !world_size || !out) return fail(BCP_E_INVALID, "%s: null argument", who);
    if (!h->have_path || !h->have_state) return fail(BCP_E_STATE, "%s: paths and state must be set first", who);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->static_dirty) BCP_TRY(upload_step_static(h, s));
    const ObsRows R = obs_rows(h, rec);
    hipLaunchKernelGGL(goal_direction_state_kernel, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, s, h->dev_static.get(), R,
                       world_size[0], world_size[1], out);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
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

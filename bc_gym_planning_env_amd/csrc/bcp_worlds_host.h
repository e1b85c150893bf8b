// bcp_worlds_host.h -- entry points of the world samplers: RandomMiniEnv worlds and their refreshed ring (kernels in
// bcp_sample.h), RandomAisleTurnEnv worlds (bcp_aisle.h).  Included by bcplan.hip after bcp_ego_host.h.
#pragma once

// ---- RandomMiniEnv worlds sampled on the device ----------------------------------------------------------------
extern "C" int bcp_mini_world_seed(bcp_handle* h, const int64_t* seeds, int64_t n_chains, uint32_t* mt_state, void* stream)
{
    if (!h || !seeds || !mt_state || n_chains <= 0) return fail(BCP_E_INVALID, "bcp_mini_world_seed: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(mt_seed_kernel, dim3((unsigned)((n_chains + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seeds,
                       n_chains, mt_state);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

static int sample_mini_worlds(bcp_handle* h, const bcp_mini_world_params* p, uint32_t* mt_state, int64_t n_chains,
                              int32_t episodes, int32_t rows, int32_t cols, const int32_t* counts, const int64_t* first_world,
                              double* worlds, uint8_t* maps, int32_t* status, void* stream)
{
    if (!(p->resolution > 0) || !check_kernel_size(h->params, p->resolution))
        return fail(BCP_E_INVALID, "bcp_sample_mini_worlds: bad resolution for this footprint");
    if ((int)(0.05 / p->resolution) > 1)   // Wall.render: thickness = max(1, int(width / resolution))
        return fail(BCP_E_INVALID, "bcp_sample_mini_worlds: walls thicker than one pixel are not supported");
    const int wpr = (cols + 31) / 32;
    const size_t lds = sample_lds_words(rows, wpr) * sizeof(uint32_t);
    if (rows <= 0 || cols <= 0 || lds > 60 * 1024) return fail(BCP_E_INVALID, "bcp_sample_mini_worlds: unsupported map shape");
    HIP_TRY(hipSetDevice(h->device));
    DevParams P = h->dev;
    scale_footprint(P, h->params, p->resolution);
    MiniWorldParams mp;
    mp.inner_h = p->inner_h;
    mp.inner_w = p->inner_w;
    mp.mid_margin = p->mid_margin;
    mp.out_margin = p->out_margin;
    mp.min_obstacle_angle = p->min_obstacle_angle;
    mp.max_obstacle_angle = p->max_obstacle_angle;
    mp.lim_euc_dist = p->lim_euc_dist;
    mp.lim_ang_dist = p->lim_ang_dist;
    mp.angular_pose_noise_scale = p->angular_pose_noise_scale;
    mp.resolution = p->resolution;
    mp.goal_spat_dist = p->goal_spat_dist;
    mp.goal_ang_dist = p->goal_ang_dist;
    if (footprint_is_wide(h->params, p->resolution))
        hipLaunchKernelGGL(mini_world_sample_kernel<true>, dim3((unsigned)n_chains), dim3(64), lds, (hipStream_t)stream, P, mp,
                           mt_state, n_chains, (int)episodes, (int)rows, (int)cols, counts, first_world, worlds, maps, status);
    else
        hipLaunchKernelGGL(mini_world_sample_kernel<false>, dim3((unsigned)n_chains), dim3(64), lds, (hipStream_t)stream, P, mp,
                           mt_state, n_chains, (int)episodes, (int)rows, (int)cols, counts, first_world, worlds, maps, status);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_sample_mini_worlds(bcp_handle* h, const bcp_mini_world_params* p, uint32_t* mt_state, int64_t n_chains,
                                      int32_t episodes, int32_t rows, int32_t cols, double* worlds, uint8_t* maps,
                                      int32_t* status, void* stream)
{
    if (!h || !p || !mt_state || !worlds || !maps || !status || n_chains <= 0 || episodes <= 0)
        return fail(BCP_E_INVALID, "bcp_sample_mini_worlds: bad argument");
    return sample_mini_worlds(h, p, mt_state, n_chains, episodes, rows, cols, nullptr, nullptr, worlds, maps, status, stream);
}

static int check_ring(const bcp_handle* h, int32_t episodes, const char* who)
{
    if (episodes < 2 || h->n_geoms <= 0 || (int64_t)h->n_geoms != h->n * episodes || !h->next_geom)
        return fail(BCP_E_STATE, "%s: needs a geometry pool of n_envs x episodes (>= 2) entries with next_geom", who);
    if (!h->have_map || !h->have_path || !h->have_init || h->map.shared || h->path.shared || h->map_valid_rows ||
        h->map_valid_cols)
        return fail(BCP_E_STATE, "%s: pool costmaps, paths and initial state must be set first", who);
    return BCP_OK;
}

extern "C" int bcp_plan_mini_worlds(bcp_handle* h, int32_t episodes, int64_t* generated, int32_t* info, void* stream)
{
    if (!h || !generated || !info) return fail(BCP_E_INVALID, "bcp_plan_mini_worlds: null argument");
    BCP_TRY(check_ring(h, episodes, "bcp_plan_mini_worlds"));
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = h->n, G = h->n_geoms;
    const size_t bytes = (size_t)n * sizeof(int64_t) + (size_t)(n + G + 4) * sizeof(int32_t);
    HIP_TRY(h->ring.reserve(bytes));
    int64_t* first_world = (int64_t*)h->ring.get();
    int32_t* counts = (int32_t*)(first_world + n);
    int32_t* dirty = counts + n;
    int32_t* tally = dirty + G;
    HIP_TRY(hipMemsetAsync(tally, 0, 4 * sizeof(int32_t), s));
    hipLaunchKernelGGL(mini_world_ring_plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, (int)episodes,
                       h->geom_of_env, const_cast<int32_t*>(h->next_geom), generated, counts, first_world, dirty, tally);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(info, tally, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    h->ring_episodes = episodes;
    h->ring_planned = true;
    return BCP_OK;
}

extern "C" int bcp_refresh_mini_worlds(bcp_handle* h, const bcp_mini_world_params* p, uint32_t* mt_state, double* worlds,
                                       uint8_t* maps, double* paths, int32_t* lens, double* init, double path_delta,
                                       int32_t* status, int32_t* path_status, void* stream)
{
    if (!h || !p || !mt_state || !worlds || !maps || !paths || !lens || !init || !status || !path_status || !(path_delta > 0))
        return fail(BCP_E_INVALID, "bcp_refresh_mini_worlds: bad argument");
    if (!h->ring_planned) return fail(BCP_E_STATE, "bcp_refresh_mini_worlds: call bcp_plan_mini_worlds first");
    const int32_t episodes = h->ring_episodes;
    BCP_TRY(check_ring(h, episodes, "bcp_refresh_mini_worlds"));
    if (maps != h->map_data || paths != h->path_src || lens != h->path.lens)
        return fail(BCP_E_INVALID, "bcp_refresh_mini_worlds: maps / paths / lens are not the arrays this handle was given");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = h->n, G = h->n_geoms;
    const int64_t* first_world = (const int64_t*)h->ring.get();
    const int32_t* counts = (const int32_t*)(first_world + n);
    const int32_t* dirty = counts + n;
    const int32_t* tally = dirty + G;
    BCP_TRY(sample_mini_worlds(h, p, mt_state, n, episodes, h->map.rows, h->map.cols, counts, first_world, worlds, maps,
                                      status, stream));
    const EntrySelect sel = {dirty, tally, G};
    hipLaunchKernelGGL(mini_world_paths_kernel, dim3(stride_grid(G, 128, true)), dim3(128), 0, s, worlds, sel, path_delta,
                       h->params.spatial_precision, h->params.angular_precision,
                       (int)(h->params.reward_provider == BCP_REWARD_PURE_PURSUIT), (int)h->path.max_len, paths, lens, init,
                       path_status);
    launch_pack_bitmap(h, sel, G, s);
    // under the single-launch step nothing reads the uint8 fields: tiles only, the fields follow on demand
    BCP_TRY(h->field.rebuild(h, sel, G, s, DistanceField::refresh_reads_tiles_only(h)));
    launch_path_data(h, sel, G, s);
    hipLaunchKernelGGL(pool_initial_state_kernel, dim3(stride_grid(G, 256, true)), dim3(256), 0, s, sel, paths,
                       (int)h->path.max_len, init, h->init);
    HIP_TRY(hipGetLastError());
    if (!h->refresh_done) HIP_TRY(hipEventCreateWithFlags(h->refresh_done.put(), hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->refresh_done.get(), s));
    h->refresh_recorded = true;
    h->ring_planned = false;
    h->ring_refreshed = true;
    return BCP_OK;
}

extern "C" int bcp_release_mini_worlds(bcp_handle* h, void* stream)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_release_mini_worlds: null handle");
    if (!h->ring.get() || !h->ring_refreshed || (int64_t)h->n_geoms != h->n * h->ring_episodes || !h->next_geom)
        return fail(BCP_E_STATE, "bcp_release_mini_worlds: no bcp_refresh_mini_worlds to complete");
    HIP_TRY(hipSetDevice(h->device));
    const int64_t n = h->n;
    const int64_t* first_world = (const int64_t*)h->ring.get();
    const int32_t* counts = (const int32_t*)(first_world + n);
    hipLaunchKernelGGL(mini_world_ring_release_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       (int)h->ring_episodes, counts, first_world, const_cast<int32_t*>(h->next_geom));
    HIP_TRY(hipGetLastError());
    h->ring_refreshed = false;
    return BCP_OK;
}

extern "C" int bcp_mini_world_paths(bcp_handle* h, const double* worlds, int64_t n_worlds, double path_delta, int32_t max_len,
                                    double* paths, int32_t* lens, double* init, int32_t* status, void* stream)
{
    if (!h || !worlds || !paths || !lens || !init || !status || n_worlds <= 0 || max_len < 2 || !(path_delta > 0))
        return fail(BCP_E_INVALID, "bcp_mini_world_paths: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    const EntrySelect all = {nullptr, nullptr, n_worlds};
    hipLaunchKernelGGL(mini_world_paths_kernel, dim3(stride_grid(n_worlds, 128)), dim3(128), 0, (hipStream_t)stream, worlds, all,
                       path_delta, h->params.spatial_precision, h->params.angular_precision,
                       (int)(h->params.reward_provider == BCP_REWARD_PURE_PURSUIT), (int)max_len, paths, lens, init, status);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

// ---- RandomAisleTurnEnv worlds made on the device ----------------------------------------------------------------
static bool aisle_resolution_ok(double resolution)
{
    return resolution > 0 && (int)(0.05 / resolution) <= 1;   // Wall.render: thickness = max(1, int(width / resolution))
}

extern "C" int bcp_sample_aisle_worlds(bcp_handle* h, const bcp_aisle_world_params* p, uint32_t* mt_state, int64_t n_chains,
                                       int32_t episodes, double* worlds, int32_t* shapes, void* stream)
{
    if (!h || !p || !mt_state || !worlds || !shapes || n_chains <= 0 || episodes <= 0 || !(p->path_delta > 0))
        return fail(BCP_E_INVALID, "bcp_sample_aisle_worlds: bad argument");
    if (!aisle_resolution_ok(p->resolution))
        return fail(BCP_E_INVALID, "bcp_sample_aisle_worlds: resolution %g: walls thicker than one pixel are not supported",
                    p->resolution);
    HIP_TRY(hipSetDevice(h->device));
    AisleWorldParams ap;
    for (int k = 0; k < 2; ++k) {
        ap.main_length[k] = p->main_corridor_length[k];
        ap.turn_length[k] = p->turn_corridor_length[k];
        ap.angle[k] = p->turn_corridor_angle[k];
        ap.main_width[k] = p->main_corridor_width[k];
        ap.turn_width[k] = p->turn_corridor_width[k];
    }
    ap.margin = p->margin;
    ap.resolution = p->resolution;
    ap.path_delta = p->path_delta;
    hipLaunchKernelGGL(aisle_world_draw_kernel, dim3((unsigned)n_chains), dim3(64), 0, (hipStream_t)stream, ap, mt_state,
                       n_chains, (int)episodes, worlds, shapes);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_render_aisle_worlds(bcp_handle* h, const double* worlds, const int32_t* shapes, int64_t n_worlds,
                                       double resolution, int32_t rows, int32_t pitch, uint8_t* maps, void* stream)
{
    if (!h || !worlds || !shapes || !maps || n_worlds <= 0 || rows <= 0 || pitch <= 0 || (pitch & 15) ||
        ((uintptr_t)maps & 15))
        return fail(BCP_E_INVALID, "bcp_render_aisle_worlds: bad argument (pitch and maps must be 16-byte aligned)");
    if (!aisle_resolution_ok(resolution))
        return fail(BCP_E_INVALID, "bcp_render_aisle_worlds: resolution %g: walls thicker than one pixel are not supported",
                    resolution);
    if (n_worlds > 0x7fffffff) return fail(BCP_E_INVALID, "bcp_render_aisle_worlds: too many worlds");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(aisle_world_render_kernel, dim3((unsigned)n_worlds), dim3(256), 0, (hipStream_t)stream, worlds, shapes,
                       (int)rows, (int)pitch, 1.0 / resolution, maps);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_aisle_world_paths(bcp_handle* h, const double* worlds, int64_t n_worlds, double path_delta, int32_t max_len,
                                     double* paths, int32_t* lens, double* init, int32_t* status, void* stream)
{
    if (!h || !worlds || !paths || !lens || !init || !status || n_worlds <= 0 || max_len < 2 || !(path_delta > 0))
        return fail(BCP_E_INVALID, "bcp_aisle_world_paths: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(aisle_world_paths_kernel, dim3(stride_grid(n_worlds, 128)), dim3(128), 0, (hipStream_t)stream, worlds,
                       n_worlds, path_delta, h->params.spatial_precision, h->params.angular_precision,
                       (int)(h->params.reward_provider == BCP_REWARD_PURE_PURSUIT), (int)max_len, paths, lens, init, status);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}


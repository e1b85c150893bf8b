// bcp_seams_host.h -- entry points of the operator seams: binding the caller's state arrays, reset and broadcast, and the
// reference's operators one call at a time (kernels: bcp_seams.h).  Included by bcplan.hip after bcp_seams.h.
#pragma once

static DevState to_dev_state(const bcp_state* s)
{
    DevState d;
    d.x = s->x; d.y = s->y; d.angle = s->angle; d.v = s->v; d.w = s->w;
    d.steer = s->steering_motor_command; d.wheel = s->wheel_angle; d.min_dist = s->min_spat_dist_so_far;
    d.target_idx = s->target_idx; d.cur_iter = s->current_iter; d.collided = s->robot_collided;
    d.pose_seen = s->pose_seen; d.state_seen = s->robot_state_seen;
    d.control_q = s->control_queue; d.pose_q = s->poses_queue; d.state_q = s->robot_state_queue;
    return d;
}

static int check_state(const bcp_state* s, int tricycle, const bcp_params* p = nullptr, bool queues = true)
{
    if (!s) return 0;
    if (p) {   // delays > 0 need the arrays State exposes, and (for the live state) the queues
        if (p->pose_delay > 0 && (!s->pose_seen || (queues && !s->poses_queue))) return 0;
        if (p->state_delay > 0 && (!s->robot_state_seen || (queues && !s->robot_state_queue))) return 0;
        if (p->control_delay > 0 && queues && !s->control_queue) return 0;
    }
    if (!s->x || !s->y || !s->angle || !s->v || !s->w || !s->min_spat_dist_so_far || !s->target_idx ||
        !s->current_iter || !s->robot_collided)
        return 0;
    if (tricycle && (!s->steering_motor_command || !s->wheel_angle)) return 0;
    return 1;
}

extern "C" int bcp_bind_state(bcp_handle* h, const bcp_state* state)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_bind_state: null handle");
    if (!check_state(state, h->params.model == BCP_MODEL_TRICYCLE, &h->params))
        return fail(BCP_E_INVALID, "bcp_bind_state: missing state array (delays > 0 need pose_seen / robot_state_seen "
                                   "and the queues)");
    h->st = to_dev_state(state);
    h->have_state = true;
    h->static_dirty = true;
    return BCP_OK;
}

extern "C" int bcp_bind_initial_state(bcp_handle* h, const bcp_state* initial)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_bind_initial_state: null handle");
    if (!check_state(initial, h->params.model == BCP_MODEL_TRICYCLE))
        return fail(BCP_E_INVALID, "bcp_bind_initial_state: missing state array");
    // (the initial State exposes the initial pose / robot state themselves and has empty queues: nothing more to bind)
    h->init = to_dev_state(initial);
    h->have_init = true;
    h->init_declared = false;   // (a plain bind never reads device memory: whoever binds declares again)
    h->static_dirty = true;
    return BCP_OK;
}

// Bind-time work: the eleven arrays come to the host, are compared with their entry 0 (init_uniform_pack, bcp_init_uniform.h)
// and, when every entry agrees, entry 0 becomes the handle's snapshot -- the steps of the shared-geometry kernel then reset from
// the parameter block instead of loading the arrays (launch_step: kStepInitUniform).
extern "C" int bcp_declare_uniform_initial_state(bcp_handle* h, int on, void* stream)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_declare_uniform_initial_state: null handle");
    if (!on) {
        if (h->init_declared) h->static_dirty = true;
        h->init_declared = false;
        return BCP_OK;
    }
    if (!h->have_init) return fail(BCP_E_STATE, "bcp_declare_uniform_initial_state: no initial state bound");
    if (h->n_geoms > 0)
        return fail(BCP_E_STATE, "bcp_declare_uniform_initial_state: the handle has a geometry pool (an initial state per entry)");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const bool tri = h->params.model == BCP_MODEL_TRICYCLE;
    const size_t n = (size_t)h->n;
    const DevState& d = h->init;
    const double* const src[8] = {d.x, d.y, d.angle, d.v, d.w, tri ? d.steer : nullptr, tri ? d.wheel : nullptr, d.min_dist};
    std::vector<double> f64[8];
    std::vector<int32_t> target(n), iter(n);
    std::vector<uint8_t> collided(n);
    InitHostArrays a = {};
    for (int f = 0; f < 8; ++f) {
        if (!src[f]) continue;
        f64[f].resize(n);
        HIP_TRY(hipMemcpyAsync(f64[f].data(), src[f], n * sizeof(double), hipMemcpyDeviceToHost, s));
        a.f64[f] = f64[f].data();
    }
    HIP_TRY(hipMemcpyAsync(target.data(), d.target_idx, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(iter.data(), d.cur_iter, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(collided.data(), d.collided, n * sizeof(uint8_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    a.target = target.data();
    a.iter = iter.data();
    a.collided = collided.data();
    InitUniform packed;
    const InitDifference diff = init_uniform_pack(a, h->n, tri, &packed);
    if (diff.env >= 0) {
        if (h->init_declared) h->static_dirty = true;
        h->init_declared = false;
        return fail(BCP_E_INVALID, "bcp_declare_uniform_initial_state: env %lld differs from env 0 in %s -- the initial state is not uniform",
                    (long long)diff.env, init_field_name(diff.field));
    }
    h->init_snapshot = packed;
    h->init_declared = true;
    h->static_dirty = true;
    return BCP_OK;
}

extern "C" int bcp_reset_masked(bcp_handle* h, const uint8_t* mask, void* stream)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_reset_masked: null handle");
    if (!h->have_state || !h->have_init) return fail(BCP_E_STATE, "bcp_reset_masked: state / initial state not bound");
    HIP_TRY(hipSetDevice(h->device));
    const int threads = 256;
    const int blocks = (int)((h->n + threads - 1) / threads);
    hipLaunchKernelGGL(reset_kernel, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, h->st, h->init, mask, h->n,
                       (int)(h->params.model == BCP_MODEL_TRICYCLE), h->geom_of_env, h->next_geom,
                       h->have_rec ? h->rec.ret : nullptr);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_broadcast_state(bcp_handle* h, int64_t src, const uint8_t* mask, void* stream)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_broadcast_state: null handle");
    if (!h->have_state) return fail(BCP_E_STATE, "bcp_broadcast_state: state not bound");
    if (src < 0 || src >= h->n) return fail(BCP_E_INVALID, "bcp_broadcast_state: source env %lld of %lld", (long long)src,
                                            (long long)h->n);
    HIP_TRY(hipSetDevice(h->device));
    const bcp_params& p = h->params;
    hipLaunchKernelGGL(broadcast_state_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->st,
                       h->n_geoms > 0 ? h->geom_of_env : nullptr, mask, h->n, src, (int)(p.model == BCP_MODEL_TRICYCLE),
                       p.control_delay, p.pose_delay, p.state_delay);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_robot_step(bcp_handle* h, double* state7_io, int64_t n, const double* actions, const double* noise_z,
                              int32_t* err, void* stream)
{
    if (!h || !state7_io || !actions || n <= 0) return fail(BCP_E_INVALID, "bcp_robot_step: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    const int blocks = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(robot_step_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, h->dev, state7_io, n,
                       actions, noise_z, err);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

static int pose_collides_launch(bcp_handle* h, const double* poses, int64_t n, uint8_t* out, void* stream, int origin_in_map,
                                const char* who)
{
    if (!h || !poses || !out || n <= 0) return fail(BCP_E_INVALID, "%s: bad argument", who);
    if (!h->have_map) return fail(BCP_E_STATE, "%s: costmaps not set", who);
    HIP_TRY(hipSetDevice(h->device));
    BCP_TRY(h->field.ensure_fields(h, (hipStream_t)stream));
    const int blocks = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pose_collides_kernel, dim3(blocks), dim3(kBlock),
                       collision_lds_bytes(h->params.n_verts, h->map.in_lds, h->map.rows, h->map.wpr),
                       (hipStream_t)stream, h->dev, h->map, h->cull, h->tune.exact_mode, h->tune.dense_threshold, h->wide, poses, n,
                       h->n, h->geom_of_env, out, origin_in_map, h->map_valid_rows, h->map_valid_cols);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_pose_collides(bcp_handle* h, const double* poses, int64_t n, uint8_t* out, void* stream)
{
    return pose_collides_launch(h, poses, n, out, stream, 0, "bcp_pose_collides");
}

extern "C" int bcp_is_robot_colliding(bcp_handle* h, const double* poses, int64_t n, uint8_t* out, void* stream)
{
    return pose_collides_launch(h, poses, n, out, stream, 1, "bcp_is_robot_colliding");
}

extern "C" int bcp_pixel_footprint(bcp_handle* h, const double* angles, int64_t n, double resolution, uint8_t* masks,
                                   int32_t side, int32_t* shape_hw, void* stream)
{
    if (!h || !angles || !masks || !shape_hw || n <= 0 || side <= 0)
        return fail(BCP_E_INVALID, "bcp_pixel_footprint: bad argument");
    if (!(resolution > 0) || !check_kernel_size(h->params, resolution))
        return fail(BCP_E_INVALID, "bcp_pixel_footprint: footprint radius / resolution exceeds %d px", BCP_MAX_KERNEL_HALF);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    DevParams P = h->dev;
    scale_footprint(P, h->params, resolution);
    HIP_TRY(hipMemsetAsync(masks, 0, (size_t)n * side * side, s));
    if (h->tune.exact_mode == 2) {  // per-thread rasteriser
        const int blocks = (int)((n + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(pixel_footprint_thread_kernel, dim3(blocks), dim3(kBlock),
                           (size_t)h->params.n_verts * 2 * kBlock * sizeof(uint32_t), s, P, angles, n, masks, side, shape_hw);
    } else {                   // cooperative rasteriser: one wave per angle
        hipLaunchKernelGGL(pixel_footprint_kernel, dim3((unsigned)n), dim3(kBlock),
                           (size_t)h->params.n_verts * 2 * sizeof(double), s, P, angles, n, masks, side, shape_hw);
    }
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_pack_mask_bits(const uint8_t* mask, int64_t n, uint32_t* bits, void* stream)
{
    if (!mask || !bits || n <= 0) return fail(BCP_E_INVALID, "bcp_pack_mask_bits: bad argument");
    hipLaunchKernelGGL(pack_mask_bits_kernel, dim3(stride_grid((n + 31) / 32, 256)), dim3(256), 0, (hipStream_t)stream, mask, n, bits);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_unpack_mask_bits(const uint32_t* bits, int64_t n, uint8_t* mask, void* stream)
{
    if (!mask || !bits || n <= 0) return fail(BCP_E_INVALID, "bcp_unpack_mask_bits: bad argument");
    hipLaunchKernelGGL(unpack_mask_bits_kernel, dim3(stride_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, bits, n, mask);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_normalize_angle(bcp_handle* h, const double* in, double* out, int64_t n, void* stream)
{
    if (!h || !in || !out || n <= 0) return fail(BCP_E_INVALID, "bcp_normalize_angle: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(normalize_angle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in,
                       out, n);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_world_to_pixel(bcp_handle* h, const double* xy, int64_t n, const double* origin, double resolution,
                                  int64_t* out, void* stream)
{
    if (!h || !xy || !origin || !out || n <= 0 || !(resolution > 0))
        return fail(BCP_E_INVALID, "bcp_world_to_pixel: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(world_to_pixel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xy, n,
                       origin[0], origin[1], 1.0 / resolution, out);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}


// ---- reward-provider / path-tools operator seams ---------------------------------------------------------------
static int ready_static(bcp_handle* h, hipStream_t s, const char* who)
{
    if (!h->have_path) return fail(BCP_E_STATE, "%s: paths must be set first", who);
    if (h->static_dirty) return upload_step_static(h, s);
    return BCP_OK;
}

extern "C" int bcp_reward(bcp_handle* h, const double* poses, int64_t n, double* min_spat_dist_so_far, int32_t* target_idx,
                          const uint8_t* robot_collided, double* reward, uint8_t* goal_reached, void* stream)
{
    if (!h || !poses || !min_spat_dist_so_far || !target_idx || !reward || n <= 0)
        return fail(BCP_E_INVALID, "bcp_reward: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    BCP_TRY(ready_static(h, s, "bcp_reward"));
    hipLaunchKernelGGL(reward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->dev_static.get(), poses, n,
                       min_spat_dist_so_far, target_idx, robot_collided, reward, goal_reached);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_find_last_reached(bcp_handle* h, const double* poses, int64_t n, int32_t* out, void* stream)
{
    if (!h || !poses || !out || n <= 0) return fail(BCP_E_INVALID, "bcp_find_last_reached: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    BCP_TRY(ready_static(h, s, "bcp_find_last_reached"));
    hipLaunchKernelGGL(find_last_reached_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->dev_static.get(), poses, n,
                       out);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_path_velocity(bcp_handle* h, const double* path_txyth, int64_t n_rows, double* v, double* w, int32_t* err,
                                 void* stream)
{
    if (!h || !path_txyth || !v || !w || n_rows < 2) return fail(BCP_E_INVALID, "bcp_path_velocity: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(path_velocity_kernel, dim3((unsigned)((n_rows - 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       path_txyth, n_rows, v, w, err);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

extern "C" int bcp_is_footprint_colliding(bcp_handle* h, const uint8_t* image_slices, const uint8_t* blit_masks, int64_t n,
                                          int32_t rows, int32_t cols, uint8_t lethal, uint8_t* out, void* stream)
{
    if (!h || !image_slices || !blit_masks || !out || n <= 0 || rows <= 0 || cols <= 0)
        return fail(BCP_E_INVALID, "bcp_is_footprint_colliding: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(footprint_colliding_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       image_slices, blit_masks, n, (int64_t)rows * cols, (uint32_t)lethal, out);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}


extern "C" int bcp_device_normals(bcp_handle* h, int64_t first_env, int64_t n_envs, uint64_t first_step, int32_t n_steps,
                                  double* out, void* stream)
{
    if (!h || !out || n_envs <= 0 || n_steps <= 0 || first_env < 0) return fail(BCP_E_INVALID, "bcp_device_normals: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(device_normals_kernel, dim3(stride_grid(n_envs * n_steps, 256)), dim3(256), 0, (hipStream_t)stream,
                       h->seed, h->env_id_base + first_env, n_envs, first_step, n_steps, out);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

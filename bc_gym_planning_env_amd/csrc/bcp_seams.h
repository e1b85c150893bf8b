// bcp_seams.h -- the small kernels behind the operator seams: reset and broadcast of the state, and the reference's
// operators one call at a time (robot step, pose collision, pixel footprint, angle and pixel arithmetic, reward, path tools,
// the noise stream, done masks as bits).  They call the device functions the step kernels use.  Entry points:
// bcp_seams_host.h.  Included by bcplan.hip after bcp_step_host.h.
#pragma once

__global__ void reset_kernel(DevState st, DevState init, const uint8_t* __restrict__ mask, int64_t n, int tri,
                             int32_t* __restrict__ geom_of_env, const int32_t* __restrict__ next_geom, double* __restrict__ ret)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    if (ret) ret[i] = 0.0;   // (episode record: a new episode's return)
    int64_t k = i;
    if (geom_of_env) {  // geometry pool: a reset draws the env's next geometry (mini_env.py:469-481)
        k = geom_of_env[i];
        if (next_geom) k = next_geom[k];
        geom_of_env[i] = (int32_t)k;
    }
    st.x[i] = init.x[k];
    st.y[i] = init.y[k];
    st.angle[i] = init.angle[k];
    st.v[i] = init.v[k];
    st.w[i] = init.w[k];
    if (tri) {
        st.steer[i] = init.steer[k];
        st.wheel[i] = init.wheel[k];
    }
    st.min_dist[i] = init.min_dist[k];
    st.target_idx[i] = init.target_idx[k];
    st.cur_iter[i] = init.cur_iter[k];
    st.collided[i] = init.collided[k];
    // delays > 0: the restored State exposes the initial pose / robot state; the queues are empty (pushes restart)
    if (st.pose_seen) {
        st.pose_seen[0 * n + i] = init.x[k];
        st.pose_seen[1 * n + i] = init.y[k];
        st.pose_seen[2 * n + i] = init.angle[k];
    }
    if (st.state_seen) {
        st.state_seen[0 * n + i] = init.x[k];
        st.state_seen[1 * n + i] = init.y[k];
        st.state_seen[2 * n + i] = init.angle[k];
        st.state_seen[3 * n + i] = init.v[k];
        st.state_seen[4 * n + i] = init.w[k];
        st.state_seen[5 * n + i] = tri ? init.steer[k] : 0.0;
        st.state_seen[6 * n + i] = tri ? init.wheel[k] : 0.0;
    }
}

// Monte-Carlo fan-out: env `src`'s complete state copied into every selected env
__global__ void broadcast_state_kernel(DevState st, int32_t* __restrict__ geom_of_env, const uint8_t* __restrict__ mask,
                                       int64_t n, int64_t src, int tri, int control_delay, int pose_delay, int state_delay)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || i == src) return;
    if (mask && !mask[i]) return;
    st.x[i] = st.x[src];
    st.y[i] = st.y[src];
    st.angle[i] = st.angle[src];
    st.v[i] = st.v[src];
    st.w[i] = st.w[src];
    if (tri) {
        st.steer[i] = st.steer[src];
        st.wheel[i] = st.wheel[src];
    }
    st.min_dist[i] = st.min_dist[src];
    st.target_idx[i] = st.target_idx[src];
    st.cur_iter[i] = st.cur_iter[src];
    st.collided[i] = st.collided[src];
    if (geom_of_env) geom_of_env[i] = geom_of_env[src];
    if (st.pose_seen)
        for (int c = 0; c < 3; ++c) st.pose_seen[c * n + i] = st.pose_seen[c * n + src];
    if (st.state_seen)
        for (int c = 0; c < 7; ++c) st.state_seen[c * n + i] = st.state_seen[c * n + src];
    if (st.control_q)
        for (int c = 0; c < 2 * control_delay; ++c) st.control_q[c * n + i] = st.control_q[c * n + src];
    if (st.pose_q)
        for (int c = 0; c < 3 * pose_delay; ++c) st.pose_q[c * n + i] = st.pose_q[c * n + src];
    if (st.state_q)
        for (int c = 0; c < 7 * state_delay; ++c) st.state_q[c * n + i] = st.state_q[c * n + src];
}

__global__ void __launch_bounds__(kBlock) robot_step_kernel(DevParams P, double* __restrict__ st7, int64_t n,
                                                            const double* __restrict__ actions,
                                                            const double* __restrict__ noise_z, int32_t* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Robot r;
    r.p.x = st7[0 * n + i];
    r.p.y = st7[1 * n + i];
    r.p.th = st7[2 * n + i];
    r.v = st7[3 * n + i];
    r.w = st7[4 * n + i];
    r.steer = st7[5 * n + i];
    r.wheel = st7[6 * n + i];
    double z[3] = {0.0, 0.0, 0.0};
    if (noise_z) {
        z[0] = noise_z[3 * i];
        z[1] = noise_z[3 * i + 1];
        z[2] = noise_z[3 * i + 2];
    }
    int drawn = 0;
    const int e = robot_step(P, r, actions[2 * i], actions[2 * i + 1], z, drawn);
    st7[0 * n + i] = r.p.x;
    st7[1 * n + i] = r.p.y;
    st7[2 * n + i] = r.p.th;
    st7[3 * n + i] = r.v;
    st7[4 * n + i] = r.w;
    st7[5 * n + i] = r.steer;
    st7[6 * n + i] = r.wheel;
    if (err) err[i] = e;
}

__global__ void __launch_bounds__(kBlock) pose_collides_kernel(DevParams P, MapDesc map, CullDesc cull, int exact_mode,
                                                               int dense_threshold, int wide,
                                                               const double* __restrict__ poses, int64_t n, int64_t n_envs,
                                                               const int32_t* __restrict__ geom_of_env,
                                                               uint8_t* __restrict__ out, int origin_in_map,
                                                               const int32_t* __restrict__ valid_rows,
                                                               const int32_t* __restrict__ valid_cols)
{
    const int tid = threadIdx.x;
    const int64_t gi = (int64_t)blockIdx.x * kBlock + tid;
    const bool active = gi < n;
    const int64_t i = active ? gi : n - 1;
    const CollisionLds L = collision_lds_setup(P, map, tid);
    const int64_t env = geom_of_env ? (int64_t)geom_of_env[i % n_envs] : i % n_envs;
    bool hit = collides_wave(P, map, cull, L, exact_mode, dense_threshold, wide != 0, active, env, poses[3 * i],
                             poses[3 * i + 1], poses[3 * i + 2]);
    if (origin_in_map) {   // is_robot_colliding: a robot whose own pixel is off the map never collides (costmap_utils.py:127-130)
        const double ox = map.origins ? map.origins[2 * env] : map.ox, oy = map.origins ? map.origins[2 * env + 1] : map.oy;
        const int64_t px = (int64_t)rint((poses[3 * i] - ox) * map.inv_res), py = (int64_t)rint((poses[3 * i + 1] - oy) * map.inv_res);
        const int rows = (!map.shared && valid_rows) ? valid_rows[env] : map.rows;
        const int cols = (!map.shared && valid_cols) ? valid_cols[env] : map.cols;
        if (px < 0 || py < 0 || px >= cols || py >= rows) hit = false;
    }
    if (active) out[i] = (uint8_t)hit;
}

// get_pixel_footprint: one wave per angle, rasterised by the cooperative path; lane = image row
struct MaskRowSink {
    uint8_t* img;
    int side, hx, hy;
    __device__ __forceinline__ void extent(int, int) {}
    __device__ __forceinline__ bool chunk_matters(int, bool) const { return true; }
    __device__ __forceinline__ bool rows(int y, bool valid, const uint32_t cover[8], int ubase) const
    {
        const int ky = y + hy;
        if (valid && (unsigned)ky < (unsigned)side) {
            for (int b = 0; b < 256; ++b) {
                const int kx = ubase + b + hx;
                if ((cover[b >> 5] >> (b & 31)) & 1u)
                    if ((unsigned)kx < (unsigned)side) img[ky * side + kx] = 255;
            }
        }
        return false;
    }
};

__global__ void __launch_bounds__(kBlock) pixel_footprint_kernel(DevParams P, const double* __restrict__ angles, int64_t n,
                                                                 uint8_t* __restrict__ masks, int side,
                                                                 int32_t* __restrict__ shape_hw)
{
    const int tid = threadIdx.x;
    __attribute__((address_space(3))) double* q = (__attribute__((address_space(3))) double*)lds_dyn;
    for (int k = tid; k < 2 * P.n_verts; k += kBlock) q[k] = P.qverts[k >> 1][k & 1];
    __syncthreads();
    const int64_t i = blockIdx.x;
    const double c = cos(angles[i]), s = sin(angles[i]);
    MaskRowSink sink;
    sink.img = masks + i * (int64_t)side * side;
    sink.side = side;
    footprint_half_sizes(P, c, s, sink.hx, sink.hy);
    if (tid == 0) {
        shape_hw[2 * i] = 2 * sink.hy + 1;
        shape_hw[2 * i + 1] = 2 * sink.hx + 1;
    }
    coop_raster<8, 1>(P, tid < P.n_verts ? q[2 * tid] : 0.0, tid < P.n_verts ? q[2 * tid + 1] : 0.0, c, s, sink);
}

// same image through the per-thread rasteriser (one thread per angle): cross-checks the two exact paths
struct MaskSink {
    uint8_t* img;
    int side, hx, hy;
    __device__ __forceinline__ bool span(int v, int ua, int ub) const
    {
        const int y = v + hy;
        if ((unsigned)y < (unsigned)side)
            for (int x = max(ua + hx, 0); x <= min(ub + hx, side - 1); ++x) img[y * side + x] = 255;
        return false;
    }
    __device__ __forceinline__ bool pixel(int v, int u) const { return span(v, u, u); }
};

__global__ void __launch_bounds__(kBlock) pixel_footprint_thread_kernel(DevParams P, const double* __restrict__ angles,
                                                                        int64_t n, uint8_t* __restrict__ masks, int side,
                                                                        int32_t* __restrict__ shape_hw)
{
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
    VertLds E;
    E.base = (LdsU32)lds_dyn + tid;
    E.stride = kBlock;
    if (i >= n) return;
    MaskSink sink;
    sink.img = masks + i * (int64_t)side * side;
    sink.side = side;
    const double c = cos(angles[i]), s = sin(angles[i]);
    footprint_half_sizes(P, c, s, sink.hx, sink.hy);
    shape_hw[2 * i] = 2 * sink.hy + 1;
    shape_hw[2 * i + 1] = 2 * sink.hx + 1;
    raster_runs(P, c, s, E, sink);
}

__global__ void normalize_angle_kernel(const double* __restrict__ in, double* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = normalize_angle(in[i]);
}

__global__ void world_to_pixel_kernel(const double* __restrict__ xy, int64_t n, double ox, double oy, double inv_res,
                                      int64_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[2 * i] = (int64_t)rint((xy[2 * i] - ox) * inv_res);
    out[2 * i + 1] = (int64_t)rint((xy[2 * i + 1] - oy) * inv_res);
}


// ---- reward-provider / path-tools operator seams (envs/base/reward.py:184-259, utilities/path_tools.py:298-448) ----
// reward_provider.reward(state) + .done(state) for n (pose, provider state) pairs; pose i is scored against the path of
// env i % n_envs (its current pool entry in geometry-pool mode) with the very device functions the step kernels use.
__global__ void reward_kernel(const StepStatic* __restrict__ S, const double* __restrict__ poses, int64_t n,
                              double* __restrict__ min_dist_io, int32_t* __restrict__ target_io,
                              const uint8_t* __restrict__ collided, double* __restrict__ reward, uint8_t* __restrict__ goal)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DevParams& P = S->P;
    const int64_t e = i % S->n;
    const int64_t g = S->path.shared ? 0 : (S->geom_of_env ? (int64_t)S->geom_of_env[e] : e);
    const double* pts = S->path.pts + g * (int64_t)S->path.max_len * 5;
    const int m = S->path.shared ? S->path.max_len : S->path.lens[g];
    const double x = poses[3 * i], y = poses[3 * i + 1], th = poses[3 * i + 2];
    double min_dist = min_dist_io[i];
    int target = target_io[i];
    double rew;
    bool reached;
    if (P.reward_provider == BCP_REWARD_PURE_PURSUIT) {
        rew = reward_pure_pursuit(pts, m, x, y, collided && collided[i], min_dist, target);
        reached = hypot(pts[5 * (m - 1)] - x, pts[5 * (m - 1) + 1] - y) < 1.0;   // reward.py:141-150
    } else {
        const PathWindow w = path_window_of(P, S->path.shared != 0, S->path.bbox, S->path.index, g, x, y);
        rew = reward_step(P, pts, w, m, x, y, th, min_dist, target);
        reached = target > m - 1;                                                 // reward.py:66-69
    }
    min_dist_io[i] = min_dist;
    target_io[i] = target;
    reward[i] = rew;
    if (goal) goal[i] = (uint8_t)reached;
}

// find_last_reached(pose, path, spatial_precision, angular_precision) (path_tools.py:432-448): index of the LAST way
// point of the whole path the pose has reached, -1 for None
__global__ void find_last_reached_kernel(const StepStatic* __restrict__ S, const double* __restrict__ poses, int64_t n,
                                         int32_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t e = i % S->n;
    const int64_t g = S->path.shared ? 0 : (S->geom_of_env ? (int64_t)S->geom_of_env[e] : e);
    const double* pts = S->path.pts + g * (int64_t)S->path.max_len * 5;
    const int m = S->path.shared ? S->path.max_len : S->path.lens[g];
    const double x = poses[3 * i], y = poses[3 * i + 1], th = poses[3 * i + 2];
    const PathWindow w = path_window_of(S->P, S->path.shared != 0, S->path.bbox, S->path.index, g, x, y);
    out[i] = last_reached_from(S->P, pts, w, m, 0, x, y, th);
}

// path_velocity(path) (path_tools.py:298-323) for an n-row (t, x, y, angle) path: row j of the output belongs to the
// segment j -> j + 1.  err: BCP_ERR_ANGLE_JUMP where the reference raises, BCP_ERR_TIME_ORDER where its assert fires.
__global__ void path_velocity_kernel(const double* __restrict__ path, int64_t n, double* __restrict__ v,
                                     double* __restrict__ w, int32_t* __restrict__ err)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n - 1) return;
    const double* a = path + 4 * j;
    const double* b = a + 4;
    const double dt = b[0] - a[0];
    Pose p0 = {a[1], a[2], a[3]}, p1 = {b[1], b[2], b[3]};
    double vv, ww;
    int e = path_velocity(p0, p1, dt, vv, ww);
    if (!(dt > 0)) e |= BCP_ERR_TIME_ORDER;
    v[j] = vv;
    w[j] = ww;
    if (err) err[j] = e;
}

// is_footprint_colliding_impl(image_slice, blit_mask, lethal) (costmap_utils.py:106-136): any(image_slice[blit_mask] ==
// lethal) for n (slice, mask) pairs of one shape; one wavefront per pair, 4 cells per lane and load, wave-wide OR.
__global__ void __launch_bounds__(256) footprint_colliding_kernel(const uint8_t* __restrict__ slices,
                                                                  const uint8_t* __restrict__ masks, int64_t n,
                                                                  int64_t cells, uint32_t lethal, uint8_t* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint8_t* s = slices + i * cells;
    const uint8_t* k = masks + i * cells;
    // the pair's first byte is only byte aligned: peel up to the first 4-byte boundary of BOTH arrays when they agree,
    // otherwise go byte by byte (n * cells is rarely worth more)
    bool hit = false;
    const bool words = (((uintptr_t)s | (uintptr_t)k) & 3) == 0;
    const int64_t n4 = words ? cells / 4 : 0;
    const uint32_t l4 = lethal * 0x01010101u;
    for (int64_t q = lane; q < n4 && !hit; q += 64) {
        const uint32_t sv = reinterpret_cast<const uint32_t*>(s)[q], kv = reinterpret_cast<const uint32_t*>(k)[q];
        const uint32_t x = sv ^ l4;   // a zero byte <=> the cell is lethal
#pragma unroll
        for (int b = 0; b < 4; ++b) hit |= ((x >> (8 * b)) & 0xFFu) == 0 && ((kv >> (8 * b)) & 0xFFu) != 0;
    }
    for (int64_t q = 4 * n4 + lane; q < cells && !hit; q += 64) hit |= s[q] == lethal && k[q] != 0;
    hit = __any(hit);
    if (lane == 0) out[i] = (uint8_t)hit;
}


// the standard normals the step kernels draw for (seed, global env index, step counter): introspection of the noise stream
__global__ void device_normals_kernel(uint64_t seed, int64_t env_id_base, int64_t n, uint64_t step0, int32_t n_steps,
                                      double* __restrict__ out)
{
    const int64_t total = n * n_steps;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = it / n, i = it % n;
        double z[3];
        device_normals(seed, (uint64_t)(env_id_base + i), step0 + (uint64_t)k, z);
        out[3 * it + 0] = z[0];
        out[3 * it + 1] = z[1];
        out[3 * it + 2] = z[2];
    }
}

// done masks as bits: word w, bit b = mask[32 w + b] != 0 (a sharded job sends its masks over xGMI in this form)
__global__ void pack_mask_bits_kernel(const uint8_t* __restrict__ mask, int64_t n, uint32_t* __restrict__ bits)
{
    const int64_t words = (n + 31) / 32;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
        uint32_t word = 0;
        if (32 * w + 32 <= n && ((uintptr_t)(mask + 32 * w) & 15) == 0) {
            const uint4* src = reinterpret_cast<const uint4*>(mask + 32 * w);
            const uint4 lo = src[0], hi = src[1];
            const uint32_t q[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) word |= (uint32_t)(((q[k] >> (8 * j)) & 255u) != 0) << (4 * k + j);
        } else {
            for (int b = 0; b < 32 && 32 * w + b < n; ++b) word |= (uint32_t)(mask[32 * w + b] != 0) << b;
        }
        bits[w] = word;
    }
}

__global__ void unpack_mask_bits_kernel(const uint32_t* __restrict__ bits, int64_t n, uint8_t* __restrict__ mask)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        mask[i] = (uint8_t)((bits[i >> 5] >> (i & 31)) & 1u);
}

// bcplan.hip -- libbcplan.so: batched PlanEnv.step() for MI355X (gfx950).  C ABI in include/bcplan.h.
//
// One translation unit.  The device code is in bcp_device.h, bcp_raster.h, bcp_coop.h and bcp_step.h (the step: robot model ->
// collision classification / exact rasteriser -> rollback -> reward provider -> done -> optional reset -> state write-back),
// bcp_lookahead.h and bcp_mppi.h (the planners), bcp_ego.h (egocentric views), bcp_sample.h and bcp_aisle.h (world samplers),
// bcp_inflate.h (costmap inflation), bcp_scan.h (range scans; the walk: bcp_scan_march.h, no HIP in it).  The host side is
// split by subsystem:
//   bcp_host.h         errors, the handle (its device buffers are DevBuf, bcp_devbuf.h), EgoCells, the launch helpers
//   bcp_field.h        distance field and tiles: kernels, and the launchers of everything derived from maps and paths
//   bcp_step_host.h    step forms, the step's parameter block and launcher, bcp_step / bcp_rollout / bcp_lookahead / bcp_mppi
//   bcp_ego_host.h     egocentric costmaps (routed by bcp_ego_route.h, which has no HIP in it), goal-state vectors, the
//                      episode record and its final observations
//   bcp_worlds_host.h  mini-world and aisle-world entry points
//   bcp_inflate_host.h bcp_inflate_costmaps (kernel: bcp_inflate.h)
//   bcp_scan_host.h    bcp_range_scan / bcp_final_range_scan (kernel: bcp_scan.h)
// This file holds the footprint geometry, create / destroy / seed / pool / tuning, bcp_set_costmaps, bcp_set_paths, bind /
// reset / broadcast, and the operator seams with their small kernels.
// Compiled with -ffp-contract=off (numpy rounds every product and sum separately).  No CPU path exists here.
#include <hip/hip_runtime.h>
#include <mutex>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <utility>
#include <vector>

#include "bcp_device.h"
#include "bcp_raster.h"
#include "bcp_coop.h"
#include "bcp_step.h"
#include "bcp_lookahead.h"
#include "bcp_mppi.h"
#include "bcp_ego.h"
#include "bcp_sample.h"
#include "bcp_aisle.h"
#include "bcp_inflate.h"
#include "bcp_scan.h"

using namespace bcp;

#include "bcp_host.h"

extern "C" const char* bcp_last_error(void) { return g_err; }
extern "C" int bcp_abi_version(void) { return BCP_ABI_VERSION; }

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

// ------------------------------------------------------------------------------------------------ footprint geometry
// ---- sample points of the distance-field classification (see bcp_coop.h) -----------------------------------
static double seg_dist(double px, double py, double ax, double ay, double bx, double by)
{
    const double vx = bx - ax, vy = by - ay, wx = px - ax, wy = py - ay;
    const double vv = vx * vx + vy * vy;
    double t = vv > 0 ? (wx * vx + wy * vy) / vv : 0.0;
    t = t < 0 ? 0 : (t > 1 ? 1 : t);
    const double cx = ax + t * vx, cy = ay + t * vy;
    return std::sqrt((px - cx) * (px - cx) + (py - cy) * (py - cy));
}

static bool point_in_polygon(double px, double py, const double (*v)[2], int k)
{
    bool in = false;
    for (int i = 0, j = k - 1; i < k; j = i++) {
        if (((v[i][1] > py) != (v[j][1] > py)) &&
            (px < (v[j][0] - v[i][0]) * (py - v[i][1]) / (v[j][1] - v[i][1]) + v[i][0]))
            in = !in;
    }
    return in;
}

// Worst-case slack, in pixels, between the real rotated footprint and the pixel set cv2.fillPoly produces from it:
// vertex rounding moves the contour by <= sqrt(.5), Bresenham strays <= .5 from the rounded contour, 16.16 slopes
// add < .01; a sample centre is itself rounded to a pixel (<= sqrt(.5)).
static const double kSlackOuter = 0.7072 + 0.5 + 0.01 + 0.7072;
static const double kSlackInner = 0.7072 + 0.7072 + 0.05;

static void build_cull_geometry(const bcp_params& p, double res, CullDesc* C)
{
    const int K = p.n_verts;
    double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300, rmax = 0;
    for (int k = 0; k < K; ++k) {
        xmin = std::min(xmin, p.verts[k][0]);
        xmax = std::max(xmax, p.verts[k][0]);
        ymin = std::min(ymin, p.verts[k][1]);
        ymax = std::max(ymax, p.verts[k][1]);
        rmax = std::max(rmax, std::sqrt(p.verts[k][0] * p.verts[k][0] + p.verts[k][1] * p.verts[k][1]));
    }
    C->reach = (int)std::ceil(rmax / res) + 2;
    C->pad = 2 * C->reach + 4;
    const double ay = 0.5 * (ymin + ymax), half_w = 0.5 * (ymax - ymin);
    // axis segment: pulled in from the ends by a quarter of the half width, so that the round caps of the capsule
    // still cover the corners of a box-like footprint without inflating the radius (corner distance hypot(w/4, w))
    double a0 = xmin + 0.25 * half_w, a1 = xmax - 0.25 * half_w;
    if (a0 > a1) a0 = a1 = 0.5 * (xmin + xmax);
    // OUTER: capsule around the axis segment [a0,a1] x {ay} that contains every vertex (hence the polygon), covered
    // by n_out discs: a disc row of spacing h covers the capsule of radius rho when its radius is sqrt(rho^2+(h/2)^2)
    double rho = 0;
    for (int k = 0; k < K; ++k) rho = std::max(rho, seg_dist(p.verts[k][0], p.verts[k][1], a0, ay, a1, ay));
    // (compared as doubles: a footprint that lies ON its axis has rho == 0, and an infinite quotient must not reach an int)
    const double want_out = a1 > a0 ? std::ceil((a1 - a0) / (0.5 * rho)) + 1 : 1;
    const int n_out = a1 > a0 ? (want_out >= kMaxSamples ? kMaxSamples : std::max(2, (int)want_out)) : 1;
    const double h = n_out > 1 ? (a1 - a0) / (n_out - 1) : 0.0;
    const double r_out = std::sqrt(rho * rho + 0.25 * h * h) / res + kSlackOuter;
    C->n_out = n_out;
    for (int i = 0; i < n_out; ++i) C->out_x[i] = (a0 + i * h) / res;
    C->t_out = (int)std::floor(r_out) + 1;  // floor(d) >= t_out  =>  d > r_out
    // INNER: discs centred on the same axis that lie inside the polygon
    C->n_in = 0;
    for (int j = 0; j < kMaxSamples; ++j) {
        const double bx = kMaxSamples > 1 ? a0 + (a1 - a0) * j / (kMaxSamples - 1) : a0;
        if (!point_in_polygon(bx, ay, p.verts, K)) continue;
        double rin = 1e300;
        for (int k = 0; k < K; ++k) {
            const int kn = (k + 1) % K;
            rin = std::min(rin, seg_dist(bx, ay, p.verts[k][0], p.verts[k][1], p.verts[kn][0], p.verts[kn][1]));
        }
        const double r = rin / res - kSlackInner;   // lethal cell within r of the sample pixel => inside the mask
        const int t = (int)std::floor(r) - 1;       // floor(d) <= t  =>  d < t + 1 <= r
        if (t < 0) continue;
        C->in_x[C->n_in] = bx / res;
        C->t_in[C->n_in] = t;
        ++C->n_in;
        if (a1 <= a0) break;
    }
    C->axis_y = ay / res;
}

static int footprint_is_wide(const bcp_params& p, double res)
{
    double d2 = 0;
    for (int i = 0; i < p.n_verts; ++i)
        for (int j = 0; j < i; ++j) {
            const double dx = p.verts[i][0] - p.verts[j][0], dy = p.verts[i][1] - p.verts[j][1];
            d2 = std::max(d2, dx * dx + dy * dy);
        }
    return std::sqrt(d2) / res + 3.0 > 96.0;  // row masks of the cooperative path: 3 words unless wider
}

// robot_footprint / map_resolution (path_tools.py:145), divided on the host in fp64, and its bounding box
static void scale_footprint(DevParams& d, const bcp_params& p, double res)
{
    d.qbox[0] = d.qbox[2] = 1e30f;
    d.qbox[1] = d.qbox[3] = -1e30f;
    for (int k = 0; k < p.n_verts; ++k) {
        d.qverts[k][0] = p.verts[k][0] / res;
        d.qverts[k][1] = p.verts[k][1] / res;
        d.qbox[0] = std::min(d.qbox[0], (float)d.qverts[k][0]);
        d.qbox[1] = std::max(d.qbox[1], (float)d.qverts[k][0]);
        d.qbox[2] = std::min(d.qbox[2], (float)d.qverts[k][1]);
        d.qbox[3] = std::max(d.qbox[3], (float)d.qverts[k][1]);
    }
}

static void fill_dev_params(bcp_handle* h)
{
    const bcp_params& p = h->params;
    DevParams& d = h->dev;
    memset(&d, 0, sizeof(d));
    d.model = p.model;
    d.n_verts = p.n_verts;
    d.dynamic_model = p.dynamic_model;
    d.model_front_column_pid = p.model_front_column_pid;
    d.noise_on = p.noise_on;
    d.iteration_timeout = p.iteration_timeout;
    d.dt = p.dt;
    d.L = p.front_wheel_from_axis;
    d.max_wheel_angle = p.max_front_wheel_angle;
    d.max_wheel_speed = p.max_front_wheel_speed;
    d.max_lin_acc = p.max_linear_acceleration;
    d.max_ang_acc = p.max_angular_acceleration;
    d.p_gain = p.front_column_p_gain;
    d.inv_dt = 1.0 / p.dt;                       // (correctly rounded: what div_by_const needs)
    d.inv_L = 1.0 / p.front_wheel_from_axis;
    for (int k = 0; k < 6; ++k) d.alpha[k] = p.alpha[k];
    d.sp = p.spatial_precision;
    d.ap = p.angular_precision;
    d.progress_mult = p.spatial_progress_multiplier;
    d.par_thr = -p.spatial_precision / 9;
    d.ap_cos_min = p.angular_precision >= 3.14159265358979 ? -2.0f : (float)(std::cos(p.angular_precision) - 1e-4);
    d.sp_prune = std::nextafter(std::nextafter(p.spatial_precision, INFINITY), INFINITY);
    d.sp2_lo = p.spatial_precision * p.spatial_precision * (1.0 - 1e-13);
    d.sp2_hi = p.spatial_precision * p.spatial_precision * (1.0 + 1e-13);
    d.reward_provider = p.reward_provider;
    d.control_delay = p.control_delay;
    d.pose_delay = p.pose_delay;
    d.state_delay = p.state_delay;
    const double res = h->resolution > 0 ? h->resolution : 1.0;
    scale_footprint(d, p, res);
}

static int check_kernel_size(const bcp_params& p, double res)
{
    double r2 = 0;
    for (int k = 0; k < p.n_verts; ++k) {
        double d2 = p.verts[k][0] * p.verts[k][0] + p.verts[k][1] * p.verts[k][1];
        if (d2 > r2) r2 = d2;
    }
    return std::sqrt(r2) / res + 2.0 <= BCP_MAX_KERNEL_HALF;
}

// ------------------------------------------------------------------------------------------------ the subsystems
// (each needs the ones before it, and the helpers above)
#include "bcp_field.h"
#include "bcp_step_host.h"
#include "bcp_ego_host.h"
#include "bcp_worlds_host.h"
#include "bcp_inflate_host.h"
#include "bcp_scan_host.h"

// ------------------------------------------------------------------------------------------------ kernels (one-time, operator seams)
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

// ------------------------------------------------------------------------------------------------ host API
extern "C" int bcp_create(const bcp_params* params, int64_t n_envs, int device, int64_t env_id_base, bcp_handle** out)
{
    if (!params || !out) return fail(BCP_E_INVALID, "bcp_create: null argument");
    if (params->abi_version != BCP_ABI_VERSION)
        return fail(BCP_E_INVALID, "bcp_create: abi_version %d != %d", params->abi_version, BCP_ABI_VERSION);
    if (n_envs <= 0) return fail(BCP_E_INVALID, "bcp_create: n_envs must be positive");
    if (params->n_verts < 3 || params->n_verts > BCP_MAX_VERTS)
        return fail(BCP_E_INVALID, "bcp_create: n_verts %d outside [3, %d]", params->n_verts, BCP_MAX_VERTS);
    for (int k = 0; k < params->n_verts; ++k)
        if (!std::isfinite(params->verts[k][0]) || !std::isfinite(params->verts[k][1]))
            return fail(BCP_E_INVALID, "bcp_create: footprint vertex %d is not finite", k);
    if (params->model != BCP_MODEL_TRICYCLE && params->model != BCP_MODEL_DIFFDRIVE)
        return fail(BCP_E_INVALID, "bcp_create: unknown robot model %d", params->model);
    if (!(params->dt > 0)) return fail(BCP_E_INVALID, "bcp_create: dt must be > 0 (path_tools.py:307)");
    {   // div_by_const (bcp_device.h) divides by dt and by the wheel base through their reciprocals; the sequence is the IEEE
        // quotient for every divisor but those whose significand is all ones (0.99999999999999989 and its like)
        const auto all_ones = [](double d) {
            uint64_t bits;
            memcpy(&bits, &d, sizeof(bits));
            return (bits & 0x000FFFFFFFFFFFFFull) == 0x000FFFFFFFFFFFFFull;
        };
        if (all_ones(params->dt) || (params->model == BCP_MODEL_TRICYCLE && all_ones(params->front_wheel_from_axis)))
            return fail(BCP_E_INVALID, "bcp_create: dt / front_wheel_from_axis with an all-ones significand is not supported");
    }
    if (params->model == BCP_MODEL_DIFFDRIVE && params->noise_on && !(params->options & BCP_OPT_DIFFDRIVE_NOISE))
        return fail(BCP_E_INVALID, "bcp_create: the reference's DiffDriveRobot raises IndexError with noise_parameters "
                                   "(differential_drive.py:73); set BCP_OPT_DIFFDRIVE_NOISE in bcp_params.options to opt in to "
                                   "the unpinned 1-pose analogue");
    if (params->reward_provider != BCP_REWARD_CONTINUOUS && params->reward_provider != BCP_REWARD_PURE_PURSUIT)
        return fail(BCP_E_INVALID, "bcp_create: unknown reward provider %d", params->reward_provider);
    if (params->control_delay < 0 || params->pose_delay < 0 || params->state_delay < 0)
        return fail(BCP_E_INVALID, "bcp_create: delays must be >= 0");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(BCP_E_NO_DEVICE, "bcp_create: no HIP device available (%s); libbcplan has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(BCP_E_INVALID, "bcp_create: device %d of %d", device, count);
    HIP_TRY(hipSetDevice(device));
    bcp_handle* h = new (std::nothrow) bcp_handle();   // (the defaults are the member initialisers: bcp_host.h)
    if (!h) return fail(BCP_E_INVALID, "bcp_create: out of host memory");
    h->params = *params;
    h->n = n_envs;
    h->device = device;
    h->env_id_base = env_id_base;
    if (const char* e = getenv("BCP_NEAR_SHIFT")) {   // (default of BCP_TUNE_NEAR_SHIFT for every handle of the process)
        const int v = atoi(e);
        if (v >= 0 && v <= 3) h->near_shift = v;
    }
    if (const char* e = getenv("BCP_LOCAL_PAIRS")) {   // (default of BCP_TUNE_LOCAL_PAIRS for every handle of the process)
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4) h->local_pairs = v;
    }
    fill_dev_params(h);
    if (h->tick.reserve(kTickWords) != hipSuccess || hipMemset(h->tick.get(), 0, kTickWords * sizeof(uint64_t)) != hipSuccess) {
        delete h;
        return fail(BCP_E_HIP, "bcp_create: cannot allocate device memory");
    }
    *out = h;
    return BCP_OK;
}

extern "C" int bcp_destroy(bcp_handle* h)
{
    if (!h) return BCP_OK;
    (void)hipSetDevice(h->device);   // (the buffers' destructors free on this device, too)
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->refresh_done) (void)hipEventDestroy(h->refresh_done);
    if (h->waits_event) (void)hipEventDestroy(h->waits_event);
    if (h->waits_host) (void)hipHostFree(h->waits_host);
    delete h;
    return BCP_OK;
}

extern "C" int bcp_seed(bcp_handle* h, uint64_t seed)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_seed: null handle");
    h->seed = seed;
    // The noise stream restarts: step counter 0 again.  The alternating counter sets of the parking scheme are keyed
    // by the counter's parity, so they are re-armed with it (rare call: synchronous).
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const uint64_t tick[4] = {0, 0, seed, 0};
    HIP_TRY(hipMemcpy(h->tick.get(), tick, sizeof(tick), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(h->tick.get() + kTickLocalTicket, 0, sizeof(uint64_t)));
    if (h->pending_count.get()) HIP_TRY(hipMemset(h->pending_count.get(), 0, 2 * kShards * sizeof(int32_t)));
    if (h->adapt.get()) {
        HIP_TRY(hipMemset(h->adapt.get(), 0, (2 + 2 * kShards) * sizeof(int32_t)));
        const int32_t init[2] = {h->dense_threshold, h->dense_threshold};
        HIP_TRY(hipMemcpy(h->adapt.get(), init, sizeof(init), hipMemcpyHostToDevice));
    }
    return BCP_OK;
}

extern "C" int bcp_set_geometry_pool(bcp_handle* h, int32_t n_geoms, int32_t* geom_of_env, const int32_t* next_geom)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_set_geometry_pool: null handle");
    if (n_geoms < 0 || (n_geoms > 0 && !geom_of_env))
        return fail(BCP_E_INVALID, "bcp_set_geometry_pool: n_geoms > 0 needs geom_of_env");
    if ((n_geoms > 0) != (h->n_geoms > 0) || (n_geoms > 0 && n_geoms != h->n_geoms)) {
        // the non-shared arrays change their entry count: they have to be given again
        h->have_map = h->have_path = h->have_init = false;
    }
    h->n_geoms = n_geoms;
    h->geom_of_env = n_geoms > 0 ? geom_of_env : nullptr;
    h->next_geom = n_geoms > 0 ? next_geom : nullptr;
    h->static_dirty = true;
    return BCP_OK;
}

extern "C" int bcp_set_tuning(bcp_handle* h, int32_t key, int32_t value)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_set_tuning: null handle");
    h->static_dirty = true;
    switch (key) {
        case BCP_TUNE_EXACT_MODE:
            if (value < 0 || value > 3) return fail(BCP_E_INVALID, "bcp_set_tuning: exact mode must be 0, 1, 2 or 3");
            h->exact_mode = value;
            return BCP_OK;
        case BCP_TUNE_DENSE_THRESHOLD:
            h->dense_threshold = value;
            h->adaptive = 0;   // an explicit threshold is taken as is
            return BCP_OK;
        case BCP_TUNE_DEFER:
            h->defer = value ? 1 : 0;
            return BCP_OK;
        case BCP_TUNE_EDT_LDS:
            h->edt_in_lds = value ? 1 : 0;
            return BCP_OK;
        case BCP_TUNE_NEAR_DILATE:
            if (value < 0 || value > 2) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_NEAR_DILATE takes 0, 1 or 2");
            h->near_dilate = value;
            return BCP_OK;
        case BCP_TUNE_EGO_SPARSE:
            if (value < 0) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_EGO_SPARSE takes 0, 1 or a limit of cells per map");
            if (value != h->ego_sparse) h->ego_cells.invalidate();   // (the lists are sized for the limit in force)
            h->ego_sparse = value;
            return BCP_OK;
        case BCP_TUNE_EGO_LIST_STRIDE:
            if (value < 0 || (value & 63)) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_EGO_LIST_STRIDE takes 0 or a multiple of 64");
            if (value != h->ego_stride) h->ego_cells.invalidate();
            h->ego_stride = value;
            return BCP_OK;
        case BCP_TUNE_FUSED:
            h->fused = value ? 1 : 0;
            return BCP_OK;
        case BCP_TUNE_NEAR_SHIFT:
            if (value < -1 || value > 3) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_NEAR_SHIFT takes -1 (default), 0, 1, 2 or 3");
            h->near_shift = value;   // (in force from the next bcp_set_costmaps on)
            return BCP_OK;
        case BCP_TUNE_LOCAL_PAIRS:
            if (value != 0 && value != 1 && value != 2 && value != 4)
                return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_LOCAL_PAIRS takes 0 (default), 1, 2 or 4");
            h->local_pairs = value;
            return BCP_OK;
        case BCP_TUNE_INFLATE_ROUTE:
            if (value != 0 && value != 2) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_INFLATE_ROUTE takes 0 or 2");
            h->inflate_route = value;
            return BCP_OK;
        case BCP_TUNE_CULL:
            h->cull_enabled = value ? 1 : 0;
            h->cull.on = (value && h->cull.edt) ? 1 : 0;
            return BCP_OK;
        default:
            return fail(BCP_E_INVALID, "bcp_set_tuning: unknown key %d", key);
    }
}

extern "C" int bcp_side_stream(bcp_handle* h, int32_t cu_percent, void** stream)
{
    if (!h || !stream) return fail(BCP_E_INVALID, "bcp_side_stream: null argument");
    if (cu_percent < 1 || cu_percent > 100) return fail(BCP_E_INVALID, "bcp_side_stream: cu_percent must be 1 .. 100");
    HIP_TRY(hipSetDevice(h->device));
    if (h->side_stream && h->side_share != cu_percent) {
        HIP_TRY(hipStreamSynchronize(h->side_stream));
        HIP_TRY(hipStreamDestroy(h->side_stream));
        h->side_stream = nullptr;
    }
    if (!h->side_stream) {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        // one bit per CU; the enabled ones are spread evenly (every k-th bit, whatever order the driver numbers the CUs of
        // the shader engines and XCDs in, every one of them keeps the same share)
        const int words = (cus + 31) / 32;
        std::vector<uint32_t> mask((size_t)std::max(words, 1), 0u);
        int enabled = 0;
        for (int c = 0; c < cus; ++c)
            if ((int64_t)(c + 1) * cu_percent / 100 > (int64_t)c * cu_percent / 100) {
                mask[(size_t)c / 32] |= 1u << (c % 32);
                ++enabled;
            }
        if (enabled == 0) mask[0] |= 1u;
        hipStream_t s = nullptr;
        if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BCP_E_HIP, "bcp_side_stream: the runtime refused a CU-masked stream");
        }
        h->side_stream = s;
        h->side_share = cu_percent;
    }
    *stream = (void*)h->side_stream;
    return BCP_OK;
}

extern "C" int bcp_set_costmaps(bcp_handle* h, const uint8_t* data, int32_t rows, int32_t cols, int32_t shared,
                                const int32_t* valid_rows, const int32_t* valid_cols, const double* origins,
                                int32_t origins_per_env, double resolution, void* stream)
{
    if (!h || !data || !origins) return fail(BCP_E_INVALID, "bcp_set_costmaps: null argument");
    if (rows <= 0 || cols <= 0 || !(resolution > 0)) return fail(BCP_E_INVALID, "bcp_set_costmaps: bad shape/resolution");
    if (!check_kernel_size(h->params, resolution))
        return fail(BCP_E_INVALID, "bcp_set_costmaps: footprint radius / resolution exceeds %d px", BCP_MAX_KERNEL_HALF);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int wpr = (cols + 31) / 32;
    const int64_t n_maps = shared ? 1 : n_slots(h);
    HIP_TRY(h->bitmap.reserve((size_t)n_maps * rows * wpr));
    HIP_TRY(h->map_tiles.reserve((size_t)n_maps * map_tile_words(rows, wpr)));
    h->resolution = resolution;
    h->map_data = data;
    h->map_valid_rows = valid_rows;
    h->map_valid_cols = valid_cols;
    fill_dev_params(h);
    MapDesc& m = h->map;
    m.bits = h->bitmap.get();
    m.tiles = h->map_tiles.get();
    m.rows = rows;
    m.cols = cols;
    m.wpr = wpr;
    m.shared = shared ? 1 : 0;
    m.env_stride = shared ? 0 : (int64_t)rows * wpr;
    m.inv_res = 1.0 / resolution;  // anti_resolution = 1./resolution (coordinate_transformations.py:204)
    if (origins_per_env) {
        m.origins = origins;
        m.ox = m.oy = 0;
    } else {
        m.origins = nullptr;
        m.ox = origins[0];
        m.oy = origins[1];
    }
    // stage the shared bitmap in LDS when the whole collision scratch then stays within 64 KiB per workgroup
    m.in_lds = (shared && collision_lds_bytes(h->params.n_verts, 1, rows, wpr) <= 64 * 1024) ? 1 : 0;
    h->wide = footprint_is_wide(h->params, resolution);
    const EntrySelect all_maps = {nullptr, nullptr, n_maps};
    launch_pack_bitmap(h, all_maps, n_maps, s);
    HIP_TRY(hipGetLastError());
    // distance field for the O(1) pre-classification (shared maps)
    CullDesc& C = h->cull;
    memset(&C, 0, sizeof(C));
    build_cull_geometry(h->params, resolution, &C);
    if (h->cull_enabled) {
        // shared map: padding wide enough that every sample of a pose whose image touches the map is stored;
        // private maps: just enough that a sample outside the stored rectangle (more than `pad` px away from every
        // cell of the map) is known to clear the outer test
        if (!shared) C.pad = std::max(8, C.t_out);
        const int clamp = std::min(255, std::max(C.t_out + 1, 2));
        const int W = cols + 2 * C.pad, H = rows + 2 * C.pad;
        const size_t cells = (size_t)n_maps * W * H;
        HIP_TRY(h->edt.reserve(cells));
        HIP_TRY(h->edt_col.reserve(cells));
        // the 1-bit form for the outer test (near_tiles_kernel)
        const int tiles_x = (W + 31) / 32, tiles_y = (H + 31) / 32;
        HIP_TRY(h->near.reserve((size_t)n_maps * tiles_x * tiles_y * 32));
        C.near = h->near.get();
        C.near_tx = tiles_x;
        C.near_words = tiles_x * tiles_y * 32;
        C.near_stride = shared ? 0 : (int64_t)C.near_words;
        // what the single-launch step reads: the tiles themselves for a shared map (it stays in cache), a coarser copy for
        // private maps -- see CullDesc::step_near
        const int shift = shared ? 0 : (h->near_shift >= 0 ? h->near_shift : kNearShiftPrivate);
        C.step_near = h->near.get();
        C.step_near_stride = C.near_stride;
        C.step_near_tx = tiles_x;
        C.step_near_shift = 0;
        if (shift > 0) {
            const int cw = (W + (1 << shift) - 1) >> shift, ch = (H + (1 << shift) - 1) >> shift;
            const int ctx = (cw + 31) / 32, cty = (ch + 31) / 32;
            HIP_TRY(h->near_coarse.reserve((size_t)n_maps * ctx * cty * 32));
            C.step_near = h->near_coarse.get();
            C.step_near_stride = (int64_t)ctx * cty * 32;
            C.step_near_tx = ctx;
            C.step_near_shift = shift;
        }
        C.edt = h->edt.get();
        C.width = W;
        C.height = H;
        C.clamp = clamp;
        C.env_stride = shared ? 0 : (int64_t)W * H;
        C.on = C.t_out <= clamp ? 1 : 0;
        // the stale marks of tiles-only refreshes (launch_distance_field): every field is rebuilt below, so none is stale
        h->edt_lazy = false;
        if (!shared) {   // (the marks and their list go together: without the list there are no marks)
            hipError_t e = h->edt_stale.reserve((size_t)n_maps);
            if (e == hipSuccess) e = h->edt_stale_list.reserve((size_t)n_maps + 1);
            if (e != hipSuccess) (void)h->edt_stale.reset();
            HIP_TRY(e);
        }
        if (h->edt_stale.get()) HIP_TRY(hipMemsetAsync(h->edt_stale.get(), 0, h->edt_stale.capacity(), s));
        {
            // Many private maps under the single-launch step: only the 1-bit tiles are read, so they are made directly from the
            // lethal masks (near_dilate_kernel) and the uint8 fields are left to whoever asks for them (ensure_fields) -- what a
            // pool refresh has done since round 3.  65 536 maps of 256 x 256: 75 ms of edt_lds_kernel -> a few ms (round 4).
            const bool tiles_only = !shared && n_maps >= 32 && h->fused && h->adaptive && C.on && h->near_dilate == 1;
            BCP_TRY(launch_distance_field(h, all_maps, n_maps, s, tiles_only));
        }
        HIP_TRY(hipGetLastError());
        if (!h->pending.get()) {
            const int64_t blocks = (h->n + kBlock - 1) / kBlock;
            h->pending_cap = (int32_t)(((blocks + kShards - 1) / kShards) * kBlock);  // every env of a shard's blocks
            HIP_TRY(h->pending_count.reserve(2 * kShards));
            HIP_TRY(hipMemsetAsync(h->pending_count.get(), 0, 2 * kShards * sizeof(int32_t), s));
            // [2] thresholds (alternating by step parity), then [2][kShards] in-place counters
            HIP_TRY(h->adapt.reserve(2 + 2 * kShards));
            HIP_TRY(hipMemsetAsync(h->adapt.get(), 0, (2 + 2 * kShards) * sizeof(int32_t), s));
            const int32_t init[2] = {h->dense_threshold, h->dense_threshold};
            HIP_TRY(hipMemcpyAsync(h->adapt.get(), init, sizeof(init), hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));   // (`init` is on the stack)
            // (last: the slots mark this block as done, so a failure above is met again by the next call)
            HIP_TRY(h->pending.reserve((size_t)kShards * h->pending_cap));
        }
    }
    h->have_map = true;
    h->static_dirty = true;
    if (h->have_path && !h->path.shared) {   // the path records carry the origins
        const int64_t n_paths = n_slots(h);
        const EntrySelect all_paths = {nullptr, nullptr, n_paths};
        launch_world_records(h, all_paths, n_paths, s);
        HIP_TRY(hipGetLastError());
    }
    return BCP_OK;
}

extern "C" int bcp_get_distance_field(bcp_handle* h, int64_t first_entry, int64_t n_entries, uint8_t* out, int32_t* shape,
                                      void* stream)
{
    if (!h || !shape) return fail(BCP_E_INVALID, "bcp_get_distance_field: null argument");
    if (!h->have_map || !h->cull.edt) return fail(BCP_E_STATE, "bcp_get_distance_field: no distance field (no costmap, or culling off)");
    const CullDesc& C = h->cull;
    shape[0] = C.height;
    shape[1] = C.width;
    shape[2] = C.pad;
    shape[3] = C.clamp;
    if (!out) return BCP_OK;
    const int64_t n_maps = h->map.shared ? 1 : n_slots(h);
    if (first_entry < 0 || n_entries <= 0 || first_entry + n_entries > n_maps)
        return fail(BCP_E_INVALID, "bcp_get_distance_field: entries out of range");
    HIP_TRY(hipSetDevice(h->device));
    BCP_TRY(ensure_fields(h, (hipStream_t)stream));
    const size_t per = (size_t)C.width * C.height;
    HIP_TRY(hipMemcpyAsync(out, h->edt.get() + first_entry * per, n_entries * per, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BCP_OK;
}

extern "C" int bcp_get_near_field(bcp_handle* h, int64_t first_entry, int64_t n_entries, uint32_t* out, int32_t* shape,
                                  void* stream)
{
    if (!h || !shape) return fail(BCP_E_INVALID, "bcp_get_near_field: null argument");
    if (!h->have_map || !h->cull.near) return fail(BCP_E_STATE, "bcp_get_near_field: no distance field (no costmap, or culling off)");
    const CullDesc& C = h->cull;
    shape[0] = C.near_words / (32 * C.near_tx);
    shape[1] = C.near_tx;
    shape[2] = C.t_out;
    if (!out) return BCP_OK;
    const int64_t n_maps = h->map.shared ? 1 : n_slots(h);
    if (first_entry < 0 || n_entries <= 0 || first_entry + n_entries > n_maps)
        return fail(BCP_E_INVALID, "bcp_get_near_field: entries out of range");
    HIP_TRY(hipSetDevice(h->device));
    const size_t per = (size_t)C.near_words;
    HIP_TRY(hipMemcpyAsync(out, h->near.get() + first_entry * per, n_entries * per * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return BCP_OK;
}

extern "C" int bcp_set_paths(bcp_handle* h, const double* xytheta, const int32_t* lens, int32_t max_len, int32_t shared,
                             void* stream)
{
    if (!h || !xytheta) return fail(BCP_E_INVALID, "bcp_set_paths: null argument");
    if (max_len <= 0) return fail(BCP_E_INVALID, "bcp_set_paths: max_len must be positive");
    if (!shared && !lens) return fail(BCP_E_INVALID, "bcp_set_paths: per-env paths need lens");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (shared ? 1 : n_slots(h)) * (int64_t)max_len;
    HIP_TRY(h->path5.reserve((size_t)total * 5));
    HIP_TRY(h->path_pre.reserve(shared ? 0 : (size_t)total * 2));
    const int64_t n_paths = shared ? 1 : n_slots(h);
    HIP_TRY(h->path_bbox.reserve((size_t)n_paths * kBoxDoubles));
    HIP_TRY(h->path_index.reserve((size_t)4 * kPathBuckets));   // (a shared path's tables; private ones live in the records)
    if (max_len > 32766) return fail(BCP_E_INVALID, "bcp_set_paths: paths longer than 32766 way points are not supported");
    h->path.pts = h->path5.get();
    h->path.pre = shared ? nullptr : h->path_pre.get();
    h->path.bbox = h->path_bbox.get();
    h->path.index = h->path_index.get();
    h->path.lens = shared ? nullptr : lens;
    h->path.max_len = max_len;
    h->path.shared = shared ? 1 : 0;
    h->path_src = xytheta;
    const EntrySelect all_paths = {nullptr, nullptr, n_paths};
    launch_path_data(h, all_paths, n_paths, s);
    HIP_TRY(hipGetLastError());
    h->have_path = true;
    h->static_dirty = true;
    return BCP_OK;
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
    BCP_TRY(ensure_fields(h, (hipStream_t)stream));
    const int blocks = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pose_collides_kernel, dim3(blocks), dim3(kBlock),
                       collision_lds_bytes(h->params.n_verts, h->map.in_lds, h->map.rows, h->map.wpr),
                       (hipStream_t)stream, h->dev, h->map, h->cull, h->exact_mode, h->dense_threshold, h->wide, poses, n,
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
    if (h->exact_mode == 2) {  // per-thread rasteriser
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

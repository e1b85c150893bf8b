// bcp_aisle.h -- RandomAisleTurnEnv worlds made on the device: the turn drawn from numpy's RandomState stream
// (_draw_random_turn_params, envs/synth_turn_env.py:317-332), its corners, way points and map shape
// (path_and_costmap_from_config, :110-192), the five 1-px walls rendered into a padded pool entry, and the refined path
// with the reward provider's initial state (make_initial_state, envs/base/env.py:179-214).  Three kernels, so that a
// pool can be sized between drawing and rendering:
//   aisle_world_draw_kernel    one wavefront per stream: the MT19937 window of bcp_sample.h, lane 0 draws and computes
//   aisle_world_render_kernel  one workgroup per world: zero-fill of the padded entry, then the walls
//   aisle_world_paths_kernel   one thread per world: refine_path over the three segments, initial reward state
// Included by bcplan.hip (entry points bcp_sample_aisle_worlds, bcp_render_aisle_worlds, bcp_aisle_world_paths: bcp_worlds_host.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bcp_device.h"
#include "bcp_sample.h"

namespace bcp {

// world record: [0, 8) turn params (main / turn corridor length, angle, main / turn width, flip_oy, flip_ox, rot_theta),
// [8, 10) world origin, [10, 30) corners A .. J, [30, 42) way points B, K, L, F (x, y, theta), [42] refined path length
constexpr int kAisleRecord = 44;
constexpr int kAisleOrigin = 8, kAisleCorners = 10, kAisleWay = 30, kAisleLen = 42;

struct AisleWorldParams {   // the ranges of _draw_random_turn_params, TurnParams.margin, EnvParams.resolution / path_delta
    double main_length[2], turn_length[2], angle[2], main_width[2], turn_width[2];
    double margin, resolution, path_delta;
};

// rows appended to a refined path by one segment of refine_path (utilities/path_tools.py:178-240)
__device__ __forceinline__ int refined_rows(double x0, double y0, double x1, double y1, double path_delta)
{
    const double dx = x1 - x0, dy = y1 - y0;
    const double d = sqrt(dx * dx + dy * dy);   // np.linalg.norm(..., axis=1): sqrt(add.reduce(x * x))
    return d > path_delta ? (int)(d / path_delta) + 1 : 1;
}

// path_and_costmap_from_config (:110-192) up to the map's creation: lane 0's scalar job
__device__ void aisle_world_geometry(const double tp[8], const AisleWorldParams& ap, double* __restrict__ rec,
                                     int32_t* __restrict__ shape)
{
    const double hh = tp[0] / 2, w = tp[1] / 2, alpha = tp[2], d = tp[3], z = tp[4];
    const bool flip_oy = tp[5] != 0.0, flip_ox = tp[6] != 0.0;
    const double rot_theta = tp[7];
    const double ta = tan(alpha), ca = cos(alpha);
    // _draw_pts_in_standard_coords (:42-79): A B C D E F G H I J
    const double std_pts[10][2] = {{-d, -hh}, {0, -hh}, {d, -hh}, {d, d * ta - z / ca}, {w, w * ta - z / ca},
                                   {w, w * ta}, {d, d * ta + z / ca}, {w, w * ta + z / ca}, {-d, hh}, {d, hh}};
    // _generate_path_in_standard_coords (:82-97): B K L F
    const double std_way[4][3] = {{0, -hh, kPi / 2}, {0, d * ta - z / ca, kPi / 2}, {d, d * ta, alpha},
                                  {w * ca, w * ca * ta, alpha}};
    // transform = rotation . flip (np.dot of two 2 x 2 matrices: the products with the flip's zeros add nothing)
    const double c = cos(rot_theta), s = sin(rot_theta);
    const double fx = flip_oy ? -1. : 1., fy = flip_ox ? -1. : 1.;
    const double t00 = c * fx, t01 = -s * fy, t10 = s * fx, t11 = c * fy;
    double min_x = 0, max_x = 0, min_y = 0, max_y = 0;
    for (int k = 0; k < 10; ++k) {
        const double x = t00 * std_pts[k][0] + t01 * std_pts[k][1];
        const double y = t10 * std_pts[k][0] + t11 * std_pts[k][1];
        rec[kAisleCorners + 2 * k] = x;
        rec[kAisleCorners + 2 * k + 1] = y;
        min_x = k ? fmin(min_x, x) : x;
        max_x = k ? fmax(max_x, x) : x;
        min_y = k ? fmin(min_y, y) : y;
        max_y = k ? fmax(max_y, y) : y;
    }
    for (int k = 0; k < 4; ++k) {
        double* o = rec + kAisleWay + 3 * k;
        o[0] = t00 * std_way[k][0] + t01 * std_way[k][1];
        o[1] = t10 * std_way[k][0] + t11 * std_way[k][1];
        double a = std_way[k][2];
        if (flip_ox) a = -a;
        if (flip_oy) a = kPi - a;
        o[2] = py_mod(a + rot_theta, kTwoPi);   // np.mod
    }
    const double size_x = fabs(max_x - min_x) + 2 * ap.margin, size_y = fabs(max_y - min_y) + 2 * ap.margin;
    rec[kAisleOrigin] = min_x - ap.margin;
    rec[kAisleOrigin + 1] = min_y - ap.margin;
    // CostMap2D.create_empty (utilities/costmap_2d.py:58-69): world_to_pixel of the size, reversed
    const double inv_res = 1.0 / ap.resolution;
    shape[0] = (int32_t)rint(size_y * inv_res);
    shape[1] = (int32_t)rint(size_x * inv_res);
    const double* wp = rec + kAisleWay;
    int len = 1;
    for (int k = 0; k < 3; ++k) len += refined_rows(wp[3 * k], wp[3 * k + 1], wp[3 * k + 3], wp[3 * k + 4], ap.path_delta);
    rec[kAisleLen] = (double)len;
    rec[kAisleLen + 1] = 0.0;
}

// worlds: [n_chains * episodes][kAisleRecord], shapes: [n_chains * episodes][2] = (rows, cols); world k of chain c is
// entry c * episodes + k (world 0 = RandomAisleTurnEnv's constructor, world k = its k-th reset()).
__global__ void __launch_bounds__(64) aisle_world_draw_kernel(AisleWorldParams ap, uint32_t* __restrict__ mt_state,
                                                              int64_t n_chains, int episodes, double* __restrict__ worlds,
                                                              int32_t* __restrict__ shapes)
{
    __shared__ uint32_t lds[2 * kMtWords + 2];
    const int lane = threadIdx.x;
    const int64_t chain = blockIdx.x;
    if (chain >= n_chains) return;
    MtStream mt{(MtLds)lds, 0};
    uint32_t* record = mt_state + chain * kMtRecord;
    for (int k = lane; k < kMtWords; k += 64) mt.buf[k] = record[k];
    if (lane == 0) mt.set_pos(min(record[kMtWords], (uint32_t)kMtWords));
    wave_lds_sync();
    mt_twist(mt.block_a(), mt.block_b(), lane);
    for (int e = 0; e < episodes; ++e) {
        mt_reserve(mt, lane);   // 16 words per world: well inside the window
        if (lane == 0) {
            double tp[8];
            tp[0] = mt.next_uniform(ap.main_length[0], ap.main_length[1]);
            tp[1] = mt.next_uniform(ap.turn_length[0], ap.turn_length[1]);
            tp[2] = mt.next_uniform(ap.angle[0], ap.angle[1]);
            tp[3] = mt.next_uniform(ap.main_width[0], ap.main_width[1]);
            tp[4] = mt.next_uniform(ap.turn_width[0], ap.turn_width[1]);
            tp[5] = mt.next_real() < 0.5 ? 1.0 : 0.0;
            tp[6] = mt.next_real() < 0.5 ? 1.0 : 0.0;
            tp[7] = mt.next_uniform(0, kTwoPi);
            const int64_t g = chain * episodes + e;
            double* rec = worlds + g * kAisleRecord;
            for (int k = 0; k < 8; ++k) rec[k] = tp[k];
            aisle_world_geometry(tp, ap, rec, shapes + 2 * g);
        }
    }
    mt_reserve(mt, lane);
    for (int k = lane; k < kMtWords; k += 64) record[k] = mt.block_a()[k];
    if (lane == 0) record[kMtWords] = mt.pos();
}

// the five walls A-I, C-D, D-E, J-G, G-H (:174-180) as corner indices
__constant__ const int8_t kAisleWalls[5][2] = {{0, 8}, {2, 3}, {3, 4}, {9, 6}, {6, 7}};

// maps: [n_worlds][rows][pitch] uint8, pitch a multiple of 16 bytes and >= every world's cols, rows >= every world's
// rows.  The whole entry is zeroed with 16-byte stores; then the walls are drawn into the world's own rows x cols
// (cv2.line clips to the image), so the padding stays 0.
__global__ void __launch_bounds__(256) aisle_world_render_kernel(const double* __restrict__ worlds,
                                                                 const int32_t* __restrict__ shapes, int rows, int pitch,
                                                                 double inv_res, uint8_t* __restrict__ maps)
{
    const int64_t g = blockIdx.x;
    uint8_t* map = maps + g * (int64_t)rows * pitch;
    const int64_t quads = (int64_t)rows * pitch / 16;
    uint4* q = reinterpret_cast<uint4*>(map);
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t i = threadIdx.x; i < quads; i += blockDim.x) q[i] = zero;
    __syncthreads();   // (the walls overwrite zeros of other threads)
    const int vr = shapes[2 * g], vc = shapes[2 * g + 1];
    if (vr <= 0 || vc <= 0 || vr > rows || vc > pitch) return;   // the host sized the pool from these shapes
    const double* rec = worlds + g * kAisleRecord;
    const double ox = rec[kAisleOrigin], oy = rec[kAisleOrigin + 1];
    for (int k = 0; k < 5; ++k) {
        const double* p0 = rec + kAisleCorners + 2 * kAisleWalls[k][0];
        const double* p1 = rec + kAisleCorners + 2 * kAisleWalls[k][1];
        // world_to_pixel (coordinate_transformations.py:185-205), then cv2.line: clip, left to right, closed-form minor
        int64_t x1 = (int64_t)rint((p0[0] - ox) * inv_res), y1 = (int64_t)rint((p0[1] - oy) * inv_res);
        int64_t x2 = (int64_t)rint((p1[0] - ox) * inv_res), y2 = (int64_t)rint((p1[1] - oy) * inv_res);
        if (!clip_segment(vc, vr, x1, y1, x2, y2)) continue;
        if (x2 < x1) {
            int64_t t = x1;
            x1 = x2;
            x2 = t;
            t = y1;
            y1 = y2;
            y2 = t;
        }
        const int dx = (int)(x2 - x1), ady = (int)(y2 >= y1 ? y2 - y1 : y1 - y2);
        const int sy = y2 >= y1 ? 1 : -1;
        const bool vert = ady > dx;
        const int major = vert ? ady : dx, minor = vert ? dx : ady;
        for (int i = threadIdx.x; i <= major; i += blockDim.x) {
            const int across = major > 0 ? (int)((2 * (int64_t)minor * i + major - 1) / (2 * (int64_t)major)) : 0;
            const int x = (int)x1 + (vert ? across : i);
            const int y = (int)y1 + sy * (vert ? i : across);
            if ((unsigned)x < (unsigned)vc && (unsigned)y < (unsigned)vr) map[(int64_t)y * pitch + x] = (uint8_t)BCP_LETHAL;
        }
    }
}

// make_initial_state for every world: refine_path of B K L F (numpy's linspace arithmetic, inserted points carry
// the heading of their segment's first point) and the reward provider's initial state.  paths [G][max_len][3],
// lens [G], init [G][2], status [G] as bcp_mini_world_paths.
__global__ void aisle_world_paths_kernel(const double* __restrict__ worlds, int64_t n_worlds, double path_delta, double sp,
                                         double ap, int pure_pursuit, int max_len, double* __restrict__ paths,
                                         int32_t* __restrict__ lens, double* __restrict__ init,
                                         int32_t* __restrict__ status)
{
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_worlds; g += (int64_t)gridDim.x * blockDim.x) {
        const double* wp = worlds + g * kAisleRecord + kAisleWay;
        double* p = paths + g * (int64_t)max_len * 3;
        int m = 0, rc = 0;
        for (int k = 0; k < 3 && !rc; ++k) {
            const double x0 = wp[3 * k], y0 = wp[3 * k + 1], th0 = wp[3 * k + 2];
            const double dx = wp[3 * k + 3] - x0, dy = wp[3 * k + 4] - y0;
            const double d = sqrt(dx * dx + dy * dy);
            if (d > path_delta) {
                const int npoints = (int)(d / path_delta) + 2;
                if (m + npoints - 1 >= max_len) {
                    rc = 1;
                    break;
                }
                const double sx = dx / (double)(npoints - 1), sy = dy / (double)(npoints - 1);
                for (int i = 0; i < npoints - 1; ++i, ++m) {
                    p[3 * m + 0] = (double)i * sx + x0;
                    p[3 * m + 1] = (double)i * sy + y0;
                    p[3 * m + 2] = th0;
                }
            } else {
                if (m + 1 >= max_len) {
                    rc = 1;
                    break;
                }
                p[3 * m + 0] = x0;
                p[3 * m + 1] = y0;
                p[3 * m + 2] = th0;
                ++m;
            }
        }
        if (rc) {
            lens[g] = 0;
            init[2 * g] = 0.0;
            init[2 * g + 1] = 0.0;
            status[g] = rc;
            continue;
        }
        p[3 * m + 0] = wp[9];
        p[3 * m + 1] = wp[10];
        p[3 * m + 2] = wp[11];
        ++m;
        lens[g] = m;
        double min_dist;
        int target;
        path_initial_reward(p, m, sp, ap, pure_pursuit, min_dist, target, rc, DeviceNormalizeAngle());
        init[2 * g] = min_dist;
        init[2 * g + 1] = (double)target;
        status[g] = rc;
    }
}

}  // namespace bcp

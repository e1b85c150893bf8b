// bcp_path_init.h -- the reward provider's initial state on a path: the one statement that mini_world_path (bcp_sample.h),
// aisle_world_path (bcp_aisle.h) and goal_route_row (bcp_goal_cell.h) share.  Plain C++ with no HIP in it, host and device:
// the kernels call it with the device's normalize_angle (DeviceNormalizeAngle, bcp_device.h) and the device's hypot / cos /
// sin, tests/c_abi/goal_route_main.cpp with the host's.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BCP_HD __host__ __device__
#else
#define BCP_HD
#endif

namespace bcp {

// The reward provider's initial state on a refined path p[0 .. m) that starts at the initial pose p[0]; rc becomes 2 for
// "Goal pose too close to initial pose" (ValueError in the reference), else it is left as it is.  normalize(z): z wrapped to
// [-pi, pi) (utilities/coordinate_transformations.py:28-36).
template <typename Normalize>
BCP_HD inline __attribute__((always_inline)) void path_initial_reward(const double* __restrict__ p, int m, double sp, double ap,
                                                                      int pure_pursuit, double& min_dist, int& target, int& rc,
                                                                      const Normalize& normalize)
{
    const double x0 = p[0], y0 = p[1], th0 = p[2];
    const double x1 = p[3 * (m - 1)], y1 = p[3 * (m - 1) + 1];
    if (pure_pursuit) {   // reward.py:355-371
        target = 1;
        min_dist = hypot(x1 - x0, y1 - y0);
    } else {              // find_last_reached(path[0], path) (path_tools.py:408-448), reward.py:261-288
        int last = -1;
        for (int j = 0; j < m; ++j) {
            const double xj = p[3 * j], yj = p[3 * j + 1], tj = p[3 * j + 2];
            const bool near = hypot(xj - x0, yj - y0) < sp;
            if (!near) continue;   // (three independent predicates: the other two cost a cos, a sin and an fmod per way point)
            const bool aligned = fabs(normalize(th0 - tj)) < ap;
            const bool ahead = cos(tj) * (x0 - xj) + sin(tj) * (y0 - yj) >= -sp / 9;
            if (aligned && ahead) last = j;
        }
        if (last == m - 1) rc = 2;
        target = last + 1 < m - 1 ? last + 1 : m - 1;
        min_dist = hypot(p[3 * target] - x0, p[3 * target + 1] - y0);
    }
}

}  // namespace bcp

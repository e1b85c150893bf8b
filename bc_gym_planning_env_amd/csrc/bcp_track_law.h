// bcp_track_law.h -- the law of the path tracker (bcp_track, include/bcplan.h): which way point a lane steers for (the
// carrot), the curvature of the arc through it, and the command that asks the robot for that arc.  Plain C++ with no HIP in
// it, host and device: track_kernel (bcp_track.h) calls these functions with the device's sincos / atan / normalize_angle
// (DeviceTrackMath there), tests/c_abi/track_main.cpp calls the same ones with the host's, and there is no other copy.
// Everything is float64 with every product, quotient and sum rounded on its own (-ffp-contract=off).
// The conversion to a tricycle command restates the reference's diff_drive_control_to_tricycle statement by statement; the
// lines cited are robot_models/tricycle_model.py's unless another file is named (paths relative to bc_gym_planning_env/).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define BCP_HD __host__ __device__
#else
#define BCP_HD
#endif

namespace bcp {

constexpr int kTrackPointStride = 5;          // doubles per way-point record as the handle keeps them: x, y first
constexpr double kTrackMinDist2 = 1e-12;      // a carrot closer than 1e-6 m asks for no turn
constexpr double kTrackStillSpeed = 1e-6;     // :206, :228
constexpr double kTrackPiOver8 = 3.14159265358979323846 / 8;   // np.pi/8 (:228): a division by a power of two, exact

// what a lane's gains must be for the law to run: both finite, speed >= 0, reach > 0 (a NaN fails every comparison)
BCP_HD inline bool track_gains_ok(double speed, double reach)
{
    const double lim = 1.7976931348623157e308;
    return speed >= 0.0 && speed <= lim && reach > 0.0 && reach <= lim;
}

// np.clip == minimum(maximum(a, lo), hi)
BCP_HD inline double track_clip(double a, double lo, double hi)
{
    const double t = a < lo ? lo : a;
    return t > hi ? hi : t;
}

// The carrot: from j0 = min(max(c_prev, target_idx), m - 1) the first way point at least `reach` away from (x, y), compared
// on squares; the last way point if there is none.  m >= 1.  The index never goes backwards within a roll-out (c_prev is
// the previous trip's result), so H trips scan at most m + H records.  dx, dy: the carrot's offset from (x, y).
template <typename Points>   // pts[kTrackPointStride * j + 0 / 1] = way point j's x / y
BCP_HD inline int track_carrot(Points pts, int m, double x, double y, double reach, int c_prev, int target_idx, double& dx,
                               double& dy)
{
    int j = c_prev > target_idx ? c_prev : target_idx;
    if (j > m - 1) j = m - 1;
    if (j < 0) j = 0;
    const double r2 = reach * reach;
    for (;; ++j) {
        dx = pts[kTrackPointStride * j] - x;
        dy = pts[kTrackPointStride * j + 1] - y;
        if (j >= m - 1 || dx * dx + dy * dy >= r2) return j;
    }
}

// (dx, dy) in the frame of a robot heading along (c, s) = (cos th, sin th)
BCP_HD inline void track_robot_frame(double c, double s, double dx, double dy, double& lx, double& ly)
{
    lx = c * dx + s * dy;
    ly = -s * dx + c * dy;
}

// Pure pursuit: the curvature of the arc that leaves the robot along its heading and passes through (lx, ly), clamped to
// +- max_curvature (finite, > 0); 0 for a carrot on top of the robot.
BCP_HD inline double track_curvature(double lx, double ly, double max_curvature)
{
    const double d2 = lx * lx + ly * ly;
    const double kappa = d2 < kTrackMinDist2 ? 0.0 : 2.0 * ly / d2;
    return track_clip(kappa, -max_curvature, max_curvature);
}

// diff_drive_control_to_tricycle (:191-231): the wheel speed and wheel angle with which a tricycle approximates the body
// motion (v, w), given its current wheel angle.  math.cos_sin(a, c, s), math.atan(x), math.normalize(z) (z wrapped to
// [-pi, pi), utilities/coordinate_transformations.py:28-36).
template <typename Math>
BCP_HD inline void track_diff_drive_to_tricycle(double v, double w, double wheel_angle, double max_wheel_angle, double L,
                                                const Math& math, double& wheel_v, double& angle)
{
    const bool still = (v < 0.0 ? -v : v) < kTrackStillSpeed;            // :206 np.abs(linear_vel) < 1e-6
    double desired;
    if (still) {
        const double sign = (double)((w > 0.0) - (w < 0.0));               // :207 np.sign(angular_vel) * max
        desired = sign * max_wheel_angle;
    } else {
        desired = math.atan(L * w / v);                                    // :209
    }
    desired = track_clip(desired, -max_wheel_angle, max_wheel_angle);     // :211
    double wheel_cos, wheel_sin;
    math.cos_sin(wheel_angle, wheel_cos, wheel_sin);                       // :218-219
    double fw = v * wheel_cos + w * L * wheel_sin;                         // :224
    if (0.0 > fw) fw = 0.0;                                                // :225 max(fw, 0.)
    if (still) {   // :228-229, diff_angles: utilities/coordinate_transformations.py:148-155
        const double diff = math.normalize(wheel_angle - desired);
        if ((diff < 0.0 ? -diff : diff) > kTrackPiOver8) fw = 0.0;
    }
    wheel_v = fw;
    angle = desired;
}

struct TrackCommand {
    double cmd0, cmd1;
    int carrot;
};

// One evaluation of the law for a lane with valid gains: carrot, robot frame, curvature, the desired body motion
// (speed, speed * kappa), the handle's command for it, and the action box.
template <typename Points, typename Math>
BCP_HD inline TrackCommand track_law(Points pts, int m, double x, double y, double th, double wheel_angle, int target_idx,
                                     int c_prev, double speed, double reach, double max_curvature, bool tricycle,
                                     double max_wheel_angle, double L, const double low[2], const double high[2], const Math& math)
{
    TrackCommand out;
    double dx, dy, c, s, lx, ly;
    out.carrot = track_carrot(pts, m, x, y, reach, c_prev, target_idx, dx, dy);
    math.cos_sin(th, c, s);
    track_robot_frame(c, s, dx, dy, lx, ly);
    const double kappa = track_curvature(lx, ly, max_curvature);
    const double v = speed, w = speed * kappa;
    double a0 = v, a1 = w;
    if (tricycle) track_diff_drive_to_tricycle(v, w, wheel_angle, max_wheel_angle, L, math, a0, a1);
    out.cmd0 = track_clip(a0, low[0], high[0]);
    out.cmd1 = track_clip(a1, low[1], high[1]);
    return out;
}

// The cap a speed profile puts on a lane's speed: the smaller of the profile at the way point the robot is heading for,
// min(target_idx, m - 1), and at the carrot -- numpy's minimum, a NaN if either is one.  profile[j]: way point j's speed.
template <typename Profile>
BCP_HD inline double track_speed_cap(Profile profile, int m, int target_idx, int carrot)
{
    int at = target_idx < m - 1 ? target_idx : m - 1;
    if (at < 0) at = 0;
    const double a = profile[at], b = profile[carrot];
    if (a != a) return a;
    if (b != b) return b;
    return b < a ? b : a;
}

// the gain's speed under a cap: a cap that is NaN or negative leaves it as it is
BCP_HD inline double track_capped_speed(double speed, double cap) { return (cap >= 0.0 && cap < speed) ? cap : speed; }

// track_law with step 4 reading a speed profile (bcp_track_profile): v = the gain's speed capped by track_speed_cap, w = v *
// kappa.  Everything else is track_law's, statement by statement; a profile of speeds >= the gain's gives its bits.
template <typename Points, typename Profile, typename Math>
BCP_HD inline TrackCommand track_law_profile(Points pts, Profile profile, int m, double x, double y, double th, double wheel_angle,
                                             int target_idx, int c_prev, double speed, double reach, double max_curvature,
                                             bool tricycle, double max_wheel_angle, double L, const double low[2],
                                             const double high[2], const Math& math)
{
    TrackCommand out;
    double dx, dy, c, s, lx, ly;
    out.carrot = track_carrot(pts, m, x, y, reach, c_prev, target_idx, dx, dy);
    math.cos_sin(th, c, s);
    track_robot_frame(c, s, dx, dy, lx, ly);
    const double kappa = track_curvature(lx, ly, max_curvature);
    const double v = track_capped_speed(speed, track_speed_cap(profile, m, target_idx, out.carrot)), w = v * kappa;
    double a0 = v, a1 = w;
    if (tricycle) track_diff_drive_to_tricycle(v, w, wheel_angle, max_wheel_angle, L, math, a0, a1);
    out.cmd0 = track_clip(a0, low[0], high[0]);
    out.cmd1 = track_clip(a1, low[1], high[1]);
    return out;
}

// what bcp_track refuses with BCP_E_INVALID after the handle's own checks, in the order it looks
enum TrackRefusal { kTrackOk = 0, kTrackShape = 1, kTrackCurvature = 2, kTrackBoxFinite = 3, kTrackBoxOrder = 4, kTrackNull = 5,
                    kTrackBest = 6, kTrackLarge = 7 };

BCP_HD inline int track_check_args(int32_t horizon, int32_t n_candidates, double max_curvature, const double low[2],
                                   const double high[2], bool have_required, bool have_best, bool have_best_outputs,
                                   int64_t n_envs, int* d_out)
{
    const double lim = 1.7976931348623157e308;
    if (horizon < 1 || n_candidates < 1) return kTrackShape;
    if (!(max_curvature > 0.0) || !(max_curvature <= lim)) return kTrackCurvature;
    for (int d = 0; d < 2; ++d) {
        *d_out = d;
        if (!(low[d] >= -lim && low[d] <= lim && high[d] >= -lim && high[d] <= lim)) return kTrackBoxFinite;
        if (low[d] > high[d]) return kTrackBoxOrder;
    }
    if (!have_required) return kTrackNull;
    if (have_best_outputs && !have_best) return kTrackBest;
    // element offsets are int64: the largest is 6 * N * K * H (trace)
    const int64_t limit = (int64_t)1 << 62;
    if (n_envs > limit / 6 / horizon / n_candidates) return kTrackLarge;
    return kTrackOk;
}

}  // namespace bcp

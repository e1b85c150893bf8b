"""A numpy restatement of bcp_track's law (include/bcplan.h, csrc/bcp_track_law.h), one roll-out at a time, for the tracker's
tests: the carrot rule, the pure-pursuit curvature, the command (diff_drive_control_to_tricycle written out with numpy's own
sin / cos / arctan / clip / sign, statement by statement as the contract lists them), the box -- and roll-outs whose forward
step is the CPU oracle's, driven as tests/lookahead_ref.py drives it.  No product code is involved.

The error bound of a command (law_bound).  u = 2^-53 is the unit roundoff; a rounded operation is off by at most u times its
result.  Two implementations of the law run the same IEEE operations on the same inputs and differ only in sin, cos and atan.
Each of the libraries involved (glibc, numpy's vector loops, the device's ocml) states at most 4 ulp for sin and cos and at most
5 ulp for atan (the OpenCL limits, the loosest of the three), an ulp being at most 2 u |value|: two sines or cosines of one
angle differ by at most T = 16 u (|value| <= 1), two arctangents of one argument by at most 18 u |value|.  From there on every
step is first order in u, doubled once at the end to cover the higher orders:
    lx, ly:   delta = (T + 6 u) (|dx| + |dy|)                      two products and a sum each
    d2:       D = 2 (|lx| + |ly|) delta + 6 u d2
    kappa:    dk = 2 delta / d2 + 2 |ly| D / d2^2 + 4 u |kappa|      (the clamp is 1-Lipschitz; |d2 - 1e-12| <= D: no bound)
    w:        dw = speed dk + 2 u |w|
    diff-drive:  (0, dw)                                             v = speed is exact
    tricycle, |v| >= 1e-6:  angle: L dw / v + 4 u |L w / v| + 18 u |angle|      (atan is 1-Lipschitz)
                            wheel speed: (T + 8 u) (|v| + |w L|) + L dw
    tricycle, v == 0:       w = +-0 on both sides, the angle 0 exactly; wheel speed as above
The box clip is 1-Lipschitz.  For diff_drive_control_to_tricycle alone (dd2tri_bound) dw = 0: the inputs are the same bits."""
import numpy as np

import lookahead_ref as LR

U = 2.0 ** -53
T = 16 * U


def gains_ok(speed, reach):
    return bool(np.isfinite(speed) and np.isfinite(reach) and speed >= 0 and reach > 0)


def carrot(pts, m, x, y, reach, c_prev, target_idx):
    """-> (j, dx, dy); pts [>= m, >= 2]"""
    j0 = min(max(int(c_prev), int(target_idx)), m - 1)
    r2 = np.float64(reach) * np.float64(reach)
    for j in range(j0, m):
        dx, dy = np.float64(pts[j, 0]) - x, np.float64(pts[j, 1]) - y
        if dx * dx + dy * dy >= r2:
            return j, dx, dy
    return m - 1, np.float64(pts[m - 1, 0]) - x, np.float64(pts[m - 1, 1]) - y


def normalize_angle(z):
    return (np.float64(z) + np.pi) % (2 * np.pi) - np.pi


def dd2tri(v, w, wheel_angle, max_wheel_angle, dist):
    """the contract's step 5 for the tricycle"""
    v, w, wheel_angle = np.float64(v), np.float64(w), np.float64(wheel_angle)
    if np.abs(v) < 1e-6:
        desired = np.sign(w) * max_wheel_angle
    else:
        desired = np.arctan(dist * w / v)
    desired = np.clip(desired, -max_wheel_angle, max_wheel_angle)
    fw = v * np.cos(wheel_angle) + w * dist * np.sin(wheel_angle)
    fw = max(fw, 0.)
    if np.abs(v) < 1e-6 and np.abs(normalize_angle(wheel_angle - desired)) > np.pi / 8:
        fw = 0.
    return np.float64(fw), np.float64(desired)


def dd2tri_bound(v, w, dist, angle):
    """-> (bound on the wheel speed, bound on the angle) between two faithful implementations on the same inputs"""
    b0 = 2 * (T + 8 * U) * (abs(v) + abs(w * dist))
    b1 = 0.0 if abs(v) < 1e-6 else 2 * 18 * U * abs(angle)
    return b0, b1


def curvature(lx, ly, max_curvature):
    d2 = lx * lx + ly * ly
    kappa = np.float64(0.0) if d2 < 1e-12 else 2 * ly / d2
    return np.clip(kappa, -max_curvature, max_curvature)


class Robot(object):
    """what the law needs to know of the handle"""

    def __init__(self, tricycle=True, max_wheel_angle=0.5 * 170 * np.pi / 180., dist=0.964):
        self.tricycle, self.max_wheel_angle, self.dist = tricycle, max_wheel_angle, dist


def law(pts, m, x, y, th, wheel_angle, target_idx, c_prev, speed, reach, max_curvature, low, high, robot, with_bound=False):
    """-> (carrot, cmd0, cmd1[, bound0, bound1])"""
    x, y, th, speed = np.float64(x), np.float64(y), np.float64(th), np.float64(speed)
    j, dx, dy = carrot(pts, m, x, y, reach, c_prev, target_idx)
    c, s = np.cos(th), np.sin(th)
    lx = c * dx + s * dy
    ly = -s * dx + c * dy
    kappa = curvature(lx, ly, max_curvature)
    v, w = speed, speed * kappa
    if robot.tricycle:
        a0, a1 = dd2tri(v, w, wheel_angle, robot.max_wheel_angle, robot.dist)
    else:
        a0, a1 = v, w
    cmd0, cmd1 = np.clip(a0, low[0], high[0]), np.clip(a1, low[1], high[1])
    if not with_bound:
        return j, cmd0, cmd1
    d2 = lx * lx + ly * ly
    delta = (T + 6 * U) * (abs(dx) + abs(dy))
    big_d = 2 * (abs(lx) + abs(ly)) * delta + 6 * U * d2
    if abs(d2 - 1e-12) <= big_d or (0 < speed < 1e-6):
        return j, cmd0, cmd1, np.inf, np.inf
    dk = 0.0 if d2 < 1e-12 else 2 * delta / d2 + 2 * abs(ly) * big_d / (d2 * d2) + 4 * U * abs(kappa)
    dw = speed * dk + 2 * U * abs(w)
    if not robot.tricycle:
        return j, cmd0, cmd1, 0.0, 2 * dw
    b0 = (T + 8 * U) * (abs(v) + abs(w * robot.dist)) + robot.dist * dw
    b1 = 0.0 if speed == 0 else robot.dist * dw / v + 4 * U * abs(robot.dist * w / v) + 18 * U * abs(a1)
    return j, cmd0, cmd1, 2 * b0, 2 * b1


def select_best(ret, reason, ok):
    """bcp_lookahead's key with a class below 'collided' for settings whose gains the law refuses; ties -> lowest k.
    ok: [K] or [N, K] bool"""
    ret = np.asarray(ret, np.float64)
    ok = np.broadcast_to(np.asarray(ok, bool), ret.shape)
    cls = np.where(ok, np.where((np.asarray(reason) & LR.DONE_COLLIDED) != 0, 0, 1), -1)
    best = np.zeros(ret.shape[0], np.int32)
    for i in range(ret.shape[0]):
        for k in range(1, ret.shape[1]):
            b = best[i]
            if (cls[i, k], ret[i, k]) > (cls[i, b], ret[i, b]):
                best[i] = k
    return best


def rollout(oracle, params, world, start, gains, horizon, max_curvature, low, high, robot, threads=8):
    """K settings per env rolled out with the law above and the oracle's step (as LR.oracle_lookahead steps it: no auto-reset,
    stop after the first done step).  gains [K, 2] or [N, K, 2].  -> dict(actions [N, K, H, 2], ret, steps, reason, final_pose,
    final_target_idx, trace [N, K, H, 6], best)"""
    n = start.n
    gains = np.asarray(gains, np.float64)
    if gains.ndim == 2:
        gains = np.broadcast_to(gains, (n,) + gains.shape)
    k = gains.shape[1]
    nk = n * k
    flat = gains.reshape(nk, 2)
    rep = lambda a: np.repeat(a, k, axis=-1)
    paths = np.asarray(world["paths"], dtype=np.float64)
    private = paths.ndim == 3 or np.asarray(world["costmaps"]).ndim == 3
    geom = None
    if private:
        geom = rep(start.geom if start.geom is not None else np.arange(n, dtype=np.int32))
    ob = oracle.OracleBatch(params, nk, world["costmaps"], world["origins"], world["resolution"], world["paths"],
                            lens=world.get("lens"), rows=world.get("rows"), cols=world.get("cols"), geom=geom)
    for f in range(7):
        ob.st[f][:] = rep(start.robot[f])
    ob.min_dist[:], ob.target_idx[:], ob.cur_iter[:], ob.collided[:] = (rep(start.min_dist), rep(start.target_idx),
                                                                        rep(start.cur_iter), rep(start.collided))
    ob.obs_pose[:] = np.stack(ob.st[:3], axis=1)
    ob.obs_state[:] = np.stack(ob.st, axis=1)

    def lane_path(c):
        if paths.ndim == 2:
            return paths, paths.shape[0]
        g = geom[c]
        return paths[g], int(world["lens"][g]) if world.get("lens") is not None else paths.shape[1]

    ok = np.array([gains_ok(*flat[c]) for c in range(nk)])
    actions, trace = np.zeros((nk, horizon, 2)), np.zeros((nk, horizon, 6))
    ret, steps, reason = np.zeros(nk), np.zeros(nk, np.int32), np.zeros(nk, np.uint8)
    final_pose, final_target = np.stack(ob.st[:3], axis=1).copy(), ob.target_idx.copy().astype(np.int32)
    running = ok.copy()
    c_prev = ob.target_idx.copy().astype(np.int64)
    cmd = np.zeros((nk, 2))
    for t in range(horizon):
        if not running.any():
            break
        for c in np.nonzero(running)[0]:
            pts, m = lane_path(c)
            state = [ob.st[0][c], ob.st[1][c], ob.st[2][c], ob.st[6][c] if robot.tricycle else 0.0, int(ob.target_idx[c])]
            j, c0, c1 = law(pts, m, state[0], state[1], state[2], state[3], state[4], c_prev[c], flat[c, 0], flat[c, 1],
                            max_curvature, low, high, robot)
            trace[c, t] = state + [j]
            c_prev[c] = j
            cmd[c] = (c0, c1)
            actions[c, t] = cmd[c]
        ob.step(cmd.copy(), None, auto_reset=False, threads=threads)
        ret[running] += ob.reward[running]
        steps[running] = t + 1
        pose = np.stack(ob.st[:3], axis=1)
        final_pose[running] = pose[running]
        final_target[running] = ob.target_idx[running]
        m_all = np.array([lane_path(c)[1] for c in range(nk)])
        goal = ob.target_idx > m_all - 1
        timeout = ob.cur_iter >= params.iteration_timeout
        why = (goal * LR.DONE_GOAL + timeout * LR.DONE_TIMEOUT + (ob.collided != 0) * LR.DONE_COLLIDED).astype(np.uint8)
        ends = running & (ob.done != 0)
        reason[ends] = why[ends]
        running &= ~ends
    for c in range(nk):
        actions[c, steps[c]:] = cmd[c]
    out = dict(actions=actions.reshape(n, k, horizon, 2), ret=ret.reshape(n, k), steps=steps.reshape(n, k),
               reason=reason.reshape(n, k), final_pose=final_pose.reshape(n, k, 3), final_target_idx=final_target.reshape(n, k),
               trace=trace.reshape(n, k, horizon, 6))
    out["best"] = select_best(out["ret"], out["reason"], ok.reshape(n, k))
    return out

"""Expectations for the look-ahead tests, made on the CPU oracle alone (no GPU, no product code): N * K oracle envs
stepped H times without auto-reset, rewards summed in step order until each candidate's first done step; the `best`
rule restated in numpy; windows of recorded reference trajectories; the scattered scenarios the GPU tests run."""
import os

import numpy as np

from util import GOLDEN, z_in

DONE_GOAL, DONE_TIMEOUT, DONE_COLLIDED = 1, 2, 4


def select_best(ret, reason):
    """Per env the candidate with the largest key (not collided, ret), compared lexicographically; ties -> lowest k."""
    ret = np.asarray(ret, dtype=np.float64)
    free = (np.asarray(reason) & DONE_COLLIDED) == 0
    best = np.zeros(ret.shape[0], dtype=np.int32)
    for i in range(ret.shape[0]):
        for k in range(1, ret.shape[1]):
            b = best[i]
            if (bool(free[i, k]), ret[i, k]) > (bool(free[i, b]), ret[i, b]):
                best[i] = k
    return best


class StartState(object):
    """State of N envs before the look-ahead: robot [7, N], min_dist, target_idx, cur_iter, collided [N], geom [N] or None"""

    def __init__(self, robot, min_dist, target_idx, cur_iter, collided=None, geom=None):
        self.robot = np.ascontiguousarray(robot, dtype=np.float64)
        n = self.robot.shape[1]
        self.min_dist = np.ascontiguousarray(min_dist, dtype=np.float64).reshape(n)
        self.target_idx = np.ascontiguousarray(target_idx, dtype=np.int32).reshape(n)
        self.cur_iter = np.ascontiguousarray(cur_iter, dtype=np.int32).reshape(n)
        self.collided = np.zeros(n, np.uint8) if collided is None else np.ascontiguousarray(collided, dtype=np.uint8).reshape(n)
        self.geom = None if geom is None else np.ascontiguousarray(geom, dtype=np.int32).reshape(n)

    @property
    def n(self):
        return self.robot.shape[1]


def oracle_lookahead(oracle, params, world, start, actions, z=None, threads=8):
    """world: dict(costmaps, origins, resolution, paths[, lens, rows, cols]) as OracleBatch takes them (private entries
    are indexed by env, or by start.geom); actions [H, K, 2] or [H, N, K, 2]; z None or [H, N, K, 3] (poisoned where
    the reference drew nothing).  Returns dict(ret, steps, reason, final_pose, final_target_idx, err) over [N, K]; err is the OR
    of the oracle's error word over the steps a candidate ran."""
    actions = np.asarray(actions, dtype=np.float64)
    n = start.n
    if actions.ndim == 3:
        actions = np.broadcast_to(actions[:, None], (actions.shape[0], n) + actions.shape[1:])
    h, _, k, _ = actions.shape
    nk = n * k
    rep = lambda a: np.repeat(a, k, axis=-1)
    private = np.asarray(world["paths"]).ndim == 3 or np.asarray(world["costmaps"]).ndim == 3
    geom = None
    if private:   # every oracle env names its entry: env i's own (no pool) or the pool entry it is on
        geom = rep(start.geom if start.geom is not None else np.arange(n, dtype=np.int32))
    ob = oracle.OracleBatch(params, nk, world["costmaps"], world["origins"], world["resolution"], world["paths"],
                            lens=world.get("lens"), rows=world.get("rows"), cols=world.get("cols"), geom=geom)
    for f in range(7):
        ob.st[f][:] = rep(start.robot[f])
    ob.min_dist[:], ob.target_idx[:], ob.cur_iter[:], ob.collided[:] = (rep(start.min_dist), rep(start.target_idx),
                                                                        rep(start.cur_iter), rep(start.collided))
    ob.obs_pose[:] = np.stack(ob.st[:3], axis=1)
    ob.obs_state[:] = np.stack(ob.st, axis=1)
    paths = np.asarray(world["paths"], dtype=np.float64)
    if paths.ndim == 2:
        m = np.full(nk, paths.shape[0], np.int64)
        last = np.broadcast_to(paths[-1, :2], (nk, 2))
    else:
        lens = np.asarray(world["lens"]) if world.get("lens") is not None else np.full(paths.shape[0], paths.shape[1])
        m = lens[geom].astype(np.int64)
        last = paths[geom, m - 1, :2]
    pure_pursuit = params.reward_provider == oracle.REWARD_PURE_PURSUIT
    ret, steps, reason = np.zeros(nk), np.zeros(nk, np.int32), np.zeros(nk, np.uint8)
    final_pose, final_target, errs = np.zeros((nk, 3)), np.zeros(nk, np.int32), np.zeros(nk, np.int32)
    running = np.ones(nk, bool)
    for t in range(h):
        if not running.any():
            break
        ob.step(actions[t].reshape(nk, 2), None if z is None else np.asarray(z[t], np.float64).reshape(nk, 3),
                auto_reset=False, threads=threads)
        ret[running] += ob.reward[running]          # (one addition per step, in step order)
        steps[running] = t + 1
        errs[running] |= ob.err[running]
        pose = np.stack(ob.st[:3], axis=1)
        final_pose[running] = pose[running]
        final_target[running] = ob.target_idx[running]
        if pure_pursuit:
            goal = np.hypot(last[:, 0] - pose[:, 0], last[:, 1] - pose[:, 1]) < 1.0
        else:
            goal = ob.target_idx > m - 1
        timeout = ob.cur_iter >= params.iteration_timeout
        why = (goal * DONE_GOAL + timeout * DONE_TIMEOUT + (ob.collided != 0) * DONE_COLLIDED).astype(np.uint8)
        assert ((why != 0) == (ob.done != 0)).all(), "the reason restates the oracle's done law"
        ends = running & (ob.done != 0)
        reason[ends] = why[ends]
        running &= ~ends
    out = dict(ret=ret.reshape(n, k), steps=steps.reshape(n, k), reason=reason.reshape(n, k),
               final_pose=final_pose.reshape(n, k, 3), final_target_idx=final_target.reshape(n, k), err=errs.reshape(n, k))
    out["best"] = select_best(out["ret"], out["reason"])
    return out


def shared_world(g):
    return dict(costmaps=g["costmap"], origins=g["origin"], resolution=float(g["resolution"]), paths=g["path"])


def recorded_windows(g, starts, horizon, noisy=True):
    """The recorded trajectory cut into windows: env j starts from the recorded state before step starts[j] and replays
    the recorded actions (and normals).  Returns (StartState, actions [H, N, 1, 2], z [H, N, 1, 3] or None)."""
    n = len(starts)
    robot, md, tgt, coll = np.zeros((7, n)), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    actions, z = np.zeros((horizon, n, 1, 2)), np.full((horizon, n, 1, 3), 1e300)
    total = len(g["actions"])
    for j, t0 in enumerate(starts):
        if t0 == 0:
            robot[:, j], md[j], tgt[j] = g["init_state"], float(g["init_min_dist"]), int(g["init_target_idx"])
        else:
            robot[:, j], md[j], tgt[j], coll[j] = g["states"][t0 - 1], g["min_dist"][t0 - 1], g["target_idx"][t0 - 1], g["collided"][t0 - 1]
        span = min(horizon, total - t0)
        actions[:span, j, 0] = g["actions"][t0:t0 + span]
        if noisy:
            z[:span, j, 0] = z_in(g["z"][t0:t0 + span])
    return StartState(robot, md, tgt, np.asarray(starts, np.int32), coll), actions, (z if noisy else None)


def recorded_expectation(g, starts, horizon):
    """What the recording itself says about those windows: steps, ret (added in step order), collided / done at the end,
    final pose, final target_idx"""
    steps, ret, done, coll = [], [], [], []
    pose, tgt = [], []
    for t0 in starts:
        s, r = 0, 0.0
        for t in range(t0, min(t0 + horizon, len(g["reward"]))):
            r += float(g["reward"][t])
            s += 1
            if g["done"][t]:
                break
        steps.append(s)
        ret.append(r)
        done.append(int(g["done"][t0 + s - 1]))
        coll.append(int(g["collided"][t0 + s - 1]))
        pose.append(g["states"][t0 + s - 1][:3])
        tgt.append(int(g["target_idx"][t0 + s - 1]))
    return dict(steps=np.array(steps, np.int32), ret=np.array(ret), done=np.array(done), collided=np.array(coll),
                final_pose=np.array(pose), final_target_idx=np.array(tgt, np.int32))


def random_library(rng, k, horizon):
    """k constant commands drawn uniformly from [0, 1.2] x [-1.3, 1.3], held for the whole horizon: [H, k, 2] float32"""
    cmd = np.stack([rng.uniform(0.0, 1.2, k), rng.uniform(-1.3, 1.3, k)], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(cmd, (horizon, k, 2)))


def mini_fixture():
    return np.load(os.path.join(GOLDEN, "g8_traj_mini_00.npz"))


def scenario_start(g, n, kind):
    """Start states on g8_traj_mini_00's world.  'scatter': the initial state kicked by sigma = 0.05 m / 0.6 rad
    (RandomState(5), as tests/test_gpu_rollout.py scatters its robots); 'timeout': the same with current_iter = 1170 of
    1200; 'goal': 8 way points before the path's end (target_idx = m - 8, pose on way point m - 9 plus sigma = 0.02 m /
    0.1 rad, RandomState(7))."""
    path = g["path"]
    m = len(path)
    robot = np.zeros((7, n))
    if kind in ("scatter", "timeout"):
        rng = np.random.RandomState(5)
        robot[:] = np.asarray(g["init_state"], np.float64)[:, None]
        robot[0:3] += np.concatenate([rng.normal(0, 0.05, (2, n)), rng.normal(0, 0.6, (1, n))])
        tgt = np.full(n, int(g["init_target_idx"]), np.int32)
        md = np.full(n, float(g["init_min_dist"]))
        it = np.full(n, 1170 if kind == "timeout" else 0, np.int32)
    else:
        rng = np.random.RandomState(7)
        robot[0:3] = path[m - 9][:, None] + np.concatenate([rng.normal(0, 0.02, (2, n)), rng.normal(0, 0.1, (1, n))])
        tgt = np.full(n, m - 8, np.int32)
        md = np.hypot(path[m - 8, 0] - robot[0], path[m - 8, 1] - robot[1])
        it = np.zeros(n, np.int32)
    return StartState(robot, md, tgt, it)

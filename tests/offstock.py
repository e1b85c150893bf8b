"""The parameter grid away from the stock point -- dt, tricycle dimensions, alphas, (spatial precision, angular precision,
progress multiplier), time-out -- and the batches that run on it.  tests/test_offstock_host.py steps them on the CPU oracle
alone and asserts that they are not vacuous; tests/test_gpu_offstock.py steps the same batches on the GPU and on the oracle
side by side.  Robot dimensions and alphas are read from tests/golden/g16_robot_step_params.npz (oracle/gen_golden.py made
them with the genuine reference): nothing is restated here."""
import os

import numpy as np

from util import ATOL, GOLDEN, random_batch, z_in

N_ENVS = 600        # two full 256-env workgroups and a tail of 88
STEPS = 32
AISLE_NAMES = ["g8_traj_aisle_c4_00.npz", "g8_traj_aisle_c4_10.npz", "g8_traj_aisle_c4_01.npz", "g8_traj_aisle_c4_11.npz"]
PLANENV_ALPHA = (0.0, 0.0, 1.e-2, 1.e-2, 1.e-3, 1.e-3)      # envs/base/env.py:228-231
MAX_FRONT_WHEEL_SPEED = 60. * np.pi / 180.                  # (the action box of PlanEnv is the stock robot's, env.py:237-240)

REACH_MID, REACH_TIGHT, REACH_WIDE = (0.35, np.pi / 3, 0.5), (0.05, 0.05, 0.0), (2.5, 3.2, 2.0)
ROWS = {
    1: dict(dt=0.1),
    2: dict(dt=0.02),
    3: dict(dt=1. / 30.),
    4: dict(robot="short"),
    5: dict(robot="long"),
    6: dict(alpha="all_six"),
    7: dict(reach=REACH_MID),
    8: dict(reach=REACH_TIGHT),
    9: dict(reach=REACH_WIDE),
    10: dict(iteration_timeout=3),
    11: dict(dt=0.1, robot="short", alpha="all_six", reach=REACH_MID),
    12: dict(dt=0.02, robot="long", dynamic_model=False, model_front_column_pid=False, reach=REACH_WIDE),
    # alpha1 alone, alpha2 alone: slot 0 is drawn (the host's `noise_slot0`) although slots 1 and 2 never are
    13: dict(alpha=(0.03, 0.0, 0.0, 0.0, 0.0, 0.0)),
    14: dict(alpha=(0.0, 0.02, 0.0, 0.0, 0.0, 0.0)),
}
# Seed of a (world, row) batch: 1600 + row unless listed here.  An entry is added under the straddle rule only (the GPU within
# ATOL of the oracle, the oracle itself within ATOL of the limit a flag sits on), with its evidence in the commit message.
SEEDS = {}

_cache = {}


def _golden(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name)))
    return _cache[name]


def robot_constants(robot):
    """dict of the six tricycle constants of g16's 'short' / 'long' robot"""
    g = _golden("g16_robot_step_params.npz")
    c = [i for i, nm in enumerate(g["names"]) if str(nm).startswith("tri-%s-" % robot)][0]
    return dict(zip([str(k) for k in g["constant_keys"]], g["constants"][c].tolist()))


def alpha_set(name):
    g = _golden("g16_robot_step_params.npz")
    c = [i for i, nm in enumerate(g["names"]) if str(nm).endswith("-" + name)][0]
    assert g["noise_on"][c]
    return tuple(g["alpha"][c].tolist())


class Config(object):
    """One grid row, resolved.  `reach` defaults to the world's own (sp, ap, multiplier)."""

    def __init__(self, row, default_reach, noise=True, model="tricycle"):
        spec = ROWS[row]
        self.row, self.model = row, model
        self.dt = spec.get("dt", 0.05)
        self.constants = robot_constants(spec["robot"]) if "robot" in spec and model == "tricycle" else None
        alpha = spec.get("alpha", PLANENV_ALPHA)
        self.alpha = None if not noise else (alpha_set(alpha) if isinstance(alpha, str) else alpha)
        self.sp, self.ap, self.mult = spec.get("reach", default_reach)
        self.iteration_timeout = spec.get("iteration_timeout", 1200)
        self.dynamic_model = spec.get("dynamic_model", True)
        self.model_front_column_pid = spec.get("model_front_column_pid", True)

    def oracle_params(self, oracle, noise=True):
        return oracle.make_params(self.model, dt=self.dt, noise=self.alpha if noise else None, iteration_timeout=self.iteration_timeout,
                                  spatial_precision=self.sp, angular_precision=self.ap, spatial_progress_multiplier=self.mult,
                                  dynamic_model=self.dynamic_model, model_front_column_pid=self.model_front_column_pid,
                                  **(self.constants or {}))

    def env_params(self, resolution):
        from bc_gym_planning_env_amd import EnvParams, RewardParams
        robot = 'industrial_tricycle_v1' if self.model == "tricycle" else 'industrial_diffdrive_v1'
        return EnvParams(dt=self.dt, goal_spat_dist=self.sp, goal_ang_dist=self.ap, iteration_timeout=self.iteration_timeout,
                         resolution=resolution, refine_path=False, robot_name=robot,
                         reward_provider_params=RewardParams(spatial_precision=self.sp, angular_precision=self.ap,
                                                             spatial_progress_multiplier=self.mult))

    def env_kwargs(self):
        noise = None if self.alpha is None else dict(("alpha%d" % (k + 1), self.alpha[k]) for k in range(6))
        return dict(noise_parameters=noise, robot_constants=self.constants, dynamic_model=self.dynamic_model,
                    model_front_column_pid=self.model_front_column_pid)


def action_box():
    from bc_gym_planning_env_amd import Box
    return Box(low=np.array([MAX_FRONT_WHEEL_SPEED / 10, -np.pi / 2]), high=np.array([MAX_FRONT_WHEEL_SPEED / 2, np.pi / 2]),
               dtype=np.float32)


class Batch(object):
    """N_ENVS envs of one world on one grid row: the oracle batch, the start state and the action stream, all from the row's
    seed.  world: 'mini' (shared map and path of g8_traj_mini_00, tricycle, noise), 'dd64' (diff-drive robot on the shared
    64 x 64 map, noise off), 'aisle' (private maps and paths: the four g8_traj_aisle_c4 templates, env i on template i % 4)."""

    def __init__(self, oracle, world, row, n=N_ENVS):
        self.world, self.row, self.n = world, row, n
        self.seed = SEEDS.get((world, row), 1600 + row)
        rng = self.rng = np.random.RandomState(self.seed)
        self.action_scale = 1.0
        if world == "mini":
            g = _golden("g8_traj_mini_00.npz")
            cfg = self.cfg = Config(row, (0.2, np.pi / 8, 0.0))
            self.res = float(g["resolution"])
            self.maps, self.origins, self.paths, self.lens = g["costmap"], g["origin"], g["path"], None
            tight = cfg.sp < 0.1    # (a tight goal is only ever reached from close by)
            start = random_batch(oracle, rng, n, g, None, timeout=cfg.iteration_timeout, xy_sigma=0.02 if tight else 0.15,
                                 th_sigma=0.02 if tight else 0.3)
        elif world == "dd64":
            from bc_gym_planning_env_amd import host_init
            g = _golden("g6_pose_collides.npz")
            cfg = self.cfg = Config(row, (0.2, np.pi / 8, 0.0), noise=False, model="diffdrive")
            self.res = float(g["mini64_res"])
            self.maps, self.origins, self.lens = g["mini64_map"], g["mini64_origin"], None
            self.paths = np.ascontiguousarray(host_init.refine_path(np.array([[-1.5, -1.0, 0.4], [1.2, 0.6, 0.9]]), 0.05))
            st = np.zeros((7, n))
            st[0:3] = self.paths[0][:, None]
            st[0] += rng.uniform(-0.5, 2.0, n)
            st[1] += rng.uniform(-0.5, 1.5, n)
            st[2] += rng.uniform(-1, 1, n)
            start = (st, None, None, np.zeros(n, np.int32))
        else:
            gs = [_golden(nm) for nm in AISLE_NAMES]
            cfg = self.cfg = Config(row, (1.0, np.pi / 2, 0.0))
            self.res = float(gs[0]["resolution"])
            self.templates = gs
            self.maps = np.stack([gs[i % 4]["costmap"] for i in range(n)])
            self.origins = np.stack([gs[i % 4]["origin"] for i in range(n)])
            self.paths = np.stack([gs[i % 4]["path"] for i in range(n)])
            self.lens = [self.paths.shape[1]] * n
            self.action_scale = 2.0
            st, md, tgt = np.zeros((7, n)), np.zeros(n), np.zeros(n, np.int32)
            tight = cfg.sp < 0.1
            for t in range(4):
                sel = np.arange(t, n, 4)
                s_, m_, t_, it = random_batch(oracle, rng, len(sel), gs[t], None, timeout=cfg.iteration_timeout,
                                              xy_sigma=0.02 if tight else 0.15, th_sigma=0.02 if tight else 0.3)
                st[:, sel], md[sel], tgt[sel] = s_, m_, t_
            start = (st, md, tgt, rng.randint(0, cfg.iteration_timeout, n).astype(np.int32))
        self.box = action_box()
        self.ref = oracle.OracleBatch(cfg.oracle_params(oracle), n, self.maps, self.origins, self.res, self.paths, lens=self.lens)
        self.ref.reset_from_paths()
        st, md, tgt, it = start
        self.start = (st, self.ref.min_dist.copy() if md is None else md, self.ref.target_idx.copy() if tgt is None else tgt, it)
        st, md, tgt, it = self.start
        for f in range(7):
            self.ref.st[f][:] = st[f]
        self.ref.min_dist[:], self.ref.target_idx[:], self.ref.cur_iter[:] = md, tgt, it
        self.oracle = oracle
        self.counts = dict(done=0, collided=0, advanced=0, timeout=0, drawn=np.zeros(3, np.int64))
        self.t = 0

    def next_actions(self):
        a = self.box.sample_batch(self.n, self.rng)
        a[:, 0] *= self.action_scale
        return a

    def step_oracle(self, actions, z=None, count_drawn=False):
        """One auto-reset step of the oracle.  z [n, 3]: the normals of this step, NaN where none was drawn (as the GPU hands
        them back); None: this batch has no noise, or (count_drawn) standard normals of the batch's own stream, with the slots
        the robot model really draws found by stepping each robot on its own."""
        ref, cfg = self.ref, self.cfg
        a64 = actions.astype(np.float64)
        if cfg.alpha is not None:
            if z is None:
                z = self.rng.standard_normal((self.n, 3))
                if count_drawn:
                    p = cfg.oracle_params(self.oracle)
                    st = np.stack(ref.st, axis=1)
                    bits = np.array([self.oracle.robot_step(p, st[i], a64[i], z[i])[2] for i in range(self.n)])
                    self.counts["drawn"] += [int(((bits >> k) & 1).sum()) for k in range(3)]
            else:
                self.counts["drawn"] += (~np.isnan(z)).sum(axis=0)
        before_iter, before_target = ref.cur_iter.copy(), ref.target_idx.copy()
        ref.step(a64, None if cfg.alpha is None else z_in(z), auto_reset=True, threads=8)
        done = ref.done != 0
        self.counts["done"] += int(done.sum())
        self.counts["collided"] += int(ref.collided_now.sum())
        self.counts["timeout"] += int((done & (before_iter + 1 >= cfg.iteration_timeout)).sum())
        # (an env that was reset shows its initial target again: a way point reached on the last step of an episode is not counted)
        self.counts["advanced"] += int((~done & (ref.target_idx > before_target)).sum())
        self.t += 1

    def assert_floors(self):
        """what the comparisons of a row rely on having happened"""
        c = self.counts
        tag = "%s row %d: %s" % (self.world, self.row, c)
        assert c["done"] >= 20 and c["collided"] >= 20 and c["advanced"] >= 10, tag
        if self.row == 10:
            assert c["timeout"] >= 500, tag
        if self.row == 6:
            assert (c["drawn"] >= 100).all(), tag
        if self.row in (13, 14):
            assert c["drawn"][0] >= 100 and c["drawn"][1] == c["drawn"][2] == 0, tag


# ---- the oracle's own margin to the limit a differing flag sits on (printed with a finding) ------------------------
def describe_flag_difference(batch, i, before_state, before_target, actions, z, gpu_state):
    """env i of `batch` differs from the GPU in a flag after the step just taken (before_*: ahead of that step; z: its
    normals, NaN = not drawn, or None).  Returns text with the pose the oracle's robot model proposed, how far the GPU's state is
    from the oracle's, and the oracle's margins: |distance - sp| and | |heading difference| - ap | to the way points from the
    old target on, and whether the collision verdict changes within +-ATOL of the proposed pose (a lethal cell under the
    footprint's edge)."""
    ref, cfg, oracle = batch.ref, batch.cfg, batch.oracle
    p = cfg.oracle_params(oracle)
    zi = None if (z is None or cfg.alpha is None) else z_in(z[i])
    pose = oracle.robot_step(p, before_state[:, i], actions[i].astype(np.float64), zi)[0][:3]
    path = batch.paths if np.ndim(batch.paths) == 2 else batch.paths[i]
    cm = batch.maps if np.ndim(batch.maps) == 2 else batch.maps[i]
    org = batch.origins if np.ndim(batch.origins) == 1 else batch.origins[i]
    tail = path[int(before_target[i]):]
    now = np.array([ref.st[f][i] for f in range(7)])
    out = ["env %d step %d (seed %d): proposed pose %r, max |GPU - oracle| state %.3g" % (
        i, batch.t - 1, batch.seed, pose.tolist(), np.abs(gpu_state[:, i] - now).max())]
    if len(tail):
        dist = np.hypot(tail[:, 0] - pose[0], tail[:, 1] - pose[1])
        ang = np.abs((tail[:, 2] - pose[2] + np.pi) % (2 * np.pi) - np.pi)
        out.append("margin to sp %.3g, to ap %.3g" % (np.abs(dist - cfg.sp).min(), np.abs(ang - cfg.ap).min()))
    fp = oracle.footprint_of(p)
    c, s = np.cos(pose[2]), np.sin(pose[2])
    verdicts = [oracle.pose_collides(pose[0] + dx * c - dy * s, pose[1] + dx * s + dy * c, pose[2] + da, fp, cm, org, batch.res)
                for dx in (-ATOL, 0.0, ATOL) for dy in (-ATOL, 0.0, ATOL) for da in (-ATOL, 0.0, ATOL)]
    out.append("collision verdict within +-ATOL of the proposed pose: %s" % (
        "mixed (a lethal cell under the footprint's edge)" if len(set(verdicts)) > 1 else verdicts[0]))
    return "; ".join(out)

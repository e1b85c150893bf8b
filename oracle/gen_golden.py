#!/usr/bin/env python
"""Generate tests/golden/*.npz from the GENUINE reference, imported in the build container through
oracle/ref_harness.py.  Run from the repo root:  python oracle/gen_golden.py

The fixtures are data only (inputs + expected outputs).  Nothing here travels as reference source.
Fixture list:
  g1_tricycle_step.npz      TricycleRobot.step, noise off          (tricycle_model.py:478-538)
  g2_tricycle_step_noise.npz  same with noise, normals in slot form  (differential_drive.py:55-74)
  g3_diffdrive_step.npz     DiffDriveRobot.step with/without noise (differential_drive.py:236-265)
  g4_scalar_utils.npz       normalize_angle / world_to_pixel / path_velocity incl. the reference's KAT values
  g5_footprint_vertices.npz pre-fill output of get_pixel_footprint (integer polygon + half size)
  g6_pose_collides.npz      pose_collides verdicts on random poses (fill = oracle restatement, see harness note)
  g7_reward.npz             ContinuousRewardProvider traces
  g8_traj_*.npz             full PlanEnv.step trajectories (RandomMiniEnv seeds, AisleTurnEnv variants)
  g9 .. g12                 RandomMiniEnv worlds, egocentric observations, delays / pure pursuit, coloured ego costmap
  g13_serialized_*.npz      PlanEnv.serialize() records taken mid-episode + the next 100 steps of the live env
  g16_robot_step_params.npz, g16_traj_*.npz   robot steps and PlanEnv trajectories away from the stock parameters: other dt,
                            other tricycle dimensions, other alphas, other reward parameters, a short time-out
  g15_footprint_zoo.npz     the footprint zoo of tests/footprints.py: pre-fill polygons, scaled stock footprints and
                            pose_collides verdicts on the g6 maps   (python oracle/gen_golden.py footprint_zoo)
  g17_headings.npz          robot steps from headings up to 50 turns outside [-pi, pi) -- with a `raised` flag where path_velocity
                            raised -- and two PlanEnv trajectories on paths whose angles are shifted by whole turns
                            (python oracle/gen_golden.py headings; written with fixed time stamps: a re-run is byte-identical)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle as O  # noqa: E402
from oracle import ref_harness as H  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    print("wrote %-32s %7.1f KiB" % (name, os.path.getsize(path) / 1024.))


class SlotTap(object):
    """Records the standard normals consumed by one noisy motion step in SLOT form (slot = index of the
    _gaussian_noise call inside kinematic_body_pose_motion_step_with_noise; NaN = not drawn)."""

    def __init__(self, dd_module, seed):
        self.dd = dd_module
        self.tap = H.NoiseTap(seed)
        self.slots = []
        self._orig = None

    def __enter__(self):
        self.tap.__enter__()
        self._orig = self.dd._gaussian_noise
        orig = self._orig
        tap = self.tap
        slots = self.slots

        def counting(variance):
            before = len(tap.calls)
            r = orig(variance)
            slots.append(tap.calls[-1] if len(tap.calls) > before else np.nan)
            return r
        self.dd._gaussian_noise = counting
        return self

    def __exit__(self, *exc):
        self.dd._gaussian_noise = self._orig
        self.tap.__exit__(*exc)
        return False

    def take(self):
        assert len(self.slots) in (0, 3), self.slots
        out = np.array(self.slots if self.slots else [np.nan] * 3, dtype=np.float64)
        del self.slots[:]
        del self.tap.calls[:]
        return out


def tri_state_vec(s):
    return np.array([s.x, s.y, s.angle, s.v, s.w, s.steering_motor_command, s.wheel_angle], dtype=np.float64)


def dd_state_vec(s):
    return np.array([s.x, s.y, s.angle, s.v, s.w, 0.0, 0.0], dtype=np.float64)


def random_robot_inputs(rng, n, tricycle):
    st = np.zeros((n, 7))
    st[:, 0:2] = rng.uniform(-3, 3, (n, 2))
    st[:, 2] = rng.uniform(-np.pi, np.pi, n)
    st[:, 3] = rng.uniform(-0.2, 1.2, n) * (rng.rand(n) > 0.1)
    st[:, 4] = rng.uniform(-1.0, 1.0, n) * (rng.rand(n) > 0.1)
    if tricycle:
        st[:, 6] = rng.uniform(-1.6, 1.6, n)
    cmd = np.stack([rng.uniform(-0.2, 1.5, n), rng.uniform(-2.0, 2.0, n)], axis=1)
    # a share of float32 commands, as action_space.sample() produces (envs/base/spaces.py:134-141)
    f32 = rng.rand(n) < 0.5
    cmd[f32] = cmd[f32].astype(np.float32).astype(np.float64)
    # angles right at the wrap-around
    st[:16, 2] = np.pi - 1e-9 * np.arange(16)
    st[16:32, 2] = -np.pi + 1e-9 * np.arange(16)
    cmd[32:40] = 0.0
    return st, cmd, f32


def gen_robot_steps():
    from bc_gym_planning_env.robot_models import differential_drive as dd
    from bc_gym_planning_env.robot_models.tricycle_model import TricycleRobot, TricycleRobotState
    from bc_gym_planning_env.robot_models.differential_drive import DiffDriveRobot, DiffdriveRobotState
    from bc_gym_planning_env.robot_models.robot_dimensions_examples import get_dimensions_example
    from bc_gym_planning_env.envs.base.action import Action
    tri_dims = get_dimensions_example('industrial_tricycle_v1')
    dd_dims = get_dimensions_example('industrial_diffdrive_v1')
    dt = 0.05

    def run_tricycle(st, cmd, f32, noise, seed, dynamic=True, pid=True):
        n = len(st)
        out = np.zeros((n, 7))
        z = np.full((n, 3), np.nan)
        robot = TricycleRobot(dimensions=tri_dims, noise_parameters=noise, dynamic_model=dynamic,
                              model_front_column_pid=pid)
        with SlotTap(dd, seed) as tap:
            for i in range(n):
                robot.set_state(TricycleRobotState(x=st[i, 0], y=st[i, 1], angle=st[i, 2], v=st[i, 3], w=st[i, 4],
                                                   steering_motor_command=st[i, 5], wheel_angle=st[i, 6]))
                c = cmd[i].astype(np.float32) if f32[i] else cmd[i]
                robot.step(dt, Action(command=c))
                out[i] = tri_state_vec(robot.get_state())
                z[i] = tap.take()
        return out, z

    rng = np.random.RandomState(101)
    st, cmd, f32 = random_robot_inputs(rng, 2048, True)
    out, _ = run_tricycle(st, cmd, f32, None, 1)
    save("g1_tricycle_step.npz", state=st, cmd=cmd, dt=dt, out=out)
    # kinematic-only / no front-column PID variants (tricycle_model.py:38-68, :61, :110)
    outs = {}
    for name, (dyn, pid) in dict(kin_pid=(False, True), kin_nopid=(False, False), dyn_nopid=(True, False)).items():
        # without the front-column PID a float32 command stays float32 through np.clip/np.cos (a dtype artefact of
        # a mode PlanEnv never enables, tricycle_model.py:61,110): those variants are pinned on float64 commands.
        outs[name], _ = run_tricycle(st[:512], cmd[:512], f32[:512] & pid, None, 1, dynamic=dyn, pid=pid)
    save("g1b_tricycle_variants.npz", state=st[:512], cmd=cmd[:512], dt=dt, **outs)

    rng = np.random.RandomState(102)
    st, cmd, f32 = random_robot_inputs(rng, 2048, True)
    alphas = np.array([O.PLANENV_NOISE, (1e-2, 1e-3, 1e-2, 1e-2, 1e-3, 1e-3), (0.05, 0.0, 0.0, 0.02, 0.0, 0.01),
                       (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)])
    outs, zs, aidx = [], [], []
    for a_i, a in enumerate(alphas):
        noise = dict(("alpha%d" % (k + 1), a[k]) for k in range(6))
        sl = slice(a_i * 512, (a_i + 1) * 512)
        o, z = run_tricycle(st[sl], cmd[sl], f32[sl], noise, 200 + a_i)
        outs.append(o)
        zs.append(z)
        aidx.append(np.full(512, a_i))
    save("g2_tricycle_step_noise.npz", state=st, cmd=cmd, dt=dt, alphas=alphas, alpha_idx=np.concatenate(aidx),
         z=np.concatenate(zs), out=np.concatenate(outs))

    # DiffDriveRobot.step: noise off only -- with noise the reference itself raises IndexError
    # (differential_drive.py:73 indexes a 1-D pose with [:, 2]), so there is nothing to pin.
    rng = np.random.RandomState(103)
    st, cmd, f32 = random_robot_inputs(rng, 2048, False)
    st[:, 5:] = 0.0
    robot = DiffDriveRobot(dimensions=dd_dims, noise_parameters=None)
    o = np.zeros((2048, 7))
    for i in range(2048):
        robot.set_state(DiffdriveRobotState(x=st[i, 0], y=st[i, 1], angle=st[i, 2], v=st[i, 3], w=st[i, 4]))
        # The command VALUES are float32-representable for half the rows but are handed over as float64: the
        # diff-drive model does scalar arithmetic on the command (differential_drive.py:34-35), which numpy 1.x
        # (the reference's era, value-based promotion) performs in float64 and numpy >= 2 (NEP 50) in float32.
        # The build follows the numpy 1.x semantics: commands are widened to float64 first.
        robot.step(dt, Action(command=cmd[i]))
        o[i] = dd_state_vec(robot.get_state())
    save("g3_diffdrive_step.npz", state=st, cmd=cmd, dt=dt, out=o)


def gen_scalar_utils():
    from bc_gym_planning_env.utilities.coordinate_transformations import normalize_angle, world_to_pixel, diff_angles
    from bc_gym_planning_env.utilities.path_tools import path_velocity, pose_distances
    rng = np.random.RandomState(104)
    # normalize_angle: KAT inputs of test_coordinate_transformations.py:32-83 plus random / boundary values
    kat = np.array([0., 1., -1., np.pi, -np.pi, 3 * np.pi, -3 * np.pi, 2 * np.pi, -2 * np.pi, 4 * np.pi, 0.5 * np.pi,
                    -0.5 * np.pi, 1.5 * np.pi, -1.5 * np.pi, 2.5 * np.pi, 100., -100., 1e-12, -1e-12,
                    np.pi + 1e-12, -np.pi - 1e-12, np.nextafter(np.pi, 4), np.nextafter(-np.pi, -4)])
    na_in = np.concatenate([kat, rng.uniform(-30, 30, 4096), rng.uniform(-np.pi, np.pi, 1024)])
    na_out = normalize_angle(na_in)
    da_a, da_b = rng.uniform(-7, 7, 2048), rng.uniform(-7, 7, 2048)
    da_out = diff_angles(da_a, da_b)
    # world_to_pixel: the KAT cases of test_coordinate_transformations.py:1544-1649 (half-to-even and
    # multiply-by-reciprocal) + random
    w2p_cases = []
    for xy, origin, res in [
        (np.array([[0., 0.], [1., 1.], [2.5, 3.5], [-1.5, -0.5], [0.025, 0.075]]), np.array([0., 0.]), 0.05),
        (np.array([[0.5, 1.5], [2.5, 3.5], [-0.5, -1.5]]), np.array([0., 0.]), 1.0),
        (np.array([[1.45, 2.85], [0.15, 0.25], [0.35, 0.45]]), np.array([-0.3, 0.1]), 0.1),
        (np.array([[4.35, 0.29], [0.57, 1.14]]), np.array([0., 0.]), 0.03),
        (rng.uniform(-5, 5, (2048, 2)), np.array([-2.75, -2.75]), 0.03),
        (rng.uniform(-5, 5, (1024, 2)), np.array([-3.1, 1.7]), 5.5 / 64),
        (np.round(rng.uniform(-100, 100, (1024, 2))) * 0.015, np.array([0., 0.]), 0.03),  # many exact halves
    ]:
        w2p_cases.append((xy, origin, res, world_to_pixel(xy, origin, res)))
    # path_velocity two-row cases (as called from the robot models)
    n = 2048
    p0 = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-np.pi, np.pi, n)], axis=1)
    d = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    d[:64, :2] = 0.0                    # no motion: sign() == 0 path
    d[64:128, 0] = 0.0
    p0[128:192, 2] = np.pi - 0.01       # wrap-around of the angle difference
    d[128:192, 2] = 0.05
    p1 = p0 + d
    p1[:, 2] = normalize_angle(p1[:, 2])
    pv = np.zeros((n, 2))
    for i in range(n):
        v, w = path_velocity(np.vstack([np.hstack([0., p0[i]]), np.hstack([0.05, p1[i]])]))
        pv[i] = v[0], w[0]
    a, b = p0.copy(), p1.copy()
    pd_lin, pd_ang = pose_distances(a, b)
    save("g4_scalar_utils.npz", na_in=na_in, na_out=na_out, da_a=da_a, da_b=da_b, da_out=da_out,
         pv_p0=p0, pv_p1=p1, pv_dt=0.05, pv_out=pv, pd_lin=pd_lin, pd_ang=pd_ang,
         **dict(("w2p%d_%s" % (i, k), v) for i, c in enumerate(w2p_cases)
                for k, v in zip(("xy", "origin", "res", "out"), c)))


def gen_footprints():
    import cv2  # the harness stub
    from bc_gym_planning_env.utilities.path_tools import get_pixel_footprint
    rng = np.random.RandomState(105)
    captured = {}
    orig_fill = cv2.fillPoly

    def capture(img, pts, color, *a, **k):
        captured["shape"] = img.shape
        captured["pts"] = np.array(pts[0], dtype=np.int32)
        return orig_fill(img, pts, color, *a, **k)
    cv2.fillPoly = capture
    try:
        out = {}
        for fname, fp in (("tri", O.TRICYCLE_FOOTPRINT), ("dd", O.DIFFDRIVE_FOOTPRINT)):
            for rname, res in (("r003", 0.03), ("r64", 5.5 / 64), ("r256", 10. / 256)):
                angles = np.concatenate([rng.uniform(-np.pi, np.pi, 2000),
                                         np.arange(-8, 9) * np.pi / 8, rng.uniform(-10, 10, 31)])
                pts = np.zeros((len(angles), len(fp), 2), dtype=np.int32)
                shapes = np.zeros((len(angles), 2), dtype=np.int32)
                area = np.zeros(len(angles), dtype=np.int32)
                for i, a in enumerate(angles):
                    kern = get_pixel_footprint(a, fp, res)
                    pts[i] = captured["pts"]
                    shapes[i] = captured["shape"]
                    area[i] = np.count_nonzero(kern)
                key = "%s_%s" % (fname, rname)
                out[key + "_angles"] = angles
                out[key + "_pts"] = pts
                out[key + "_shape"] = shapes
                out[key + "_area"] = area  # area depends on the (unpinned) fill; informational
                out[key + "_res"] = res
        save("g5_footprint_vertices.npz", **out)
    finally:
        cv2.fillPoly = orig_fill


class _FootprintOnly(object):
    """All that pose_collides asks of a robot"""

    def __init__(self, footprint):
        self._footprint = np.array(footprint, dtype=np.float64)

    def get_footprint(self):
        return self._footprint


def gen_footprint_zoo():
    """The zoo of tests/footprints.py (the shapes are imported from there, nothing is restated here) through the genuine
    get_pixel_footprint (what it hands to cv2.fillPoly), create_standard_robot(..., footprint_scale=s).get_footprint()
    and envs.base.env.pose_collides on the maps of g6."""
    import cv2  # the harness stub
    from bc_gym_planning_env.envs.base.env import pose_collides
    from bc_gym_planning_env.robot_models.robot_examples_factory import create_standard_robot
    from bc_gym_planning_env.utilities.costmap_2d import CostMap2D
    from bc_gym_planning_env.utilities.path_tools import get_pixel_footprint
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import footprints as F
    g6 = np.load(os.path.join(OUT, "g6_pose_collides.npz"))
    rng = np.random.RandomState(115)
    captured = {}
    orig_fill = cv2.fillPoly

    def capture(img, pts, color, *a, **k):
        captured["shape"] = img.shape
        captured["pts"] = np.array(pts[0], dtype=np.int32)
        return orig_fill(img, pts, color, *a, **k)
    out = {"names": np.array(sorted(F.ZOO))}
    for stock, (robot_name, _) in sorted(F.STOCK.items()):
        for s in F.SCALES:
            out["scaled_%s_x%g" % (stock, s)] = np.array(create_standard_robot(robot_name, footprint_scale=s).get_footprint())
    cv2.fillPoly = capture
    try:
        for name in sorted(F.ZOO):
            fp = F.ZOO[name]
            rs = F.resolutions(name)
            out[name + "_res"] = np.array(rs)
            for ri, res in enumerate(rs):
                angles = np.concatenate([rng.uniform(-np.pi, np.pi, 24), F.angle_set(0, 0)])
                pts = np.zeros((len(angles), len(fp), 2), dtype=np.int32)
                shapes = np.zeros((len(angles), 2), dtype=np.int32)
                for i, a in enumerate(angles):
                    get_pixel_footprint(a, fp, res)
                    pts[i], shapes[i] = captured["pts"], captured["shape"]
                key = "%s_r%d" % (name, ri)
                out[key + "_angles"], out[key + "_pts"], out[key + "_shape"] = angles, pts, shapes
    finally:
        cv2.fillPoly = orig_fill
    n = 1500
    for tag in ("mini0", "mini3", "mini64"):
        res = float(g6[tag + "_res"])
        costmap = CostMap2D(g6[tag + "_map"].copy(), res, g6[tag + "_origin"].copy())
        # the same poses for every footprint; the rim lets an image lie partly or wholly off the map
        poses = np.stack([rng.uniform(-4.6, 4.6, n), rng.uniform(-4.6, 4.6, n), rng.uniform(-np.pi, np.pi, n)], axis=1)
        out[tag + "_poses"] = poses
        for name in sorted(F.ZOO):
            robot = _FootprintOnly(F.ZOO[name])
            verdict = np.array([pose_collides(p[0], p[1], p[2], robot, costmap) for p in poses], dtype=np.uint8)
            out["%s_%s_collides" % (name, tag)] = np.packbits(verdict)
            print("   %-16s %s: %d/%d collide" % (name, tag, verdict.sum(), n))
    save("g15_footprint_zoo.npz", **out)


def make_mini_env(seed, resolution=0.03, robot_name=None):
    from bc_gym_planning_env.envs.mini_env import RandomMiniEnv, RandomMiniEnvParams
    from bc_gym_planning_env.envs.base.params import EnvParams
    kw = dict(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, resolution=resolution)
    if robot_name is not None:
        kw["robot_name"] = robot_name
    params = RandomMiniEnvParams(env_params=EnvParams(**kw))
    return RandomMiniEnv(params=params, rng=np.random.RandomState(seed), draw_new_turn_on_reset=False)


def gen_pose_collides():
    from bc_gym_planning_env.envs.base.env import pose_collides
    from bc_gym_planning_env.robot_models.tricycle_model import TricycleRobot
    from bc_gym_planning_env.robot_models.differential_drive import DiffDriveRobot
    from bc_gym_planning_env.robot_models.robot_dimensions_examples import get_dimensions_example
    rng = np.random.RandomState(106)
    out = {}
    for tag, seed, res, robot in (("mini0", 0, 0.03, "tri"), ("mini3", 3, 0.03, "tri"), ("mini64", 0, 5.5 / 64, "dd")):
        env = make_mini_env(seed, res)
        costmap = env._env._state.costmap
        robot_obj = (TricycleRobot(dimensions=get_dimensions_example('industrial_tricycle_v1')) if robot == "tri"
                     else DiffDriveRobot(dimensions=get_dimensions_example('industrial_diffdrive_v1')))
        n = 1500
        poses = np.stack([rng.uniform(-3.6, 3.6, n), rng.uniform(-3.6, 3.6, n), rng.uniform(-np.pi, np.pi, n)], axis=1)
        verdict = np.array([pose_collides(p[0], p[1], p[2], robot_obj, costmap) for p in poses], dtype=np.uint8)
        out[tag + "_map"] = costmap.get_data().copy()
        out[tag + "_origin"] = np.array(costmap.get_origin())
        out[tag + "_res"] = costmap.get_resolution()
        out[tag + "_poses"] = poses
        out[tag + "_collides"] = verdict
        out[tag + "_robot"] = np.array(0 if robot == "tri" else 1)
        print("   %s: %d/%d collide" % (tag, verdict.sum(), n))
    save("g6_pose_collides.npz", **out)


def gen_reward():
    from bc_gym_planning_env.envs.base.reward import ContinuousRewardProvider, RewardParams
    from bc_gym_planning_env.utilities.path_tools import refine_path
    rng = np.random.RandomState(107)
    out = {}
    for tag, (sp, ap, mult) in dict(a=(0.2, np.pi / 8, 0.0), b=(1.0, np.pi / 2, 0.0), c=(0.3, 0.5, 2.5)).items():
        coarse = np.array([[0., 0., 0.3], [1.5, 0.5, 0.3], [2.5, 2.0, 1.2], [2.5, 3.5, np.pi / 2]])
        path = refine_path(coarse, 0.05)
        params = RewardParams(spatial_precision=sp, angular_precision=ap, spatial_progress_multiplier=mult)
        prov = ContinuousRewardProvider(params=params)
        prov.set_state(ContinuousRewardProvider.generate_initial_state(path, params))
        init = prov.get_state()

        class S(object):
            pass
        # a noisy walk along the path (sometimes jumping back / far away)
        n = 600
        idx = np.clip((np.arange(n) * len(path) / 500.).astype(int) + rng.randint(-3, 4, n), 0, len(path) - 1)
        poses = path[idx] + np.stack([rng.normal(0, 0.05, n), rng.normal(0, 0.05, n), rng.normal(0, 0.15, n)], axis=1)
        poses[::37] += np.array([1.0, -1.0, 0.5])
        rew = np.zeros(n)
        md = np.zeros(n)
        ti = np.zeros(n, dtype=np.int32)
        for i in range(n):
            s = S()
            s.pose = poses[i]
            rew[i] = prov.reward(s)
            st = prov.get_state()
            md[i], ti[i] = st.min_spat_dist_so_far, st.target_idx
        out.update({tag + "_path": path, tag + "_params": np.array([sp, ap, mult]), tag + "_poses": poses,
                    tag + "_reward": rew, tag + "_min_dist": md, tag + "_target_idx": ti,
                    tag + "_init": np.array([init.min_spat_dist_so_far, init.target_idx])})
    save("g7_reward.npz", **out)


def record_trajectory(env, plan_env, n_steps, action_seed, noise_seed, robot_kind="tri"):
    """Drive the reference PlanEnv with action_space.sample() actions and record everything."""
    from bc_gym_planning_env.robot_models import differential_drive as dd
    from bc_gym_planning_env.envs.base import spaces
    spaces.SPACE_LOCAL_RANDOM_STATE.seed(action_seed)
    state0 = plan_env.get_state()
    rs = state0.robot_state
    rec = dict(
        costmap=state0.costmap.get_data().copy(), origin=np.array(state0.costmap.get_origin()),
        resolution=np.float64(state0.costmap.get_resolution()),
        path=np.array(state0.reward_provider_state.path), init_target_idx=np.int32(state0.reward_provider_state.target_idx),
        init_min_dist=np.float64(state0.reward_provider_state.min_spat_dist_so_far),
        init_state=tri_state_vec(rs) if robot_kind == "tri" else dd_state_vec(rs),
    )
    T = n_steps
    act = np.zeros((T, 2))
    z = np.full((T, 3), np.nan)
    st = np.zeros((T, 7))
    rew = np.zeros(T)
    done = np.zeros(T, dtype=np.uint8)
    coll = np.zeros(T, dtype=np.uint8)
    tidx = np.zeros(T, dtype=np.int32)
    mind = np.zeros(T)
    tm = np.zeros(T)
    obs_path_len = np.zeros(T, dtype=np.int32)
    with SlotTap(dd, noise_seed) as tap:
        for t in range(T):
            a = env.action_space.sample()
            act[t] = a.command.astype(np.float64)
            assert a.command.dtype == np.float32
            obs, r, d, _ = env.step(a)
            z[t] = tap.take()
            s = plan_env._state
            st[t] = tri_state_vec(s.robot_state) if robot_kind == "tri" else dd_state_vec(s.robot_state)
            assert (obs.pose == st[t, :3]).all()
            rew[t], done[t], coll[t] = r, d, s.robot_collided
            tidx[t] = s.reward_provider_state.target_idx
            mind[t] = s.reward_provider_state.min_spat_dist_so_far
            tm[t] = obs.time
            obs_path_len[t] = len(obs.path)
    rec.update(actions=act, z=z, states=st, reward=rew, done=done, collided=coll, target_idx=tidx, min_dist=mind,
               time=tm, obs_path_len=obs_path_len)
    return rec


def gen_trajectories():
    from bc_gym_planning_env.envs.synth_turn_env import AisleTurnEnv, AisleTurnEnvParams, TurnParams
    from bc_gym_planning_env.envs.base.params import EnvParams
    # RandomMiniEnv (metric config): 24 seeds x 400 steps, tricycle, PlanEnv's default noise
    for seed in range(24):
        env = make_mini_env(seed)
        rec = record_trajectory(env, env._env, 400, action_seed=1000 + seed, noise_seed=2000 + seed)
        save("g8_traj_mini_%02d.npz" % seed, **rec)
    # noise off (set_noise_parameters(None), tricycle_model.py:575-579), runs to the timeout
    for seed in (40, 41):
        env = make_mini_env(seed)
        env._env._robot.set_noise_parameters(None)
        rec = record_trajectory(env, env._env, 1250, action_seed=1000 + seed, noise_seed=2000 + seed)
        save("g8_traj_mini_nonoise_%02d.npz" % seed, **rec)
    # AisleTurnEnv variants: default res, and the C4 config (res 10/256, flips)
    variants = [("default", dict(), dict()),
                ("c4_00", dict(resolution=10. / 256), dict()),
                ("c4_10", dict(resolution=10. / 256), dict(flip_arnd_oy=True)),
                ("c4_01", dict(resolution=10. / 256), dict(flip_arnd_ox=True)),
                ("c4_11", dict(resolution=10. / 256), dict(flip_arnd_oy=True, flip_arnd_ox=True))]
    for i, (tag, ekw, tkw) in enumerate(variants):
        env = AisleTurnEnv(AisleTurnEnvParams(env_params=EnvParams(**ekw), turn_params=TurnParams(**tkw)))
        rec = record_trajectory(env, env, 500, action_seed=3000 + i, noise_seed=4000 + i)
        save("g8_traj_aisle_%s.npz" % tag, **rec)


def gen_diffdrive_trajectories():
    """C2 shape: PlanEnv hard-codes the tricycle, so the diff-drive robot is driven the way SURVEY 8(a9) says:
    _env_step(costmap, DiffDriveRobot, dt, action) (envs/base/env.py:442-461) + the reward provider, by hand, with
    the bookkeeping of PlanEnv._resolve_state_transition / step (env.py:334-398)."""
    from bc_gym_planning_env.envs.base.env import _env_step
    from bc_gym_planning_env.envs.base.action import Action
    from bc_gym_planning_env.envs.base.reward import ContinuousRewardProvider, RewardParams
    from bc_gym_planning_env.robot_models.differential_drive import DiffDriveRobot
    from bc_gym_planning_env.robot_models.robot_dimensions_examples import get_dimensions_example
    from bc_gym_planning_env.utilities.path_tools import refine_path
    for seed, toward_wall in ((0, False), (5, False), (3, True), (9, True)):
        env = make_mini_env(seed, resolution=5.5 / 64)
        costmap = env._env._state.costmap
        path = np.array(env._env._state.original_path)
        rng = np.random.RandomState(900 + seed)
        robot = DiffDriveRobot(dimensions=get_dimensions_example('industrial_diffdrive_v1'), noise_parameters=None)
        rp = RewardParams(spatial_precision=0.2, angular_precision=np.pi / 8)
        prov = ContinuousRewardProvider(params=rp)
        prov.set_state(ContinuousRewardProvider.generate_initial_state(path, rp))
        init = prov.get_state()
        robot.set_pose(*path[0])
        if toward_wall:  # start 1.4 m in front of a lethal cell, heading at it: collisions and rollbacks for sure
            ly, lx = np.nonzero(costmap.get_data() == 254)
            k = len(ly) // 2
            wx = costmap.get_origin()[0] + lx[k] * costmap.get_resolution()
            wy = costmap.get_origin()[1] + ly[k] * costmap.get_resolution()
            th0 = 0.3 + seed
            robot.set_pose(wx - 1.4 * np.cos(th0), wy - 1.4 * np.sin(th0), np.arctan2(np.sin(th0), np.cos(th0)))
        start_state = dd_state_vec(robot.get_state())

        class S(object):
            pass
        T = 500
        act = np.zeros((T, 2)); st = np.zeros((T, 7)); rew = np.zeros(T); done = np.zeros(T, np.uint8)
        coll = np.zeros(T, np.uint8); tidx = np.zeros(T, np.int32); mind = np.zeros(T)
        collided = False
        for t in range(T):
            # (v, w): mostly forward, float32-representable values handed over as float64 (see gen_robot_steps)
            a = np.array([rng.uniform(0.1, 0.6), rng.uniform(-1.2, 1.2) * (0.15 if toward_wall else 1.0)])
            a = a.astype(np.float32).astype(np.float64)
            act[t] = a
            hit = _env_step(costmap, robot, 0.05, Action(command=a))
            collided = collided or hit
            s = S(); s.pose = robot.get_pose()
            rew[t] = prov.reward(s)
            ps = prov.get_state()
            st[t] = dd_state_vec(robot.get_state())
            done[t] = ps.done() or (t + 1 >= 1200) or collided
            coll[t], tidx[t], mind[t] = collided, ps.target_idx, ps.min_spat_dist_so_far
        save("g8dd_traj_mini64_%02d.npz" % seed, costmap=costmap.get_data().copy(), origin=np.array(costmap.get_origin()),
             resolution=np.float64(costmap.get_resolution()), path=path, init_target_idx=np.int32(init.target_idx),
             init_min_dist=np.float64(init.min_spat_dist_so_far), start_state=start_state, actions=act, states=st, reward=rew, done=done,
             collided=coll, target_idx=tidx, min_dist=mind)
        print("   dd traj seed %d: collided at %s, final target %d/%d" % (seed, np.nonzero(coll)[0][:1], tidx[-1], len(path)))


def gen_kat_collision_table():
    """Inputs of the reference KAT test_costmap_utils.py:251-314 (its 20 expected verdicts are written in the
    test itself and restated in tests/test_oracle_kat.py); here we only store the costmap the reference's own
    map-building code produces through the harness' cv2.line stand-in."""
    from bc_gym_planning_env.utilities.costmap_2d import CostMap2D
    from bc_gym_planning_env.utilities.map_drawing_utils import add_wall_to_static_map
    costmap = CostMap2D.create_empty((10, 6), 0.05, (-1, -3))
    add_wall_to_static_map(costmap, (3.9, -4.), (3.9, -1 + 1.5))
    add_wall_to_static_map(costmap, (1.5, -4.), (1.5, -1 + 1.5))
    add_wall_to_static_map(costmap, (5., -4.), (5. + 1, -1 + 4.5))
    save("kat_collision_map.npz", costmap=costmap.get_data(), origin=np.array(costmap.get_origin()),
         resolution=costmap.get_resolution())


def gen_mini_geometry():
    """G9: the worlds RandomMiniEnv(seed=s) goes through on construction and on three successive reset() calls."""
    from bc_gym_planning_env.envs.mini_env import RandomMiniEnv
    seeds, episodes = list(range(12)), 4
    worlds = np.zeros((len(seeds), episodes, 14))
    maps, paths, lens, init = [], [], [], []
    for si, s in enumerate(seeds):
        env = RandomMiniEnv(seed=s)
        for e in range(episodes):
            if e:
                env.reset()
            cfg = env._env._config
            worlds[si, e] = np.concatenate([cfg.start_pos.as_np(), cfg.end_pos.as_np(), cfg.obstacle_a.as_np(),
                                            cfg.obstacle_o.as_np(), cfg.obstacle_b.as_np(), [cfg.h, cfg.w]])
            st = env._env.get_state()
            data = st.costmap.get_data()
            assert set(np.unique(data)) <= {0, 254}
            maps.append(np.packbits(data == 254, axis=1))
            paths.append(st.original_path)
            lens.append(len(st.original_path))
            init.append([st.pose[0], st.pose[1], st.pose[2], st.reward_provider_state.min_spat_dist_so_far,
                         st.reward_provider_state.target_idx])
    save("g9_mini_geometry.npz", seeds=np.array(seeds), worlds=worlds, maps=np.stack(maps),
         map_shape=np.array(data.shape), origin=np.array(st.costmap.get_origin()),
         resolution=st.costmap.get_resolution(), paths=np.concatenate(paths), lens=np.array(lens),
         init=np.array(init))


def record_delayed(env, plan_env, n_steps, action_seed, noise_seed, speed=1.0):
    """Like record_trajectory, for envs with delays / the pure-pursuit provider: the robot's true state and what the
    State / Observation expose are recorded separately."""
    from bc_gym_planning_env.robot_models import differential_drive as dd
    from bc_gym_planning_env.envs.base import spaces
    spaces.SPACE_LOCAL_RANDOM_STATE.seed(action_seed)
    state0 = plan_env.get_state()
    rec = dict(
        costmap=state0.costmap.get_data().copy(), origin=np.array(state0.costmap.get_origin()),
        resolution=np.float64(state0.costmap.get_resolution()),
        path=np.array(state0.reward_provider_state.path), init_target_idx=np.int32(state0.reward_provider_state.target_idx),
        init_min_dist=np.float64(state0.reward_provider_state.min_spat_dist_so_far),
        init_state=tri_state_vec(state0.robot_state),
    )
    act, z, true_st, seen_pose, seen_st = [], [], [], [], []
    rew, done, coll, tidx, mind, plen = [], [], [], [], [], []
    with SlotTap(dd, noise_seed) as tap:
        for t in range(n_steps):
            a = env.action_space.sample()
            a = type(a)(command=np.array([a.command[0] * speed, a.command[1]]))
            act.append(np.asarray(a.command, dtype=np.float64))
            obs, r, d, _ = env.step(a)
            z.append(tap.take())
            s = plan_env._state
            true_st.append(tri_state_vec(plan_env._robot.get_state()))
            seen_pose.append(np.array(obs.pose, dtype=np.float64))
            seen_st.append(tri_state_vec(obs.robot_state))
            assert (np.asarray(s.pose) == obs.pose).all()
            rew.append(r); done.append(d); coll.append(s.robot_collided)
            tidx.append(s.reward_provider_state.target_idx)
            mind.append(s.reward_provider_state.min_spat_dist_so_far)
            plen.append(len(obs.path))
    rec.update(actions=np.stack(act), z=np.stack(z), true_states=np.stack(true_st), seen_pose=np.stack(seen_pose),
               seen_states=np.stack(seen_st), reward=np.array(rew, dtype=np.float64), done=np.array(done, dtype=np.uint8),
               collided=np.array(coll, dtype=np.uint8), target_idx=np.array(tidx, dtype=np.int32),
               min_dist=np.array(mind, dtype=np.float64), obs_path_len=np.array(plen, dtype=np.int32))
    return rec


def gen_delays_and_pure_pursuit():
    """G11: EnvParams delays > 0 (env.py:27-49, 363-398) and the pure-pursuit reward provider (reward.py:78-159, 291-371)."""
    from bc_gym_planning_env.envs.mini_env import RandomMiniEnv, RandomMiniEnvParams
    from bc_gym_planning_env.envs.synth_turn_env import AisleTurnEnv, AisleTurnEnvParams
    from bc_gym_planning_env.envs.base.params import EnvParams
    cases = [
        ("delay_p1s1", dict(pose_delay=1, state_delay=1), 2, 1.0),          # the runner scripts' setting
        ("delay_c2p3s1", dict(control_delay=2, pose_delay=3, state_delay=1), 4, 1.0),
        ("delay_c1_wall", dict(control_delay=1, pose_delay=2, state_delay=2), 9, 3.0),   # drives into the wall
    ]
    for tag, kw, seed, speed in cases:
        params = RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, **kw))
        env = RandomMiniEnv(params=params, rng=np.random.RandomState(seed), draw_new_turn_on_reset=False)
        rec = record_delayed(env, env._env, 300, 500 + seed, 600 + seed, speed)
        rec.update(control_delay=np.int32(kw.get("control_delay", 0)), pose_delay=np.int32(kw.get("pose_delay", 0)),
                   state_delay=np.int32(kw.get("state_delay", 0)), pure_pursuit=np.int32(0))
        save("g11_traj_%s.npz" % tag, **rec)
    for tag, kw, speed in (("pp", dict(), 2.0), ("pp_delay", dict(pose_delay=1, control_delay=1), 3.0)):
        ep = EnvParams(reward_provider_name='continuous_reward_pure_pursuit', **kw)
        env = AisleTurnEnv(AisleTurnEnvParams(env_params=ep))
        rec = record_delayed(env, env, 400, 700, 701, speed)
        rec.update(control_delay=np.int32(kw.get("control_delay", 0)), pose_delay=np.int32(kw.get("pose_delay", 0)),
                   state_delay=np.int32(kw.get("state_delay", 0)), pure_pursuit=np.int32(1))
        save("g11_traj_%s.npz" % tag, **rec)
        print("   %s: reward range %.3f .. %.3f, collided %d, done at %s" % (
            tag, rec["reward"].min(), rec["reward"].max(), rec["collided"].sum(), np.argmax(rec["done"])))


def gen_serialized_records():
    """G13: genuine PlanEnv.serialize() records (env.py:251-261, State.serialize :163-176) taken mid-episode -- with delay
    queues filled and with both reward providers -- followed by the next 100 steps of the SAME live env.  The record is
    what a batch is rebuilt from (BatchedPlanEnv.deserialize); the continuation is what it must then reproduce."""
    import copy
    from oracle import records
    from bc_gym_planning_env.envs.mini_env import RandomMiniEnv, RandomMiniEnvParams
    from bc_gym_planning_env.envs.synth_turn_env import AisleTurnEnv, AisleTurnEnvParams
    from bc_gym_planning_env.envs.base.params import EnvParams
    from bc_gym_planning_env.envs.base import spaces

    def mini(seed, **kw):
        params = RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, **kw))
        env = RandomMiniEnv(params=params, rng=np.random.RandomState(seed), draw_new_turn_on_reset=False)
        return env, env._env

    def aisle(**kw):
        env = AisleTurnEnv(AisleTurnEnvParams(env_params=EnvParams(reward_provider_name='continuous_reward_pure_pursuit', **kw)))
        return env, env

    cases = [("plain", lambda: mini(3), 37, 1.0),
             ("delay_p1s1", lambda: mini(2, pose_delay=1, state_delay=1), 23, 1.0),
             ("delay_c2p3s1", lambda: mini(4, control_delay=2, pose_delay=3, state_delay=1), 41, 1.0),
             ("delay_c2p3", lambda: mini(5, control_delay=2, pose_delay=3), 29, 1.0),   # no state delay: State holds the robot's true state
             ("delay_filling", lambda: mini(6, control_delay=3, pose_delay=2, state_delay=3), 2, 1.0),   # queues not full yet
             ("delay_fresh", lambda: mini(7, control_delay=1, pose_delay=1, state_delay=1), 0, 1.0),    # empty queues
             ("pp", lambda: aisle(), 60, 2.0),
             ("pp_delay", lambda: aisle(pose_delay=1, control_delay=1), 35, 2.0)]
    for tag, make, before, speed in cases:
        env, plan_env = make()
        spaces.SPACE_LOCAL_RANDOM_STATE.seed(900)
        np.random.seed(901)
        for _ in range(before):
            a = env.action_space.sample()
            env.step(type(a)(command=np.array([a.command[0] * speed, a.command[1]], dtype=np.float32)))
        skeleton, arrays = records.pack(copy.deepcopy(plan_env.serialize()))
        rec = record_delayed(env, plan_env, 100, 910, 911, speed)
        cont = dict(("cont_" + k, v) for k, v in rec.items() if k in (
            "actions", "z", "true_states", "seen_pose", "seen_states", "reward", "done", "collided", "target_idx",
            "min_dist", "obs_path_len"))
        save("g13_serialized_%s.npz" % tag, record=np.array(skeleton), steps_before=np.int32(before), **dict(arrays, **cont))


def gen_colored_ego():
    """G12: ColoredEgoCostmapRandomAisleTurnEnv observations (envs/synth_turn_env.py:376-451): 133 x 133 egocentric
    costmap + the 5-vector (unit goal direction, v, w, wheel angle), along a sampled-action trajectory."""
    from bc_gym_planning_env.envs.synth_turn_env import ColoredEgoCostmapRandomAisleTurnEnv
    from bc_gym_planning_env.envs.base import spaces
    from bc_gym_planning_env.robot_models import differential_drive as dd
    env = ColoredEgoCostmapRandomAisleTurnEnv()
    env.seed(3)
    env.reset()
    plan_env = env._env
    spaces.SPACE_LOCAL_RANDOM_STATE.seed(78)
    st0 = plan_env.get_state()
    imgs, vecs, states = [], [], []
    with SlotTap(dd, 6):
        for t in range(120):
            a = env.action_space.sample()
            a = type(a)(command=np.array([a.command[0] * 2.5, a.command[1]]))
            obs, _r, done, _ = env.step(a)
            img = obs['environment'][:, :, 0]
            assert set(np.unique(img)) <= {0, 254}
            imgs.append(np.packbits(img == 254, axis=1))
            vecs.append(obs['goal'][:, 0].copy())
            states.append(tri_state_vec(plan_env._robot.get_state()))
            if done:
                break
    save("g12_colored_ego.npz", costmap=st0.costmap.get_data().copy(), origin=np.array(st0.costmap.get_origin()),
         resolution=np.float64(st0.costmap.get_resolution()), path=np.array(st0.reward_provider_state.path),
         images=np.stack(imgs), image_shape=np.array(img.shape), goal=np.stack(vecs), states=np.stack(states),
         window_origin=np.array([-0.5, -2.0]), window_size=np.array([4.0, 4.0]))


def gen_egocentric():
    """G10: EgocentricCostmap(env).step observations (envs/egocentric.py:102-160) along sampled-action trajectories:
    the 133 x 117 egocentric costmap and the goal_n_state vector, with the state they were computed from."""
    from bc_gym_planning_env.envs.egocentric import EgocentricCostmap
    from bc_gym_planning_env.envs.synth_turn_env import AisleTurnEnv, AisleTurnEnvParams
    from bc_gym_planning_env.envs.base import spaces
    from bc_gym_planning_env.robot_models import differential_drive as dd
    cases = [("mini_00", lambda: make_mini_env(0), 120), ("mini_05", lambda: make_mini_env(5), 120),
             ("aisle", lambda: AisleTurnEnv(AisleTurnEnvParams()), 150)]
    for tag, make, steps in cases:
        base = make()
        plan_env = base._env if hasattr(base, "_env") else base
        env = EgocentricCostmap(base)
        spaces.SPACE_LOCAL_RANDOM_STATE.seed(77)
        st0 = plan_env.get_state()
        imgs, vecs, states, tidx = [], [], [], []
        with SlotTap(dd, 5):
            for t in range(steps):
                a = env.action_space.sample()
                a = type(a)(command=np.array([a.command[0] * 2.5, a.command[1]]))    # drive faster: see more of the map
                obs, _r, done, _ = env.step(a)
                s = plan_env._state
                img = obs['env'][:, :, 0]
                assert set(np.unique(img)) <= {0, 254}
                imgs.append(np.packbits(img == 254, axis=1))
                vecs.append(obs['goal_n_state'][:, 0].copy())
                states.append(tri_state_vec(s.robot_state))
                tidx.append(s.reward_provider_state.target_idx)
                if done:
                    break
        save("g10_ego_%s.npz" % tag, costmap=st0.costmap.get_data().copy(), origin=np.array(st0.costmap.get_origin()),
             resolution=np.float64(st0.costmap.get_resolution()), path=np.array(st0.reward_provider_state.path),
             images=np.stack(imgs), image_shape=np.array(img.shape), goal_n_state=np.stack(vecs),
             states=np.stack(states), target_idx=np.array(tidx, dtype=np.int32),
             window_origin=np.array([-0.5, -2.0]), window_size=np.array([3.5, 4.0]))


# ---- G16: away from the stock parameters ------------------------------------------------------------------------
ROBOT_CONSTANT_KEYS = ("front_wheel_from_axis", "max_front_wheel_angle", "max_front_wheel_speed",
                       "max_linear_acceleration", "max_angular_acceleration", "front_column_p_gain")
OFFSTOCK_ROBOTS = dict(
    short=(0.5, 1.0, 2.0, 1.5, 2.0, 0.5),       # short and twitchy
    long=(1.7, 0.6, 0.3, 0.1, 0.15, 0.05))      # long and sluggish
OFFSTOCK_DTS = (0.02, 1. / 30., 0.1, 0.25)
OFFSTOCK_ALPHAS = dict(all_six=(0.02, 0.005, 0.01, 0.02, 0.003, 0.004), first_two=(0.03, 0.01, 0.0, 0.0, 0.0, 0.0))
# tag -> (RandomMiniEnv seed, steps, EnvParams keywords, (sp, ap, multiplier) or None = EnvParams' own)
OFFSTOCK_TRAJ = [
    ("dt0100", 2, 200, dict(dt=0.1), None),
    ("dt0020", 1, 250, dict(dt=0.02), None),
    ("dt0033", 4, 400, dict(dt=1. / 30.), None),
    ("reach_mid", 2, 200, dict(dt=0.1), (0.35, np.pi / 3, 0.5)),
    ("reach_ap_pi", 3, 150, dict(dt=0.1), (0.1, 3.2, 2.0)),
    ("timeout7", 1, 150, dict(iteration_timeout=7), None),
]


def gen_offstock():
    """G16: TricycleRobot.step / DiffDriveRobot.step at four dt, with two tricycles of other dimensions than the stock one,
    with and without the dynamic model and the front-column PID, and with two other alpha sets; and six PlanEnv
    trajectories at other dt, reward parameters and time-out.  Every constant used is stored next to the arrays."""
    from bc_gym_planning_env.robot_models import differential_drive as dd
    from bc_gym_planning_env.robot_models.tricycle_model import TricycleRobot, TricycleRobotState
    from bc_gym_planning_env.robot_models.differential_drive import DiffDriveRobot, DiffdriveRobotState
    from bc_gym_planning_env.robot_models.robot_dimensions_examples import get_dimensions_example
    from bc_gym_planning_env.envs.base.action import Action
    from bc_gym_planning_env.envs.base.params import EnvParams
    from bc_gym_planning_env.envs.base.reward import RewardParams
    from bc_gym_planning_env.envs.mini_env import RandomMiniEnv, RandomMiniEnvParams
    stock = get_dimensions_example('industrial_tricycle_v1')
    method_of = dict(zip(ROBOT_CONSTANT_KEYS, ROBOT_CONSTANT_KEYS[:5] + ("front_column_model_p_gain",)))

    def dimensions(values):
        members = dict((method_of[k], staticmethod(lambda v=v: v)) for k, v in zip(ROBOT_CONSTANT_KEYS, values))
        return type("OffstockTricycleDimensions", (stock,), members)
    robots = [("stock", stock)] + [(name, dimensions(v)) for name, v in sorted(OFFSTOCK_ROBOTS.items())]
    n = 256
    tri_st, tri_cmd, tri_f32 = random_robot_inputs(np.random.RandomState(161), n, True)
    dd_st, dd_cmd, _ = random_robot_inputs(np.random.RandomState(162), n, False)
    dd_st[:, 5:] = 0.0
    meta = dict(model=[], dt=[], constants=[], dynamic_model=[], pid=[], noise_on=[], alpha=[], name=[])
    outs, zs = [], []

    def tricycle(name, dims, dt, dyn, pid, alpha_name):
        alpha = OFFSTOCK_ALPHAS[alpha_name] if alpha_name else None
        noise = dict(("alpha%d" % (k + 1), alpha[k]) for k in range(6)) if alpha else None
        robot = TricycleRobot(dimensions=dims, noise_parameters=noise, dynamic_model=dyn, model_front_column_pid=pid)
        out, z = np.zeros((n, 7)), np.full((n, 3), np.nan)
        with SlotTap(dd, 1600 + len(outs)) as tap:
            for i in range(n):
                robot.set_state(TricycleRobotState(
                    x=tri_st[i, 0], y=tri_st[i, 1], angle=tri_st[i, 2], v=tri_st[i, 3], w=tri_st[i, 4],
                    steering_motor_command=tri_st[i, 5], wheel_angle=tri_st[i, 6]))
                # (without the PID a float32 command stays float32 through the model, see gen_robot_steps: float64 there)
                c = tri_cmd[i].astype(np.float32) if tri_f32[i] and pid else tri_cmd[i]
                robot.step(dt, Action(command=c))
                out[i] = tri_state_vec(robot.get_state())
                z[i] = tap.take()
        meta["model"].append(0); meta["dt"].append(dt); meta["dynamic_model"].append(int(dyn)); meta["pid"].append(int(pid))
        meta["constants"].append([getattr(dims, method_of[k])() for k in ROBOT_CONSTANT_KEYS])
        meta["noise_on"].append(int(alpha is not None)); meta["alpha"].append(alpha or (0.,) * 6)
        meta["name"].append("tri-%s-dt%.4f-dyn%d-pid%d%s" % (name, dt, dyn, pid, "-" + alpha_name if alpha_name else ""))
        outs.append(out); zs.append(z)
    for name, dims in robots:
        for dt in OFFSTOCK_DTS:
            for dyn in (True, False):
                for pid in (True, False):
                    tricycle(name, dims, dt, dyn, pid, None)
    for alpha_name in sorted(OFFSTOCK_ALPHAS):
        for (name, dims), dt in zip(robots + robots[:1], OFFSTOCK_DTS):
            tricycle(name, dims, dt, True, True, alpha_name)
    n_drawn = (~np.isnan(np.stack(zs))).reshape(len(zs), -1, 3).sum(axis=(0, 1))
    assert (n_drawn > 500).all(), n_drawn          # (every slot, the first included, is drawn by these alphas)
    for dt in OFFSTOCK_DTS:
        robot = DiffDriveRobot(dimensions=get_dimensions_example('industrial_diffdrive_v1'), noise_parameters=None)
        out = np.zeros((n, 7))
        for i in range(n):
            robot.set_state(DiffdriveRobotState(x=dd_st[i, 0], y=dd_st[i, 1], angle=dd_st[i, 2], v=dd_st[i, 3], w=dd_st[i, 4]))
            robot.step(dt, Action(command=dd_cmd[i]))      # (float64 commands: see gen_robot_steps)
            out[i] = dd_state_vec(robot.get_state())
        meta["model"].append(1); meta["dt"].append(dt); meta["dynamic_model"].append(1); meta["pid"].append(1)
        meta["constants"].append([getattr(stock, method_of[k])() for k in ROBOT_CONSTANT_KEYS])
        meta["noise_on"].append(0); meta["alpha"].append((0.,) * 6)
        meta["name"].append("dd-dt%.4f" % dt)
        outs.append(out); zs.append(np.full((n, 3), np.nan))
    save("g16_robot_step_params.npz", tri_state=tri_st, tri_cmd=tri_cmd, dd_state=dd_st, dd_cmd=dd_cmd,
         constant_keys=np.array(ROBOT_CONSTANT_KEYS), names=np.array(meta["name"]),
         model=np.array(meta["model"], dtype=np.int32), dt=np.array(meta["dt"]), constants=np.array(meta["constants"]),
         dynamic_model=np.array(meta["dynamic_model"], dtype=np.int32), pid=np.array(meta["pid"], dtype=np.int32),
         noise_on=np.array(meta["noise_on"], dtype=np.int32), alpha=np.array(meta["alpha"]),
         out=np.stack(outs), z=np.stack(zs))

    n_collide = 0
    for tag, seed, steps, kw, reach in OFFSTOCK_TRAJ:
        defaults = EnvParams()
        sp, ap, mult = reach if reach else (defaults.goal_spat_dist, defaults.goal_ang_dist, 0.0)
        ep = EnvParams(goal_spat_dist=sp, goal_ang_dist=ap, reward_provider_params=RewardParams(
            spatial_precision=sp, angular_precision=ap, spatial_progress_multiplier=mult), **kw)
        env = RandomMiniEnv(params=RandomMiniEnvParams(env_params=ep), rng=np.random.RandomState(seed),
                            draw_new_turn_on_reset=False)
        assert 150 <= steps <= 400
        rec = record_trajectory(env, env._env, steps, action_seed=1600 + seed, noise_seed=2600 + seed)
        assert rec["done"].any(), tag
        n_collide += int(rec["collided"].any())
        rec.update(dt=np.float64(ep.dt), iteration_timeout=np.int32(ep.iteration_timeout), spatial_precision=np.float64(sp),
                   angular_precision=np.float64(ap), spatial_progress_multiplier=np.float64(mult))
        save("g16_traj_%s.npz" % tag, **rec)
    assert n_collide >= 2, n_collide


# ---- G17: headings outside [-pi, pi) ----------------------------------------------------------------------------
def save_reproducible(name, **arrays):
    """np.savez_compressed stamps every member with the time of day; this writes the same container with a fixed stamp, so
    that making the fixture again gives the same bytes"""
    import zipfile
    path = os.path.join(OUT, name)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[key]), allow_pickle=False)
    print("wrote %-32s %7.1f KiB" % (name, os.path.getsize(path) / 1024.))


def heading_cases(rng):
    """Start states [n, 7] and commands [n, 2] (float32 values held in float64, from PlanEnv's action box) whose headings cover
    [-pi, pi) and +-1, +-2, +-3, +-50 turns away from it; exactly +-pi and +-3 pi with their neighbouring doubles; and
    +-(3 pi - eps), eps in {0, 1e-4, 1e-3, 5e-3, 2e-2}, each with commands of both turning signs (four per sign) from rest."""
    box_low = np.array([60. * np.pi / 180. / 10, -np.pi / 2])
    box_high = np.array([60. * np.pi / 180. / 2, np.pi / 2])
    heads, turning, rest = [], [], []
    for th in rng.uniform(-np.pi, np.pi, 24):
        for turns in (0, 1, -1, 2, -2, 3, -3, 50, -50):
            heads.append(th + turns * 2 * np.pi)
            turning.append(0)
            rest.append(False)
    for base in (np.pi, -np.pi, 3 * np.pi, -3 * np.pi):
        for th in (np.nextafter(base, -100.0), base, np.nextafter(base, 100.0)):
            for sign in (1, -1):
                heads.append(th)
                turning.append(sign)
                rest.append(True)
    for eps in (0.0, 1e-4, 1e-3, 5e-3, 2e-2):
        for side in (1.0, -1.0):
            for sign in (1, -1):
                for _ in range(4):
                    heads.append(side * (3 * np.pi - eps))
                    turning.append(sign)
                    rest.append(True)
    n = len(heads)
    turning, rest = np.array(turning), np.array(rest)
    st = np.zeros((n, 7))
    st[:, 0:2] = rng.uniform(-3, 3, (n, 2))
    st[:, 2] = heads
    st[:, 3] = np.where(rest, 0.0, rng.uniform(0.0, 0.5, n))
    st[:, 4] = np.where(rest, 0.0, rng.uniform(-0.5, 0.5, n))
    st[:, 6] = np.where(rest, 0.0, rng.uniform(-0.6, 0.6, n))
    cmd = rng.uniform(box_low, box_high, (n, 2))
    cmd[:, 1] = np.where(turning != 0, turning * np.abs(cmd[:, 1]), cmd[:, 1])
    return st, cmd.astype(np.float32).astype(np.float64), turning


def gen_headings():
    """G17: TricycleRobot.step (dynamic model + PID, and kinematic without PID) and DiffDriveRobot.step from the headings of
    heading_cases -- the output state, or raised = 1 where the step raised "Path has missing/corrupted angle data" (the
    state is not recorded there) -- and two PlanEnv trajectories (refine_path = False) on the g8 mini map and on one aisle
    template with the path angles of way points j >= 1 shifted by whole turns (tests/headings.shift_path; path[0], the
    start heading, stays)."""
    from bc_gym_planning_env.robot_models.tricycle_model import TricycleRobot, TricycleRobotState
    from bc_gym_planning_env.robot_models.differential_drive import DiffDriveRobot, DiffdriveRobotState
    from bc_gym_planning_env.robot_models.robot_dimensions_examples import get_dimensions_example
    from bc_gym_planning_env.envs.base.action import Action
    from bc_gym_planning_env.envs.base.env import PlanEnv
    from bc_gym_planning_env.envs.base.params import EnvParams
    from bc_gym_planning_env.utilities.costmap_2d import CostMap2D
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import headings as HD
    dt = 0.05
    st, cmd, turning = heading_cases(np.random.RandomState(171))
    n = len(st)
    tri_dims = get_dimensions_example('industrial_tricycle_v1')
    models = [("tri_dyn_pid", lambda: TricycleRobot(dimensions=tri_dims, noise_parameters=None)),
              ("tri_kin_nopid", lambda: TricycleRobot(dimensions=tri_dims, noise_parameters=None, dynamic_model=False,
                                                      model_front_column_pid=False)),
              ("dd", lambda: DiffDriveRobot(dimensions=get_dimensions_example('industrial_diffdrive_v1'), noise_parameters=None))]
    out = dict(state=st, cmd=cmd, turning=turning.astype(np.int32), dt=np.float64(dt), models=np.array([m for m, _ in models]))
    for name, make in models:
        robot = make()
        res, raised = np.full((n, 7), np.nan), np.zeros(n, dtype=np.uint8)
        for i in range(n):
            if name == "dd":   # (the diff-drive command is (v, w): the steering column of cmd serves as w)
                robot.set_state(DiffdriveRobotState(x=st[i, 0], y=st[i, 1], angle=st[i, 2], v=st[i, 3], w=st[i, 4]))
            else:
                robot.set_state(TricycleRobotState(x=st[i, 0], y=st[i, 1], angle=st[i, 2], v=st[i, 3], w=st[i, 4],
                                                   steering_motor_command=st[i, 5], wheel_angle=st[i, 6]))
            try:
                robot.step(dt, Action(command=cmd[i]))
            except Exception as e:
                assert "missing/corrupted angle data" in str(e), e
                raised[i] = 1
                continue
            res[i] = dd_state_vec(robot.get_state()) if name == "dd" else tri_state_vec(robot.get_state())
        print("   %-14s raised %d of %d" % (name, raised.sum(), n))
        out[name + "_out"], out[name + "_raised"] = res, raised
    # (sp, ap) as the g8 trajectories of these worlds were recorded with; the short time-outs end the episodes
    for tag, src, kw, steps, seeds in (("mini", "g8_traj_mini_00.npz", dict(goal_spat_dist=0.2, goal_ang_dist=np.pi / 8, iteration_timeout=60), 100, (1700, 2700)),
                                       ("aisle", "g8_traj_aisle_c4_00.npz", dict(iteration_timeout=120), 150, (1701, 2701))):
        g = np.load(os.path.join(OUT, src))
        path = HD.shift_path(g["path"])
        ep = EnvParams(resolution=float(g["resolution"]), refine_path=False, **kw)
        env = PlanEnv(CostMap2D(g["costmap"].copy(), float(g["resolution"]), g["origin"].copy()), path, ep)
        rec = record_trajectory(env, env, steps, action_seed=seeds[0], noise_seed=seeds[1])
        assert rec["done"].any() and (rec["path"] == path).all() and rec["init_state"][2] == g["path"][0, 2], tag
        rec.pop("costmap"), rec.pop("origin"), rec.pop("resolution")     # (those of `world`)
        rec.update(world=np.array(src), dt=np.float64(ep.dt), iteration_timeout=np.int32(ep.iteration_timeout),
                   spatial_precision=np.float64(ep.goal_spat_dist), angular_precision=np.float64(ep.goal_ang_dist),
                   spatial_progress_multiplier=np.float64(0.0))
        print("   traj %-6s done at %s, collided %d, final target %d of %d" % (
            tag, np.nonzero(rec["done"])[0][:1], rec["collided"].any(), rec["target_idx"][-1], len(path)))
        out.update(("traj_%s_%s" % (tag, k), v) for k, v in rec.items())
    save_reproducible("g17_headings.npz", **out)


def main():
    os.makedirs(OUT, exist_ok=True)
    O.build()
    H.load()
    if sys.argv[1:] == ["footprint_zoo"]:   # (added after the others: writes its own file only)
        gen_footprint_zoo()
        return
    if sys.argv[1:] == ["offstock"]:
        gen_offstock()
        return
    if sys.argv[1:] == ["headings"]:
        gen_headings()
        return
    gen_robot_steps()
    gen_scalar_utils()
    gen_footprints()
    gen_pose_collides()
    gen_reward()
    gen_kat_collision_table()
    gen_mini_geometry()
    gen_egocentric()
    gen_colored_ego()
    gen_delays_and_pure_pursuit()
    gen_serialized_records()
    gen_diffdrive_trajectories()
    gen_trajectories()
    gen_footprint_zoo()
    gen_offstock()
    gen_headings()


if __name__ == "__main__":
    main()

"""GPU tests of the operator seams added in round 2 (reward provider, find_last_reached, path_velocity,
is_robot_colliding / is_footprint_colliding), of the flag hygiene of bcp_step and of switching the step form mid-run.
Everything goes through the C ABI (ctypes -> libbcplan.so)."""
import ctypes as C
import os

import numpy as np
import pytest

from util import ATOL, GOLDEN, env_from_traj, oracle_params_for, z_in

pytestmark = pytest.mark.gpu


def load(name):
    return np.load(os.path.join(GOLDEN, name))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_g7_reward_trace_on_the_gpu(torch_cuda, tag):
    """ContinuousRewardProvider.reward along the poses the genuine reference recorded (g7), one bcp_reward call per
    pose -- the provider state is carried exactly like reward.py:214-259 carries it."""
    from bc_gym_planning_env_amd import EnvParams, NativeOps, host_init
    from bc_gym_planning_env_amd.api import RewardParams
    g = load("g7_reward.npz")
    sp, ap, mult = g[tag + "_params"]
    params = EnvParams(goal_spat_dist=sp, goal_ang_dist=ap,
                       reward_provider_params=RewardParams(spatial_precision=sp, angular_precision=ap,
                                                           spatial_progress_multiplier=mult))
    ops = NativeOps(params=params)
    path = g[tag + "_path"]
    ops.set_path(path)
    md, ti = host_init.initial_reward_state(path, params.reward_provider_params)
    assert (md, ti) == (g[tag + "_init"][0], int(g[tag + "_init"][1]))
    md_t = np.array([md])
    ti_t = np.array([ti], dtype=np.int32)
    for pose, er, emd, eti in zip(g[tag + "_poses"], g[tag + "_reward"], g[tag + "_min_dist"], g[tag + "_target_idx"]):
        r, md_t, ti_t, goal = ops.reward(pose[None], md_t, ti_t)
        assert int(ti_t[0]) == int(eti)
        assert abs(float(r[0]) - er) <= ATOL and abs(float(md_t[0]) - emd) <= ATOL
        assert bool(goal[0]) == (eti > len(path) - 1)


def test_reward_and_find_last_reached_batch_vs_oracle(torch_cuda, oracle):
    """20 000 random (pose, provider state) pairs around a self-crossing path: reward, new state, goal flag and the
    plain find_last_reached index against the oracle."""
    from bc_gym_planning_env_amd import EnvParams, NativeOps
    from bc_gym_planning_env_amd.api import RewardParams
    rng = np.random.RandomState(5)
    t = np.linspace(0, 4 * np.pi, 400)
    path = np.stack([2 * np.sin(t), 1.5 * np.sin(2 * t), np.zeros_like(t)], 1)   # a figure of eight, twice around
    d = np.diff(path[:, :2], axis=0)
    path[:-1, 2] = np.arctan2(d[:, 1], d[:, 0])
    path[-1, 2] = path[-2, 2]
    sp, ap, mult = 0.25, np.pi / 5, 0.7
    params = EnvParams(reward_provider_params=RewardParams(spatial_precision=sp, angular_precision=ap,
                                                           spatial_progress_multiplier=mult))
    ops = NativeOps(params=params)
    ops.set_path(path)
    n = 20000
    k = rng.randint(0, len(path), n)
    poses = path[k] + np.stack([rng.normal(0, 0.15, n), rng.normal(0, 0.15, n), rng.normal(0, 0.4, n)], 1)
    poses[::50] += 5.0   # some far off the path
    target = np.clip(k + rng.randint(-30, 30, n), 0, len(path) + 1).astype(np.int32)
    md = rng.uniform(0, 0.5, n)
    rew, md2, ti2, goal = [v.cpu().numpy() for v in ops.reward(poses, md, target)]
    last = ops.find_last_reached(poses).cpu().numpy()
    p = oracle.make_params("tricycle", spatial_precision=sp, angular_precision=ap, spatial_progress_multiplier=mult)
    hits = 0
    for i in range(n):
        er, emd, eti = oracle.reward(p, poses[i], path, md[i], int(target[i]))
        assert int(ti2[i]) == eti and abs(rew[i] - er) <= ATOL and abs(md2[i] - emd) <= ATOL, i
        assert bool(goal[i]) == (eti > len(path) - 1)
        el = oracle.find_last_reached(poses[i], path, sp, ap)
        assert int(last[i]) == (-1 if el is None else el), i
        hits += el is not None
    assert hits > n // 4


def test_path_velocity_vs_reference(torch_cuda):
    """path_velocity: the reference's own two-row outputs (g4) and the same rows chained into one long path."""
    from bc_gym_planning_env_amd import NativeOps
    g = load("g4_scalar_utils.npz")
    ops = NativeOps()
    dt = float(g["pv_dt"])
    p0, p1, exp = g["pv_p0"], g["pv_p1"], g["pv_out"]
    rows = np.zeros((2 * len(p0), 4))
    rows[0::2, 0] = np.arange(len(p0)) * 10.0
    rows[1::2, 0] = rows[0::2, 0] + dt
    rows[0::2, 1:] = p0
    rows[1::2, 1:] = p1
    ok = np.isfinite(exp).all(1)
    # one call per pair would be 2048 launches: chain the pairs, every even segment is a recorded pair (odd ones join them)
    import torch
    p = torch.from_numpy(rows).cuda()
    v = torch.empty(len(rows) - 1, dtype=torch.float64, device="cuda")
    w = torch.empty_like(v)
    err = torch.zeros(len(rows) - 1, dtype=torch.int32, device="cuda")
    from bc_gym_planning_env_amd import _lib
    _lib.check(ops._lib.bcp_path_velocity(ops._h, p.data_ptr(), len(rows), v.data_ptr(), w.data_ptr(), err.data_ptr(), None))
    v, w, err = v.cpu().numpy()[0::2], w.cpu().numpy()[0::2], err.cpu().numpy()[0::2]
    # (t1 - t0 is dt up to the rounding of the time stamps: compare with the value recomputed for that dt)
    dts = rows[1::2, 0] - rows[0::2, 0]
    np.testing.assert_allclose(v[ok] * dts[ok] / dt, exp[ok, 0], rtol=1e-12, atol=ATOL)
    np.testing.assert_allclose(w[ok] * dts[ok] / dt, exp[ok, 1], rtol=1e-12, atol=ATOL)
    assert ((err & 1) != 0).tolist() == (~ok).tolist()   # the reference raised exactly there
    # reference KAT (utilities/test_path_tools.py:215-272 style): straight line forwards, then backwards, then a turn
    kat = np.array([[0., 0., 0., 0.], [1., 1., 0., 0.], [2., 0., 0., 0.], [3., 0., 0., np.pi / 2]])
    v, w = ops.path_velocity(kat)
    np.testing.assert_allclose(v.cpu().numpy(), [1., -1., 0.], atol=1e-15)
    np.testing.assert_allclose(w.cpu().numpy(), [0., 0., np.pi / 2], atol=1e-15)
    v, w = ops.path_velocity(np.array([[0., 0., 0., 3.], [1., 0., 0., -0.2]]))   # -3.2 wraps to 2 pi - 3.2: fine
    assert abs(float(w[0]) - (2 * np.pi - 3.2)) < 1e-12
    with pytest.raises(Exception, match="corrupted angle data"):
        ops.path_velocity(np.array([[0., 0., 0., 0.], [1., 0., 0., np.pi]]))     # |dtheta| == pi: the reference raises


def test_is_robot_colliding_table(torch_cuda):
    """The reference's 20-pose truth table (utilities/test_costmap_utils.py:251-314) through bcp_is_robot_colliding."""
    from bc_gym_planning_env_amd import NativeOps
    from footprints import ZOO, registered
    g = load("kat_collision_map.npz")
    with registered("kat_rect", ZOO["kat_rect"]):
        ops = NativeOps("kat_rect")
        ops.set_costmap(g["costmap"], g["origin"], float(g["resolution"]))
        poses = [(x, 0., 0.2) for x in range(7)] + [(x, 1.2, np.pi / 2 + 0.4) for x in range(7)]
        poses += [(0., -3, 0.2), (1., -3, 0.2), (2., -3, 0.2), (0., -3.2, 0.2), (1., -3.2, 0.2), (2., -3.2, 0.2)]
        expected = [0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0]
        got = ops.is_robot_colliding(np.array(poses, dtype=np.float64)).cpu().numpy()
        np.testing.assert_array_equal(got, expected)


def test_is_footprint_colliding_vs_numpy(torch_cuda):
    """is_footprint_colliding_impl(image_slice, blit_mask, lethal) == np.any(image_slice[blit_mask] == lethal)."""
    from bc_gym_planning_env_amd import NativeOps
    ops = NativeOps()
    rng = np.random.RandomState(2)
    for rows, cols in ((33, 91), (17, 17), (64, 64), (1, 5)):
        n = 3000
        sl = rng.randint(0, 256, (n, rows, cols)).astype(np.uint8)
        sl[sl == 254] = 0
        mk = (rng.uniform(size=(n, rows, cols)) < 0.4).astype(np.uint8) * rng.randint(1, 256, (n, rows, cols)).astype(np.uint8)
        # a single lethal cell in a third of the slices, under the mask in about 40 % of those
        for i in range(0, n, 3):
            sl[i, rng.randint(rows), rng.randint(cols)] = 254
        exp = np.array([np.any(sl[i][mk[i] > 0] == 254) for i in range(n)])
        got = ops.is_footprint_colliding(sl, mk).cpu().numpy().astype(bool)
        np.testing.assert_array_equal(got, exp)
        assert 0.05 < exp.mean() < 0.3
        got255 = ops.is_footprint_colliding(sl, mk, lethal=255).cpu().numpy().astype(bool)
        np.testing.assert_array_equal(got255, [np.any(sl[i][mk[i] > 0] == 255) for i in range(n)])


def test_step_rejects_undefined_flag_bits(torch_cuda):
    """bcp_step only accepts BCP_STEP_AUTO_RESET | BCP_STEP_ACTIONS_F32: the ablation switches of the diagnostic build
    and the internal step-advance bit are not reachable through the shipping ABI."""
    from bc_gym_planning_env_amd import _lib
    g = load("g8_traj_mini_00.npz")
    env = env_from_traj(g, "g8_traj_mini_00.npz", n_envs=128)
    a = env.action_space.sample_batch(128, np.random.RandomState(0))
    env.step(a)
    import torch
    act = torch.from_numpy(a).cuda()
    env._io.actions = act.data_ptr()
    for bad in (1 << 16, 1 << 17, 1 << 19, 1 << 21, 1 << 22, 1 << 24, 4, 1 << 31):
        rc = env._lib.bcp_step(env._h, env._io_ref, _lib.STEP_ACTIONS_F32 | bad, None)
        assert rc == -1 and b"undefined flag" in env._lib.bcp_last_error()
        ms = C.c_float()
        assert env._lib.bcp_time_steps(env._h, env._io_ref, _lib.STEP_ACTIONS_F32 | bad, 1, None, C.byref(ms)) == -1
    assert env._lib.bcp_step(env._h, env._io_ref, _lib.STEP_ACTIONS_F32, None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("base", [dict(), dict(fused=0)], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("pattern", [(("defer", 0), 1), (("defer", 0), 3), (("exact_mode", 1), 1), (("exact_mode", 2), 3),
                                     (("cull", 0), 1), (("cull", 0), 2), (("fused", 0), 1), (("fused", 0), 3)],
                         ids=lambda p: "%s=%d_x%d" % (p[0][0], p[0][1], p[1]))
def test_switching_the_step_form_mid_episode(torch_cuda, oracle, pattern, base):
    """bcp_set_tuning between steps moves the batch between the step forms (one launch with parked poses settled inside
    it, two launches, the general single kernel); the parity-keyed parking counters / queues must be re-armed when a
    form that uses them resumes (an odd number of single-kernel steps used to leave the two-launch step on a stale
    counter set).  Every step is compared with the oracle."""
    import torch
    (key, val), single_steps = pattern
    g = load("g8_traj_mini_03.npz")
    n = 4096
    env = env_from_traj(g, "g8_traj_mini_03.npz", n_envs=n, auto_reset=True, seed=9)
    p = oracle_params_for(oracle, "g8_traj_mini_03.npz")
    ref = oracle.OracleBatch(p, n, g["costmap"], g["origin"], float(g["resolution"]), g["path"])
    ref.reset_from_paths()
    rng = np.random.RandomState(3)
    zout = torch.zeros(n, 3, dtype=torch.float64, device="cuda")
    defaults = dict(defer=1, exact_mode=0, cull=1, fused=1)
    defaults.update(base)
    env.set_tuning(**base)
    collisions = 0
    # drive towards the walls so that parked poses really collide: the stale-counter bug needs hits among them
    schedule = ([None] * 40 + [(key, val)] * single_steps) * 4 + [None] * 20
    mode = None
    for want in schedule:
        if want != mode:
            env.set_tuning(**({want[0]: want[1]} if want else {key: defaults[key]}))
            mode = want
        a = env.action_space.sample_batch(n, rng)
        a[:, 0] = np.float32(0.5)
        env.step(a, noise_z_out=zout)
        ref.step(a.astype(np.float64), z_in(zout.cpu().numpy()), auto_reset=True)
        assert (env.done.cpu().numpy() == ref.done).all()
        assert (env.collided_now.cpu().numpy() == ref.collided_now).all()
        assert (env.state.target_idx.cpu().numpy() == ref.target_idx).all()
        assert (env.state.current_iter.cpu().numpy() == ref.cur_iter).all()
        assert np.abs(env.state.robot.cpu().numpy() - np.stack(ref.st)).max() < ATOL
        assert np.abs(env.reward.cpu().numpy() - ref.reward).max() < ATOL
        collisions += int(ref.collided_now.sum())
    assert collisions > 50
    env.check_errors()

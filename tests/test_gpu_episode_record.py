"""Episode ends under auto-reset (bcp_bind_episode_record, BatchedPlanEnv.enable_episode_record): the reason, final state,
return and final observation of every env whose episode ends, kept although the step has already reset the env.

Pinned by the reference's recorded terminal states (g14), and by twin runs: handle A steps with auto-reset and a record,
handle B with the same actions and noise steps without auto-reset and calls reset(mask=A.done) after every step -- the
reference's own protocol (envs/base/env.py:334-361, 293-303) -- so B's state between its step and its reset is what A's
record must hold, bit for bit."""
import os

import numpy as np
import pytest

from util import ATOL, GOLDEN, z_in

pytestmark = pytest.mark.gpu

GOAL, TIMEOUT, COLLIDED = 1, 2, 4


# ---------------------------------------------------------------------------------------------------------------------
# pinned by the reference: the terminal states of g14 (ColoredEgoCostmapRandomAisleTurnEnv)
@pytest.mark.parametrize("sampler", ["host", "device", "device_resident"])
def test_g14_terminal_states_and_observations(torch_cuda, sampler):
    torch = torch_cuda
    from bc_gym_planning_env_amd import aisle_env
    from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap
    g = np.load(os.path.join(GOLDEN, "g14_aisle_worlds.npz"))
    ends_seen = 0
    for j in range(int(g["n_traj"])):
        t_ = lambda k: g["t%d_%s" % (j, k)]   # noqa: E731
        env = aisle_env.BatchedRandomAisleTurnEnv(1, seeds=[int(t_("seed"))], episodes=4, sampler=sampler, auto_reset=True)
        env.geom_of_env.fill_(3)
        wrap = BatchedColoredEgoCostmap(env, final_observation=True)
        wrap.reset()
        ends = env.episode_ends
        cols = int(t_("image_cols"))
        imgs = np.unpackbits(t_("images"), axis=2)[:, :, :cols]
        reset_imgs = np.unpackbits(t_("reset_images"), axis=2)[:, :, :cols]
        resets, since = 0, 0
        for t in range(len(t_("done"))):
            a = torch.from_numpy(t_("actions")[t:t + 1].copy()).cuda()
            z = torch.from_numpy(z_in(t_("z")[t:t + 1])).cuda()
            obs, r, d, info = wrap.step(a, noise_z=z)
            since += 1
            assert info["episode_ends"] is ends
            done = int(t_("done")[t])
            assert int(d[0]) == done and int(ends.count[0]) == done, (j, t)
            if done:
                ends_seen += 1
                assert int(ends.env_ids[0]) == 0
                fin = info["final_observation"]
                np.testing.assert_allclose(ends.final_state.robot[:, 0].cpu().numpy(), t_("states")[t], rtol=0, atol=ATOL)
                img = fin["environment"][0, :, :, 0].cpu().numpy()
                assert ((img == 254) == imgs[t]).all(), (j, t)
                np.testing.assert_allclose(fin["goal"][0, :, 0].cpu().numpy(), t_("goal")[t], rtol=0, atol=ATOL)
                want = COLLIDED if t_("collided")[t] else GOAL
                assert int(ends.reason[0]) & (GOAL | COLLIDED) == want, (j, t, int(ends.reason[0]))
                assert int(ends.length[0]) == since
                assert int(ends.geom[0]) == resets % 4
                # the ordinary observation shows the reset env
                want_img = reset_imgs[resets]
                assert ((obs["environment"][0, :, :, 0].cpu().numpy() == 254) == want_img).all()
                np.testing.assert_allclose(env.state.robot[:, 0].cpu().numpy(), t_("reset_states")[resets], rtol=0,
                                           atol=ATOL)
                resets += 1
                since = 0
            else:
                assert int(ends.reason[0]) == 0
        env.check_errors()
    assert ends_seen >= 3


# ---------------------------------------------------------------------------------------------------------------------
# twin runs
def _mini_pool_pair(n=4096, timeout=60, **kw):
    from bc_gym_planning_env_amd import EnvParams, mini_env
    params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2,
                                                               iteration_timeout=timeout))
    pool = mini_env.sample_pool_device(params, list(range(40, 72)), 4, 0)
    return [mini_env.BatchedRandomMiniEnv(n, params, pool=pool, auto_reset=ar, seed=11, **kw) for ar in (True, False)]


def _aisle_pair(n=2048):
    from bc_gym_planning_env_amd import EnvParams, aisle_env
    ep = EnvParams(iteration_timeout=50)
    pool = aisle_env.sample_aisle_pool_device(ep, list(range(64)), 4, keep_on_device=True)
    return [aisle_env.BatchedRandomAisleTurnEnv(n, ep, pool=pool, episodes=4, auto_reset=ar, seed=5) for ar in (True, False)]


def _g8(name="g8_traj_mini_03.npz"):
    return np.load(os.path.join(GOLDEN, name))


def _private_pair(n=1024):
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    g = _g8()
    res = float(g["resolution"])
    params = EnvParams(goal_spat_dist=0.2, goal_ang_dist=np.pi / 8, resolution=res, refine_path=False, iteration_timeout=40)
    maps = [CostMap2D(g["costmap"], res, g["origin"] + np.array([0.05 * k, -0.03 * k])) for k in range(4)]
    paths = [g["path"] + np.array([0.05 * k, -0.03 * k, 0.0]) for k in range(4)]
    tix = np.arange(n) % 4
    return [BatchedPlanEnv(maps, paths, params, n_envs=n, auto_reset=ar, seed=3, template_of_env=tix, map_storage=(256, 256))
            for ar in (True, False)]


def _shared_pair(n=2048, diffdrive=False, **cfg):
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams, INDUSTRIAL_DIFFDRIVE_V1
    g = _g8()
    res = float(g["resolution"])
    pp = cfg.pop("pure_pursuit", 0)
    params = EnvParams(goal_spat_dist=0.2, goal_ang_dist=np.pi / 8, resolution=res, refine_path=False, iteration_timeout=30,
                       reward_provider_name='continuous_reward_pure_pursuit' if pp else 'continuous_reward', **cfg)
    kw = dict(robot_name=INDUSTRIAL_DIFFDRIVE_V1, noise_parameters=None) if diffdrive else {}
    return [BatchedPlanEnv(CostMap2D(g["costmap"], res, g["origin"]), g["path"], params, n_envs=n, auto_reset=ar, seed=3,
                           **kw) for ar in (True, False)]


def _spread(torch, envs, seed):
    """a third of the robots next to a wall of their map: collisions (and their rollbacks) in every step"""
    rng = np.random.RandomState(seed)
    e = envs[0]
    n = e.n_envs
    geom = e.geom_of_env.cpu().numpy() if e.geom_of_env is not None else None
    pick_xy = np.zeros((n, 2))
    for i in range(0, n, 3):
        cm = e.costmap_of(i) if geom is None else e._costmaps[int(geom[i])]
        d = cm.get_data()
        lethal = np.argwhere(d == 254)
        if not len(lethal):
            continue
        p = lethal[rng.randint(0, len(lethal))]
        pick_xy[i] = np.asarray(cm.get_origin()) + (p[::-1] + rng.uniform(-6, 6, 2)) * cm.get_resolution()
    third = torch.from_numpy(np.arange(n) % 3 == 0).cuda() & torch.from_numpy(np.abs(pick_xy).sum(1) > 0).cuda()
    xy = torch.from_numpy(pick_xy.T.copy()).cuda()
    th = torch.from_numpy(rng.uniform(-np.pi, np.pi, n)).cuda()
    for env in envs:
        env.state.robot[0:2, third] = xy[:, third]
        env.state.robot[2, third] = th[third]
        if env.state.pose_seen is not None:
            env.state.pose_seen.copy_(env.state.robot[0:3])
        if env.state.robot_state_seen is not None:
            env.state.robot_state_seen.copy_(env.state.robot)


def _path_lens(env):
    """int64 [N] length of every env's current path (for the goal term target_idx > len - 1)"""
    import torch
    if env.geom_of_env is not None:
        lens = torch.tensor([len(env._paths[k]) for k in range(len(env._paths))], device=env.device)
        return lens[env.geom_of_env.long()]
    return torch.tensor([len(env.path_of(i)) for i in range(env.n_envs)], device=env.device)


def _check_state_rows(ends, B, ids, m):
    torch = __import__("torch")
    f, s = ends.final_state, B.state
    idx = ids.long()
    assert torch.equal(f.robot[:, :m], s.robot[:, idx]) if B.is_tricycle else torch.equal(f.robot[:5, :m], s.robot[:5, idx])
    for name in ("min_spat_dist_so_far", "target_idx", "current_iter", "robot_collided"):
        assert torch.equal(getattr(f, name)[:m], getattr(s, name)[idx]), name
    for name in ("pose_seen", "robot_state_seen"):
        if getattr(s, name) is not None:
            assert torch.equal(getattr(f, name)[:, :m], getattr(s, name)[:, idx]), name


def _full_state_equal(A, B):
    torch = __import__("torch")
    for name in ("robot", "min_spat_dist_so_far", "target_idx", "current_iter", "robot_collided", "pose_seen",
                 "robot_state_seen", "control_queue", "poses_queue", "robot_state_queue"):
        a, b = getattr(A.state, name), getattr(B.state, name)
        if a is not None:
            if name == "robot" and not A.is_tricycle:
                a, b = a[:5], b[:5]
            assert torch.equal(a, b), name
    if A.geom_of_env is not None:
        assert torch.equal(A.geom_of_env, B.geom_of_env)


def _run_twins(torch, A, B, steps, seed, scale=2.0, wrap=None, pure_pursuit=False, tuning=None):
    """A: auto-reset + record (+ final observations through `wrap`), B: no auto-reset + reset(mask).  Returns the reasons
    seen (OR of all steps) and whether an ended env changed its pool entry."""
    for env in (A, B):
        if tuning:
            env.set_tuning(**tuning)
    WA = WB = None
    if wrap is not None:
        WA, WB = wrap(A, final_observation=True), wrap(B)
        ends = A.episode_ends
    else:
        ends = A.enable_episode_record()
    n = A.n_envs
    rng = np.random.RandomState(seed)
    ret = np.zeros(n)
    timeout = A.params.iteration_timeout
    seen_bits, changed, total, checked_host = 0, False, 0, False
    for t in range(steps):
        a = A.action_space.sample_batch(n, rng)
        a[:, 0] *= scale
        at = torch.from_numpy(a).cuda()
        if WA is not None:
            _o, ra, da, info = WA.step(at)
        else:
            _o, ra, da, info = A.step(at)
        assert info["episode_ends"] is ends
        _o, rb, db, _i = B.step(at)
        assert torch.equal(da, db) and torch.equal(ra, rb), t
        ret += rb.cpu().numpy()
        done = db.bool()
        ids_want = torch.nonzero(done).flatten().int()
        m = int(ends.count[0])
        assert m == int(ids_want.numel()), t
        total += m
        ids = ends.env_ids[:m]
        order = torch.argsort(ids)
        assert torch.equal(ids[order], ids_want), t
        # final state == B's state before its reset, bit for bit
        _check_state_rows(ends, B, ids, m)
        if B.geom_of_env is not None:
            assert torch.equal(ends.geom[:m], B.geom_of_env[ids.long()]), t
            changed = changed or bool((A.geom_of_env[ids.long()] != ends.geom[:m]).any())
        else:
            assert int((ends.geom[:m] != -1).sum()) == 0
        # reason == the done law recomputed from B's state
        reason = ends.reason.cpu().numpy()
        assert ((reason != 0) == done.cpu().numpy()).all(), t
        tmo = (B.state.current_iter >= timeout).cpu().numpy()
        col = B.state.robot_collided.bool().cpu().numpy()
        d_np = done.cpu().numpy()
        assert (((reason & TIMEOUT) != 0) == (tmo & d_np)).all(), t
        assert (((reason & COLLIDED) != 0) == (col & d_np)).all(), t
        if not pure_pursuit:
            goal = (B.state.target_idx.long() > _path_lens(B) - 1).cpu().numpy()
            assert (((reason & GOAL) != 0) == (goal & d_np)).all(), t
        seen_bits |= int(np.bitwise_or.reduce(reason)) if len(reason) else 0
        # terminated / truncated
        term, trunc = ends.terminated().cpu().numpy(), ends.truncated().cpu().numpy()
        assert (term == ((reason & (GOAL | COLLIDED)) != 0)).all() and (trunc == (reason == TIMEOUT)).all()
        # the return: B's running float64 sum, bit for bit
        ids_np = ids.cpu().numpy()
        assert (ends.final_return[:m].cpu().numpy() == ret[ids_np]).all(), t
        assert (ends.length[:m].cpu().numpy() == B.state.current_iter[ids.long()].cpu().numpy()).all()
        if m and not checked_host:   # the host view: env ids, reasons, returns, lengths and the reference State
            checked_host = True
            rows = ends.to_host()
            assert len(rows) == m
            for j, (i, st, why, r, length) in enumerate(rows):
                assert i == int(ids_np[j]) and why == int(reason[i]) and r == ret[i] and length == int(ends.length[j])
                assert st.current_iter == length and st.robot_collided == bool(B.state.robot_collided[i])
                np.testing.assert_array_equal(st.pose, (B.state.pose_seen if B.state.pose_seen is not None
                                                        else B.state.robot[0:3])[:, i].cpu().numpy())
        # final observations == B's observation before its reset
        if WB is not None:
            want = {k: v.clone() for k, v in WB.observation().items()}
            fin = info["final_observation"]
            for k in want:
                assert torch.equal(fin[k][:m], want[k][ids.long()]), (t, k)
        ret[d_np] = 0.0
        B.reset(mask=db)
        _full_state_equal(A, B)
        assert (ends.ret.cpu().numpy() == ret).all(), t
    A.check_errors()
    assert total > 0
    return seen_bits, changed


@pytest.mark.parametrize("form", [dict(local_pairs=4), dict(local_pairs=2), dict(local_pairs=1), dict(fused=0),
                                  dict(defer=0)], ids=["16-waves", "8-waves", "4-waves", "two-launch", "general"])
def test_twin_mini_pool_every_step_form(torch_cuda, form):
    torch = torch_cuda
    A, B = _mini_pool_pair(2048)
    A.set_tuning(**form)
    if "fused" in form:
        assert "step_pending_kernel" in A.step_kernels()
    bits, _ = _run_twins(torch, A, B, 90, 7, scale=3.0, tuning=form)
    assert bits & COLLIDED and bits & TIMEOUT


def test_twin_mini_pool_4096_every_reason(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    A, B = _mini_pool_pair(4096)
    _spread(torch, (A, B), 3)
    bits, changed = _run_twins(torch, A, B, 100, 7, scale=3.0, wrap=BatchedEgocentricCostmap)
    assert bits == GOAL | TIMEOUT | COLLIDED, bits
    assert changed


@pytest.mark.parametrize("ego_sparse", [0, 1])
def test_twin_aisle_pool_final_observations(torch_cuda, ego_sparse):
    torch = torch_cuda
    from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap
    A, B = _aisle_pair(2048)
    bits, changed = _run_twins(torch, A, B, 70, 9, scale=3.0, wrap=BatchedColoredEgoCostmap,
                               tuning=dict(ego_sparse=ego_sparse))
    assert changed and bits & TIMEOUT


def test_twin_private_256_maps(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    A, B = _private_pair()
    _spread(torch, (A, B), 5)
    _run_twins(torch, A, B, 60, 4, scale=2.0, wrap=BatchedEgocentricCostmap)


def test_twin_delays_pure_pursuit(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    A, B = _shared_pair(pose_delay=1, state_delay=1, pure_pursuit=1)
    _spread(torch, (A, B), 6)
    _run_twins(torch, A, B, 60, 5, scale=2.0, wrap=BatchedEgocentricCostmap, pure_pursuit=True)


def test_twin_diffdrive(torch_cuda):
    torch = torch_cuda
    A, B = _shared_pair(diffdrive=True)
    _spread(torch, (A, B), 8)
    _run_twins(torch, A, B, 60, 6, scale=2.0)


# ---------------------------------------------------------------------------------------------------------------------
def test_overflow(torch_cuda):
    torch = torch_cuda
    A, B = _mini_pool_pair(1024, timeout=3)
    ends = A.enable_episode_record(capacity=8)
    rng = np.random.RandomState(1)
    overflowed = False
    for t in range(4):
        a = torch.from_numpy(A.action_space.sample_batch(A.n_envs, rng)).cuda()
        _o, _r, d, _i = A.step(a)
        m = int(ends.count[0])
        assert m == int(d.sum()), t
        if m > 8:
            overflowed = True
            assert ends.overflowed()
            ids = ends.env_ids[:8].long()
            assert bool(d[ids].all()) and int(torch.unique(ids).numel()) == 8
    assert overflowed
    with pytest.raises(RuntimeError):
        A.check_errors()
    A.check_errors()   # (reported once)


def test_graph_replay(torch_cuda):
    """5 steps captured in one graph, replayed 10 times (50 steps): the count is published and re-armed by the device
    inside the graph, and after every replay the record holds the last step's ends, as a twin stepping ordinarily sees"""
    torch = torch_cuda
    A, B = _mini_pool_pair(2048, timeout=25)
    ends = A.enable_episode_record()
    n, per = A.n_envs, 5
    rng = np.random.RandomState(2)
    acts = torch.from_numpy(np.stack([A.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], np.float32)
                                      for _ in range(11)])).cuda()
    # one ordinary step each (uploads the parameter blocks), then capture `per` steps of A
    A.step(acts[0])
    B.step(acts[0])
    B.reset(mask=B.done.clone())
    static_a = acts[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            for _ in range(per):
                A.step(static_a)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    # (the capture did not run the steps: A and B are still on the same state)
    for k in range(1, 11):
        static_a.copy_(acts[k])
        graph.replay()
        torch.cuda.synchronize()
        for t in range(per):
            B.step(acts[k])
            if t < per - 1:
                B.reset(mask=B.done.clone())
        m = int(ends.count[0])
        assert m == int(A.done.sum()) == int(B.done.sum()), k
        ids = torch.sort(ends.env_ids[:m]).values
        assert torch.equal(ids, torch.nonzero(B.done).flatten().int()), k
        _check_state_rows(ends, B, ends.env_ids[:m], m)
        B.reset(mask=B.done.clone())
        _full_state_equal(A, B)
    A.check_errors()


def test_endless_pool_final_images_across_refreshes(torch_cuda, oracle):
    """BatchedRandomMiniEnv(endless=True) with refresh(overlap=True) every 16 steps: the final images equal the images the
    reference's extract_egocentric_costmap draws from the pool entries downloaded before the refresh (the wrapper draws
    them in step(), before a refresh can release the worlds the envs have just left)"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, mini_env
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    params = mini_env.RandomMiniEnvParams(
        env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=12))
    n = 96
    env = mini_env.BatchedRandomMiniEnv(n, params, seeds=list(range(500, 500 + n)), episodes=5, endless=True,
                                        auto_reset=True, seed=9)
    wrap = BatchedEgocentricCostmap(env, final_observation=True)
    ends = env.episode_ends
    res = params.env_params.resolution
    rng = np.random.RandomState(3)
    pending, checked, refreshes = [], 0, 0

    def check_window():
        nonlocal checked
        torch.cuda.synchronize()
        pool = env.pool
        maps = pool.maps.cpu().numpy()
        vr = pool.valid_rows.cpu().numpy() if pool.valid_rows is not None else None
        vc = pool.valid_cols.cpu().numpy() if pool.valid_cols is not None else None
        orgs = pool.origins.cpu().numpy() if pool.origins is not None else None
        for imgs, geom, poses in pending:
            for j in range(len(geom)):
                g = int(geom[j])
                data = maps[g] if vr is None else maps[g, :vr[g], :vc[g]]
                origin = pool.origin if orgs is None else orgs[g]
                ref = oracle.extract_egocentric(data, origin, res, poses[:, j], (-0.5, -2.0), (3.5, 4.0))
                assert (ref == imgs[j]).all(), (g, j)
                checked += 1
        pending.clear()

    for t in range(80):
        a = env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32)
        _o, _r, d, info = wrap.step(a)
        m = int(ends.count[0])
        assert m == int(d.sum())
        if m:
            pending.append((info["final_observation"]["env"][:m, :, :, 0].cpu().numpy(), ends.geom[:m].cpu().numpy(),
                            ends.final_state.robot[0:3, :m].cpu().numpy()))
        if t % 16 == 15:
            check_window()           # the entries as they are before the refresh
            env.refresh(overlap=True)
            refreshes += 1
    check_window()
    env.finish_refresh()
    env.check_errors()
    assert refreshes == 5 and checked > 100


def test_full_size_aisle_with_final_observations(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import aisle_env
    from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap
    n = 65536
    env = aisle_env.BatchedRandomAisleTurnEnv(n, seeds=list(range(1024)), episodes=4, sampler="device_resident",
                                              auto_reset=True, seed=1)
    wrap = BatchedColoredEgoCostmap(env, final_observation=True)
    wrap.reset()
    ends = env.episode_ends
    rng = np.random.RandomState(0)
    total = 0
    for t in range(200):
        a = torch.from_numpy(env.action_space.sample_batch(n, rng)).cuda()
        _o, _r, d, info = wrap.step(a)
        assert "final_observation" in info
        if t % 20 == 19:
            m = int(ends.count[0])
            assert m == int(d.sum()) and not ends.overflowed()
            total += m
    env.check_errors()
    assert total > 0


def test_refusals_and_default(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import _lib
    A, B = _mini_pool_pair(512)
    C_, _ = _mini_pool_pair(512)
    rng = np.random.RandomState(4)
    for t in range(30):
        a = torch.from_numpy(A.action_space.sample_batch(512, rng)).cuda()
        _o, _r, _d, info = A.step(a)
        assert info == {}
        C_.step(a)
        if t == 0:
            C_.enable_episode_record()
        if t == 15:
            C_.disable_episode_record()
    _full_state_equal(A, C_)
    ends = A.enable_episode_record()
    with pytest.raises(_lib.BcpError):
        A.rollout(torch.zeros(2, 512, 2, dtype=torch.float64, device="cuda"))
    assert ends is A.episode_ends

"""Aisle-turn worlds on the GPU (bc_gym_planning_env_amd/aisle_env.py, csrc/bcp_aisle.h): the device sampler against
the reference's worlds (g14, g12) and against the host sampler, and BatchedRandomAisleTurnEnv stepping and resetting
onto new turns against the reference's recorded trajectories and the oracle."""
import os

import numpy as np
import pytest

from util import ATOL, GOLDEN, z_in

pytestmark = pytest.mark.gpu

COORD = 1e-12   # device transcendentals can move a last bit (the mini sampler's rule)


def _g14():
    return np.load(os.path.join(GOLDEN, "g14_aisle_worlds.npz"))


def _lethal(g, k):
    rows, cols = [int(v) for v in g["shape"].reshape(-1, 2)[k]]
    bits = g["lethal"][g["lethal_offset"][k]:g["lethal_offset"][k + 1]].reshape(rows, -1)
    return np.unpackbits(bits, axis=1)[:, :cols].astype(bool)


def _turn_vec(w):
    return np.array([w.main_corridor_length, w.turn_corridor_length, w.turn_corridor_angle, w.main_corridor_width,
                     w.turn_corridor_width, w.flip_arnd_oy, w.flip_arnd_ox, w.rot_theta], dtype=np.float64)


def _check_padding(dp):
    import torch
    rows, pitch = dp.maps.shape[1:]
    r = torch.arange(rows, device=dp.maps.device)[None, :, None]
    c = torch.arange(pitch, device=dp.maps.device)[None, None, :]
    outside = (r >= dp.valid_rows[:, None, None]) | (c >= dp.valid_cols[:, None, None])
    assert int((dp.maps * outside).max()) == 0
    assert pitch % 64 == 0 and pitch - 64 < int(dp.valid_cols.max()) <= pitch and int(dp.valid_rows.max()) == rows


def test_device_sampler_reproduces_g14_and_g12(torch_cuda):
    from bc_gym_planning_env_amd import EnvParams, aisle_env
    g = _g14()
    seeds, K = [int(s) for s in g["seeds"]], g["turn_params"].shape[1]
    pool = aisle_env.sample_aisle_pool_device(EnvParams(), seeds, K)
    for k in range(len(pool)):
        s, e = divmod(k, K)
        np.testing.assert_allclose(_turn_vec(pool.worlds[k]), g["turn_params"][s, e], rtol=0, atol=COORD)
        cm = pool.costmaps[k]
        assert cm.get_data().shape == tuple(g["shape"][s, e]), k
        assert ((cm.get_data() == 254) == _lethal(g, k)).all(), k
        assert set(np.unique(cm.get_data())) <= {0, 254}
        np.testing.assert_allclose(cm.get_origin(), g["origin"][s, e], rtol=0, atol=COORD)
        np.testing.assert_allclose(pool.paths[k], g["coarse_path"][s, e], rtol=0, atol=COORD)
    dp = aisle_env.sample_aisle_pool_device(EnvParams(), seeds, K, keep_on_device=True)
    _check_padding(dp)
    for k in range(len(dp)):
        s, e = divmod(k, K)
        want = g["path"][g["path_offset"][k]:g["path_offset"][k + 1]]
        got = dp.paths[k]
        assert got.shape == want.shape, k
        np.testing.assert_allclose(got, want, rtol=0, atol=COORD)
        assert float(dp.init[k, 1]) == g["init"][s, e, 1]
        np.testing.assert_allclose(float(dp.init[k, 0]), g["init"][s, e, 0], rtol=0, atol=COORD)
        assert ((dp.costmaps[k].get_data() == 254) == _lethal(g, k)).all(), k
    g12 = np.load(os.path.join(GOLDEN, "g12_colored_ego.npz"))
    k3 = seeds.index(3) * K
    cm = dp.costmaps[k3]
    assert cm.get_data().shape == g12["costmap"].shape and (cm.get_data() == g12["costmap"]).all()
    np.testing.assert_allclose(cm.get_origin(), g12["origin"], rtol=0, atol=COORD)
    np.testing.assert_allclose(dp.paths[k3], g12["path"], rtol=0, atol=COORD)


def test_device_sampler_matches_host_sampler(torch_cuda):
    """1024 seeds x 4 worlds: maps and shapes identical, padding zero, coordinates within 1e-12; the device-resident
    refined paths and initial reward states against the host's"""
    from bc_gym_planning_env_amd import EnvParams, aisle_env, host_init
    ep = EnvParams()
    seeds = list(range(5000, 6024))
    host = aisle_env.sample_aisle_pool(ep, seeds, 4)
    dp = aisle_env.sample_aisle_pool_device(ep, seeds, 4, keep_on_device=True)
    _check_padding(dp)
    maps = dp.maps.cpu().numpy()
    shapes = dp.shapes.cpu().numpy()
    origins = dp.origins.cpu().numpy()
    rec = dp.world_params.cpu().numpy()
    paths, lens, init = dp.path_points.cpu().numpy(), dp.lens.cpu().numpy(), dp.init.cpu().numpy()
    rp = ep.reward_provider_params
    for k in range(len(host)):
        cm = host.costmaps[k]
        rows, cols = cm.get_data().shape
        assert tuple(shapes[k]) == (rows, cols), k
        assert (maps[k, :rows, :cols] == cm.get_data()).all(), k
        np.testing.assert_allclose(origins[k], cm.get_origin(), rtol=0, atol=COORD)
        np.testing.assert_allclose(rec[k, :8], _turn_vec(host.worlds[k]), rtol=0, atol=COORD)
        np.testing.assert_allclose(rec[k, 30:42].reshape(4, 3), host.paths[k], rtol=0, atol=COORD)
        refined = host_init.refine_path(host.paths[k], ep.path_delta)
        assert lens[k] == len(refined) == rec[k, 42], k
        np.testing.assert_allclose(paths[k, :lens[k]], refined, rtol=0, atol=COORD)
        md, ti = host_init.initial_reward_state(refined, rp)
        assert init[k, 1] == ti
        np.testing.assert_allclose(init[k, 0], md, rtol=0, atol=COORD)
    del maps
    # the same worlds downloaded into host objects (the padded pool holds more than 2^31 cells: grouped downloads)
    down = aisle_env.sample_aisle_pool_device(ep, seeds, 4)
    assert len(down) == len(host)
    for k in range(len(host)):
        a, b = down.costmaps[k], host.costmaps[k]
        assert a.get_data().shape == b.get_data().shape and (a.get_data() == b.get_data()).all(), k
        np.testing.assert_allclose(a.get_origin(), b.get_origin(), rtol=0, atol=COORD)
        np.testing.assert_allclose(down.paths[k], host.paths[k], rtol=0, atol=COORD)


@pytest.mark.parametrize("sampler", ["host", "device", "device_resident"])
def test_env_reproduces_g14_trajectories(torch_cuda, sampler):
    """ColoredEgoCostmapRandomAisleTurnEnv trajectories of the reference, through an episode end and the reset onto the
    chain's next turn: done / collision bit-exact, state and reward within 1e-9, observation images and goal vectors"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import aisle_env
    from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap
    g = _g14()
    for j in range(int(g["n_traj"])):
        t_ = lambda k: g["t%d_%s" % (j, k)]   # noqa: E731
        env = aisle_env.BatchedRandomAisleTurnEnv(1, seeds=[int(t_("seed"))], episodes=4, sampler=sampler, auto_reset=True)
        # seed(s); reset(): the env goes to world 0 of its chain (the constructor left it on world 1)
        env.geom_of_env.fill_(3)
        wrap = BatchedColoredEgoCostmap(env)
        wrap.reset()
        cols = int(t_("image_cols"))
        imgs, resets = np.unpackbits(t_("images"), axis=2)[:, :, :cols], 0
        reset_imgs = np.unpackbits(t_("reset_images"), axis=2)[:, :, :cols]
        for t in range(len(t_("done"))):
            a = torch.from_numpy(t_("actions")[t:t + 1].copy()).cuda()
            z = torch.from_numpy(z_in(t_("z")[t:t + 1])).cuda()
            obs, r, d, _ = wrap.step(a, noise_z=z)
            assert int(d[0]) == t_("done")[t], (j, t)
            assert int(env.collided_now[0]) == t_("collided")[t], (j, t)
            assert abs(float(r[0]) - t_("reward")[t]) <= ATOL, (j, t)
            if t_("done")[t]:
                want_state, want_img, want_goal = t_("reset_states")[resets], reset_imgs[resets], t_("reset_goal")[resets]
                resets += 1
                assert int(env.geom_of_env[0]) == resets % 4
            else:
                want_state, want_img, want_goal = t_("states")[t], imgs[t], t_("goal")[t]
            np.testing.assert_allclose(env.state.robot[:, 0].cpu().numpy(), want_state, rtol=0, atol=ATOL)
            img = obs['environment'][0, :, :, 0].cpu().numpy()
            assert ((img == 254) == want_img).all(), (j, t)
            np.testing.assert_allclose(obs['goal'][0, :, 0].cpu().numpy(), want_goal, rtol=0, atol=ATOL)
        assert resets >= 1
        st = env.envs[0].get_state()
        cm = env.pool.costmaps[int(env.geom_of_env[0])]
        assert st.costmap.get_data().shape == cm.get_data().shape and (st.costmap.get_data() == cm.get_data()).all()
        assert (st.costmap.get_origin() == cm.get_origin()).all()
        env.check_errors()


def _largest_chains(aisle_env, ep, n_chains, n_big):
    """n_chains seeds for a pool that holds the largest maps of a 2048-seed sweep"""
    sweep = aisle_env.sample_aisle_pool_device(ep, list(range(2048)), 4, keep_on_device=True)
    area = (sweep.shapes[:, 0].long() * sweep.shapes[:, 1].long()).reshape(2048, 4).max(1).values.cpu().numpy()
    big = list(np.argsort(-area)[:n_big])
    rest = list(range(2048, 2048 + n_chains - n_big))
    return [int(s) for s in big] + rest, int(area.max())


def test_batch_with_auto_reset_vs_oracle(torch_cuda, oracle):
    """2048 envs on 128 chains x 4 turns (the 24 chains with the largest maps of a 2048-seed sweep among them), short
    episodes, 300 auto-reset steps: every env against the oracle fed with the env's downloaded world"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, aisle_env
    ep = EnvParams(iteration_timeout=60)
    seeds, biggest = _largest_chains(aisle_env, ep, 128, 24)
    n, steps = 2048, 300
    env = aisle_env.BatchedRandomAisleTurnEnv(n, ep, seeds=seeds, episodes=4, sampler="device_resident", auto_reset=True,
                                              seed=5)
    dp = env.pool
    rows, cols = [int(v) for v in dp.shapes.cpu().numpy().max(0)]
    assert rows * cols >= biggest and max(rows, cols) > 512
    padded = dp.maps.cpu().numpy()
    vr, vc = dp.valid_rows.cpu().numpy(), dp.valid_cols.cpu().numpy()
    maps = np.zeros((len(dp), rows, cols), dtype=np.uint8)   # the oracle reads entry g as vr[g] rows of vc[g] cells
    for g_ in range(len(dp)):
        maps[g_].reshape(-1)[:vr[g_] * vc[g_]] = padded[g_, :vr[g_], :vc[g_]].ravel()
    del padded
    lens = dp.lens.cpu().numpy()
    p = oracle.make_params("tricycle", noise=oracle.PLANENV_NOISE, spatial_precision=ep.goal_spat_dist,
                           angular_precision=ep.goal_ang_dist, iteration_timeout=60)
    i = np.arange(n)
    geom0 = (i % 128) * 4 + (i // 128) % 4
    ref = oracle.OracleBatch(p, n, maps, dp.origins.cpu().numpy(), ep.resolution, dp.path_points.cpu().numpy(),
                             lens=lens, rows=vr, cols=vc, geom=geom0, next_geom=dp.next_geom)
    ref.reset_from_paths()
    ref.reset_all_to_geom(advance=True)
    rng = np.random.RandomState(21)
    zout = torch.zeros(n, 3, dtype=torch.float64, device="cuda")
    resets = hits = 0
    for t in range(steps):
        a = env.action_space.sample_batch(n, rng)
        a[:, 0] *= 3.0
        env.step(a, noise_z_out=zout)
        ref.step(a.astype(np.float64), z_in(zout.cpu().numpy()), auto_reset=True, threads=16)
        np.testing.assert_array_equal(env.done.cpu().numpy(), ref.done, err_msg="done step %d" % t)
        np.testing.assert_array_equal(env.collided_now.cpu().numpy(), ref.collided_now, err_msg="collided step %d" % t)
        np.testing.assert_allclose(env.reward.cpu().numpy(), ref.reward, rtol=0, atol=ATOL)
        np.testing.assert_array_equal(env.geom_of_env.cpu().numpy(), ref.geom)
        np.testing.assert_array_equal(env.state.target_idx.cpu().numpy(), ref.target_idx)
        np.testing.assert_allclose(env.state.robot.cpu().numpy(), np.stack(ref.st), rtol=0, atol=ATOL)
        resets += int(ref.done.sum())
        hits += int(ref.collided_now.sum())
    assert resets > n and hits > 100
    env.check_errors()


def test_full_size_65536_envs(torch_cuda):
    """65 536 envs on 1024 chains x 4 turns (device-resident pool): construct, 200 auto-reset steps, check_errors()"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import aisle_env
    from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap
    n = 65536
    env = aisle_env.BatchedRandomAisleTurnEnv(n, n_chains=1024, episodes=4, sampler="device_resident", auto_reset=True)
    wrap = BatchedColoredEgoCostmap(env)
    print("aisle pool: %d worlds, maps %s, %.1f MB on the device" % (len(env.pool), tuple(env.pool.maps.shape),
                                                                     env.pool.nbytes() / 1e6))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    lo = torch.tensor(env.action_space.low, dtype=torch.float64, device="cuda")
    hi = torch.tensor(env.action_space.high, dtype=torch.float64, device="cuda")
    done_total = torch.zeros((), dtype=torch.int64, device="cuda")
    for t in range(200):
        a = lo + (hi - lo) * torch.rand((n, 2), dtype=torch.float64, device="cuda", generator=gen)
        a[:, 0] *= 3.0
        obs, _r, d, _ = wrap.step(a)
        done_total += d.long().sum()
    torch.cuda.synchronize()
    env.check_errors()
    assert int(done_total) > n // 4
    assert set(np.unique(obs['environment'][:64].cpu().numpy())) <= {0, 254}
    assert len(np.unique(env.geom_of_env.cpu().numpy())) > 2048


def test_egocentric_wrapper_on_aisle_envs(torch_cuda, oracle):
    """EgocentricCostmap over BatchedRandomAisleTurnEnv: after every step each env's observation matches the oracle on
    that env's own map and state, also right after an auto-reset onto the chain's next turn"""
    from bc_gym_planning_env_amd import EnvParams, aisle_env
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    ep = EnvParams(iteration_timeout=15)
    n = 48
    env = aisle_env.BatchedRandomAisleTurnEnv(n, ep, n_chains=6, episodes=3, sampler="device_resident", auto_reset=True,
                                              seed=2)
    wrap = BatchedEgocentricCostmap(env)
    rng = np.random.RandomState(0)
    res = ep.resolution
    rows, cols = wrap.image_shape
    world = np.array([(-0.5 + res * cols) - -0.5, (-2.0 + res * rows) - -2.0])
    seen = set()
    for t in range(40):
        obs, _r, _d, _ = wrap.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
        img = obs['env'].cpu().numpy()[..., 0]
        vec = obs['goal_n_state'].cpu().numpy()[..., 0]
        st = env.state.robot.cpu().numpy()
        geom = env.geom_of_env.cpu().numpy()
        tidx = env.state.target_idx.cpu().numpy()
        for i in range(0, n, 5):
            cm = env.costmap_of(i)
            ref = oracle.extract_egocentric(cm.get_data(), cm.get_origin(), res, st[:3, i], (-0.5, -2.0), (3.5, 4.0))
            assert (ref == img[i]).all(), (t, i)
            rs = np.array([st[0, i], st[1, i], st[2, i], st[3, i], st[4, i], st[6, i]])
            want = oracle.goal_n_state(st[:3, i], env.path_of(i)[tidx[i]:], world, rs)
            np.testing.assert_allclose(vec[i], want, rtol=0, atol=1e-6)
            seen.add(int(geom[i]))
    assert len(seen) > 6


def test_thick_walls_are_refused_on_the_device(torch_cuda):
    """resolutions under 0.025 m would make the walls 2 px thick: the C ABI refuses them (as the host does)"""
    from bc_gym_planning_env_amd import EnvParams, _lib, aisle_env
    with pytest.raises(_lib.BcpError, match="thicker than one pixel"):
        aisle_env.sample_aisle_pool_device(EnvParams(resolution=0.024), [0], 1)
    with pytest.raises(NotImplementedError):
        aisle_env.sample_aisle_pool(EnvParams(resolution=0.024), [0], 1)

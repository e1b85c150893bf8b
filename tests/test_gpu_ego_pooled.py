"""The pooled egocentric observation (bcp_egocentric_costmaps_pooled: the maximum of every pool x pool block of the image
bcp_egocentric_costmaps would have written) on the GPU, bit for bit against block_max (tests/ego_pooled_ref.py) of the
reference's recorded images and of the oracle's images -- never against the full-resolution call."""
import ctypes as C
import os

import numpy as np
import pytest

from ego_pooled_ref import block_max
from util import GOLDEN

pytestmark = pytest.mark.gpu

SPARSE, SAMPLED = "ego_pooled_sparse_kernel", "ego_pooled_sampled_kernel"
E_INVALID = -1
PATH = np.array([[0., 0., 0.], [1., 0., 0.], [2., 0., 0.]])
REF_WINDOW = (np.array((-0.5, -2.0)), np.array((3.5, 4.0)))     # the reference's window: 80 x 70 px at 5 cm


def _f64p(v):
    return v.ctypes.data_as(C.POINTER(C.c_double)) if v is not None else None


def _route(env):
    from bc_gym_planning_env_amd import _lib
    info = (C.c_int32 * 4)()
    _lib.check(env._lib.bcp_egocentric_route(env._h, info))
    return _lib.EGO_KERNELS[int(info[0])], int(info[1]), int(info[2]), int(info[3])


def _pooled_shape(env, s, pool):
    from bc_gym_planning_env_amd import _lib
    shape = (C.c_int32 * 2)()
    _lib.check(env._lib.bcp_egocentric_pooled_shape(env._h, _f64p(s), pool, shape))
    return int(shape[0]), int(shape[1])


def _draw(torch, env, pt, o, s, border, pool, poison=99):
    """bcp_egocentric_costmaps_pooled into a poisoned buffer; a 16-byte guard tensor must come back untouched"""
    from bc_gym_planning_env_amd import _lib
    n = pt.shape[0]
    shape = _pooled_shape(env, s, pool)
    out = torch.full((n,) + shape, poison, dtype=torch.uint8, device="cuda")
    guard = torch.full((16,), 123, dtype=torch.uint8, device="cuda")
    _lib.check(env._lib.bcp_egocentric_costmaps_pooled(env._h, pt.data_ptr(), n, _f64p(o), _f64p(s), border, pool,
                                                       out.data_ptr(), None))
    got = out.cpu().numpy()
    assert (guard.cpu().numpy() == 123).all()
    return got


def _full(torch, env, pt, o, s, border):
    from bc_gym_planning_env_amd import _lib
    shape = (C.c_int32 * 2)()
    _lib.check(env._lib.bcp_egocentric_shape(env._h, _f64p(s), shape))
    out = torch.full((pt.shape[0], shape[0], shape[1]), 99, dtype=torch.uint8, device="cuda")
    _lib.check(env._lib.bcp_egocentric_costmaps(env._h, pt.data_ptr(), pt.shape[0], _f64p(o), _f64p(s), border, out.data_ptr(), None))
    return out.cpu().numpy()


# ---- 1. the reference's recorded images --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g10_ego_mini_00.npz", "g10_ego_mini_05.npz", "g10_ego_aisle.npz"])
def test_g10_pooled_observation_from_reference_states(torch_cuda, name):
    """pool 2, 7 and 8 on the 133 x 117 window: 7 divides 133 (exact edge blocks), 8 divides neither side (partial ones)"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    g = np.load(os.path.join(GOLDEN, name))
    n, res = len(g["states"]), float(g["resolution"])
    env = BatchedPlanEnv(CostMap2D(g["costmap"], res, g["origin"]), g["path"], EnvParams(resolution=res, refine_path=False),
                         n_envs=n)
    env.state.robot.copy_(torch.from_numpy(np.ascontiguousarray(g["states"].T)).cuda())
    env.state.target_idx.copy_(torch.from_numpy(g["target_idx"]).cuda())
    rows, cols = (int(v) for v in g["image_shape"])
    recorded = np.unpackbits(g["images"], axis=2)[:, :, :cols].astype(np.uint8) * 254
    for pool in (2, 7, 8):
        wrap = BatchedEgocentricCostmap(env, pool=pool)
        assert wrap.full_image_shape == (rows, cols) and wrap.image_shape == (-(-rows // pool), -(-cols // pool))
        obs = wrap.observation()
        img = obs['env'].cpu().numpy()
        assert img.shape == (n,) + wrap.image_shape + (1,)
        assert (img[..., 0] == block_max(recorded, pool)).all(), pool
        # (these maps are far under the limit: the sparse route, at pool = 2 with three waves per workgroup instead of eight)
        assert wrap.route()["kernel"] == SPARSE
        np.testing.assert_allclose(obs['goal_n_state'].cpu().numpy()[:, :, 0], g["goal_n_state"], rtol=0, atol=1e-6)
    assert (block_max(recorded, 8) != 0).any()


def test_g12_colored_pooled_observation(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap
    g = np.load(os.path.join(GOLDEN, "g12_colored_ego.npz"))
    n, res = len(g["states"]), float(g["resolution"])
    env = BatchedPlanEnv(CostMap2D(g["costmap"], res, g["origin"]), g["path"], EnvParams(resolution=res, refine_path=False),
                         n_envs=n)
    env.state.robot.copy_(torch.from_numpy(np.ascontiguousarray(g["states"].T)).cuda())
    wrap = BatchedColoredEgoCostmap(env, pool=8)
    assert wrap.full_image_shape == (133, 133) and wrap.image_shape == (17, 17)
    obs = wrap.observation()
    recorded = np.unpackbits(g["images"], axis=2)[:, :, :133].astype(np.uint8) * 254
    img = obs['environment'].cpu().numpy()
    assert img.shape == (n, 17, 17, 1) and (img[..., 0] == block_max(recorded, 8)).all()
    assert wrap.route()["kernel"] == SPARSE
    assert (img != 0).any()
    np.testing.assert_allclose(obs['goal'].cpu().numpy()[:, :, 0], g["goal"], rtol=0, atol=1e-9)


# ---- 2. random poses, dense maps with arbitrary bytes, every window and border of test_random_poses_vs_oracle ------------
@pytest.mark.parametrize("shared", [True, False, "large", "medium"],
                         ids=["shared-map", "private-maps", "large-shared-map", "medium-shared-map"])
def test_pooled_random_poses_vs_oracle(torch_cuda, oracle, shared):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    rng = np.random.RandomState(8)
    n, res = 96, 0.05
    large = shared in ("large", "medium")
    medium = shared == "medium"
    shared = bool(shared)
    shapes = [(330, 290)] if medium else [(420, 400)] if large else ([(90, 70)] if shared else [(90, 70), (64, 101), (300, 260)])
    maps = [rng.randint(0, 256, s).astype(np.uint8) for s in shapes]
    orgs = [rng.uniform(-2, 0, 2) for _ in shapes]
    params = EnvParams(resolution=res, refine_path=False)
    if shared:
        env = BatchedPlanEnv(CostMap2D(maps[0], res, orgs[0]), PATH, params, n_envs=n)
    else:
        env = BatchedPlanEnv([CostMap2D(maps[i % 3], res, orgs[i % 3]) for i in range(n)], [PATH] * n, params, n_envs=n)
    hi = 23 if large else 6
    poses = np.stack([rng.uniform(-4, hi, n), rng.uniform(-4, hi, n), rng.uniform(-7, 7, n)], axis=1)
    poses[0] = (0., 0., 0.)
    poses[1] = (1.0, 1.0, np.pi)
    poses[2:6, 2] = (15.0, -15.0, 40 * np.pi + 0.3, -1000.7)
    pt = torch.from_numpy(poses).cuda()
    for org, size, border in (((-0.5, -2.0), (3.5, 4.0), 0), ((-1.0, -1.0), (2.0, 2.0), 255), (None, None, 7),
                              ((-3.0, -0.7), (6.05, 1.45), 100), ((-0.1, -0.15), (0.3, 0.25), 9)):
        o = None if org is None else np.array(org, dtype=np.float64)
        s = None if size is None else np.array(size, dtype=np.float64)
        compare = not (size is None and not shared)   # (whole-map output of padded private maps has no reference counterpart)
        ref = None
        if compare:
            ref = np.stack([oracle.extract_egocentric(maps[0 if shared else i % 3], orgs[0 if shared else i % 3], res, poses[i],
                                                      o, s, border) for i in range(n)])
        full_shape = _pooled_shape(env, s, 1)
        for pool in (1, 2, 3, 5, 8, 16, 64):
            got = _draw(torch, env, pt, o, s, border, pool)
            assert got.shape == (n, -(-full_shape[0] // pool), -(-full_shape[1] // pool))
            if pool == 1:
                assert (got == _full(torch, env, pt, o, s, border)).all()
            else:
                assert _route(env)[0] == SAMPLED    # (dense maps, or a non-zero border)
            if not compare:
                # no expectation for these bytes, but every one of them is written: a second poison gives the same image
                assert (got == _draw(torch, env, pt, o, s, border, pool, poison=100)).all(), pool
            if compare:
                want = block_max(ref, pool)
                assert want.shape == got.shape and (want == got).all(), (org, size, pool, int((want != got).sum()))


# ---- 3 .. 6: the sparse route ---------------------------------------------------------------------------------------------
def _sparse_map(rng, shape, fraction=0.03):
    m = np.zeros(shape, dtype=np.uint8)
    k = int(round(fraction * shape[0] * shape[1]))
    m[rng.randint(0, shape[0], k), rng.randint(0, shape[1], k)] = rng.randint(1, 256, k)
    return m


def _sparse_env(kind, n, seed):
    """shared 90 x 70 map, or a geometry pool of 3 entries: zero except ~3 % of the cells, random values 1 .. 255"""
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    rng = np.random.RandomState(seed)
    res = 0.05
    params = EnvParams(resolution=res, refine_path=False)
    if kind == "shared":
        maps, orgs = [_sparse_map(rng, (90, 70))], [rng.uniform(-2, 0, 2)]
        env = BatchedPlanEnv(CostMap2D(maps[0], res, orgs[0]), PATH, params, n_envs=n)
        map_of = lambda i: 0
    else:
        maps = [_sparse_map(rng, s) for s in ((90, 70), (64, 101), (80, 80))]
        orgs = [rng.uniform(-2, 0, 2) for _ in maps]
        geom = (np.arange(n) * 7 % 3).astype(np.int32)
        env = BatchedPlanEnv([CostMap2D(m, res, o) for m, o in zip(maps, orgs)], [PATH] * 3, params, n_envs=n, geom_of_env=geom)
        geom = env.geom_of_env.cpu().numpy()
        map_of = lambda i: int(geom[i])
    assert max(int((m != 0).sum()) for m in maps) < 512
    poses = np.stack([rng.uniform(-1, 4, n), rng.uniform(-1, 4, n), rng.uniform(-7, 7, n)], axis=1)
    poses[0] = (1.0, 1.0, 0.3)
    return env, maps, orgs, map_of, poses, res


def _oracle_images(oracle, maps, orgs, map_of, poses, res, o, s, border=0):
    return np.stack([oracle.extract_egocentric(maps[map_of(i)], orgs[map_of(i)], res, poses[i], o, s, border)
                     for i in range(len(poses))])


def _blocks_with_two_values(ref, pool):
    """blocks over the batch that hold two or more distinct non-zero values (from the oracle's images alone)"""
    top = block_max(ref, pool).astype(np.int32)
    low = 255 - block_max(np.where(ref != 0, 255 - ref, 0).astype(np.uint8), pool).astype(np.int32)   # least non-zero value
    return int(((top != 0) & (low != top)).sum())


@pytest.mark.parametrize("kind", ["shared", "pool"])
def test_sparse_route_where_the_maximum_matters(torch_cuda, oracle, kind):
    """cells with different values meet in one block: a plain store would keep whichever landed last"""
    torch = torch_cuda
    n = 96
    env, maps, orgs, map_of, poses, res = _sparse_env(kind, n, 31)
    pt = torch.from_numpy(poses).cuda()
    o, s = REF_WINDOW
    ref = _oracle_images(oracle, maps, orgs, map_of, poses, res, o, s)
    for pool in (4, 8, 2):    # (2: 1 400 words per image, six waves per workgroup instead of eight)
        assert pool == 2 or _blocks_with_two_values(ref, pool) >= 50
        got = _draw(torch, env, pt, o, s, 0, pool)
        assert _route(env)[0] == SPARSE
        want = block_max(ref, pool)
        assert (want == got).all(), (pool, int((want != got).sum()))


def test_entry_with_more_cells_than_its_list_inside_the_sparse_launch(torch_cuda, oracle):
    """BCP_TUNE_EGO_LIST_STRIDE = 64 and one of three private maps with ~700 cells: that entry's images are sampled inside
    the pooled sparse launch, the others come from their lists"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    rng = np.random.RandomState(11)
    res, n = 0.05, 96
    maps = []
    for k, shp in enumerate([(90, 70), (64, 101), (120, 120)]):
        m = np.zeros(shp, dtype=np.uint8)
        cells = 60 if k < 2 else 700
        m[rng.randint(0, shp[0], cells), rng.randint(0, shp[1], cells)] = rng.randint(1, 256, cells)
        maps.append(m)
    orgs = [rng.uniform(-2, 0, 2) for _ in maps]
    env = BatchedPlanEnv([CostMap2D(maps[i % 3], res, orgs[i % 3]) for i in range(n)], [PATH] * n,
                         EnvParams(resolution=res, refine_path=False), n_envs=n)
    env.set_tuning(ego_sparse=4096, ego_list_stride=64)
    poses = np.stack([rng.uniform(-1, 5, n), rng.uniform(-1, 5, n), rng.uniform(-7, 7, n)], axis=1)
    pt = torch.from_numpy(poses).cuda()
    o, s = REF_WINDOW
    got = _draw(torch, env, pt, o, s, 0, 8)
    kernel, counted, stride, _limit = _route(env)
    assert kernel == SPARSE and stride == 64 and counted > 500
    ref = _oracle_images(oracle, maps, orgs, lambda i: i % 3, poses, res, o, s)
    want = block_max(ref, 8)
    assert (want == got).all(), int((want != got).sum())
    assert int((want[2::3] != 0).sum()) > 100 and int((want[0::3] != 0).sum()) > 10


def test_window_with_more_cells_than_a_wave_holds(torch_cuda, oracle):
    """a filled 40 x 40 block under the robot: more than kEgoHeld = 768 cells inside one window, the pooled words accumulate
    over several passes"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    rng = np.random.RandomState(5)
    res, n = 0.05, 64
    m = np.zeros((150, 160), dtype=np.uint8)
    m[60:100, 50:90] = rng.randint(1, 256, (40, 40))
    m[10, 5:150] = 254
    org = np.array([-1.0, -0.5])
    env = BatchedPlanEnv(CostMap2D(m, res, org), PATH, EnvParams(resolution=res, refine_path=False), n_envs=n)
    poses = np.stack([rng.uniform(0.5, 4.5, n), rng.uniform(1.5, 5.0, n), rng.uniform(-7, 7, n)], axis=1)
    pt = torch.from_numpy(poses).cuda()
    o, s = REF_WINDOW
    env.set_tuning(ego_sparse=4096)
    got = _draw(torch, env, pt, o, s, 0, 8)
    assert _route(env)[0] == SPARSE
    ref = _oracle_images(oracle, [m], [org], lambda i: 0, poses, res, o, s)
    assert int(((ref != 0).sum(axis=(1, 2)) > 768).sum()) > 10
    want = block_max(ref, 8)
    assert (want == got).all(), int((want != got).sum())


def test_forced_routes_agree(torch_cuda, oracle):
    """BCP_TUNE_EGO_SPARSE = 0 (sampled) and a large explicit limit (sparse): the same bytes, and the oracle's"""
    torch = torch_cuda
    n = 96
    env, maps, orgs, map_of, poses, res = _sparse_env("pool", n, 47)
    pt = torch.from_numpy(poses).cuda()
    for o, s in (REF_WINDOW, (np.array((-3.0, -0.7)), np.array((6.05, 1.45)))):
        ref = _oracle_images(oracle, maps, orgs, map_of, poses, res, o, s)
        for pool in (3, 8):
            env.set_tuning(ego_sparse=0)
            sampled = _draw(torch, env, pt, o, s, 0, pool)
            assert _route(env)[0] == SAMPLED
            env.set_tuning(ego_sparse=100000)
            sparse = _draw(torch, env, pt, o, s, 0, pool)
            assert _route(env)[0] == SPARSE and _route(env)[3] == 100000
            want = block_max(ref, pool)
            assert (sampled == sparse).all() and (want == sparse).all(), (pool, int((want != sparse).sum()))
            assert (want != 0).any()


@pytest.mark.parametrize("n", [257, 1])
def test_batch_edges(torch_cuda, oracle, n):
    """one more image than a multiple of the waves per workgroup and of 64; a single image"""
    torch = torch_cuda
    env, maps, orgs, map_of, poses, res = _sparse_env("shared", n, 63)
    pt = torch.from_numpy(poses).cuda()
    o, s = REF_WINDOW
    got = _draw(torch, env, pt, o, s, 0, 8)
    assert _route(env)[0] == SPARSE
    want = block_max(_oracle_images(oracle, maps, orgs, map_of, poses, res, o, s), 8)
    assert got.shape == want.shape == (n, 10, 9) and (want == got).all() and (want != 0).any()


# ---- 7. the episode record's final observations ------------------------------------------------------------------------
def test_final_pooled_observations_of_the_record(torch_cuda, oracle):
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, mini_env
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    params = mini_env.RandomMiniEnvParams(
        env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=12))
    pool = mini_env.sample_pool(params, [1, 2, 3], 3)
    n = 64
    env = mini_env.BatchedRandomMiniEnv(n, params, pool=pool, auto_reset=True, seed=2)
    wrap = BatchedEgocentricCostmap(env, final_observation=True, pool=8)
    assert wrap.image_shape == (17, 15) and wrap.final_images.shape[1:] == (17, 15, 1)
    ends = env.episode_ends
    rng = np.random.RandomState(0)
    res = params.env_params.resolution
    checked = 0
    for t in range(30):
        wrap.final_images.fill_(99)
        _o, _r, d, info = wrap.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
        m = int(ends.count[0])
        assert m == int(d.sum())
        fin = info["final_observation"]["env"].cpu().numpy()[..., 0]
        assert fin.shape == (ends.capacity, 17, 15)
        assert (fin[m:] == 99).all()
        geom = ends.geom[:m].cpu().numpy()
        poses = ends.final_state.robot[0:3, :m].cpu().numpy()
        for j in range(m):
            cm = pool.costmaps[int(geom[j])]
            ref = oracle.extract_egocentric(cm.get_data(), cm.get_origin(), res, poses[:, j], (-0.5, -2.0), (3.5, 4.0))
            assert ref.shape == (133, 117) and (block_max(ref, 8) == fin[j]).all(), (t, j)
            checked += 1
    assert checked > 20


# ---- 8. the wrapper on a refreshing pool, interleaved with a full-resolution wrapper --------------------------------------
def test_wrapper_shares_the_lists_with_the_full_call_across_a_refresh(torch_cuda, oracle):
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, mini_env
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=6))
    n = 128
    env = mini_env.BatchedRandomMiniEnv(n, params, episodes=4, endless=True, auto_reset=True, seed=4)
    pooled, full = BatchedEgocentricCostmap(env, pool=8), BatchedEgocentricCostmap(env)
    assert pooled.full_image_shape == full.image_shape == (133, 117) and pooled.image_shape == (17, 15)
    assert pooled.images.shape == (n, 17, 15, 1)
    rng = np.random.RandomState(3)
    res = params.env_params.resolution

    def check(t):
        small = pooled.observation()['env'].cpu().numpy()
        assert small.shape == (n, 17, 15, 1) and pooled.route()["kernel"] == SPARSE
        big = full.observation()['env'].cpu().numpy()[..., 0]
        assert full.route()["kernel"] == "ego_sparse_kernel"
        again = pooled.observation()['env'].cpu().numpy()
        st = env.state.robot.cpu().numpy()
        geom = env.geom_of_env.cpu().numpy()
        maps = env.pool.maps.cpu().numpy()
        lit = 0
        for i in range(n):
            ref = oracle.extract_egocentric(maps[geom[i]], env.pool.origin, res, st[:3, i], (-0.5, -2.0), (3.5, 4.0))
            assert (ref == big[i]).all(), (t, i)
            want = block_max(ref, 8)
            assert (want == small[i, ..., 0]).all() and (want == again[i, ..., 0]).all(), (t, i)
            lit += int((want != 0).sum())
        assert lit > 0

    for t in range(24):
        env.step(env.action_space.sample_batch(n, rng))
        if t % 8 == 7:
            env.refresh(overlap=True)
        if t in (5, 9, 23):
            if t == 23:
                env.finish_refresh()
            torch.cuda.synchronize()
            check(t)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    n = 4
    env, _maps, _orgs, _map_of, poses, _res = _sparse_env("shared", n, 5)
    pt = torch.from_numpy(poses).cuda()
    o, s = REF_WINDOW
    out = torch.zeros((n, 80, 70), dtype=torch.uint8, device="cuda")
    shape = (C.c_int32 * 2)()
    L = env._lib
    for pool in (0, -1, 65):
        assert L.bcp_egocentric_pooled_shape(env._h, _f64p(s), pool, shape) == E_INVALID
        assert L.bcp_egocentric_costmaps_pooled(env._h, pt.data_ptr(), n, _f64p(o), _f64p(s), 0, pool, out.data_ptr(), None) == E_INVALID
    narrow = np.array((0.15, 0.25))    # 3 px wide
    assert L.bcp_egocentric_costmaps(env._h, pt.data_ptr(), n, _f64p(o), _f64p(narrow), 0, out.data_ptr(), None) == E_INVALID
    assert L.bcp_egocentric_costmaps_pooled(env._h, pt.data_ptr(), n, _f64p(o), _f64p(narrow), 0, 2, out.data_ptr(), None) == E_INVALID
    assert L.bcp_last_error().startswith(b"bcp_egocentric_costmaps_pooled: ")    # (the entry point the caller used)
    assert L.bcp_egocentric_costmaps_pooled(env._h, pt.data_ptr(), n, _f64p(o), _f64p(s), 0, 8, None, None) == E_INVALID
    assert L.bcp_egocentric_costmaps_pooled(env._h, pt.data_ptr(), n, _f64p(o), None, 0, 8, out.data_ptr(), None) == E_INVALID
    torch.cuda.synchronize()
    assert int(out.sum()) == 0       # (nothing was drawn)
    assert L.bcp_egocentric_pooled_shape(env._h, _f64p(s), 64, shape) == 0 and tuple(shape) == (2, 2)

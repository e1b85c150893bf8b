"""bcp_inflate_costmaps on the GPU against the numpy restatement (tests/inflate_ref.py, itself pinned to the genuine reference by
tests/test_inflate_host.py): cost bytes and float32 distances must be EQUAL -- every comparison here is exact.  The restatement's
margin() is asserted for every case first: no pre-truncation value lies within 1e-9 of an integer, so the last bits of the device's
exp() cannot change a byte."""
import ctypes as C
import os

import numpy as np
import pytest

import inflate_ref as R
from ego_pooled_ref import block_max
from util import GOLDEN, env_from_traj

pytestmark = pytest.mark.gpu

E_INVALID = -1
RES, RADIUS, FACTOR = 0.05, 0.3697396548708213, 3.0   # the stock resolution, the tricycle's inscribed radius
REF_WINDOW = ((-0.5, -2.0), (3.5, 4.0))


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from bc_gym_planning_env_amd import NativeOps
    o = NativeOps()
    yield o
    o.close()


def _check(torch, ops, data, resolution=RES, radius=RADIUS, factor=FACTOR, expected=None):
    """one map through NativeOps.inflate_costmap: costs and distances equal the restatement's"""
    if expected is None:
        expected = R.inflate_and_margin(data, resolution, radius, factor)
    assert expected[2] > 1e-9
    cost, dist = ops.inflate_costmap(data, resolution, factor, inscribed_radius=radius, return_distance=True)
    assert cost.dtype == torch.uint8 and dist.dtype == torch.float32 and tuple(cost.shape) == data.shape == tuple(dist.shape)
    assert torch.equal(dist.cpu(), torch.from_numpy(np.array(expected[1])))
    assert torch.equal(cost.cpu(), torch.from_numpy(np.array(expected[0])))
    # without the distances the far field takes a shortcut (cost 0 from d2 alone, shorter walks): the same bytes
    assert torch.equal(ops.inflate_costmap(data, resolution, factor, inscribed_radius=radius), cost)
    return cost


# ---- 1. the fixture cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.case_names())
def test_fixture_case(torch_cuda, ops, name):
    """the 350 x 512 case is the one beyond LDS: its plane goes through the handle's global scratch"""
    c = R.golden_case(name)
    cost = _check(torch_cuda, ops, c["data"], c["resolution"], c["inscribed_radius"], c["cost_scaling_factor"],
                  expected=R.restated_case(name))
    assert torch_cuda.equal(cost.cpu(), torch_cuda.from_numpy(c["expected"]))   # ... and the genuine reference's bytes


def test_footprint_argument_and_default(torch_cuda, ops):
    """footprint=None is the handle's own (the tricycle's); an explicit footprint goes through robots.inscribed_radius"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import robots
    from bc_gym_planning_env_amd.api import INDUSTRIAL_DIFFDRIVE_V1
    c = R.golden_case("mini_00_tricycle_f3")
    assert torch.equal(ops.inflate_costmap(c["data"], c["resolution"], 3.0).cpu(), torch.from_numpy(c["expected"]))
    d = R.golden_case("mini_00_diffdrive_f3")
    got = ops.inflate_costmap(torch.from_numpy(d["data"]), d["resolution"], 3.0, footprint=robots.get_footprint(INDUSTRIAL_DIFFDRIVE_V1))
    assert torch.equal(got.cpu(), torch.from_numpy(d["expected"]))


# ---- 2. small shapes --------------------------------------------------------------------------------------------------------
def test_single_cells(torch_cuda, ops):
    lethal = _check(torch_cuda, ops, np.full((1, 1), 254, dtype=np.uint8))
    assert int(lethal[0, 0]) == 254
    free = _check(torch_cuda, ops, np.zeros((1, 1), dtype=np.uint8))
    assert int(free[0, 0]) == 0


@pytest.mark.parametrize("shape", [(1, 70), (70, 1)])
def test_lines(torch_cuda, ops, shape):
    data = np.zeros(shape, dtype=np.uint8)
    data.reshape(-1)[[3, 40]] = 254
    _check(torch_cuda, ops, data)


@pytest.mark.parametrize("cols", [31, 32, 33, 63, 64, 65])
def test_word_boundaries(torch_cuda, ops, cols):
    """obstacles in the first and the last column, and on both sides of every 32-cell word of the row masks"""
    data = np.zeros((9, cols), dtype=np.uint8)
    data[0, 0] = data[8, cols - 1] = data[4, 0] = data[5, cols - 1] = 254
    _check(torch_cuda, ops, data)
    rng = np.random.RandomState(cols)
    more = np.where(rng.rand(37, cols) < 0.01, 254, 0).astype(np.uint8)
    more[20, 0] = more[7, cols - 1] = 254
    _check(torch_cuda, ops, more)


def test_distances_beyond_eight_bits(torch_cuda, ops):
    """a 183 x 183 map whose only obstacle is the corner cell: distances reach 257.4"""
    data = np.zeros((183, 183), dtype=np.uint8)
    data[0, 0] = 254
    expected = R.inflate_and_margin(data, RES, RADIUS, FACTOR)
    assert expected[1].max() == np.float32(np.sqrt(2.0 * 182 * 182)) > 257
    _check(torch_cuda, ops, data, expected=expected)


def test_map_without_obstacles(torch_cuda, ops):
    torch = torch_cuda
    data = np.zeros((37, 45), dtype=np.uint8)
    data[3, 4], data[5, 6] = 255, 253   # not obstacles
    cost, dist = ops.inflate_costmap(data, RES, FACTOR, inscribed_radius=RADIUS, return_distance=True)
    assert int(cost.max()) == 0 and bool(torch.isinf(dist).all()) and bool((dist > 0).all())


def _padded_batch():
    rng = np.random.RandomState(11)
    valid = np.array([[40, 50], [0, 50], [17, 33], [40, 0], [1, 1]], dtype=np.int32)
    batch = np.where(rng.rand(5, 40, 50) < 0.02, 254, 0).astype(np.uint8)
    batch[2, 16, 32] = batch[2, 0, 0] = batch[4, 0, 0] = 254
    batch[2, 17, 10] = batch[2, 5, 33] = batch[2, 39, 49] = batch[4, 0, 1] = batch[4, 1, 0] = 254   # in the padding
    return batch, valid


def test_batch_with_valid_shapes(torch_cuda, ops):
    """5 maps of 40 x 50 with valid shapes from nothing to everything; 254s in the padding are ignored, the padding comes out 0"""
    torch = torch_cuda
    batch, valid = _padded_batch()
    cost, dist = ops.inflate_costmap(batch, RES, FACTOR, inscribed_radius=RADIUS, valid_rows=valid[:, 0], valid_cols=valid[:, 1],
                                     return_distance=True)
    for m in range(5):
        want, want_d, margin = R.inflate_and_margin(batch[m], RES, RADIUS, FACTOR, valid=valid[m])
        assert margin > 1e-9
        assert torch.equal(cost[m].cpu(), torch.from_numpy(want)), m
        assert torch.equal(dist[m].cpu(), torch.from_numpy(want_d)), m
        assert not want[valid[m, 0]:].any() and not want[:, valid[m, 1]:].any()
    # out-of-range valid shapes are clamped to the storage
    wild = ops.inflate_costmap(batch[:2], RES, FACTOR, inscribed_radius=RADIUS, valid_rows=[99, -3], valid_cols=[50, 50])
    assert torch.equal(wild[0].cpu(), torch.from_numpy(R.inflate(batch[0], RES, RADIUS, FACTOR)[0])) and int(wild[1].max()) == 0


# ---- 3. in place, batches, routes -------------------------------------------------------------------------------------------
def _raw(ops, data, out, n, rows, cols, res=RES, radius=RADIUS, factor=FACTOR, vr=None, vc=None, dist=None):
    return ops._lib.bcp_inflate_costmaps(ops._h, data, n, rows, cols, vr, vc, res, radius, factor, out, dist, ops._stream())


@pytest.mark.parametrize("name", ["mini_00_tricycle_f3", "colored_350x512_tricycle_f3"])
def test_in_place_equals_out_of_place(torch_cuda, ops, name):
    torch = torch_cuda
    c = R.golden_case(name)
    rows, cols = c["data"].shape
    # an odd byte offset into the buffer as well: the maps need not start on a dword
    for offset in (0, 3):
        buf = torch.zeros(offset + rows * cols + 5, dtype=torch.uint8, device="cuda")
        buf[offset:offset + rows * cols] = torch.from_numpy(c["data"]).cuda().reshape(-1)
        ptr = buf.data_ptr() + offset
        assert _raw(ops, ptr, ptr, 1, rows, cols, c["resolution"], c["inscribed_radius"], c["cost_scaling_factor"]) == 0
        got = buf.cpu()
        assert torch.equal(got[offset:offset + rows * cols].reshape(rows, cols), torch.from_numpy(c["expected"])), offset
        assert int(got[:offset].sum()) == 0 and int(got[offset + rows * cols:].sum()) == 0   # the neighbours are untouched


def test_batch_equals_single_calls_in_place_too(torch_cuda, ops):
    torch = torch_cuda
    names = ["mini_00_tricycle_f3", "mini_05_tricycle_f3", "mini_00_odd_values_tricycle_f3"]
    cases = [R.golden_case(n) for n in names]
    batch = np.stack([c["data"] for c in cases])
    want = torch.from_numpy(np.stack([c["expected"] for c in cases]))
    res = cases[0]["resolution"]
    assert torch.equal(ops.inflate_costmap(batch, res, 3.0).cpu(), want)
    singles = torch.stack([ops.inflate_costmap(c["data"], res, 3.0) for c in cases])
    assert torch.equal(singles.cpu(), want)
    dev = torch.from_numpy(batch).cuda()
    assert _raw(ops, dev.data_ptr(), dev.data_ptr(), 3, 183, 183, res, cases[0]["inscribed_radius"], 3.0) == 0
    assert torch.equal(dev.cpu(), want)


def test_both_routes_give_the_same_bytes(torch_cuda, ops):
    """BCP_TUNE_INFLATE_ROUTE = 2 sends maps that fit the LDS through the global-scratch plane as well"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import _lib
    c = R.golden_case("mini_05_tricycle_f1")
    batch, valid = _padded_batch()
    try:
        _lib.check(ops._lib.bcp_set_tuning(ops._h, _lib.TUNE_INFLATE_ROUTE, 2))
        cost, dist = ops.inflate_costmap(c["data"], c["resolution"], 1.0, return_distance=True)
        padded = ops.inflate_costmap(batch, RES, FACTOR, inscribed_radius=RADIUS, valid_rows=valid[:, 0], valid_cols=valid[:, 1])
    finally:
        _lib.check(ops._lib.bcp_set_tuning(ops._h, _lib.TUNE_INFLATE_ROUTE, 0))
    assert torch.equal(cost.cpu(), torch.from_numpy(c["expected"]))
    assert torch.equal(dist.cpu(), torch.from_numpy(np.array(R.restated_case("mini_05_tricycle_f1")[1])))
    again = ops.inflate_costmap(batch, RES, FACTOR, inscribed_radius=RADIUS, valid_rows=valid[:, 0], valid_cols=valid[:, 1])
    assert torch.equal(padded, again)
    assert ops._lib.bcp_set_tuning(ops._h, _lib.TUNE_INFLATE_ROUTE, 1) == E_INVALID


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda, ops):
    torch = torch_cuda
    L = ops._lib
    data = torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
    data[0, 2, 2] = 254
    out = torch.full((2, 8, 8), 7, dtype=torch.uint8, device="cuda")
    v = torch.full((2,), 8, dtype=torch.int32, device="cuda")
    d, o = data.data_ptr(), out.data_ptr()

    def refused(*args, **kw):
        L.bcp_seed(ops._h, 0)   # (any successful call; the message below must be this refusal's)
        rc = _raw(*args, **kw) if args[0] is ops else L.bcp_inflate_costmaps(*args)
        msg = L.bcp_last_error()
        return rc == E_INVALID and msg.startswith(b"bcp_inflate_costmaps: ") and len(msg) > 30

    assert refused(None, d, 2, 8, 8, None, None, RES, RADIUS, FACTOR, o, None, None)         # NULL handle
    assert refused(ops, d, o, -1, 8, 8)
    assert refused(ops, None, o, 2, 8, 8) and refused(ops, d, None, 2, 8, 8)
    for rows, cols in ((0, 8), (8, 0), (2049, 8), (8, 2049), (-1, 8)):
        assert refused(ops, d, o, 2, rows, cols), (rows, cols)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert refused(ops, d, o, 2, 8, 8, res=bad) and refused(ops, d, o, 2, 8, 8, radius=bad) and refused(ops, d, o, 2, 8, 8, factor=bad), bad
    assert refused(ops, d, o, 2, 8, 8, vr=v.data_ptr()) and refused(ops, d, o, 2, 8, 8, vc=v.data_ptr())
    assert refused(ops, d, d + 64, 1, 8, 9) and refused(ops, d + 1, d, 2, 8, 7)              # overlapping, not equal
    torch.cuda.synchronize()
    assert int((out != 7).sum()) == 0 and int(data.sum()) == 254                            # nothing ran
    assert _raw(ops, d, o, 0, 8, 8) == 0 and _raw(ops, None, None, 0, 8, 8) == 0             # n_maps = 0: a no-op
    torch.cuda.synchronize()
    assert int((out != 7).sum()) == 0
    assert _raw(ops, d, d + 64, 1, 8, 8) == 0                                                # adjacent is fine: map 0 -> map 1
    assert _raw(ops, d, o, 2, 8, 8, vr=v.data_ptr(), vc=v.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(data[0, 2, 2]) == 254 and int(data[0].sum()) == 254 and torch.equal(out[0], data[1]) and torch.equal(out[1], data[1])


# ---- 5. envs ----------------------------------------------------------------------------------------------------------------
N_ENVS, N_STEPS = 64, 40


def _state_tensors(env):
    s = env.state
    return [env.reward, env.done, env.collided_now, s.robot, s.min_spat_dist_so_far, s.target_idx, s.current_iter, s.robot_collided]


def _step_twins(torch, raw, inflated, seed):
    rng = np.random.RandomState(seed)
    for t in range(N_STEPS):
        a = raw.action_space.sample_batch(N_ENVS, rng)
        raw.step(a)
        inflated.step(a)
        for k, (x, y) in enumerate(zip(_state_tensors(raw), _state_tensors(inflated))):
            assert torch.equal(x, y), (t, k)
    raw.check_errors()
    inflated.check_errors()


def _check_ego(torch, oracle, env, map_of_env, origin_of_env, pool):
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    images = BatchedEgocentricCostmap(env, pool=pool).observation()['env'].cpu().numpy()[..., 0]
    st = env.state.robot.cpu().numpy()
    lit = 0
    for i in range(16):
        ref = oracle.extract_egocentric(map_of_env(i), origin_of_env(i), env.resolution, st[:3, i], *REF_WINDOW)
        want = ref if pool == 1 else block_max(ref, pool)
        assert (want == images[i]).all(), (pool, i)
        lit += int(((want > 0) & (want < 253)).sum())
    assert lit > 0   # the gradient is in the images


def test_shared_map_env_steps_as_before_and_shows_the_gradient(torch_cuda, oracle):
    torch = torch_cuda
    name = "g8_traj_mini_00.npz"
    g = np.load(os.path.join(GOLDEN, name))
    raw = env_from_traj(g, name, n_envs=N_ENVS, auto_reset=True, seed=5)
    inflated = env_from_traj(g, name, n_envs=N_ENVS, auto_reset=True, seed=5)
    inflated.inflate_costmaps(3.0)
    want = torch.from_numpy(R.golden_case("mini_00_tricycle_f3")["expected"])
    assert torch.equal(inflated.costmap_tensor.cpu(), want) and torch.equal(raw.costmap_tensor.cpu(), torch.from_numpy(g["costmap"]))
    _step_twins(torch, raw, inflated, 1)
    host = want.numpy()
    _check_ego(torch, oracle, inflated, lambda i: host, lambda i: g["origin"], 1)
    _check_ego(torch, oracle, inflated, lambda i: host, lambda i: g["origin"], 8)
    assert (inflated.envs[3].get_state().costmap.get_data() == host).all()
    assert (raw.envs[3].get_state().costmap.get_data() == g["costmap"]).all()
    with pytest.raises(RuntimeError, match="inflated already"):
        inflated.inflate_costmaps(3.0)


def test_mini_pool_env_steps_as_before_and_shows_the_gradient(torch_cuda, oracle):
    torch = torch_cuda
    from bc_gym_planning_env_amd import mini_env, robots
    raw = mini_env.BatchedRandomMiniEnv(N_ENVS, n_chains=8, episodes=2, auto_reset=True, seed=9)
    inflated = mini_env.BatchedRandomMiniEnv(N_ENVS, n_chains=8, episodes=2, auto_reset=True, seed=9)
    inflated.inflate_costmaps(3.0)
    before, after = raw.costmap_tensor.cpu().numpy(), inflated.costmap_tensor.cpu()
    assert before.shape[0] == 16 and after.shape == before.shape
    radius = robots.inscribed_radius(raw.footprint())
    for k in range(16):
        want, _, margin = R.inflate_and_margin(before[k], raw.resolution, radius, 3.0)
        assert margin > 1e-9 and torch.equal(after[k], torch.from_numpy(want)), k
    _step_twins(torch, raw, inflated, 2)
    host = after.numpy()
    geom = inflated.geom_of_env.cpu().numpy()
    assert (geom == raw.geom_of_env.cpu().numpy()).all()
    origin = lambda i: inflated.costmap_of(i).get_origin()
    _check_ego(torch, oracle, inflated, lambda i: host[geom[i]], origin, 1)
    _check_ego(torch, oracle, inflated, lambda i: host[geom[i]], origin, 8)
    assert (inflated.envs[5].get_state().costmap.get_data() == host[geom[5]]).all()
    with pytest.raises(RuntimeError, match="inflated already"):
        inflated.inflate_costmaps(3.0)


def test_device_resident_pool_is_inflated_where_it_lives(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import mini_env
    raw = mini_env.BatchedRandomMiniEnv(8, n_chains=2, episodes=2, sampler="device_resident")
    env = mini_env.BatchedRandomMiniEnv(8, n_chains=2, episodes=2, sampler="device_resident")
    env.inflate_costmaps(3.0)
    before = raw.pool.maps.cpu().numpy()
    for k in range(4):
        assert torch.equal(env.pool.maps[k].cpu(), torch.from_numpy(R.inflate(before[k], env.resolution, RADIUS, 3.0)[0])), k
    assert (env.envs[1].get_state().costmap.get_data() == env.pool.maps[int(env.geom_of_env[1])].cpu().numpy()).all()


def test_endless_pool_is_refused(torch_cuda):
    from bc_gym_planning_env_amd import mini_env
    env = mini_env.BatchedRandomMiniEnv(8, episodes=2, endless=True, auto_reset=True)
    with pytest.raises(RuntimeError, match="endless"):
        env.inflate_costmaps(3.0)


def test_aisle_pool_entries_within_their_valid_shapes(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import aisle_env, robots
    raw = aisle_env.BatchedRandomAisleTurnEnv(8, n_chains=2, episodes=4)
    env = aisle_env.BatchedRandomAisleTurnEnv(8, n_chains=2, episodes=4)
    env.inflate_costmaps(3.0)
    before, after = raw.costmap_tensor.cpu().numpy(), env.costmap_tensor.cpu().numpy()
    vr, vc = env._keep["vr"].cpu().numpy(), env._keep["vc"].cpu().numpy()
    assert before.shape[0] == 8 and (vr > 0).all() and (vc > 0).all()
    assert (vr < before.shape[1]).any() or (vc < before.shape[2]).any()   # some entry really is padded
    radius = robots.inscribed_radius(env.footprint())
    for k in range(8):
        want, _, margin = R.inflate_and_margin(before[k], env.resolution, radius, 3.0, valid=(vr[k], vc[k]))
        assert margin > 1e-9 and (after[k] == want).all(), k
        assert not after[k, vr[k]:].any() and not after[k, :, vc[k]:].any()
    assert (env.envs[2].get_state().costmap.get_data() == after[int(env.geom_of_env[2]), :vr[int(env.geom_of_env[2])], :vc[int(env.geom_of_env[2])]]).all()

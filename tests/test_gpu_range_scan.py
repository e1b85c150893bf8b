"""bcp_range_scan / bcp_final_range_scan on the GPU, bit for bit against the contract restated in numpy
(tests/range_scan_ref.py).  Every comparison feeds the call's own heading_cs_out to the reference -- a walk is only bit for
bit the same from the same direction -- and requires ranges and hit to be equal in every bit; separately heading_cs_out
must lie within 4 * 2^-52 of numpy's cos / sin for |theta| <= 1000 (OpenCL's 4-ulp bound for double sin / cos on values
<= 1: a sanity check, not a precision claim).  Outputs go into poisoned buffers with a guard behind them.
Every case is small: rows <= 130, beams <= 200, max_range <= 200 cells."""
import ctypes as C

import numpy as np
import pytest

import range_scan_ref as RR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
PATH = np.array([[0., 0., 0.], [1., 0., 0.], [2., 0., 0.]])
GUARD = 64
POISON_F, POISON_I, POISON_D = -7.5, -77, -9.25


def _maps_of(env):
    """what the env has bound, as the reference takes it: data [E, rows, cols], valid rows / cols [E], origins [E, 2]"""
    data = env.costmap_tensor.cpu().numpy()
    if data.ndim == 2:
        return data[None], [data.shape[0]], [data.shape[1]], np.asarray(env._origin_host, dtype=np.float64)[None]
    k = env._keep
    vr = k["vr"].cpu().numpy() if k.get("vr") is not None else np.full(len(data), data.shape[1])
    vc = k["vc"].cpu().numpy() if k.get("vc") is not None else np.full(len(data), data.shape[2])
    return data, vr, vc, k["origins"].cpu().numpy()


def _entry_of(env, n):
    """the map entry of rows 0 .. n - 1 of a call on the bound state or on given poses"""
    me = np.arange(n) % env.n_envs
    if env.costmap_tensor.dim() == 2:
        return np.zeros(n, dtype=np.int64)
    return env.geom_of_env.cpu().numpy()[me].astype(np.int64) if env.geom_of_env is not None else me


class _Out(object):
    """poisoned outputs of n rows, each with GUARD poisoned elements behind it in the same allocation"""

    def __init__(self, torch, n, b):
        self.n, self.b = n, b
        self.ranges = torch.full((n * b + GUARD,), POISON_F, dtype=torch.float32, device="cuda")
        self.hit = torch.full((n * b + GUARD,), POISON_I, dtype=torch.int32, device="cuda")
        self.cs = torch.full((n * 2 + GUARD,), POISON_D, dtype=torch.float64, device="cuda")

    def read(self):
        n, b = self.n, self.b
        r, h, c = self.ranges.cpu().numpy(), self.hit.cpu().numpy(), self.cs.cpu().numpy()
        assert (r[n * b:] == POISON_F).all() and (h[n * b:] == POISON_I).all() and (c[2 * n:] == POISON_D).all(), "guard overwritten"
        return r[:n * b].reshape(n, b), h[:n * b].reshape(n, b), c[:2 * n].reshape(n, 2)


def _table(torch, beam_cs):
    return torch.from_numpy(np.ascontiguousarray(beam_cs, dtype=np.float64)).cuda()


def _scan(torch, env, beam_cs, max_range, poses=None, n=None):
    from bc_gym_planning_env_amd import _lib
    table = _table(torch, beam_cs)
    pt = None if poses is None else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).cuda()
    n = (env.n_envs if pt is None else len(poses)) if n is None else n
    out = _Out(torch, n, len(beam_cs))
    _lib.check(env._lib.bcp_range_scan(env._h, pt.data_ptr() if pt is not None else None, n, table.data_ptr(), len(beam_cs),
                                       float(max_range), out.ranges.data_ptr(), out.hit.data_ptr(), out.cs.data_ptr(), None))
    return out.read()


def _same_bits(got, want, what):
    got_r, got_h = got
    want_r, want_h = want
    assert got_r.dtype == np.float32 and got_h.dtype == np.int32
    bad = int((got_h != want_h).sum()), int((got_r.view(np.uint32) != want_r.view(np.uint32)).sum())
    print(what, "rays", got_h.size, "hits", int((want_h >= 0).sum()), "different hit / range:", bad)
    assert bad == (0, 0), (what, bad)


def _check(env, poses, got, beam_cs, max_range, what, entry=None, maps=None):
    """ranges and hit of `got` against the reference walked from got's own heading_cs; -> the reference's (ranges, hit)"""
    ranges, hit, cs = got
    data, vr, vc, origins = _maps_of(env) if maps is None else maps
    entry = _entry_of(env, len(poses)) if entry is None else entry
    want_r, want_h, trips, bound = RR.range_scan(data, vr, vc, origins, env.resolution, entry, poses, cs, beam_cs, max_range)
    assert trips.max() < bound
    _same_bits((ranges, hit), (want_r, want_h), what)
    return want_r, want_h


def _check_heading(poses, cs):
    th = poses[:, 2]
    sel = np.isfinite(poses).all(axis=1) & (np.abs(th) <= 1000) & (np.abs(poses[:, :2]) < 1e6).all(axis=1)
    err = max(np.abs(cs[sel, 0] - np.cos(th[sel])).max(), np.abs(cs[sel, 1] - np.sin(th[sel])).max())
    print("heading_cs_out: max |device - numpy| = %.3g over %d rows (bound %.3g)" % (err, int(sel.sum()), 4 * 2.0 ** -52))
    assert sel.sum() > 0 and err <= 4 * 2.0 ** -52


def _sprinkled(rng, shape, fraction=0.04):
    m = np.where(rng.uniform(size=shape) < fraction, 254, 0).astype(np.uint8)
    m[rng.uniform(size=shape) < 0.03] = 253    # free space, like 255 and every other cost
    m[rng.uniform(size=shape) < 0.03] = 255
    m[rng.uniform(size=shape) < 0.03] = 100
    m[0, :] = 254
    m[:, -1] = 254
    return m


def _shared_env(shape, n, seed, res=0.05):
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    rng = np.random.RandomState(seed)
    m = _sprinkled(rng, shape)
    org = rng.uniform(-2, 0, 2)
    env = BatchedPlanEnv(CostMap2D(m, res, org), PATH, EnvParams(resolution=res, refine_path=False), n_envs=n)
    return env, m, org, rng


# ---- 1. one shared map: every beam count, the edge rows, the headings -------------------------------------------------------
@pytest.mark.parametrize("n_beams", [1, 7, 64, 65, 200])
def test_shared_map_every_beam_count(torch_cuda, n_beams):
    """64 x 64, staged in LDS; 130 rows: in a lethal cell, outside the map on every side, non-finite, beyond 2^30 cells, and
    headings up to +- 1000; 1, 7 and 65 beams put the rows of a workgroup's 256 rays at every offset"""
    torch = torch_cuda
    n = 130
    env, m, org, rng = _shared_env((64, 64), n, 12)
    poses = RR.edge_rows(rng, m, m.shape, org, 0.05, n_inside=n - 16)
    poses[40:80, 2] = rng.uniform(-1000, 1000, 40)
    poses[80] = (org[0] + 9.5 * 0.05, org[1] + 19.5 * 0.05, 0.0)   # u, v on grid lines, or an ulp off them
    beams = RR.beam_table(RR.wrapper_angles(n_beams, 2 * np.pi)) if n_beams > 1 else np.array([[1.0, 0.0]])
    for max_range in (3.0, 1.23):    # 60 cells; 24.6 cells: R ends inside a cell
        got = _scan(torch, env, beams, max_range, poses)
        want_r, want_h = _check(env, poses, got, beams, max_range, "shared %d beams %.2f m" % (n_beams, max_range))
        if n_beams >= 7:
            assert (want_h[:4] >= 0).all() and (want_r[:4] == 0).all()      # a start cell that is lethal
            assert (want_h[10:16] == -1).all() and (want_r[10:16] == np.float32(max_range)).all()
            assert (want_h[9] == -1).all()
            assert (want_h[16:] >= 0).any() and (want_h[16:] == -1).any()
    _check_heading(poses, got[2])


def test_axis_beams_at_heading_zero(torch_cuda):
    """theta = 0 with beams (1, 0), (0, 1), (-1, 0), (0, -1): dx or dy is exactly 0; and a known range"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    res, n = 0.05, 40
    m = np.zeros((64, 64), dtype=np.uint8)
    m[:, 40] = 254
    m[50, :] = 254
    env = BatchedPlanEnv(CostMap2D(m, res, np.zeros(2)), PATH, EnvParams(resolution=res, refine_path=False), n_envs=n)
    rng = np.random.RandomState(2)
    poses = np.stack([rng.uniform(0, 3.2, n), rng.uniform(0, 3.2, n), np.zeros(n)], axis=1)
    poses[0] = (10 * res, 10 * res, 0.0)     # the centre of cell (10, 10)
    axes = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    got = _scan(torch, env, axes, 3.0, poses)
    assert (got[2] == [1.0, 0.0]).all()
    _check(env, poses, got, axes, 3.0, "axis beams")
    assert got[0][0, 0] == np.float32((40 - 10 - 0.5) * 0.05) and got[1][0, 0] == 10 * 64 + 40
    assert got[1][0, 1] == 50 * 64 + 10 and (got[1][0, 2:] == -1).all()


def test_starts_exactly_on_grid_lines(torch_cuda):
    """u, v, or both exactly integers, and rays along the lines and through the corners: at a resolution that is a power of
    two with such an origin the contract's u and v are exact, so the ties (a tie steps in y) happen on the device too"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    res, org, n = 0.25, np.array([-2.0, 1.5]), 30
    rng = np.random.RandomState(9)
    m = np.where(rng.uniform(size=(40, 45)) < 0.08, 254, 0).astype(np.uint8)
    env = BatchedPlanEnv(CostMap2D(m, res, org), PATH, EnvParams(resolution=res, refine_path=False), n_envs=n)
    ks = rng.randint(1, 39, size=(n, 2)).astype(np.float64)
    poses = np.stack([org[0] + (ks[:, 0] - 0.5) * res, org[1] + (ks[:, 1] - 0.5) * res, rng.uniform(-np.pi, np.pi, n)], axis=1)
    poses[10:20, 1] += 0.1        # only u on a line
    poses[20:, 2] = 0.0           # on a corner, heading along the axis
    u = (poses[:, 0] - org[0]) * (1.0 / res) + 0.5
    v = (poses[:, 1] - org[1]) * (1.0 / res) + 0.5
    assert (u == np.floor(u)).all() and (v[:10] == np.floor(v[:10])).all() and (v[10:20] != np.floor(v[10:20])).all()
    axes = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    beams = np.concatenate([axes, RR.beam_table(RR.wrapper_angles(16, 2 * np.pi)), RR.beam_table([np.pi / 4, -3 * np.pi / 4])])
    got = _scan(torch, env, beams, 6.0, poses)     # 24 cells
    assert (got[2][20:] == [1.0, 0.0]).all()
    _, want_h = _check(env, poses, got, beams, 6.0, "starts on grid lines")
    assert (want_h >= 0).any() and (want_h == -1).any()


@pytest.mark.parametrize("shape", [(690, 640), (800, 800)], ids=["large-staged-or-not", "beyond-lds"])
def test_large_shared_maps(torch_cuda, shape):
    """a mask of 55 KB (if staged, the workgroup's LDS passes 64 KB) and one of 80 KB (read through the cache)"""
    torch = torch_cuda
    n = 24
    env, m, org, rng = _shared_env(shape, n, 5)
    poses = RR.edge_rows(rng, m, m.shape, org, 0.05, n_inside=n - 16)
    beams = RR.beam_table(RR.wrapper_angles(16, np.pi))
    got = _scan(torch, env, beams, 10.0, poses)     # 200 cells
    _, want_h = _check(env, poses, got, beams, 10.0, "shared %s" % (shape,))
    assert (want_h >= 0).sum() > 50


# ---- 2. private maps, pools, delays ----------------------------------------------------------------------------------------
def test_private_maps_with_lethal_padding(torch_cuda):
    """three maps of different valid shapes in one padded allocation whose padding is full of 254s: free space"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    rng = np.random.RandomState(33)
    res, n = 0.05, 3
    valid = [(40, 70), (64, 33), (55, 100)]
    small = [_sprinkled(rng, s) for s in valid]
    orgs = np.array([rng.uniform(-2, 0, 2) for _ in valid])
    env = BatchedPlanEnv([CostMap2D(m, res, o) for m, o in zip(small, orgs)], [PATH] * n, EnvParams(resolution=res, refine_path=False),
                         n_envs=n, map_storage=(72, 128))
    data = np.full((n, 72, 128), 254, dtype=np.uint8)
    for k, m in enumerate(small):
        data[k, :m.shape[0], :m.shape[1]] = m
    vr = torch.tensor([s[0] for s in valid], dtype=torch.int32, device="cuda")
    vc = torch.tensor([s[1] for s in valid], dtype=torch.int32, device="cuda")
    env.set_costmap_tensors(torch.from_numpy(data).cuda(), torch.from_numpy(orgs).cuda(), res, vr, vc)
    per = 40
    poses = np.zeros((3 * per, 3))
    for k in range(3):      # row i is seen on the map of env i % 3
        poses[k::3] = RR.edge_rows(rng, small[k], valid[k], orgs[k], res, n_inside=per - 16)
    beams = RR.beam_table(RR.wrapper_angles(48, 2 * np.pi))
    got = _scan(torch, env, beams, 4.0, poses)
    want_r, want_h = _check(env, poses, got, beams, 4.0, "private maps")
    for k in range(3):
        h = want_h[k::3]
        assert (h >= 0).any() and (h[h >= 0] // 128 < valid[k][0]).all() and (h[h >= 0] % 128 < valid[k][1]).all()
    # the same maps with clean padding: the same bytes
    clean = np.zeros_like(data)
    for k, m in enumerate(small):
        clean[k, :m.shape[0], :m.shape[1]] = m
    env.set_costmap_tensors(torch.from_numpy(clean).cuda(), torch.from_numpy(orgs).cuda(), res, vr, vc)
    again = _scan(torch, env, beams, 4.0, poses)
    _same_bits(again[:2], got[:2], "clean padding")


def _mini(n, timeout, seeds=(1, 2, 3, 4), episodes=4, **kw):
    from bc_gym_planning_env_amd import EnvParams, mini_env
    delays = {k: kw.pop(k) for k in list(kw) if k.endswith("_delay")}
    params = mini_env.RandomMiniEnvParams(
        env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=timeout, **delays))
    if kw.get("endless"):
        return mini_env.BatchedRandomMiniEnv(n, params, episodes=episodes, auto_reset=True, seed=4, **kw), params
    pool = mini_env.sample_pool(params, list(seeds), episodes)
    return mini_env.BatchedRandomMiniEnv(n, params, pool=pool, auto_reset=True, seed=2, **kw), params


def _current_poses(env):
    return np.ascontiguousarray(env.state.robot[0:3].cpu().numpy().T)


def test_pool_after_auto_resets(torch_cuda):
    """16 pool entries, 64 envs, 60 steps with auto-reset: the envs sit on different entries; poses=None is the state's pose"""
    torch = torch_cuda
    n = 64
    env, _params = _mini(n, timeout=12)
    assert len(env.pool.costmaps) == 16
    rng = np.random.RandomState(1)
    for _ in range(60):
        env.step(env.action_space.sample_batch(n, rng))
    assert len(np.unique(env.geom_of_env.cpu().numpy())) > 1
    beams = RR.beam_table(RR.wrapper_angles(64, 2 * np.pi))
    poses = _current_poses(env)
    got = _scan(torch, env, beams, 3.0)
    _, want_h = _check(env, poses, got, beams, 3.0, "pool, bound state")
    assert (want_h >= 0).any() and (want_h == -1).any()
    explicit = _scan(torch, env, beams, 3.0, poses)
    _same_bits(explicit[:2], got[:2], "pool, explicit poses")
    assert (explicit[2] == got[2]).all()
    # 130 given poses: row i on the entry of env i % 64
    more = np.concatenate([poses, poses + [0.05, -0.03, 0.4], poses[:2]])
    got = _scan(torch, env, beams, 3.0, more)
    _check(env, more, got, beams, 3.0, "pool, 130 poses")
    _check_heading(more, got[2])


def test_pose_delay_scans_the_seen_pose(torch_cuda):
    torch = torch_cuda
    n = 32
    env, _params = _mini(n, timeout=40, pose_delay=2)
    rng = np.random.RandomState(6)
    for _ in range(9):
        env.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
    seen = np.ascontiguousarray(env.state.pose_seen.cpu().numpy().T)
    now = _current_poses(env)
    assert np.abs(seen - now).max() > 1e-3
    beams = RR.beam_table(RR.wrapper_angles(64, 2 * np.pi))
    got = _scan(torch, env, beams, 3.0)
    _check(env, seen, got, beams, 3.0, "pose_delay: the seen pose")
    _same_bits(_scan(torch, env, beams, 3.0, seen)[:2], got[:2], "pose_delay: explicit seen pose")
    assert (_scan(torch, env, beams, 3.0, now)[0] != got[0]).any()


def test_inflated_twin_gives_identical_bytes(torch_cuda):
    torch = torch_cuda
    n = 48
    env, m, org, rng = _shared_env((90, 70), n, 21)
    twin, _m, _org, _rng = _shared_env((90, 70), n, 21)
    twin.inflate_costmaps(3.0)
    inflated = twin.costmap_tensor.cpu().numpy()
    assert ((inflated == 254) == (m == 254)).all() and (inflated != m).sum() > 100
    poses = RR.edge_rows(rng, m, m.shape, org, 0.05, n_inside=n - 16)
    beams = RR.beam_table(RR.wrapper_angles(64, 2 * np.pi))
    a, b = _scan(torch, env, beams, 3.0, poses), _scan(torch, twin, beams, 3.0, poses)
    _same_bits(b[:2], a[:2], "inflated twin")
    _check(twin, poses, b, beams, 3.0, "inflated twin vs reference")


def test_endless_pool_after_a_refresh(torch_cuda):
    torch = torch_cuda
    n = 64
    env, _params = _mini(n, timeout=6, endless=True)
    rng = np.random.RandomState(3)
    before = env.pool.maps.clone()
    for _ in range(14):
        env.step(env.action_space.sample_batch(n, rng))
    env.refresh()
    for _ in range(8):     # (past the next time-out: the envs move on to re-sampled worlds)
        env.step(env.action_space.sample_batch(n, rng))
    torch.cuda.synchronize()
    changed = (env.pool.maps != before).flatten(1).any(dim=1).cpu().numpy()
    geom = env.geom_of_env.cpu().numpy()
    assert changed.sum() > 10 and changed[geom].any(), "no env stands on a re-sampled world"
    beams = RR.beam_table(RR.wrapper_angles(64, 2 * np.pi))
    got = _scan(torch, env, beams, 3.0)
    _, want_h = _check(env, _current_poses(env), got, beams, 3.0, "after refresh")
    assert (want_h[changed[geom]] >= 0).any()


# ---- 3. the episode record's final scans -------------------------------------------------------------------------------------
def test_final_scans_of_the_record(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import _lib
    n = 64
    env, _params = _mini(n, timeout=12, seeds=(1, 2, 3), episodes=3)
    ends = env.enable_episode_record()
    beams = RR.beam_table(RR.wrapper_angles(64, 2 * np.pi))
    table = _table(torch, beams)
    rng = np.random.RandomState(0)
    maps = _maps_of(env)
    checked = 0
    for t in range(30):
        _o, _r, d, _info = env.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
        out = _Out(torch, ends.capacity, len(beams))
        _lib.check(env._lib.bcp_final_range_scan(env._h, table.data_ptr(), len(beams), 3.0, out.ranges.data_ptr(),
                                                 out.hit.data_ptr(), out.cs.data_ptr(), None))
        ranges, hit, cs = out.read()
        m = int(ends.count[0])
        assert m == int(d.sum()) <= ends.capacity
        assert (ranges[m:] == POISON_F).all() and (hit[m:] == POISON_I).all() and (cs[m:] == POISON_D).all()
        if m:
            poses = np.ascontiguousarray(ends.final_state.robot[0:3, :m].cpu().numpy().T)
            entry = ends.geom[:m].cpu().numpy().astype(np.int64)
            _check(env, poses, (ranges[:m], hit[:m], cs[:m]), beams, 3.0, "final, step %d" % t, entry=entry, maps=maps)
            checked += m
    assert checked > 20


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import _lib
    from bc_gym_planning_env_amd.ops import NativeOps
    n, b = 4, 8
    env, m, org, rng = _shared_env((64, 64), n, 5)      # 5 cm: 4096 cells are 204.8 m
    L = env._lib
    beams = _table(torch, RR.beam_table(RR.wrapper_angles(b, 2 * np.pi)))
    poses = torch.zeros((6, 3), dtype=torch.float64, device="cuda")
    out = _Out(torch, 6, b)
    r, h, c = out.ranges.data_ptr(), out.hit.data_ptr(), out.cs.data_ptr()
    bp, pp = beams.data_ptr(), poses.data_ptr()

    def scan(handle=env._h, p=None, k=n, table=bp, nb=b, rng_=3.0, ranges=r):
        return L.bcp_range_scan(handle, p, k, table, nb, rng_, ranges, h, c, None)

    assert scan() == 0 and scan(p=pp, k=6) == 0 and scan(rng_=204.8) == 0
    assert scan(handle=None) == E_INVALID and scan(table=None) == E_INVALID and scan(ranges=None) == E_INVALID
    for nb in (0, -1, 1025):
        assert scan(nb=nb) == E_INVALID
    assert b"n_beams" in L.bcp_last_error()
    for k in (0, -2, n - 1, n + 1):
        assert scan(k=k) == E_INVALID, k
    assert scan(p=pp, k=0) == E_INVALID and scan(p=pp, k=-1) == E_INVALID
    for bad in (0.0, -1.0, float("inf"), float("nan"), 204.81, 1e300):
        assert scan(rng_=bad) == E_INVALID, bad
    assert L.bcp_last_error().startswith(b"bcp_range_scan: ")
    # the final form: no record bound -> state; then its own argument checks
    final = lambda table=bp, nb=b, rng_=3.0, ranges=r: L.bcp_final_range_scan(env._h, table, nb, rng_, ranges, h, c, None)
    assert final() == E_STATE and b"record" in L.bcp_last_error()
    assert L.bcp_final_range_scan(None, bp, b, 3.0, r, h, c, None) == E_INVALID
    env.enable_episode_record()
    assert final() == 0
    assert final(table=None) == E_INVALID and final(ranges=None) == E_INVALID and final(nb=0) == E_INVALID
    assert final(rng_=float("nan")) == E_INVALID and final(rng_=205.0) == E_INVALID
    assert L.bcp_last_error().startswith(b"bcp_final_range_scan: ")
    # a handle with nothing bound: no costmaps; with a costmap and no state: poses are required
    ops = NativeOps()
    assert L.bcp_range_scan(ops._h, pp, 6, bp, b, 3.0, r, h, c, None) == E_STATE and b"costmaps" in L.bcp_last_error()
    assert L.bcp_range_scan(ops._h, pp, 6, bp, 0, 3.0, r, h, c, None) == E_INVALID       # (arguments before state)
    ops.set_costmap(m, org, 0.05)
    assert L.bcp_range_scan(ops._h, None, 1, bp, b, 3.0, r, h, c, None) == E_STATE and b"state" in L.bcp_last_error()
    assert L.bcp_range_scan(ops._h, pp, 6, bp, b, 3.0, r, h, c, None) == 0
    torch.cuda.synchronize()
    out.read()      # (the guards are intact)


# ---- 5. a captured call ------------------------------------------------------------------------------------------------------
def test_captured_scan_replays_and_follows_the_robot(torch_cuda):
    torch = torch_cuda
    n = 64
    env, _params = _mini(n, timeout=200)
    angles = RR.wrapper_angles(64, 2 * np.pi)
    fields = ("ranges", "hit", "heading_cs")

    def call():
        return dict(zip(fields, env.range_scan(angles, 3.0, want=fields[1:])))

    eager = {f: t.clone() for f, t in call().items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = call()
    torch.cuda.synchronize()
    for f in fields:
        out[f].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(out[f], eager[f]), f
    # the replay reads the state as it is now: move the robots, replay, compare with an eager call and the reference
    env.state.robot[0:2] += 0.02
    env.state.robot[2] += 0.1
    graph.replay()
    torch.cuda.synchronize()
    replayed = {f: out[f].clone() for f in fields}
    now = call()
    for f in fields:
        assert torch.equal(now[f], replayed[f]), f
    assert not torch.equal(replayed["ranges"], eager["ranges"])
    got = tuple(replayed[f].cpu().numpy() for f in fields)
    _check(env, _current_poses(env), got, RR.beam_table(angles), 3.0, "replayed")


# ---- 6. the Python surface ---------------------------------------------------------------------------------------------------
def test_env_method_caches_table_and_buffers(torch_cuda):
    torch = torch_cuda
    n = 20
    env, m, org, rng = _shared_env((64, 64), n, 8)
    angles = RR.wrapper_angles(12, np.pi)
    ranges = env.range_scan(angles, 2.0)
    assert ranges.shape == (n, 12) and ranges.dtype == torch.float32
    r2, hit, cs = env.range_scan(list(angles), 2.0, want=("hit", "heading_cs"))
    assert r2.data_ptr() == ranges.data_ptr() and len(env._beam_tables) == 1
    assert hit.shape == (n, 12) and hit.dtype == torch.int32 and cs.shape == (n, 2) and cs.dtype == torch.float64
    poses = _current_poses(env)
    _check(env, poses, (r2.cpu().numpy(), hit.cpu().numpy(), cs.cpu().numpy()), RR.beam_table(angles), 2.0, "env.range_scan")
    some = RR.edge_rows(rng, m, m.shape, org, 0.05, n_inside=5)
    r3, h3, c3 = env.range_scan(torch.from_numpy(angles), 2.0, poses=some, want=("hit", "heading_cs"))
    assert r3.shape == (21, 12) and len(env._beam_tables) == 1
    _check(env, some, (r3.cpu().numpy(), h3.cpu().numpy(), c3.cpu().numpy()), RR.beam_table(angles), 2.0, "env.range_scan(poses)")
    with pytest.raises(ValueError):
        env.range_scan(angles, 2.0, want=("nothing",))
    # a caller that sweeps beam sets and batch sizes does not pile up device memory: both caches are bounded
    from bc_gym_planning_env_amd.batched_env import SCAN_CACHE_ENTRIES
    for k in range(3 * SCAN_CACHE_ENTRIES):
        env.range_scan(np.linspace(-1.0, 1.0, 3 + k), 2.0, poses=some[:1 + k % 5])
    assert len(env._beam_tables) == SCAN_CACHE_ENTRIES and len(env._range_scan_buffers) <= SCAN_CACHE_ENTRIES
    again = env.range_scan(angles, 2.0)      # (evicted and made again: the same answer)
    assert again.data_ptr() != ranges.data_ptr() and torch.equal(again, ranges)


def test_wrapper_shapes_keys_and_final_observation(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedRangeScan
    n = 64
    env, _params = _mini(n, timeout=12, seeds=(1, 2, 3), episodes=3)
    wrap = BatchedRangeScan(env, n_beams=48, fov=1.5 * np.pi, max_range=2.5, final_observation=True)
    assert wrap.unwrapped() is env and wrap.action_space is env.action_space
    np.testing.assert_array_equal(wrap.beam_angles, RR.wrapper_angles(48, 1.5 * np.pi))
    beams = RR.beam_table(wrap.beam_angles)
    obs = wrap.reset()
    assert list(obs.keys()) == ["scan", "goal_n_state"]
    assert obs["scan"].shape == (n, 48, 1) and obs["scan"].dtype == torch.float32
    assert obs["goal_n_state"].shape == (n, 9, 1) and obs["goal_n_state"].dtype == torch.float32
    ends, maps = env.episode_ends, _maps_of(env)
    rng = np.random.RandomState(0)
    checked = 0
    for t in range(25):
        wrap.final_scan.fill_(POISON_F)
        obs, _r, d, info = wrap.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
        fin = info["final_observation"]
        assert list(fin.keys()) == ["scan", "goal_n_state"] and fin["scan"].shape == (ends.capacity, 48, 1)
        m = int(ends.count[0])
        assert m == int(d.sum())
        scan = fin["scan"].cpu().numpy()[..., 0]
        assert (scan[m:] == POISON_F).all()
        # the observation itself: the scan of the state after the step (and its auto-resets)
        _r_now, _h_now, cs_now = env.range_scan(wrap.beam_angles, 2.5, want=("hit", "heading_cs"))
        want_now, _, _, _ = RR.range_scan(*maps, env.resolution, _entry_of(env, n), _current_poses(env), cs_now.cpu().numpy(), beams, 2.5)
        assert (obs["scan"].cpu().numpy()[..., 0].view(np.uint32) == want_now.view(np.uint32)).all(), t
        if m:
            # rows match the episode ends: slot j is the final state of env env_ids[j] on the entry it ran on.  (cos, sin) of
            # the final headings: the library's own, from a scan of those poses
            poses = np.ascontiguousarray(ends.final_state.robot[0:3, :m].cpu().numpy().T)
            entry = ends.geom[:m].cpu().numpy().astype(np.int64)
            _r2, _h2, cs = env.range_scan(wrap.beam_angles, 2.5, poses=poses, want=("hit", "heading_cs"))
            want, _, _, _ = RR.range_scan(*maps, env.resolution, entry, poses, cs.cpu().numpy(), beams, 2.5)
            assert (scan[:m].view(np.uint32) == want.view(np.uint32)).all(), t
            checked += m
    assert checked > 20
    # goal_n_state is the egocentric vector with world size (max_range, max_range)
    from bc_gym_planning_env_amd import _lib
    vec = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
    world = np.array([2.5, 2.5])
    _lib.check(env._lib.bcp_goal_n_state(env._h, world.ctypes.data_as(_lib._f64p), vec.data_ptr(), None))
    assert torch.equal(wrap.observation()["goal_n_state"][..., 0], vec)
    for name in ("lookahead", "mppi", "get_state", "set_state", "seed", "close", "unwrapped", "step", "reset", "observation"):
        assert callable(getattr(wrap, name)), name
    state = wrap.get_state()
    wrap.set_state(state)


def test_native_ops_range_scan(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd.ops import NativeOps
    rng = np.random.RandomState(14)
    m = _sprinkled(rng, (75, 90))
    org, res = np.array([-1.5, 0.25]), 0.04
    ops = NativeOps()
    ops.set_costmap(m, org, res)
    poses = RR.edge_rows(rng, m, m.shape, org, res, n_inside=20)
    angles = RR.wrapper_angles(30, 2 * np.pi)
    ranges, hit, cs = ops.range_scan(poses, angles, 3.0, want=("hit", "heading_cs"))
    assert ranges.shape == (36, 30) and ranges.dtype == torch.float32
    want_r, want_h, trips, bound = RR.range_scan(m[None], [75], [90], org[None], res, np.zeros(36, dtype=np.int64), poses,
                                                 cs.cpu().numpy(), RR.beam_table(angles), 3.0)
    _same_bits((ranges.cpu().numpy(), hit.cpu().numpy()), (want_r, want_h), "NativeOps.range_scan")
    assert (want_h >= 0).any() and trips.max() < bound
    alone = ops.range_scan(poses, angles, 3.0)
    assert torch.equal(alone, ranges) and len(ops._beam_tables) == 1

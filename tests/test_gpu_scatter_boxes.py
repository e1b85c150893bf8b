"""GPU tests of bcp_scatter_boxes (scatter_boxes_kernel), NativeOps.scatter_boxes and BatchedPlanEnv.scatter_obstacles against
the numpy restatement (tests/scatter_boxes_ref.py, the fill by oracle.fill_poly).  Every raw call writes into sentinel-filled
boxes and counts with a guard row before and behind, and into maps with a guard plane before and behind whose padding
outside the valid shapes holds a sentinel too; whole buffers are compared, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import scatter_boxes_ref as SR
import test_gpu_goal_field as TG
import test_gpu_goal_route as TR
import test_scatter_boxes_host as TH

pytestmark = pytest.mark.gpu

E_INVALID = -1
POISON_I, POISON_B = -77, 0x5A


class _Case(object):
    """one raw call's buffers on the device: maps, boxes and counts of n entries, each with a guard on either side"""

    def __init__(self, torch, data, valid, origins, frame, keep, yaw_cs, n_boxes):
        dev = lambda x, dt: None if x is None else torch.from_numpy(np.array(x, dtype=dt)).cuda()   # noqa: E731
        data = np.ascontiguousarray(data, dtype=np.uint8)
        self.n, self.rows, self.cols = data.shape
        self.n_boxes = n_boxes
        guard = np.full((1, self.rows, self.cols), POISON_B, dtype=np.uint8)
        self.start = np.concatenate([guard, data, guard])
        self.maps = dev(self.start, np.uint8)
        self.boxes = torch.full((self.n + 2, n_boxes, SR.WORDS), POISON_I, dtype=torch.int32, device="cuda")
        self.counts = torch.full((self.n + 2,), POISON_I, dtype=torch.int32, device="cuda")
        self.vr = dev(None if valid is None else np.asarray(valid)[:, 0], np.int32)
        self.vc = dev(None if valid is None else np.asarray(valid)[:, 1], np.int32)
        self.origins, self.frame, self.yaw = dev(origins, np.float64), dev(frame, np.float64), dev(yaw_cs, np.float64)
        self.keep = dev(keep, np.int32)
        self.n_keep = 0 if keep is None else int(np.asarray(keep).shape[1])

    def restore(self, torch):
        self.maps.copy_(torch.from_numpy(self.start).cuda())
        self.boxes.fill_(POISON_I)
        self.counts.fill_(POISON_I)

    def call(self, owner, p, resolution, stream=None):
        opt = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        return owner._lib.bcp_scatter_boxes(owner._h, self.maps[1:].data_ptr(), self.n, self.rows, self.cols, opt(self.vr),
                                            opt(self.vc), self.origins.data_ptr(), float(resolution), C.byref(p),
                                            self.frame.data_ptr(), opt(self.keep), self.n_keep, self.yaw.data_ptr(),
                                            self.boxes[1:].data_ptr(), self.counts[1:].data_ptr(), stream)

    def read(self):
        m, b, c = self.maps.cpu().numpy(), self.boxes.cpu().numpy(), self.counts.cpu().numpy()
        assert (m[0] == POISON_B).all() and (m[-1] == POISON_B).all()
        assert (b[0] == POISON_I).all() and (b[-1] == POISON_I).all() and c[0] == POISON_I and c[-1] == POISON_I
        return m[1:-1], b[1:-1], c[1:-1]


def _params(n_boxes, max_attempts, n_yaws, seed, along, half_size):
    from bc_gym_planning_env_amd import _lib
    p = _lib.BcpScatterParams()
    p.n_boxes, p.max_attempts, p.n_yaws, p.seed = n_boxes, max_attempts, n_yaws, seed
    p.along[0], p.along[1], p.half_size[0], p.half_size[1] = along[0], along[1], half_size[0], half_size[1]
    return p


def _raw(torch, owner, data, valid, origins, resolution, frame, keep, yaw_cs, n_boxes, max_attempts, seed, along, half_size,
         want=None):
    """the call on guarded buffers, compared with the reference byte for byte -> (maps, boxes, counts)"""
    from bc_gym_planning_env_amd import _lib
    case = _Case(torch, data, valid, origins, frame, keep, yaw_cs, n_boxes)
    _lib.check(case.call(owner, _params(n_boxes, max_attempts, len(yaw_cs), seed, along, half_size), resolution))
    torch.cuda.synchronize()
    maps, boxes, counts = case.read()
    if want is None:
        want = SR.scatter(data, valid, origins, resolution, n_boxes, max_attempts, len(yaw_cs), seed, along, half_size, frame, keep,
                          yaw_cs)
    print("entries", len(maps), "accepted", counts.min(), "..", counts.max(), "cells written", int((maps != np.asarray(data)).sum()))
    assert (counts == want[2]).all(), (counts, want[2])
    assert (boxes == want[1]).all()
    assert (maps == want[0]).all()
    return maps, boxes, counts


@pytest.fixture(scope="module")
def owner(torch_cuda):
    from bc_gym_planning_env_amd.ops import NativeOps
    return NativeOps()


def _padded():
    rows, cols = 12, 14
    valid = np.array([[12, 14], [7, 9], [10, 5]])
    origins = np.array([[0.5, -0.25], [0.0, 0.0], [-3.0, 2.0]])
    data = np.full((3, rows, cols), 77, dtype=np.uint8)
    for i, (vr, vc) in enumerate(valid):
        data[i, :vr, :vc] = 0
    frame = SR.frames(origins + 0.5, origins + (valid[:, ::-1] - 2) * 0.5, 1.5)
    return data, valid, origins, 0.5, frame


@pytest.mark.parametrize("max_attempts", [31, 257])
def test_five_entries_of_nine_by_nine(torch_cuda, owner, max_attempts):
    data, origins, frame, starts, goals = TH.small_batch()
    keep = SR.keep_outs(starts, goals, origins, 1.0, 1)
    _m, _b, counts = _raw(torch_cuda, owner, data, None, origins, 1.0, frame, keep, SR.yaw_table(16), 64, max_attempts, 11,
                          (0.1, 0.9), (0.3, 1.6))
    assert counts.max() >= 1 and (max_attempts != 257 or counts.max() == 64)


def test_the_attempt_behind_the_chunk_boundary(torch_cuda, owner):
    """257 attempts where 256 do not fill the slots: attempt 256, the second chunk's only one, is some entry's last box"""
    data, origins, frame, starts, goals = TH.small_batch(n=24, seed=5)
    keep = SR.keep_outs(starts, goals, origins, 1.0, 14)
    args = (torch_cuda, owner, data, None, origins, 1.0, frame, keep, SR.yaw_table(16), 64)
    _m, _b, c256 = _raw(*args, 256, 11, (0.0, 1.0), (0.3, 1.0))
    _m, b257, c257 = _raw(*args, 257, 11, (0.0, 1.0), (0.3, 1.0))
    grew = c257 > c256
    assert (c256 < 64).all() and grew.any() and (b257[grew, c257[grew] - 1, 0] == 256).all()


def test_three_padded_entries(torch_cuda, owner):
    data, valid, origins, res, frame = _padded()
    maps, _b, counts = _raw(torch_cuda, owner, data, valid, origins, res, frame, None, SR.yaw_table(16), 6, 40, 2, (0, 1), (0.2, 1.2))
    assert counts.min() >= 1
    for i, (vr, vc) in enumerate(valid):
        assert (maps[i, vr:] == 77).all() and (maps[i, :, vc:] == 77).all()
    # a cell on the last valid row and column is accepted, one beyond either is not
    for dr, dc, n_ok in ((0, 0, 1), (1, 0, 0), (0, 1, 0)):
        f = np.zeros((3, 6))
        f[:, 0] = origins[:, 0] + (valid[:, 1] - 1 + dc) * res
        f[:, 1] = origins[:, 1] + (valid[:, 0] - 1 + dr) * res
        _m, _b, counts = _raw(torch_cuda, owner, data, valid, origins, res, f, None, SR.yaw_table(4), 2, 1, 1, (0, 1), (0, 0))
        assert list(counts) == [n_ok] * 3


def test_the_golden_worlds_in_the_dense_configuration(torch_cuda, owner):
    maps, origins, res, _starts, _goals = SR.golden()
    want_maps, want_boxes, want_counts, frame, keep, yaw_cs = SR.dense_golden()
    d = SR.DENSE
    # the conditions on the reference's output alone
    routable = SR.dense_golden_routable(151)
    print("reference: counts", want_counts.tolist(), "unroutable", np.nonzero(~routable)[0].tolist())
    assert (want_counts < d["n_boxes"]).any()
    assert 1 <= (~routable).sum() <= len(routable) // 4
    got, _b, _c = _raw(torch_cuda, owner, maps, None, origins, res, frame, keep, yaw_cs, d["n_boxes"], d["max_attempts"], d["seed"],
                       d["along"], d["half_size"], want=(want_maps, want_boxes, want_counts))
    # ... and bcp_goal_field on the scattered maps agrees about which worlds lost their route
    s = SR.cells_of(SR.golden()[3], origins, res)
    g = SR.cells_of(SR.golden()[4], origins, res)
    fields = owner.goal_field(got.copy(), g[:, None, :].astype(np.int32), 151).cpu().numpy()
    assert ((fields[np.arange(48), s[:, 0], s[:, 1]] != 65535) == routable).all()
    # NativeOps.scatter_boxes: the same bytes, in place on a device tensor
    t = torch_cuda.from_numpy(maps.copy()).cuda()
    out, boxes, counts = owner.scatter_boxes(t, origins.copy(), res, frame.copy(), yaw_cs.copy(), d["n_boxes"], d["half_size"],
                                             d["along"], keep.copy(), None,
                                             d["seed"], d["max_attempts"])
    assert out is t and (t.cpu().numpy() == want_maps).all()
    assert (boxes.cpu().numpy() == want_boxes).all() and (counts.cpu().numpy() == want_counts).all()


def test_a_captured_call_replays_the_same_bytes(torch_cuda, owner):
    torch = torch_cuda
    maps, origins, res, _s, _g = SR.golden()
    want_maps, want_boxes, want_counts, frame, keep, yaw_cs = SR.dense_golden()
    d = SR.DENSE
    case = _Case(torch, maps[:16], None, origins[:16], frame[:16], keep[:16], yaw_cs, d["n_boxes"])
    p = _params(d["n_boxes"], d["max_attempts"], len(yaw_cs), d["seed"], d["along"], d["half_size"])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        assert case.call(owner, p, res, C.c_void_p(stream.cuda_stream)) == 0          # one ordinary call
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            assert case.call(owner, p, res, C.c_void_p(stream.cuda_stream)) == 0
    torch.cuda.synchronize()
    for _replay in range(2):
        case.restore(torch)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got_maps, boxes, counts = case.read()
        assert (got_maps == want_maps[:16]).all() and (boxes == want_boxes[:16]).all() and (counts == want_counts[:16]).all()


def test_every_refusal_and_nothing_written(torch_cuda, owner):
    torch = torch_cuda
    from bc_gym_planning_env_amd import _lib
    data, origins, frame, starts, goals = TH.small_batch()
    keep = SR.keep_outs(starts, goals, origins, 1.0, 1)
    case = _Case(torch, data, np.tile([9, 9], (5, 1)), origins, frame, keep, SR.yaw_table(16), 4)
    good = dict(n_boxes=4, max_attempts=8, n_yaws=16, seed=1, along=(0.1, 0.9), half_size=(0.3, 1.0))
    L, h = owner._lib, owner._h

    def call(h=h, p=good, n=5, rows=9, cols=9, res=1.0, vr=True, vc=True, data=True, origins=True, frame=True, keep=True, n_keep=2,
             yaw=True, boxes=True, counts=True):
        ptr = lambda t, on: t.data_ptr() if on else None   # noqa: E731
        pp = None if p is None else _params(**p)
        return L.bcp_scatter_boxes(h, ptr(case.maps[1:], data), n, rows, cols, ptr(case.vr, vr), ptr(case.vc, vc),
                                   ptr(case.origins, origins), res, None if pp is None else C.byref(pp), ptr(case.frame, frame),
                                   ptr(case.keep, keep), n_keep, ptr(case.yaw, yaw), ptr(case.boxes[1:], boxes),
                                   ptr(case.counts[1:], counts), None)

    def bad(**kw):
        p = dict(good)
        p.update(kw)
        return p

    nan, inf = float("nan"), float("inf")
    refusals = [
        dict(h=None), dict(p=None), dict(n=-1), dict(rows=0), dict(cols=2049), dict(res=0.0), dict(res=nan), dict(res=inf),
        dict(p=bad(n_boxes=0)), dict(p=bad(n_boxes=65)), dict(p=bad(max_attempts=0)), dict(p=bad(max_attempts=4097)),
        dict(p=bad(n_yaws=0)), dict(p=bad(n_yaws=4097)), dict(n_keep=-1), dict(n_keep=17),
        dict(p=bad(along=(0.9, 0.1))), dict(p=bad(along=(nan, 1.0))), dict(p=bad(along=(0.0, inf))),
        dict(p=bad(half_size=(-0.1, 1.0))), dict(p=bad(half_size=(1.0, 0.5))), dict(p=bad(half_size=(0.0, inf))),
        dict(p=bad(half_size=(0.3, 1.8))), dict(vr=False), dict(vc=False),
        dict(data=False), dict(origins=False), dict(frame=False), dict(yaw=False), dict(boxes=False), dict(counts=False),
        dict(keep=False),
    ]
    for kw in refusals:
        assert call(**kw) == E_INVALID, kw
        assert b"bcp_scatter_boxes" in L.bcp_last_error(), kw
    # the order: the earlier of two wrong arguments names the refusal
    for kw, word in ((dict(h=None, p=None), b"null handle"), (dict(p=None, n=-1), b"null params"), (dict(n=-1, rows=0), b"n_maps"),
                     (dict(rows=0, res=0.0), b"shape"), (dict(res=0.0, p=bad(n_boxes=0)), b"resolution"),
                     (dict(p=bad(n_boxes=0, max_attempts=0)), b"n_boxes"), (dict(p=bad(max_attempts=0, n_yaws=0)), b"max_attempts"),
                     (dict(p=bad(n_yaws=0), n_keep=17), b"n_yaws"), (dict(n_keep=17, p=bad(along=(1.0, 0.0))), b"n_keep"),
                     (dict(p=bad(along=(1.0, 0.0), half_size=(1.0, 0.0))), b"along"),
                     (dict(p=bad(half_size=(-1.0, 9.0))), b"half_size must"), (dict(p=bad(half_size=(0.3, 1.8)), vr=False), b"need not fit"),
                     (dict(vr=False, data=False), b"go together"), (dict(data=False), b"null data")):
        assert call(**kw) == E_INVALID and word in L.bcp_last_error(), (kw, L.bcp_last_error())
    torch.cuda.synchronize()
    maps, boxes, counts = case.read()
    assert (maps == data).all() and (boxes == POISON_I).all() and (counts == POISON_I).all()
    # accepted: no entries at all, whatever the arrays are; and no keep-outs without their array
    assert call(n=0, data=False, boxes=False) == 0 and call(keep=False, n_keep=0) == 0
    _lib.check(call())
    torch.cuda.synchronize()


# ---- scatter_obstacles ---------------------------------------------------------------------------------------------------
# (keep_clear None: the footprint's circumscribed radius, 1.35 m for the tricycle -- the start and goal poses stay free)
DENSE_ENV = dict(n_boxes=12, half_size=(0.2, 0.5), along=(0.2, 0.8), lateral=2.0, keep_clear=None, n_yaws=16, seed=7, max_attempts=32)


def _expect(env, original, cfg, clearance_d2=151):
    """what scatter_obstacles(**cfg) must leave, from the env's bound tensors and the reference alone
    -> (maps, status, counts, boxes, start cells, goal cells, scattered maps before any revert)"""
    data, valid, origins = original, TG._maps_of(env)[1], TG._maps_of(env)[2]
    starts, goals = TR._bound_ends(env)
    res = env.resolution
    frame = SR.frames(starts, goals, cfg["lateral"])
    clear = cfg["keep_clear"] if cfg["keep_clear"] is not None else float(np.linalg.norm(env.footprint(), axis=1).max())
    d2 = (int(np.ceil(clear / res)) + 1) ** 2
    keep = SR.keep_outs(starts, goals, origins, res, d2)
    maps, boxes, counts = SR.scatter(data, valid, origins, res, cfg["n_boxes"], cfg["max_attempts"], cfg["n_yaws"], cfg["seed"],
                                     cfg["along"], cfg["half_size"], frame, keep, SR.yaw_table(cfg["n_yaws"]))
    s, g = SR.cells_of(starts, origins, res), SR.cells_of(goals, origins, res)
    cut = np.array([not SR.routable(maps[k], valid[k], clearance_d2, s[k], g[k]) for k in range(len(maps))])
    status = (counts < cfg["n_boxes"]) * SR.SHORT + cut * SR.REVERTED
    final = np.where(cut[:, None, None], data, maps)
    return final, status, counts, boxes, s, g, maps


def _check_scattered(torch, env, original, cfg, got):
    """the env after scatter_obstacles(**cfg) = got: bytes, status, host copies, start and goal poses"""
    from bc_gym_planning_env_amd.ops import NativeOps
    status, counts, boxes = (t.cpu().numpy() for t in got)
    final, want_status, want_counts, want_boxes, s, _g, _scattered = _expect(env, original, cfg)
    print("counts", want_counts.tolist(), "status", want_status.tolist())
    assert (counts == want_counts).all() and (boxes == want_boxes).all() and (status == want_status).all()
    now = env.costmap_tensor.cpu().numpy()
    assert (now == final).all()
    reverted = (status & SR.REVERTED) != 0
    assert (now[reverted] == original[reverted]).all()
    _data, valid, origins = TG._maps_of(env)
    # kept entries have a value at the start cell of a fresh goal field, reverted ones had none on their scattered maps
    fresh = env.goal_field().field.cpu().numpy()
    at = fresh[np.arange(len(now)), s[:, 0], s[:, 1]]
    assert (at[~reverted] != 65535).all()
    # bcp_pose_collides is false at every start and goal pose; the host copies follow
    starts, goals = TR._bound_ends(env)
    ops = NativeOps(robot_name=env.robot_name)
    for k in range(len(now)):
        ops.set_costmap(now[k, :valid[k, 0], :valid[k, 1]].copy(), origins[k], env.resolution)
        assert not ops.pose_collides(np.stack([starts[k], goals[k]])).cpu().numpy().any(), k
    for i in range(env.n_envs):
        k = int(env.geom_of_env[i]) if env.geom_of_env is not None else i
        cm = env.envs[i].get_state().costmap
        assert (cm.get_data() == now[k, :valid[k, 0], :valid[k, 1]]).all(), i
    return status, reverted


def _golden_pool_env(n=16, **kw):
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    maps, origins, res, starts, goals = SR.golden()
    costmaps = [CostMap2D(maps[k].copy(), res, origins[k].copy()) for k in range(n)]
    paths = [np.stack([starts[k], goals[k]]) for k in range(n)]
    params = EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=60)
    return BatchedPlanEnv(costmaps, paths, params, n_envs=n, geom_of_env=np.arange(n), next_geom=np.roll(np.arange(n), -1),
                          auto_reset=True, seed=2, **kw), paths


def test_scatter_obstacles_on_a_pool_of_sixteen_golden_worlds(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, _lib
    env, paths = _golden_pool_env()
    original = env.costmap_tensor.cpu().numpy().copy()
    got = env.scatter_obstacles(**DENSE_ENV)
    status, reverted = _check_scattered(torch, env, original, DENSE_ENV, got)
    assert reverted.any() and not reverted.all() and (status & SR.SHORT).any()
    assert (_lib.SCATTER_SHORT, _lib.SCATTER_REVERTED) == (SR.SHORT, SR.REVERTED)
    # 32 steps of random actions: bit for bit those of a fresh env built from the scattered maps
    now = env.costmap_tensor.cpu().numpy()
    _m, origins, res, _s, _g = SR.golden()
    fresh = BatchedPlanEnv([CostMap2D(now[k].copy(), res, origins[k].copy()) for k in range(16)], paths, env.params, n_envs=16,
                           geom_of_env=np.arange(16), next_geom=np.roll(np.arange(16), -1), auto_reset=True, seed=2)
    fresh.reset()
    TR._step_together(torch, env, fresh, 32, seed=5)
    # routes on the new maps: every kept entry whose route fits the slots gets one
    route = env.route_paths(stride=2, max_len=200).cpu().numpy()
    assert ((route[~reverted] & ~_lib.ROUTE_LONG) == 0).all() and (route[~reverted] == 0).any()
    # refusals
    with pytest.raises(RuntimeError, match="endless"):
        TG._mini(16, timeout=6, endless=True).scatter_obstacles(2, (0.2, 0.4))
    maps, origins, res, starts, goals = SR.golden()
    shared = BatchedPlanEnv(CostMap2D(maps[0].copy(), res, origins[0]), np.stack([starts[0], goals[0]]), env.params, n_envs=4)
    with pytest.raises(RuntimeError, match="private maps with private paths"):
        shared.scatter_obstacles(2, (0.2, 0.4))
    inflated, _p = _golden_pool_env(4)
    inflated.inflate_costmaps(10.0)
    with pytest.raises(RuntimeError, match="scatter first"):
        inflated.scatter_obstacles(2, (0.2, 0.4))
    with pytest.raises(_lib.BcpError, match="n_boxes"):
        _golden_pool_env(4)[0].scatter_obstacles(65, (0.2, 0.4))


def test_scatter_obstacles_on_expanded_templates(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    maps, origins, res, starts, goals = SR.golden()
    worlds, of = (0, 5, 17), np.array([2, 0, 1, 0, 2, 1])
    costmaps = [CostMap2D(maps[w].copy(), res, origins[w].copy()) for w in worlds]
    paths = [np.stack([starts[w], goals[w]]) for w in worlds]
    params = EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=60)
    env = BatchedPlanEnv(costmaps, paths, params, n_envs=6, template_of_env=of, seed=3)
    original = env.costmap_tensor.cpu().numpy().copy()
    got = env.scatter_obstacles(**DENSE_ENV)
    _check_scattered(torch, env, original, DENSE_ENV, got)
    now = env.costmap_tensor.cpu().numpy()
    assert not (now[1] == now[3]).all()          # two envs of one template: entries 1 and 3 draw their own boxes
    fresh = BatchedPlanEnv([CostMap2D(now[i].copy(), res, origins[worlds[of[i]]].copy()) for i in range(6)],
                           [paths[t] for t in of], params, n_envs=6, seed=3)
    rng = np.random.RandomState(8)
    for t in range(32):
        act = env.action_space.sample_batch(6, rng) * np.array([3.0, 1.0], dtype=np.float32)
        _o, ra, da, _i = env.step(act)
        _o, rb, db, _i = fresh.step(act)
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(env.state.robot, fresh.state.robot), t


def test_scatter_obstacles_on_a_device_resident_pool(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, mini_env
    params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=60))
    env = mini_env.BatchedRandomMiniEnv(16, params, seeds=[1, 2, 3, 4], episodes=4, sampler="device_resident", auto_reset=True, seed=2)
    dp = env.pool
    original = dp.maps.cpu().numpy().copy()
    ptr = dp.maps.data_ptr()
    got = env.scatter_obstacles(**DENSE_ENV)
    status, reverted = _check_scattered(torch, env, original, DENSE_ENV, got)
    assert dp.maps.data_ptr() == ptr and env.costmap_tensor is dp.maps          # the pool is changed where it is
    assert (dp.maps.cpu().numpy() != original).any()
    # a fresh env on a copy of the scattered pool -- the same device-computed initial states, which an auto-reset restores
    from bc_gym_planning_env_amd import BatchedPlanEnv
    from bc_gym_planning_env_amd.geometry import DeviceGeometryPool, chain_layout
    copy = DeviceGeometryPool(dp.maps.clone(), dp.origin, dp.resolution, dp.path_points.clone(), dp.lens.clone(), dp.init.clone(),
                              origins=dp.origins, valid_rows=dp.valid_rows, valid_cols=dp.valid_cols)
    fresh = BatchedPlanEnv(copy, None, env.params, n_envs=16, geom_of_env=chain_layout(16, len(dp.seeds), dp.episodes),
                           next_geom=dp.next_geom, auto_reset=True, seed=2)
    fresh.reset()
    TR._step_together(torch, env, fresh, 32, seed=9)


def test_scatter_obstacles_on_an_aisle_pool(torch_cuda):
    """entries with their own valid shapes and origins inside one padded tensor"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, aisle_env
    env = aisle_env.BatchedRandomAisleTurnEnv(8, EnvParams(iteration_timeout=40), seeds=[0, 1], episodes=4, sampler="host",
                                              auto_reset=True, seed=1)
    original = env.costmap_tensor.cpu().numpy().copy()
    _data, valid, _origins = TG._maps_of(env)
    assert len(set(map(tuple, valid.tolist()))) > 1
    cfg = dict(DENSE_ENV, n_boxes=6, half_size=(0.1, 0.3), lateral=0.8, seed=3)
    got = env.scatter_obstacles(**cfg)
    _check_scattered(torch, env, original, cfg, got)
    now = env.costmap_tensor.cpu().numpy()
    for k, (vr, vc) in enumerate(valid):          # not a byte outside the valid shapes changed
        assert (now[k, vr:] == original[k, vr:]).all() and (now[k, :, vc:] == original[k, :, vc:]).all()
    assert (now != original).any()


def test_boxes_wider_than_a_corridor_are_reverted(torch_cuda):
    """a hand-made corridor of 21 cells between two walls; boxes of half size 0.6 .. 0.7 m at yaw 0 across it, centred on the
    axis (lateral 0): every accepted box severs it, as the reference is asked first"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    res = 0.05
    data = np.zeros((60, 120), dtype=np.uint8)
    data[19, :] = data[41, :] = 254                                   # the corridor: rows 20 .. 40
    data[:19, :] = data[42:, :] = 254
    origin = np.array([0.0, 0.0])
    start, goal = np.array([10 * res, 30 * res, 0.0]), np.array([110 * res, 30 * res, 0.0])
    params = EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=60, resolution=res)
    env = BatchedPlanEnv([CostMap2D(data.copy(), res, origin)] * 2, [np.stack([start, goal])] * 2, params, n_envs=2)
    cfg = dict(n_boxes=2, half_size=(0.6, 0.7), along=(0.3, 0.7), lateral=0.0, keep_clear=0.5, n_yaws=1, seed=1, max_attempts=8)
    original = env.costmap_tensor.cpu().numpy().copy()
    clearance = 0.2
    d2 = int(np.floor((clearance / res) ** 2))
    _final, want_status, want_counts, want_boxes, s, g, scattered = _expect(env, original, cfg, clearance_d2=d2)
    assert (want_counts >= 1).all()
    for k in range(2):                                                 # on the reference: every accepted box severs the corridor
        for b in want_boxes[k, :want_counts[k]]:
            one = original[k].copy()
            one[SR.pixel_set(one.shape, b[1:].reshape(4, 2))] = 254
            assert not SR.routable(one, one.shape, d2, s[k], g[k])
    status, counts, _boxes = env.scatter_obstacles(clearance=clearance, **cfg)
    assert (status.cpu().numpy() & SR.REVERTED).all() and (counts.cpu().numpy() == want_counts).all()
    assert (env.costmap_tensor.cpu().numpy() == original).all()
    # without ensure_route the same call keeps the boxes
    status, _c, _b = env.scatter_obstacles(ensure_route=False, **cfg)
    assert not (status.cpu().numpy() & SR.REVERTED).any() and (env.costmap_tensor.cpu().numpy() == scattered).all()

"""bcp_goal_field_cost / bcp_goal_field_cost_bound on the GPU (goal_field_kernel<.., kCost>), and the Python surface over them,
byte for byte against the contract restated in numpy / heapq (tests/goal_cost_ref.py: a weighted Dijkstra).  Nothing has a
tolerance but what the plain tests already bound (headings, min_spat_dist_so_far: 1e-9).  Fields go into sentinel-filled
buffers with a map's worth of guard on either side.  Every case uses the smallest shape at which its mechanism can go wrong;
references are computed once per session and shared."""
import functools

import attr
import numpy as np
import pytest

import goal_cost_ref as CR
import goal_field_ref as GR
import goal_route_ref as RR
import test_gpu_goal_field as TG

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
SENTINEL, POISON_I = TG.SENTINEL, TG.POISON_I
ZERO = np.zeros(256, dtype=np.uint16)


def _u16(table):
    return None if table is None else np.ascontiguousarray(np.asarray(table).astype(np.uint16))


@functools.lru_cache(maxsize=None)
def _ref_cached(data_bytes, shape, seeds, clearance_d2, table_bytes, valid):
    data = np.frombuffer(data_bytes, dtype=np.uint8).reshape(shape)
    field = CR.dijkstra(data, list(seeds), clearance_d2, np.frombuffer(table_bytes, dtype=np.uint16), valid)
    field.setflags(write=False)
    return field


def _ref(data, seeds, clearance_d2, table, valid=None):
    """the weighted Dijkstra's field, computed once per (map, seeds, clearance, table, valid shape) of the session"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    seeds = tuple((int(r), int(c)) for r, c in np.asarray(seeds).reshape(-1, 2))
    return _ref_cached(data.tobytes(), data.shape, seeds, int(clearance_d2), _u16(table).tobytes(),
                       None if valid is None else (int(valid[0]), int(valid[1])))


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from bc_gym_planning_env_amd.ops import NativeOps
    return NativeOps()


@pytest.fixture(scope="module")
def forced(torch_cuda):
    """a handle whose goal fields take the global route whatever the size"""
    from bc_gym_planning_env_amd import _lib
    from bc_gym_planning_env_amd.ops import NativeOps
    o = NativeOps()
    assert o._lib.bcp_set_tuning(o._h, _lib.TUNE_GOAL_ROUTE, 2) == 0
    return o


def _raw(torch, ops, data, seeds, clearance_d2, table, valid=None, shared=False, max_passes=0, want_rc=0, plain=False):
    """bcp_goal_field_cost through the C ABI (plain: bcp_goal_field, the table unused): data [n, rows, cols] (or [rows, cols]
    with shared), seeds [n, S, 2], valid None or (rows [n], cols [n]).  -> (fields uint16 [n, rows, cols], info int32 [n, 2]);
    the guards around `out` and `info` are checked"""
    data = np.array(data, dtype=np.uint8)
    seeds = np.ascontiguousarray(seeds, dtype=np.int32)
    n, rows, cols = seeds.shape[0], data.shape[-2], data.shape[-1]
    cells = rows * cols
    d = torch.from_numpy(data).cuda()
    s = torch.from_numpy(seeds).cuda()
    vr = vc = None
    if valid is not None:
        vr = torch.tensor(list(valid[0]), dtype=torch.int32, device="cuda")
        vc = torch.tensor(list(valid[1]), dtype=torch.int32, device="cuda")
    out = torch.from_numpy(np.full((n + 2) * cells, SENTINEL, dtype=np.uint16)).cuda()
    info = torch.full((n + 2, 2), POISON_I, dtype=torch.int32, device="cuda")
    head = (ops._h, d.data_ptr(), n, rows, cols, int(shared), vr.data_ptr() if vr is not None else None,
            vc.data_ptr() if vc is not None else None, s.data_ptr(), seeds.shape[1], int(clearance_d2), int(max_passes))
    tail = (out.data_ptr() + 2 * cells, info.data_ptr() + 8, None)
    if plain:
        rc = ops._lib.bcp_goal_field(*(head + tail))
    else:
        t = _u16(table)
        rc = ops._lib.bcp_goal_field_cost(*(head + (t.ctypes.data if t is not None else None,) + tail))
    assert rc == want_rc, ops._lib.bcp_last_error()
    torch.cuda.synchronize()
    o, i = out.cpu().numpy(), info.cpu().numpy()
    assert (o[:cells] == SENTINEL).all() and (o[(n + 1) * cells:] == SENTINEL).all(), "guard overwritten"
    assert (i[0] == POISON_I).all() and (i[n + 1] == POISON_I).all()
    return o[cells:(n + 1) * cells].reshape(n, rows, cols), i[1:n + 1]


def _one(torch, ops, data, seeds, clearance_d2, table, valid=None, max_passes=0, plain=False):
    v = None if valid is None else ([valid[0]], [valid[1]])
    f, i = _raw(torch, ops, np.asarray(data)[None], np.asarray(seeds, dtype=np.int32).reshape(1, -1, 2), clearance_d2, table, v,
                max_passes=max_passes, plain=plain)
    return f[0], i[0]


def _same(torch, got, want, info, what):
    bad = int((got != want).sum())
    print(what, "cells", got.size, "with a value", int((want != GR.NONE).sum()), "largest", int(want[want != GR.NONE].max()) if (want != GR.NONE).any() else None,
          "different:", bad, "info", info.tolist())
    assert torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(want.copy())), (what, bad)
    assert info[0] == (want != GR.NONE).sum() and info[1] == 0, (what, info)


def _table(**entries):
    t = ZERO.copy()
    for k, v in entries.items():
        t[int(k[1:])] = v
    return t


RAMP = ((np.arange(256) * 7) % 40).astype(np.uint16)          # an extra for every byte, 254 and 255 too


# ---- 1. the rule on small maps -----------------------------------------------------------------------------------------
def test_the_hand_case(torch_cuda, ops, forced):
    torch = torch_cuda
    data = np.array([[0, 7, 0, 9]], dtype=np.uint8)
    for o in (ops, forced):
        got, info = _one(torch, o, data, [(0, 0)], 0, _table(c7=5, c9=3))
        assert got.tolist() == [[0, 17, 29, 44]] and info.tolist() == [4, 0]


def test_the_three_edge_shapes(torch_cuda, ops, forced):
    torch = torch_cuda
    rng = np.random.RandomState(2)
    for o in (ops, forced):
        got, info = _one(torch, o, np.full((1, 1), 200, dtype=np.uint8), [(0, 0)], 0, RAMP)
        assert got.tolist() == [[0]] and info.tolist() == [1, 0]
        for shape, seed in (((1, 70), (0, 3)), ((70, 1), (66, 0))):
            data = rng.randint(0, 253, size=shape).astype(np.uint8)
            data[-1, -1] = 254
            for cd2 in (0, 4):
                got, info = _one(torch, o, data, [seed], cd2, RAMP)
                _same(torch, got, _ref(data, [seed], cd2, RAMP), info, "%s clearance_d2 %d" % (shape, cd2))


def test_padded_maps_with_junk_in_the_padding(torch_cuda, ops, forced):
    """five maps in one 40 x 70 allocation with valid shapes from (0, .) and (., 0) to full; the padding holds bytes whose
    extra is the largest there is, and 254s"""
    torch = torch_cuda
    rng = np.random.RandomState(8)
    valid = [(0, 50), (30, 0), (17, 33), (40, 70), (39, 65)]
    table = RAMP.copy()
    table[200] = 4095
    data = np.where(rng.uniform(size=(5, 40, 70)) < 0.5, 254, 200).astype(np.uint8)
    seeds = np.zeros((5, 2, 2), dtype=np.int32)
    for k, (vr, vc) in enumerate(valid):
        data[k, :vr, :vc] = np.where(rng.uniform(size=(vr, vc)) < 0.1, 254, rng.randint(0, 100, size=(vr, vc)))
        seeds[k] = [(vr // 2, vc // 2), (vr - 1, vc - 1)]
    clean = data.copy()
    for k, (vr, vc) in enumerate(valid):
        clean[k, vr:] = 0
        clean[k, :, vc:] = 0
    for o in (ops, forced):
        for cd2 in (0, 5):
            got, info = _raw(torch, o, data, seeds, cd2, table, ([v[0] for v in valid], [v[1] for v in valid]))
            for k, (vr, vc) in enumerate(valid):
                want = _ref(clean[k], seeds[k], cd2, table, valid[k])        # (the reference never saw the junk)
                _same(torch, got[k], want, info[k], "padded map %d clearance_d2 %d" % (k, cd2))
                assert (got[k, vr:] == GR.NONE).all() and (got[k, :, vc:] == GR.NONE).all()
            assert (got[0] == GR.NONE).all() and (got[1] == GR.NONE).all()


def test_a_costly_band_with_a_gap(torch_cuda, ops, forced):
    torch = torch_cuda
    for o in (ops, forced):
        data, table, seed, far = CR.banded(200)
        got, info = _one(torch, o, data, [seed], 0, table)
        _same(torch, got, _ref(data, [seed], 0, table), info, "band 200")
        cells = CR.route_cells(got, far)
        assert got[far] == 8 * 17 and (8, 4) in cells and not any(c == 4 and r < 8 for r, c in cells)
        got, info = _one(torch, o, data, [seed, (2, 4)], 0, table)             # a seed on a costly cell
        _same(torch, got, _ref(data, [seed, (2, 4)], 0, table), info, "band 200, a seed on it")
        assert got[2, 4] == 0 and got[1, 4] == 212 and got[far] == 2 * 17 + 2 * 12
        data, table, seed, far = CR.banded(1)
        got, info = _one(torch, o, data, [seed], 0, table)
        _same(torch, got, _ref(data, [seed], 0, table), info, "band 1")
        assert got[far] == 8 * 12 + 1 and CR.route_cells(got, far) == [(4, c) for c in range(8, -1, -1)]


# ---- 2. the reference worlds under inflation: both routes ------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 2])
@pytest.mark.parametrize("world", [5, 9, 17])
def test_inflated_worlds_equal_the_weighted_dijkstra(torch_cuda, ops, forced, world, route):
    torch = torch_cuda
    o = forced if route == 2 else ops
    cost = CR.inflated_world(world)
    _data, _origin, _res, goal, start = GR.mini_world(world)
    for weight in (2, 8):
        want = CR.world_field(world, weight)
        got, info = _one(torch, o, cost, [goal], CR.CLEARANCE_D2, CR.cost_table(weight))
        _same(torch, got, want, info, "world %d weight %d route %d" % (world, weight, route))
        assert got[goal] == 0 and got[start] != GR.NONE
        field = o.goal_field(np.array(cost), [goal], CR.CLEARANCE_D2, extra_of_cost=CR.cost_table(weight))     # NativeOps: the same bytes
        assert field.dtype == torch.uint16 and (field.cpu().numpy() == want).all()


def test_map_beyond_lds(torch_cuda, ops):
    """300 x 300: 176 KB of plane, the global route by size; random costs, about 1 % lethal cells"""
    torch = torch_cuda
    rng = np.random.RandomState(4)
    data = rng.randint(0, 253, size=(300, 300)).astype(np.uint8)
    data[rng.uniform(size=(300, 300)) < 0.01] = 254
    data[150, 20:280] = 254
    seeds = [(10, 290), (299, 0)]
    got, info = _one(torch, ops, data, seeds, 8, RAMP)
    _same(torch, got, _ref(data, seeds, 8, RAMP), info, "300 x 300")


def test_a_table_of_zeros_is_the_plain_call(torch_cuda, ops, forced):
    torch = torch_cuda
    rng = np.random.RandomState(13)
    data = rng.randint(0, 256, size=(3, 70, 65)).astype(np.uint8)
    data[rng.uniform(size=data.shape) < 0.12] = 254
    seeds = np.array([[(2, 3), (60, 60)], [(35, 32), (-1, -1)], [(69, 64), (0, 0)]], dtype=np.int32)
    valid = ([70, 55, 70], [65, 65, 40])
    for o in (ops, forced):
        for cd2 in (0, 3):
            a, ia = _raw(torch, o, data, seeds, cd2, ZERO, valid)
            b, ib = _raw(torch, o, data, seeds, cd2, None, valid, plain=True)
            assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes() and (a != GR.NONE).any()
        cost = CR.inflated_world(17)
        goal = GR.mini_world(17)[3]
        a, ia = _one(torch, o, cost, [goal], CR.CLEARANCE_D2, ZERO)
        b, ib = _one(torch, o, cost, [goal], CR.CLEARANCE_D2, None, plain=True)
        assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes()
        assert (a == GR.mini_field(17, CR.CLEARANCE_D2)).all()


# ---- 3. batches, sharing, nothing to do ----------------------------------------------------------------------------------
def test_batches_shared_maps_and_no_maps(torch_cuda, ops):
    torch = torch_cuda
    rng = np.random.RandomState(21)
    data = rng.randint(0, 253, size=(16, 50, 45)).astype(np.uint8)
    data[rng.uniform(size=data.shape) < 0.15] = 254
    seeds = rng.randint(0, 45, size=(16, 3, 2)).astype(np.int32)
    batch, info = _raw(torch, ops, data, seeds, 2, RAMP)
    for k in range(16):
        single, info1 = _one(torch, ops, data[k], seeds[k], 2, RAMP)
        assert (batch[k] == single).all() and (info[k] == info1).all(), k
        if k < 3:
            _same(torch, single, _ref(data[k], seeds[k], 2, RAMP), info1, "batch entry %d" % k)
    assert len({batch[k].tobytes() for k in range(16)}) == 16
    shared, info = _raw(torch, ops, data[0], seeds[:3], 2, RAMP, shared=True)        # one map, three seed sets
    for k in range(3):
        _same(torch, shared[k], _ref(data[0], seeds[k], 2, RAMP), info[k], "shared, seed set %d" % k)
    field = ops.goal_field(data[0], seeds[:3], 2, extra_of_cost=RAMP)
    assert field.shape == (3, 50, 45) and (field.cpu().numpy() == shared).all()
    # n_maps == 0 succeeds and does nothing, whatever the pointers -- but the table is still looked at
    L = ops._lib
    assert L.bcp_goal_field_cost(ops._h, None, 0, 50, 45, 0, None, None, None, 1, 0, 0, RAMP.ctypes.data, None, None, None) == 0
    assert L.bcp_goal_field_cost(ops._h, None, 0, 50, 45, 0, None, None, None, 1, 0, 0, None, None, None, None) == E_INVALID


def test_shared_map_on_the_global_route(torch_cuda, forced):
    torch = torch_cuda
    rng = np.random.RandomState(22)
    data = rng.randint(0, 253, size=(40, 37)).astype(np.uint8)
    data[rng.uniform(size=data.shape) < 0.1] = 254
    seeds = rng.randint(0, 37, size=(3, 2, 2)).astype(np.int32)
    shared, info = _raw(torch, forced, data, seeds, 1, RAMP, shared=True)
    for k in range(3):
        _same(torch, shared[k], _ref(data, seeds[k], 1, RAMP), info[k], "global route, shared, seed set %d" % k)


# ---- 4. saturation and the cap ---------------------------------------------------------------------------------------------
def test_serpentine_saturated_and_capped(torch_cuda, ops, forced):
    torch = torch_cuda
    data = GR.serpentine(33)
    table = _table(c0=4095)
    want = _ref(data, [(0, 0)], 0, table)
    assert (want == GR.FAR).sum() == 561 and want[0, 15] == 15 * 4107 and want[0, 16] == GR.FAR
    for o in (ops, forced):
        got, info = _one(torch, o, data, [(0, 0)], 0, table)
        _same(torch, got, want, info, "serpentine 33, extra 4095")
        assert info[0] == 577
        capped, info = _one(torch, o, data, [(0, 0)], 0, table, max_passes=20)
        print("serpentine 33, max_passes 20: info", info.tolist(), "cells with a value", int((capped != GR.NONE).sum()))
        assert info[1] == 1 and info[0] == (capped != GR.NONE).sum()
        assert (capped >= want).all() and (capped[want == GR.NONE] == GR.NONE).all()
        assert (capped != want).any()      # (20 passes of a wave per row cannot walk 576 cells of corridor)


# ---- 5. the bound form ---------------------------------------------------------------------------------------------------
def _golden_pool_env(n=16):
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    import scatter_boxes_ref as SR
    maps, origins, res, starts, goals = SR.golden()
    costmaps = [CostMap2D(maps[k].copy(), res, origins[k].copy()) for k in range(n)]
    paths = [np.stack([starts[k], goals[k]]) for k in range(n)]
    params = EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=60)
    env = BatchedPlanEnv(costmaps, paths, params, n_envs=n, geom_of_env=np.arange(n), next_geom=np.roll(np.arange(n), -1),
                         auto_reset=True, seed=2)
    return env, costmaps


@pytest.fixture(scope="module")
def pool(torch_cuda):
    """16 golden worlds, inflated on the device: (env, maps as bound, valid, origins, goal cells).  Nothing below changes it."""
    env, _costmaps = _golden_pool_env()
    env.inflate_costmaps(CR.COST_SCALING)
    env.reset()
    data, valid, origins = TG._maps_of(env)
    assert len(np.unique(data)) > 100 and ((data == 254) == (np.stack([GR.mini_world(k)[0] for k in range(16)]) == 254)).all()
    return env, data, valid, origins, TG._goal_cells(env, 16)


def _pool_ref(pool, weight):
    _env, data, valid, _origins, cells = pool
    return np.stack([_ref(data[k], [cells[k]], CR.CLEARANCE_D2, CR.cost_table(weight), valid[k]) for k in range(16)])


def _bound(torch, env, table, entries=None, count=None, n_list=16, want_rc=0, max_passes=0):
    """bcp_goal_field_cost_bound into poisoned outputs -> (field [16, 183, 183], info [16, 2])"""
    field = torch.from_numpy(np.full((16, 183, 183), SENTINEL, dtype=np.uint16)).cuda()
    info = torch.full((16, 2), POISON_I, dtype=torch.int32, device="cuda")
    et = None if entries is None else torch.tensor(entries, dtype=torch.int32, device="cuda")
    ct = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    t = _u16(table)
    rc = env._lib.bcp_goal_field_cost_bound(env._h, et.data_ptr() if et is not None else None, ct.data_ptr() if ct is not None else None,
                                            n_list, CR.CLEARANCE_D2, max_passes, t.ctypes.data if t is not None else None,
                                            field.data_ptr(), info.data_ptr(), None)
    assert rc == want_rc, env._lib.bcp_last_error()
    torch.cuda.synchronize()
    return field.cpu().numpy(), info.cpu().numpy()


def test_bound_form_is_the_raw_form(torch_cuda, pool):
    torch = torch_cuda
    env, data, valid, _origins, cells = pool
    table = CR.cost_table(2)
    raw, raw_info = _raw(torch, env, data, np.array(cells, dtype=np.int32).reshape(16, 1, 2), CR.CLEARANCE_D2, table,
                         (valid[:, 0].tolist(), valid[:, 1].tolist()))
    got, info = _bound(torch, env, table)
    assert got.tobytes() == raw.tobytes() and info.tobytes() == raw_info.tobytes()
    want = _pool_ref(pool, 2)
    assert torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(want)) and (info[:, 1] == 0).all()
    plain = np.stack([GR.mini_field(k, CR.CLEARANCE_D2) for k in range(16)])
    assert (got >= plain).all() and (got > plain).reshape(16, -1).any(axis=1).all()
    # a list with an id out of range: skipped, and only the listed entries are written
    got, info = _bound(torch, env, table, entries=[3, 99, 7, -1], n_list=4)
    for k in range(16):
        if k in (3, 7):
            assert (got[k] == raw[k]).all() and (info[k] == raw_info[k]).all()
        else:
            assert (got[k] == SENTINEL).all() and (info[k] == POISON_I).all()
    # a device count below n_list: the first two of the list
    got, info = _bound(torch, env, table, entries=[5, 9, 11, 2], count=2, n_list=4)
    written = [k for k in range(16) if (got[k] != SENTINEL).any()]
    assert written == [5, 9] and (got[5] == raw[5]).all() and (got[9] == raw[9]).all() and (info[11] == POISON_I).all()
    # the global route: the same bytes
    from bc_gym_planning_env_amd import _lib
    assert env._lib.bcp_set_tuning(env._h, _lib.TUNE_GOAL_ROUTE, 2) == 0
    try:
        got, info = _bound(torch, env, table, entries=[5, 9], n_list=2)
    finally:
        assert env._lib.bcp_set_tuning(env._h, _lib.TUNE_GOAL_ROUTE, 0) == 0
    assert (got[5] == raw[5]).all() and (got[9] == raw[9]).all() and (info[[5, 9]] == raw_info[[5, 9]]).all()
    # refusals of its own: the plain ones first (with its name), then the table; nothing is written
    L = env._lib
    got, info = _bound(torch, env, None, want_rc=E_INVALID)
    assert b"bcp_goal_field_cost_bound: null extra_of_cost" in L.bcp_last_error()
    assert (got == SENTINEL).all() and (info == POISON_I).all()
    bad = table.copy()
    bad[255] = 4096
    got, info = _bound(torch, env, bad, want_rc=E_INVALID)
    assert b"extra_of_cost[255]" in L.bcp_last_error() and (got == SENTINEL).all()
    got, info = _bound(torch, env, None, n_list=17, want_rc=E_INVALID)
    assert b"n_list" in L.bcp_last_error() and L.bcp_last_error().startswith(b"bcp_goal_field_cost_bound: ")
    assert L.bcp_goal_field_cost_bound(env._h, None, None, 0, 151, 0, table.ctypes.data, None, None, None) == E_INVALID     # null field
    f = torch.zeros(1, dtype=torch.int16, device="cuda")
    assert L.bcp_goal_field_cost_bound(env._h, None, None, 0, 151, 0, table.ctypes.data, f.data_ptr(), None, None) == 0    # n_list == 0


# ---- 6. capture ------------------------------------------------------------------------------------------------------------
def test_a_captured_call_keeps_its_table(torch_cuda, ops):
    torch = torch_cuda
    cost = CR.inflated_world(9)
    goal = GR.mini_world(9)[3]
    want = CR.world_field(9, 8)
    d = torch.from_numpy(np.array(cost)).cuda()
    s = torch.tensor([[goal]], dtype=torch.int32, device="cuda")
    poison = torch.from_numpy(np.full(3 * 183 * 183, SENTINEL, dtype=np.uint16)).cuda()
    out = poison.clone()
    info = torch.full((3, 2), POISON_I, dtype=torch.int32, device="cuda")
    table = _u16(CR.cost_table(8))

    def call():
        rc = ops._lib.bcp_goal_field_cost(ops._h, d.data_ptr(), 1, 183, 183, 0, None, None, s.data_ptr(), 1, CR.CLEARANCE_D2, 0,
                                          table.ctypes.data, out.data_ptr() + 2 * 183 * 183, info.data_ptr() + 8, ops._stream())
        assert rc == 0, ops._lib.bcp_last_error()

    def check(what):
        torch.cuda.synchronize()
        o, i = out.cpu().numpy().reshape(3, 183, 183), info.cpu().numpy()
        assert (o[0] == SENTINEL).all() and (o[2] == SENTINEL).all() and (i[0] == POISON_I).all() and (i[2] == POISON_I).all()
        assert (o[1] == want).all() and i[1].tolist() == [int((want != GR.NONE).sum()), 0], what

    call()                     # one ordinary call first: the LDS limit of the kernel is raised outside the capture
    check("eager")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            call()
    torch.cuda.synchronize()
    table[:] = 0               # the host table is the caller's again: the captured launch carries its own copy
    for replay in range(2):
        out.copy_(poison)
        info.fill_(POISON_I)
        graph.replay()
        check("replay %d" % replay)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(torch_cuda, ops):
    torch = torch_cuda
    L = ops._lib
    d = torch.zeros((2, 20, 30), dtype=torch.uint8, device="cuda")
    s = torch.zeros((2, 1, 2), dtype=torch.int32, device="cuda")
    v = torch.full((2,), 20, dtype=torch.int32, device="cuda")
    out = torch.from_numpy(np.full((2, 20, 30), SENTINEL, dtype=np.uint16)).cuda()
    info = torch.full((2, 2), POISON_I, dtype=torch.int32, device="cuda")
    good = _u16(RAMP)
    base = dict(h=ops._h, data=d.data_ptr(), n=2, rows=20, cols=30, shared=0, vr=None, vc=None, seeds=s.data_ptr(), n_seeds=1,
                cd2=4, passes=0, table=good.ctypes.data, out=out.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return L.bcp_goal_field_cost(a["h"], a["data"], a["n"], a["rows"], a["cols"], a["shared"], a["vr"], a["vc"], a["seeds"],
                                     a["n_seeds"], a["cd2"], a["passes"], a["table"], a["out"], info.data_ptr(), None)

    assert call(h=None) == E_INVALID
    assert call(n=-1) == E_INVALID and b"n_maps" in L.bcp_last_error()
    for name in ("data", "seeds", "out"):
        assert call(**{name: None}) == E_INVALID, name
    for name in ("rows", "cols"):
        for bad in (0, -3, 2049):
            assert call(**{name: bad}) == E_INVALID, (name, bad)
    for bad in (0, -1, 4097):
        assert call(n_seeds=bad) == E_INVALID, bad
    for bad in (-1, 16130):
        assert call(cd2=bad) == E_INVALID, bad
    assert b"clearance_d2" in L.bcp_last_error()
    assert call(passes=-1) == E_INVALID
    assert call(vr=v.data_ptr()) == E_INVALID and call(vc=v.data_ptr()) == E_INVALID
    assert call(vr=v.data_ptr(), vc=v.data_ptr(), shared=1) == E_INVALID and b"shared" in L.bcp_last_error()
    # the table: behind everything the plain call refuses
    assert call(table=None) == E_INVALID and b"null extra_of_cost" in L.bcp_last_error()
    assert call(table=None, passes=-1) == E_INVALID and b"max_passes" in L.bcp_last_error()
    assert call(table=None, out=None) == E_INVALID and b"null data / seeds / out" in L.bcp_last_error()
    for index in (0, 100, 254, 255):
        bad = good.copy()
        bad[index] = 4096
        assert call(table=bad.ctypes.data) == E_INVALID and (b"extra_of_cost[%d] = 4096" % index) in L.bcp_last_error(), index
    both = good.copy()
    both[7] = both[9] = 65535
    assert call(table=both.ctypes.data) == E_INVALID and b"extra_of_cost[7]" in L.bcp_last_error()        # the first one
    assert L.bcp_last_error().startswith(b"bcp_goal_field_cost: ")
    top = good.copy()
    top[:] = 4095
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (info.cpu().numpy() == POISON_I).all()            # nothing was written
    assert call(table=top.ctypes.data) == 0 and call() == 0 and call(vr=v.data_ptr(), vc=v.data_ptr()) == 0 and call(shared=1) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != SENTINEL).all()
    with pytest.raises(ValueError):
        ops.goal_field(np.zeros((4, 4), dtype=np.uint8), [(0, 0)], 0, extra_of_cost=np.full(256, 4096))


# ---- 8. the Python surface -------------------------------------------------------------------------------------------------
def test_env_goal_field_with_a_cost_weight(torch_cuda, pool):
    torch = torch_cuda
    from bc_gym_planning_env_amd import goal_field
    env = pool[0]
    fields = env.goal_field(cost_weight=2)
    want = _pool_ref(pool, 2)
    assert fields.clearance_d2 == 151 and fields.field.shape == (16, 183, 183)
    assert (fields.extra_of_cost == goal_field.cost_table(2)).all() and env.goal_field().extra_of_cost is None
    assert torch.equal(fields.field.cpu(), torch.from_numpy(want))
    info = fields.info.cpu().numpy()
    assert (info[:, 0] == (want != GR.NONE).reshape(16, -1).sum(1)).all() and (info[:, 1] == 0).all()
    explicit = env.goal_field(extra_of_cost=CR.cost_table(2))
    assert torch.equal(explicit.field, fields.field)
    assert torch.equal(env.goal_field(cost_weight=0).field, env.goal_field().field)
    metres = fields.metres().cpu().numpy()
    assert np.isinf(metres[want == GR.NONE]).all()
    assert (metres[want != GR.NONE] == (want[want != GR.NONE].astype(np.float32) * np.float32(env.resolution / 12))).all()
    with pytest.raises(ValueError):
        env.goal_field(cost_weight=2, extra_of_cost=CR.cost_table(2))
    with pytest.raises(ValueError):
        env.goal_field(cost_weight=2, follow_refresh=True)
    with pytest.raises(ValueError):
        env.goal_field(extra_of_cost=CR.cost_table(2), follow_refresh=True)
    with pytest.raises(ValueError):
        env.goal_field(cost_weight=400)
    with pytest.raises(ValueError):
        env.goal_field(extra_of_cost=np.zeros(255))
    with pytest.raises(ValueError):
        env.route_paths(fields, cost_weight=2)
    # never inflated: cost_weight has nothing to weigh; an explicit table is taken on any map
    raw_env, _cm = _golden_pool_env(4)
    with pytest.raises(RuntimeError, match="inflate_costmaps"):
        raw_env.goal_field(cost_weight=2)
    with pytest.raises(RuntimeError, match="inflate_costmaps"):
        raw_env.route_paths(cost_weight=2)
    table = _table(c0=3)
    got = raw_env.goal_field(extra_of_cost=table).field.cpu().numpy()
    for k in range(4):
        data, _o, _r, goal, _s = GR.mini_world(k)
        assert (got[k] == _ref(data, [goal], 151, table)).all(), k


def test_sampling_and_mppi_take_a_weighted_field(torch_cuda, pool):
    """bcp_goal_field_sample and bcp_mppi_field read a weighted field as they read a plain one"""
    torch = torch_cuda
    import mppi_check as MC
    import mppi_field_ref as FR
    import mppi_ref as MR
    env, _data, valid, origins, _cells = pool
    n = env.n_envs
    fields = env.goal_field(cost_weight=2)
    want = _pool_ref(pool, 2)
    entry = TG._entry_of(env, np.arange(n))
    rng = np.random.RandomState(7)
    poses = np.concatenate([GR.edge_poses(rng, 140, want[k], origins[k], env.resolution, pool[4][k]) for k in (5, 9)])
    row_env = np.concatenate([np.full(140, int(np.nonzero(entry == k)[0][0])) for k in (5, 9)]).astype(np.int32)
    got = TG._raw_sample(torch, env, fields.field, 8, 10.0, poses, row_env=row_env)
    _w3, want_v, _wc = TG._check_sample(got, want, valid, origins, env.resolution, entry[row_env], poses, 8, 10.0, "weighted field")
    assert (want_v != GR.NONE).sum() > 100
    # MPPI with the weighted field as its terminal cost: the kernel's own iterations, and the values against the reference field
    sigma, lam, penalty, weight, k, h = (0.2, 0.8), 0.4, 2.0, 1.0, 16, 8
    names = ("eps", "iter_mean", "iter_ret", "iter_reason", "err", "iter_value", "iter_score")
    res = env.mppi(MC.random_mean(env, np.random.RandomState(17), n, h), sigma, 2, k, lam, penalty, seed=11, draw_index=5, want=names,
                   goal_field=fields, terminal_weight=weight)
    MC.teacher_forced(torch, env, res, sigma, lam, penalty, fields=fields, weight=weight, tag="weighted field")
    low, high = MC.box(env)
    u = MR.candidates(res.iter_mean[0].cpu().numpy(), sigma, res.eps[0].cpu().numpy(), low, high)
    la = env.lookahead(torch.from_numpy(MR.as_lookahead_actions(u)).cuda(), want=("final_pose",))
    xy = la.final_pose.reshape(n * k, 3).cpu().numpy()[:, :2]
    value = FR.values(want, valid, origins, env.resolution, entry.repeat(k), xy)
    got_v = res.iter_value[0].cpu().numpy().reshape(-1)
    assert (got_v == value).all() and (value != GR.NONE).mean() > 0.5
    score = FR.scores(res.iter_ret[0].cpu().numpy(), res.iter_reason[0].cpu().numpy(), penalty, value.reshape(n, k), env.resolution, weight)
    assert (score == res.iter_score[0].cpu().numpy()).all()
    plain_v = FR.values(env.goal_field().field.cpu().numpy(), valid, origins, env.resolution, entry.repeat(k), xy)
    assert (got_v >= plain_v).all() and (got_v > plain_v).any()          # (costs to go, not lengths)


def test_route_paths_with_a_cost_weight(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv
    env, costmaps = _golden_pool_env()
    env.inflate_costmaps(CR.COST_SCALING)
    rp = env.params.reward_provider_params
    data, valid, origins = TG._maps_of(env)
    cells = TG._goal_cells(env, 16)
    pts, lens = env._keep["path"].cpu().numpy(), env._keep["lens"].cpu().numpy()
    starts, ends = pts[:, 0].copy(), pts[np.arange(16), lens - 1].copy()
    want_f = np.stack([_ref(data[k], [cells[k]], CR.CLEARANCE_D2, CR.cost_table(2), valid[k]) for k in range(16)])
    max_len = 160
    want = RR.route(want_f, valid, origins, env.resolution, np.arange(16), starts, ends, 2, max_len, reward_params=rp)
    assert (want[2] == 0).all() and all(RR.away_from_knife_edges(want[0][k, :want[1][k]], rp) for k in range(16))
    status = env.route_paths(stride=2, max_len=max_len, cost_weight=2)
    assert status.dtype == torch.int32 and (status.cpu().numpy() == want[2]).all()
    inv = 1.0 / env.resolution
    for i in range(16):
        k = int(env.geom_of_env[i])
        got = env.path_of(i)
        assert got.shape == (want[1][k], 3) and (got[:, :2] == want[0][k, :want[1][k], :2]).all()
        assert np.abs(got[:, 2] - want[0][k, :want[1][k], 2]).max() <= 1e-9
        if k in (5, 9):     # what the feature is for: the routed way points keep to the middle of free space
            rr = np.rint((got[:, 1] - origins[k, 1]) * inv).astype(int)
            cc = np.rint((got[:, 0] - origins[k, 0]) * inv).astype(int)
            clear = CR.min_clearance(GR.mini_world(k)[0], list(zip(rr.tolist(), cc.tolist())))
            print("world", k, "way points", len(got), "smallest distance to a lethal cell %.1f cells" % clear)
            assert clear > 30.0
    first = env._initial_state
    assert (first.target_idx.cpu().numpy() == want[3][:, 1]).all()
    assert np.abs(first.min_spat_dist_so_far.cpu().numpy() - want[3][:, 0]).max() <= 1e-9
    # 32 steps of random actions: bit for bit those of a fresh env built from the routed paths
    routed = [np.asarray(p).copy() for p in env._paths]
    fresh = BatchedPlanEnv(costmaps, routed, attr.evolve(env.params, refine_path=False), n_envs=16, geom_of_env=np.arange(16),
                           next_geom=np.roll(np.arange(16), -1), auto_reset=True, seed=2)
    fresh.reset()
    rng = np.random.RandomState(5)
    assert torch.equal(env.geom_of_env, fresh.geom_of_env)
    for t in range(32):
        act = env.action_space.sample_batch(16, rng) * np.array([3.0, 1.0], dtype=np.float32)
        _o, ra, da, _i = env.step(act)
        _o, rb, db, _i = fresh.step(act)
        assert torch.equal(ra, rb) and torch.equal(da, db), t
        for name in ("robot", "min_spat_dist_so_far", "target_idx", "current_iter", "robot_collided"):
            assert torch.equal(getattr(env.state, name), getattr(fresh.state, name)), (t, name)
        assert torch.equal(env.geom_of_env, fresh.geom_of_env)

"""bcp_goal_field / bcp_goal_field_sample / bcp_final_goal_field_sample on the GPU, bit for bit against the contract restated
in numpy / heapq (tests/goal_field_ref.py): the fields against Dijkstra, the per-row reads against the float64 sampling rule.
Only the direction (out3[:, 1:]) has a tolerance, 2^-22: the device's cos / sin may differ from numpy's in the last float64
bits, which moves a float32 result by at most one ulp, 2^-23 at 1; the bound is twice that.  Fields go into sentinel-filled
buffers with a map's worth of guard on either side.  Every case uses the smallest shape at which its mechanism can go wrong;
references are computed once per session and shared."""
import functools

import numpy as np
import pytest

import goal_field_ref as GR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
SENTINEL = 0xABCD
POISON_F, POISON_I = -7.5, -77
DIR_TOL = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def _ref_cached(data_bytes, shape, seeds, clearance_d2, valid):
    data = np.frombuffer(data_bytes, dtype=np.uint8).reshape(shape)
    field = GR.dijkstra(data, list(seeds), clearance_d2, valid)
    field.setflags(write=False)
    return field


def _ref(data, seeds, clearance_d2, valid=None):
    """Dijkstra's field, computed once per (map, seeds, clearance, valid shape) of the session"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    seeds = tuple((int(r), int(c)) for r, c in np.asarray(seeds).reshape(-1, 2))
    return _ref_cached(data.tobytes(), data.shape, seeds, int(clearance_d2), None if valid is None else (int(valid[0]), int(valid[1])))


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from bc_gym_planning_env_amd.ops import NativeOps
    return NativeOps()


def _raw_fields(torch, ops, data, seeds, clearance_d2, valid=None, shared=False, max_passes=0, want_rc=0):
    """bcp_goal_field through the C ABI: data [n, rows, cols] (or [rows, cols] with shared), seeds [n, S, 2], valid None or
    (rows [n], cols [n]).  -> (fields uint16 [n, rows, cols], info int32 [n, 2]); the guards around `out` are checked"""
    from bc_gym_planning_env_amd import _lib
    data = np.array(data, dtype=np.uint8)        # (a copy: the shared references are read-only)
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
    rc = ops._lib.bcp_goal_field(ops._h, d.data_ptr(), n, rows, cols, int(shared), vr.data_ptr() if vr is not None else None,
                                 vc.data_ptr() if vc is not None else None, s.data_ptr(), seeds.shape[1], int(clearance_d2),
                                 int(max_passes), out.data_ptr() + 2 * cells, info.data_ptr() + 8, None)
    assert rc == want_rc, ops._lib.bcp_last_error()
    torch.cuda.synchronize()
    o, i = out.cpu().numpy(), info.cpu().numpy()
    assert (o[:cells] == SENTINEL).all() and (o[(n + 1) * cells:] == SENTINEL).all(), "guard overwritten"
    assert (i[0] == POISON_I).all() and (i[n + 1] == POISON_I).all()
    assert _lib.GOAL_NONE == GR.NONE
    return o[cells:(n + 1) * cells].reshape(n, rows, cols), i[1:n + 1]


def _one(torch, ops, data, seeds, clearance_d2, valid=None, max_passes=0):
    v = None if valid is None else ([valid[0]], [valid[1]])
    f, i = _raw_fields(torch, ops, data[None], np.asarray(seeds, dtype=np.int32).reshape(1, -1, 2), clearance_d2, v, max_passes=max_passes)
    return f[0], i[0]


def _same(got, want, info, what):
    bad = int((got != want).sum())
    print(what, "cells", got.size, "with a value", int((want != GR.NONE).sum()), "different:", bad, "info", info.tolist())
    assert bad == 0, (what, bad)
    assert info[0] == (want != GR.NONE).sum() and info[1] == 0, (what, info)


# ---- 1. the reference worlds: 183 x 183, the LDS route ---------------------------------------------------------------------
@pytest.mark.parametrize("clearance_d2", [0, 151])
@pytest.mark.parametrize("world", [0, 5, 17])
def test_mini_worlds_equal_dijkstra(torch_cuda, ops, world, clearance_d2):
    torch = torch_cuda
    data, _origin, _res, goal, start = GR.mini_world(world)
    want = GR.mini_field(world, clearance_d2)
    got, info = _one(torch, ops, data, [goal], clearance_d2)
    assert torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(want.copy()))
    _same(got, want, info, "world %d clearance_d2 %d" % (world, clearance_d2))
    assert got[goal] == 0 and got[start] != GR.NONE
    # through NativeOps.goal_field: the same bytes
    field, info2 = ops.goal_field(data.copy(), [goal], clearance_d2, want_info=True)
    assert field.dtype == torch.uint16 and field.shape == data.shape and (field.cpu().numpy() == want).all()
    assert info2.cpu().numpy().tolist() == [info.tolist()]


# ---- 2. small and ragged shapes -------------------------------------------------------------------------------------------
def test_small_and_ragged_shapes(torch_cuda, ops):
    torch = torch_cuda
    got, info = _one(torch, ops, np.zeros((1, 1), dtype=np.uint8), [(0, 0)], 0)
    assert got.tolist() == [[0]] and info.tolist() == [1, 0]
    got, info = _one(torch, ops, np.full((1, 1), 254, dtype=np.uint8), [(0, 0)], 9)        # a seed on an obstacle is free
    assert got.tolist() == [[0]] and info.tolist() == [1, 0]
    for shape, seed in (((1, 70), (0, 3)), ((70, 1), (66, 0))):
        data = np.zeros(shape, dtype=np.uint8)
        data[-1, -1] = 254
        for cd2 in (0, 4):
            got, info = _one(torch, ops, data, [seed], cd2)
            _same(got, _ref(data, [seed], cd2), info, "%s clearance_d2 %d" % (shape, cd2))
    for cols in (31, 32, 33, 63, 64, 65):
        data = np.zeros((9, cols), dtype=np.uint8)
        data[1:8:2, 0] = 254
        data[0:9:3, cols - 1] = 254
        seeds = [(1, cols - 1)]
        for cd2 in (0, 2, 9):
            got, info = _one(torch, ops, data, seeds, cd2)
            _same(got, _ref(data, seeds, cd2), info, "cols %d clearance_d2 %d" % (cols, cd2))


@pytest.mark.parametrize("clearance_d2", [0, 1, 2, 9])
def test_random_maps_and_unusable_seeds(torch_cuda, ops, clearance_d2):
    """40 x 47 at 20 % obstacles; three seeds: on a blocked cell, outside the valid shape, and (-1, -1)"""
    torch = torch_cuda
    rng = np.random.RandomState(5)
    data = np.where(rng.uniform(size=(40, 47)) < 0.2, 254, 0).astype(np.uint8)
    data[:, 44:] = 254      # (padding full of 254s: not obstacles)
    valid = (37, 44)
    blocked = tuple(int(v) for v in np.argwhere(data[:37, :44] == 254)[3])
    seeds = [blocked, (38, 5), (-1, -1)]
    got, info = _one(torch, ops, data, seeds, clearance_d2, valid=valid)
    want = _ref(data, seeds, clearance_d2, valid)
    _same(got, want, info, "40 x 47 clearance_d2 %d" % clearance_d2)
    assert got[blocked] == 0 and (got[37:] == GR.NONE).all() and (got[:, 44:] == GR.NONE).all()
    got, info = _one(torch, ops, data, [(38, 5), (-1, -1), (3, 45)], clearance_d2, valid=valid)    # no usable seed
    assert (got == GR.NONE).all() and info.tolist() == [0, 0]


# ---- 3. padded batches ------------------------------------------------------------------------------------------------------
def test_padded_maps_and_untouched_neighbours(torch_cuda, ops):
    """five maps in one 40 x 70 allocation with valid shapes from (0, .) and (., 0) to full and 254s in the padding"""
    torch = torch_cuda
    rng = np.random.RandomState(8)
    valid = [(0, 50), (30, 0), (17, 33), (40, 70), (39, 65)]
    data = np.full((5, 40, 70), 254, dtype=np.uint8)
    seeds = np.zeros((5, 2, 2), dtype=np.int32)
    for k, (vr, vc) in enumerate(valid):
        data[k, :vr, :vc] = np.where(rng.uniform(size=(vr, vc)) < 0.1, 254, 0)
        seeds[k] = [(vr // 2, vc // 2), (vr - 1, vc - 1)]
    for cd2 in (0, 5):
        got, info = _raw_fields(torch, ops, data, seeds, cd2, ([v[0] for v in valid], [v[1] for v in valid]))
        for k, (vr, vc) in enumerate(valid):
            _same(got[k], _ref(data[k], seeds[k], cd2, valid[k]), info[k], "padded map %d clearance_d2 %d" % (k, cd2))
            assert (got[k, vr:] == GR.NONE).all() and (got[k, :, vc:] == GR.NONE).all()
        assert (got[0] == GR.NONE).all() and (got[1] == GR.NONE).all()
    # valid shapes beyond the allocation are clamped, negative ones too
    got, info = _raw_fields(torch, ops, data[3:4], seeds[3:4], 0, ([4000], [-5]))
    assert (got == GR.NONE).all()
    got, info = _raw_fields(torch, ops, data[3:4], seeds[3:4], 0, ([4000], [4000]))
    _same(got[0], _ref(data[3], seeds[3], 0), info[0], "clamped valid shape")


# ---- 4. the corner rule ------------------------------------------------------------------------------------------------------
def test_nothing_leaks_through_a_diagonal_wall(torch_cuda, ops):
    torch = torch_cuda
    data = GR.diagonal_wall(9)
    got, info = _one(torch, ops, data, [(0, 0)], 0)
    _same(got, _ref(data, [(0, 0)], 0), info, "9 x 9 diagonal wall")
    rr, cc = np.indices(data.shape)
    assert (got[rr + cc >= 8] == GR.NONE).all() and (got[rr + cc < 8] != GR.NONE).all() and info[0] == 36


# ---- 5. long corridors: many passes, the saturation, the cap ----------------------------------------------------------------
def test_serpentines_saturation_and_the_cap(torch_cuda, ops):
    torch = torch_cuda
    data = GR.serpentine(33)
    got, info = _one(torch, ops, data, [(0, 0)], 0)
    _same(got, _ref(data, [(0, 0)], 0), info, "serpentine 33")
    assert info[0] == 577
    data = GR.serpentine(129)
    want = _ref(data, [(0, 0)], 0)
    assert (want == GR.FAR).sum() == 2987 and want[want < GR.FAR].max() == 65532 and (want != GR.NONE).sum() == 8449
    got, info = _one(torch, ops, data, [(0, 0)], 0)            # 8 449 passes under pure Jacobi; the default cap is 16 641
    _same(got, want, info, "serpentine 129")
    capped, info = _one(torch, ops, data, [(0, 0)], 0, max_passes=100)
    print("serpentine 129, max_passes 100: info", info.tolist(), "cells with a value", int((capped != GR.NONE).sum()))
    assert info[1] == 1 and info[0] == (capped != GR.NONE).sum()
    assert (capped >= want).all() and (capped[want == GR.NONE] == GR.NONE).all()
    assert (capped != want).any()      # (100 passes of 17 rows each cannot walk 8 448 cells)


# ---- 6. the two routes -------------------------------------------------------------------------------------------------------
def test_global_route_gives_the_same_bytes(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import _lib
    from bc_gym_planning_env_amd.ops import NativeOps
    forced = NativeOps()
    L = forced._lib
    assert L.bcp_set_tuning(forced._h, _lib.TUNE_GOAL_ROUTE, 1) == E_INVALID and b"GOAL_ROUTE" in L.bcp_last_error()
    assert L.bcp_set_tuning(forced._h, _lib.TUNE_GOAL_ROUTE, 2) == 0
    rng = np.random.RandomState(13)
    data = np.where(rng.uniform(size=(3, 70, 65)) < 0.12, 254, 0).astype(np.uint8)
    seeds = np.array([[(2, 3), (60, 60)], [(35, 32), (-1, -1)], [(69, 64), (0, 0)]], dtype=np.int32)
    valid = ([70, 55, 70], [65, 65, 40])
    for cd2 in (0, 3):
        got, info = _raw_fields(torch, forced, data, seeds, cd2, valid)
        for k in range(3):
            _same(got[k], _ref(data[k], seeds[k], cd2, (valid[0][k], valid[1][k])), info[k], "global route 70 x 65 map %d" % k)
    world, origin, res, goal, _start = GR.mini_world(17)
    got, info = _one(torch, forced, world, [goal], 151)
    _same(got, GR.mini_field(17, 151), info, "global route 183 x 183")
    assert L.bcp_set_tuning(forced._h, _lib.TUNE_GOAL_ROUTE, 0) == 0


def test_map_beyond_lds(torch_cuda, ops):
    """300 x 300: 176 KB of plane, the global route by size"""
    torch = torch_cuda
    rng = np.random.RandomState(4)
    data = np.where(rng.uniform(size=(300, 300)) < 0.01, 254, 0).astype(np.uint8)
    data[150, 20:280] = 254
    seeds = [(10, 290), (299, 0)]
    got, info = _one(torch, ops, data, seeds, 8)
    _same(got, _ref(data, seeds, 8), info, "300 x 300")


# ---- 7. batches and sharing --------------------------------------------------------------------------------------------------
def test_batches_and_shared_maps(torch_cuda, ops):
    torch = torch_cuda
    rng = np.random.RandomState(21)
    data = np.where(rng.uniform(size=(16, 50, 45)) < 0.15, 254, 0).astype(np.uint8)
    seeds = rng.randint(0, 45, size=(16, 3, 2)).astype(np.int32)
    batch, info = _raw_fields(torch, ops, data, seeds, 2)
    for k in range(16):
        single, info1 = _one(torch, ops, data[k], seeds[k], 2)
        assert (batch[k] == single).all() and (info[k] == info1).all(), k
        if k < 3:
            _same(single, _ref(data[k], seeds[k], 2), info1, "batch entry %d" % k)
    assert len({batch[k].tobytes() for k in range(16)}) == 16
    shared, info = _raw_fields(torch, ops, data[0], seeds[:4], 2, shared=True)
    for k in range(4):
        single, info1 = _one(torch, ops, data[0], seeds[k], 2)
        assert (shared[k] == single).all() and (info[k] == info1).all(), k
    field = ops.goal_field(data[0], seeds[:4], 2)
    assert field.shape == (4, 50, 45) and (field.cpu().numpy() == shared).all()
    assert ops.goal_field(data, seeds, 2).shape == (16, 50, 45)
    # n_maps == 0 succeeds and does nothing, whatever the pointers
    assert ops._lib.bcp_goal_field(ops._h, None, 0, 50, 45, 0, None, None, None, 1, 0, 0, None, None, None) == 0


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_field_refusals(torch_cuda, ops):
    torch = torch_cuda
    L = ops._lib
    d = torch.zeros((2, 20, 30), dtype=torch.uint8, device="cuda")
    s = torch.zeros((2, 1, 2), dtype=torch.int32, device="cuda")
    v = torch.full((2,), 20, dtype=torch.int32, device="cuda")
    out = torch.zeros((2, 20, 30), dtype=torch.int16, device="cuda")
    base = dict(h=ops._h, data=d.data_ptr(), n=2, rows=20, cols=30, shared=0, vr=None, vc=None, seeds=s.data_ptr(), n_seeds=1,
                cd2=4, passes=0, out=out.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return L.bcp_goal_field(a["h"], a["data"], a["n"], a["rows"], a["cols"], a["shared"], a["vr"], a["vc"], a["seeds"],
                                a["n_seeds"], a["cd2"], a["passes"], a["out"], None, None)

    assert call() == 0 and call(vr=v.data_ptr(), vc=v.data_ptr()) == 0 and call(shared=1) == 0 and call(cd2=16129, passes=3) == 0
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
    assert L.bcp_last_error().startswith(b"bcp_goal_field: ")
    assert call(n=0, data=None, seeds=None, out=None) == 0
    torch.cuda.synchronize()


# ---- 9. sampling -------------------------------------------------------------------------------------------------------------
class _SampleOut(object):
    def __init__(self, torch, n):
        self.n = n
        self.out3 = torch.full((3 * n + 64,), POISON_F, dtype=torch.float32, device="cuda")
        self.value = torch.full((n + 64,), POISON_I, dtype=torch.int32, device="cuda")
        self.carrot = torch.full((2 * n + 64,), POISON_I, dtype=torch.int32, device="cuda")

    def read(self):
        n = self.n
        o, v, c = self.out3.cpu().numpy(), self.value.cpu().numpy(), self.carrot.cpu().numpy()
        assert (o[3 * n:] == POISON_F).all() and (v[n:] == POISON_I).all() and (c[2 * n:] == POISON_I).all(), "guard overwritten"
        return o[:3 * n].reshape(n, 3), v[:n], c[:2 * n].reshape(n, 2)


def _raw_sample(torch, owner, field_t, carrot_cells, max_dist, poses=None, row_env=None, n=None, final=False):
    from bc_gym_planning_env_amd import _lib
    pt = None if poses is None else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).cuda()
    rt = None if row_env is None else torch.from_numpy(np.ascontiguousarray(row_env, dtype=np.int32)).cuda()
    n = (owner.n_envs if pt is None else len(poses)) if n is None else n
    out = _SampleOut(torch, n)
    f = field_t
    if final:
        _lib.check(owner._lib.bcp_final_goal_field_sample(owner._h, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2], carrot_cells,
                                                          float(max_dist), out.out3.data_ptr(), out.value.data_ptr(),
                                                          out.carrot.data_ptr(), None))
    else:
        _lib.check(owner._lib.bcp_goal_field_sample(owner._h, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2],
                                                    pt.data_ptr() if pt is not None else None, n,
                                                    rt.data_ptr() if rt is not None else None, carrot_cells, float(max_dist),
                                                    out.out3.data_ptr(), out.value.data_ptr(), out.carrot.data_ptr(), None))
    torch.cuda.synchronize()
    return out.read()


def _check_sample(got, fields, valids, origins, resolution, entry, poses, carrot_cells, max_dist, what):
    out3, value, carrot = got
    with np.errstate(all="ignore"):
        cs = np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1)
    want3, want_v, want_c = GR.sample(fields, valids, origins, resolution, entry, poses, cs, carrot_cells, max_dist)
    has = want_v != GR.NONE
    err = float(np.abs(out3[:, 1:].astype(np.float64) - want3[:, 1:].astype(np.float64)).max())
    bad = int((value != want_v).sum()), int((carrot != want_c).sum()), int((out3[:, 0].view(np.uint32) != want3[:, 0].view(np.uint32)).sum())
    print(what, "rows", len(poses), "with a result", int(has.sum()), "different value / carrot / distance:", bad,
          "max |direction - numpy| = %.3g (bound %.3g)" % (err, DIR_TOL))
    assert bad == (0, 0, 0), (what, bad)
    assert err <= DIR_TOL, (what, err)
    return want3, want_v, want_c


@pytest.mark.parametrize("clearance_d2", [0, 151])
@pytest.mark.parametrize("world", [0, 5, 17])
def test_sampling_on_the_reference_worlds(torch_cuda, world, clearance_d2):
    torch = torch_cuda
    from bc_gym_planning_env_amd.ops import NativeOps
    data, origin, res, goal, _start = GR.mini_world(world)
    field = GR.mini_field(world, clearance_d2)
    owner = NativeOps()
    owner.set_costmap(data.copy(), origin, res)
    field_t = torch.from_numpy(field.copy()).cuda()[None]
    poses = GR.edge_poses(np.random.RandomState(100 + world), 4096, field, origin, res, goal)
    for carrot_cells, max_dist in ((1, np.inf), (8, 10.0), (256, 1.5), (256, np.inf)):
        got = _raw_sample(torch, owner, field_t, carrot_cells, max_dist, poses)
        _w3, want_v, want_c = _check_sample(got, field[None], [field.shape], [origin], res, np.zeros(len(poses), dtype=np.int64), poses,
                                            carrot_cells, max_dist, "world %d clearance_d2 %d carrot %d" % (world, clearance_d2, carrot_cells))
        has = want_v != GR.NONE
        assert has.sum() > 2000 and (~has).sum() > 200
        assert (got[0][~has] == np.float32([max_dist, 0, 0])).all() and (want_c[~has] == -1).all()
        assert want_v[0] == 0 and (got[0][0] == 0).all() and (want_c[0] == goal).all()
        assert (want_v[132:137] == GR.NONE).all()
        if clearance_d2:
            assert (want_v[2:42] == GR.NONE).all()
    # GoalField on the same owner: the same bytes, cached buffers
    from bc_gym_planning_env_amd.goal_field import GoalField
    gf = GoalField(owner, field_t, clearance_d2, resolution=res)
    out3, value, carrot = gf.sample(poses, carrot_cells=8, max_dist=10.0, want=("cell_value", "carrot"))
    again = _raw_sample(torch, owner, field_t, 8, 10.0, poses)
    assert (out3.cpu().numpy().view(np.uint32) == again[0].view(np.uint32)).all() and (value.cpu().numpy() == again[1]).all()
    assert (carrot.cpu().numpy() == again[2]).all() and gf.sample(poses, carrot_cells=8, max_dist=10.0).data_ptr() == out3.data_ptr()
    metres = gf.metres().cpu().numpy()[0]
    assert metres.dtype == np.float32 and np.isinf(metres[field == GR.NONE]).all()
    assert (metres[field != GR.NONE] == (field[field != GR.NONE].astype(np.float32) * np.float32(res / 12))).all()
    with pytest.raises(ValueError):
        gf.sample(poses, want=("nothing",))


def test_sample_refusals(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd.ops import NativeOps
    data, origin, res, goal, _start = GR.mini_world(0)
    owner = NativeOps()
    L = owner._lib
    f = torch.from_numpy(GR.mini_field(0, 0).copy()).cuda()[None]
    poses = torch.zeros((6, 3), dtype=torch.float64, device="cuda")
    env_of = torch.zeros(6, dtype=torch.int32, device="cuda")
    out = _SampleOut(torch, 6)
    o3, pp = out.out3.data_ptr(), poses.data_ptr()

    def call(h=owner._h, field=f.data_ptr(), nf=1, rows=183, cols=183, p=pp, n=6, row_env=None, carrot=8, dist=5.0, out3=o3):
        return L.bcp_goal_field_sample(h, field, nf, rows, cols, p, n, row_env, carrot, dist, out3, None, None, None)

    assert call() == E_STATE and b"costmaps" in L.bcp_last_error()
    assert call(carrot=0) == E_INVALID                                     # (arguments before state)
    owner.set_costmap(data.copy(), origin, res)
    assert call() == 0 and call(dist=float("inf")) == 0 and call(row_env=env_of.data_ptr()) == 0 and call(carrot=256) == 0
    assert call(h=None) == E_INVALID and call(field=None) == E_INVALID and call(out3=None) == E_INVALID
    for bad in (0, -1, 257):
        assert call(carrot=bad) == E_INVALID, bad
    assert b"carrot_cells" in L.bcp_last_error()
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        assert call(dist=bad) == E_INVALID, bad
    assert call(n=0) == E_INVALID and call(n=-1) == E_INVALID
    assert call(p=None, n=1) == E_STATE and b"state" in L.bcp_last_error()
    assert call(p=None, n=2) == E_INVALID
    assert call(p=None, n=1, row_env=env_of.data_ptr()) == E_INVALID
    assert call(rows=182) == E_INVALID and call(cols=184) == E_INVALID and b"shape" in L.bcp_last_error()
    assert call(nf=0) == E_INVALID and call(nf=2) == E_INVALID and b"n_fields" in L.bcp_last_error()
    assert L.bcp_last_error().startswith(b"bcp_goal_field_sample: ")
    final = lambda **kw: L.bcp_final_goal_field_sample(owner._h, f.data_ptr(), 1, 183, 183, kw.get("carrot", 8), 5.0, o3, None, None, None)
    assert final() == E_STATE and b"record" in L.bcp_last_error()
    assert L.bcp_final_goal_field_sample(None, f.data_ptr(), 1, 183, 183, 8, 5.0, o3, None, None, None) == E_INVALID
    # a row whose row_env is out of range has no result
    env_of[2], env_of[4] = 1, -1
    got = _raw_sample(torch, owner, f, 8, 5.0, np.tile([origin[0] + goal[1] * res, origin[1] + goal[0] * res, 0.3], (6, 1)),
                      row_env=env_of.cpu().numpy())
    assert got[1].tolist() == [0, 0, GR.NONE, 0, GR.NONE, 0] and (got[0][2] == np.float32([5.0, 0, 0])).all()
    torch.cuda.synchronize()
    out.read()


# ---- 10. rows: pools, delays, look-ahead poses, the record, capture -----------------------------------------------------------
def _mini(n, timeout, seeds=(1, 2, 3, 4), episodes=4, **kw):
    from bc_gym_planning_env_amd import EnvParams, mini_env
    delays = {k: kw.pop(k) for k in list(kw) if k.endswith("_delay")}
    params = mini_env.RandomMiniEnvParams(
        env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, iteration_timeout=timeout, **delays))
    if kw.get("endless"):
        return mini_env.BatchedRandomMiniEnv(n, params, episodes=episodes, auto_reset=True, seed=4, **kw)
    pool = mini_env.sample_pool(params, list(seeds), episodes)
    return mini_env.BatchedRandomMiniEnv(n, params, pool=pool, auto_reset=True, seed=2, **kw)


def _maps_of(env):
    """what the env has bound: data [E, rows, cols], valid shapes [E, 2], origins [E, 2]"""
    data = env.costmap_tensor.cpu().numpy()
    if data.ndim == 2:
        return data[None], np.array([data.shape]), np.asarray(env._origin_host, dtype=np.float64)[None]
    k = env._keep
    vr = k["vr"].cpu().numpy() if k.get("vr") is not None else np.full(len(data), data.shape[1])
    vc = k["vc"].cpu().numpy() if k.get("vc") is not None else np.full(len(data), data.shape[2])
    return data, np.stack([vr, vc], axis=1), k["origins"].cpu().numpy()


def _goal_cells(env, n_fields):
    """(row, col) of the last way point of every entry's path, on the entry's origin: numpy's own arithmetic"""
    pts = env._keep["path"].cpu().numpy()
    lens = env._keep["lens"]
    if lens is None:
        pts, lens = pts[None], np.array([len(pts)])
    else:
        lens = lens.cpu().numpy()
    _data, _valid, origins = _maps_of(env)
    cells = []
    for f in range(n_fields):
        p = pts[f % len(pts)][lens[f % len(lens)] - 1]
        o = origins[f % len(origins)]
        cells.append((int(np.rint((p[1] - o[1]) * (1.0 / env.resolution))), int(np.rint((p[0] - o[0]) * (1.0 / env.resolution)))))
    return cells


def _ref_fields(env, clearance_d2, seeds_of=None):
    data, valid, _origins = _maps_of(env)
    n = len(data)
    cells = _goal_cells(env, n)
    return np.stack([_ref(data[f], [cells[f]] if seeds_of is None else seeds_of(f), clearance_d2, valid[f]) for f in range(n)])


def _current_poses(env):
    return np.ascontiguousarray(env.state.robot[0:3].cpu().numpy().T)


def _entry_of(env, rows_env):
    return env.geom_of_env.cpu().numpy()[rows_env].astype(np.int64) if env.geom_of_env is not None else np.asarray(rows_env, dtype=np.int64)


def test_pool_after_auto_resets_and_lookahead_poses(torch_cuda):
    """16 pool entries, 64 envs after auto-resets: poses = NULL is the state's pose on the env's entry; then the [N * K, 3]
    final poses of a look-ahead with row_env"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import constant_command_library
    n = 64
    env = _mini(n, timeout=12)
    fields = env.goal_field()
    assert fields.clearance_d2 == 151 and fields.field.shape == (16, 183, 183)
    want = _ref_fields(env, 151)
    assert (fields.field.cpu().numpy() == want).all()
    info = fields.info.cpu().numpy()
    assert (info[:, 0] == (want != GR.NONE).reshape(16, -1).sum(1)).all() and (info[:, 1] == 0).all()
    rng = np.random.RandomState(1)
    for _ in range(60):
        env.step(env.action_space.sample_batch(n, rng))
    geom = env.geom_of_env.cpu().numpy()
    assert len(np.unique(geom)) > 1
    data, valid, origins = _maps_of(env)
    poses = _current_poses(env)
    got = _raw_sample(torch, env, fields.field, 8, 10.0)
    _w3, want_v, _wc = _check_sample(got, want, valid, origins, env.resolution, _entry_of(env, np.arange(n)), poses, 8, 10.0, "pool, bound state")
    assert (want_v != GR.NONE).sum() > n // 2
    explicit = _raw_sample(torch, env, fields.field, 8, 10.0, poses)
    assert all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(explicit, got))
    library = constant_command_library(env.action_space, 3, 5, 12)
    la = env.lookahead(library, want=("final_pose",))
    k = library.shape[1]
    finals = la.final_pose.reshape(n * k, 3).cpu().numpy()
    row_env = np.arange(n).repeat(k)
    got = _raw_sample(torch, env, fields.field, 4, np.inf, finals, row_env=row_env)
    _check_sample(got, want, valid, origins, env.resolution, _entry_of(env, row_env), finals, 4, np.inf, "look-ahead finals with row_env")
    # without row_env the rows would go to env i % n: other entries, other answers
    other = _raw_sample(torch, env, fields.field, 4, np.inf, finals)
    assert (other[1] != got[1]).any()
    # one field for all rows
    one = fields.field[3:4].contiguous()
    got = _raw_sample(torch, env, one, 4, np.inf, finals, row_env=row_env)
    _check_sample(got, want[3:4], valid, origins, env.resolution, _entry_of(env, row_env), finals, 4, np.inf, "n_fields = 1")


def test_pose_delay_reads_the_seen_pose(torch_cuda):
    torch = torch_cuda
    n = 32
    env = _mini(n, timeout=40, pose_delay=1)
    fields = env.goal_field(clearance=0.2)
    assert fields.clearance_d2 == 44
    want = _ref_fields(env, 44)
    assert (fields.field.cpu().numpy() == want).all()
    rng = np.random.RandomState(6)
    for _ in range(9):
        env.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
    seen = np.ascontiguousarray(env.state.pose_seen.cpu().numpy().T)
    now = _current_poses(env)
    assert np.abs(seen - now).max() > 1e-3
    data, valid, origins = _maps_of(env)
    got = _raw_sample(torch, env, fields.field, 8, 10.0)
    _check_sample(got, want, valid, origins, env.resolution, _entry_of(env, np.arange(n)), seen, 8, 10.0, "pose_delay: the seen pose")
    at_now = _raw_sample(torch, env, fields.field, 8, 10.0, now)
    assert (at_now[0] != got[0]).any()


def test_final_samples_of_the_record(torch_cuda):
    torch = torch_cuda
    n = 64
    env = _mini(n, timeout=12, seeds=(1, 2, 3), episodes=3)
    ends = env.enable_episode_record()
    fields = env.goal_field()
    want = _ref_fields(env, 151)
    data, valid, origins = _maps_of(env)
    rng = np.random.RandomState(0)
    checked = 0
    for t in range(30):
        _o, _r, d, _info = env.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
        out3, value, carrot = _raw_sample(torch, env, fields.field, 8, 10.0, n=ends.capacity, final=True)
        m = int(ends.count[0])
        assert m == int(d.sum()) <= ends.capacity
        assert (out3[m:] == POISON_F).all() and (value[m:] == POISON_I).all() and (carrot[m:] == POISON_I).all()
        if m:
            poses = np.ascontiguousarray(ends.final_state.robot[0:3, :m].cpu().numpy().T)
            entry = ends.geom[:m].cpu().numpy().astype(np.int64)
            _check_sample((out3[:m], value[:m], carrot[:m]), want, valid, origins, env.resolution, entry, poses, 8, 10.0, "final, step %d" % t)
            checked += m
    assert checked > 20


def test_captured_sample_replays_and_follows_the_robot(torch_cuda):
    torch = torch_cuda
    n = 64
    env = _mini(n, timeout=200)
    fields = env.goal_field()
    want = _ref_fields(env, 151)
    names = ("out3", "cell_value", "carrot")

    def call():
        return dict(zip(names, fields.sample(carrot_cells=8, max_dist=10.0, want=names[1:])))

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
    for f in names:
        out[f].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in names:
        assert torch.equal(out[f], eager[f]), f
    env.state.robot[0:2] += 0.07
    env.state.robot[2] += 0.1
    graph.replay()
    torch.cuda.synchronize()
    replayed = {f: out[f].clone() for f in names}
    now = call()
    for f in names:
        assert torch.equal(now[f], replayed[f]), f
    assert not torch.equal(replayed["out3"], eager["out3"])
    data, valid, origins = _maps_of(env)
    got = tuple(replayed[f].cpu().numpy() for f in names)
    _check_sample(got, want, valid, origins, env.resolution, _entry_of(env, np.arange(n)), _current_poses(env), 8, 10.0, "replayed")


# ---- 11. the Python surface ----------------------------------------------------------------------------------------------------
def _shared_world():
    rng = np.random.RandomState(31)
    data = np.where(rng.uniform(size=(90, 70)) < 0.05, 254, 0).astype(np.uint8)
    data[40, 10:60] = 254
    data[30:50, 30:40][:, :3] = 0       # (a door in the wall)
    origin, res = np.array([-1.0, -0.5]), 0.05
    return data, origin, res


def test_env_goal_field_on_a_shared_map(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    from bc_gym_planning_env_amd import robots
    data, origin, res = _shared_world()
    path = np.array([[-0.5, 0.0, 0.0], [0.5, 1.0, 0.5], [1.5, 3.2, 1.0]])
    env = BatchedPlanEnv(CostMap2D(data, res, origin), path, EnvParams(resolution=res, refine_path=False), n_envs=5)
    fields = env.goal_field()
    radius = robots.inscribed_radius(env.footprint())
    d2 = int(np.floor((radius / res) ** 2))
    goal = (int(np.rint((3.2 + 0.5) / res)), int(np.rint((1.5 + 1.0) / res)))
    assert fields.clearance_d2 == d2 and fields.field.shape == (1, 90, 70) and _goal_cells(env, 1) == [goal]
    assert (fields.field.cpu().numpy()[0] == _ref(data, [goal], d2)).all()
    # clearance in metres; seeds = "path": every way point is a source
    fields = env.goal_field(clearance=0.1, seeds="path")
    cells = [(int(np.rint((p[1] + 0.5) / res)), int(np.rint((p[0] + 1.0) / res))) for p in path]
    want = _ref(data, cells, 4)
    got = fields.field.cpu().numpy()[0]
    assert fields.clearance_d2 == 4 and (got == want).all() and all(got[c] == 0 for c in cells)
    out3, value = fields.sample(want=("cell_value",))
    assert out3.shape == (5, 3) and (value.cpu().numpy() == 0).all()        # every env starts on way point 0
    with pytest.raises(ValueError):
        env.goal_field(seeds="start")
    # inflating the maps changes no field
    env.inflate_costmaps(3.0)
    assert (env.goal_field(clearance=0.1, seeds="path").field.cpu().numpy()[0] == want).all()


def test_env_goal_field_shared_map_private_paths(torch_cuda):
    """one field per env through shared = 1; a row reads the field of its env on the one map's origin"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    data, origin, res = _shared_world()
    paths = [np.array([[-0.5, 0.0, 0.0], [1.5, 3.2, 1.0]]), np.array([[0.0, 0.2, 0.0], [0.5, 0.5, 0.0], [2.0, 0.1, 0.0]]),
             np.array([[1.0, 3.0, 0.0], [-0.7, -0.2, 0.0]])]
    env = BatchedPlanEnv(CostMap2D(data, res, origin), paths, EnvParams(resolution=res, refine_path=False), n_envs=3)
    fields = env.goal_field(clearance=0.1)
    assert fields.field.shape == (3, 90, 70)
    goals = [(int(np.rint((p[-1][1] + 0.5) / res)), int(np.rint((p[-1][0] + 1.0) / res))) for p in paths]
    want = np.stack([_ref(data, [g], 4) for g in goals])
    assert (fields.field.cpu().numpy() == want).all()
    poses = _current_poses(env)
    got = _raw_sample(torch, env, fields.field, 8, np.inf)
    fields3 = want
    _check_sample(got, fields3, [data.shape] * 3, [origin] * 3, res, np.arange(3), poses, 8, np.inf, "shared map, private paths")
    assert (got[1] != GR.NONE).any()
    # the same rows on field 0 alone: other answers
    alone = _raw_sample(torch, env, fields.field[0:1].contiguous(), 8, np.inf)
    assert (alone[1] != got[1]).any()


def test_env_goal_field_on_an_aisle_pool(torch_cuda):
    """8 entries with valid shapes and origins of their own"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, aisle_env
    ranges = aisle_env.TurnRanges(main_corridor_length=(3., 4.), turn_corridor_length=(2., 3.), main_corridor_width=(1.2, 1.8),
                                  turn_corridor_width=(1.2, 1.8), margin=0.5)
    env = aisle_env.BatchedRandomAisleTurnEnv(16, EnvParams(iteration_timeout=40, resolution=0.05), n_chains=2, episodes=4, sampler="device_resident",
                                              auto_reset=True, ranges=ranges)
    fields = env.goal_field(clearance=0.2)
    data, valid, origins = _maps_of(env)
    assert len(data) == 8 and len({tuple(v) for v in valid.tolist()}) > 1 and fields.field.shape == data.shape
    want = _ref_fields(env, fields.clearance_d2)
    got = fields.field.cpu().numpy()
    for f in range(8):
        assert (got[f] == want[f]).all(), f
        assert (got[f, valid[f, 0]:] == GR.NONE).all() and (got[f, :, valid[f, 1]:] == GR.NONE).all()
    assert (want != GR.NONE).reshape(8, -1).sum(1).min() > 100
    rng = np.random.RandomState(2)
    for _ in range(50):
        env.step(env.action_space.sample_batch(16, rng))
    sampled = _raw_sample(torch, env, fields.field, 8, 20.0)
    _check_sample(sampled, want, valid, origins, env.resolution, _entry_of(env, np.arange(16)), _current_poses(env), 8, 20.0, "aisle pool")


def test_endless_pools_are_refused(torch_cuda):
    env = _mini(16, timeout=6, endless=True)
    with pytest.raises(RuntimeError):
        env.goal_field()


def test_wrapper_shapes_keys_and_final_observation(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedGoalField, _lib
    n = 64
    env = _mini(n, timeout=12, seeds=(1, 2, 3), episodes=3)
    wrap = BatchedGoalField(env, carrot_cells=6, max_dist=4.0, final_observation=True)
    assert wrap.unwrapped() is env and wrap.fields.clearance_d2 == 151
    want = _ref_fields(env, 151)
    data, valid, origins = _maps_of(env)
    obs = wrap.reset()
    assert list(obs.keys()) == ["goal_field", "goal_n_state"]
    assert obs["goal_field"].shape == (n, 3, 1) and obs["goal_field"].dtype == torch.float32
    assert obs["goal_n_state"].shape == (n, 9, 1)
    ends = env.episode_ends
    rng = np.random.RandomState(0)
    checked = 0
    for t in range(25):
        wrap.final_goal_field.fill_(POISON_F)
        obs, _r, d, info = wrap.step(env.action_space.sample_batch(n, rng) * np.array([3.0, 1.0], dtype=np.float32))
        fin = info["final_observation"]
        assert list(fin.keys()) == ["goal_field", "goal_n_state"] and fin["goal_field"].shape == (ends.capacity, 3, 1)
        m = int(ends.count[0])
        assert m == int(d.sum())
        final = fin["goal_field"].cpu().numpy()[..., 0]
        assert (final[m:] == POISON_F).all()
        now = _raw_sample(torch, env, wrap.fields.field, 6, 4.0)
        assert (obs["goal_field"].cpu().numpy()[..., 0].view(np.uint32) == now[0].view(np.uint32)).all(), t
        if t % 6 == 0:
            _check_sample(now, want, valid, origins, env.resolution, _entry_of(env, np.arange(n)), _current_poses(env), 6, 4.0, "wrapper, step %d" % t)
        if m:
            poses = np.ascontiguousarray(ends.final_state.robot[0:3, :m].cpu().numpy().T)
            entry = ends.geom[:m].cpu().numpy().astype(np.int64)
            with np.errstate(all="ignore"):
                cs = np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1)
            want3, _v, _c = GR.sample(want, valid, origins, env.resolution, entry, poses, cs, 6, 4.0)
            assert (final[:m, 0].view(np.uint32) == want3[:, 0].view(np.uint32)).all(), t
            assert np.abs(final[:m, 1:].astype(np.float64) - want3[:, 1:]).max() <= DIR_TOL
            checked += m
    assert checked > 20
    vec = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
    world = np.array([4.0, 4.0])
    _lib.check(env._lib.bcp_goal_n_state(env._h, world.ctypes.data_as(_lib._f64p), vec.data_ptr(), None))
    assert torch.equal(wrap.observation()["goal_n_state"][..., 0], vec)


def test_shooting_planner_with_a_terminal_cost(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import ShootingPlanner, _lib, constant_command_library
    n = 48
    env = _mini(n, timeout=200)
    library = constant_command_library(env.action_space, 3, 7, 10)
    fields = env.goal_field()
    plain = ShootingPlanner(env, library)
    action = plain.act().clone()
    assert plain.goal_field is None and plain.last.best is not None          # today's code path
    # weight 0: the same choice as the kernel's `best`
    zero = ShootingPlanner(env, library, goal_field=fields, terminal_weight=0.0)
    assert torch.equal(zero.act(), action) and torch.equal(zero.last_best.to(torch.int32), plain.last.best)
    # a weight: the key restated on the host
    weighted = ShootingPlanner(env, library, goal_field=fields, terminal_weight=5.0)
    chosen = weighted.act().clone()
    la = weighted.last
    k = library.shape[1]
    finals = la.final_pose.reshape(n * k, 3).cpu().numpy()
    farthest = _lib.GOAL_FAR * env.resolution / 12
    dist = _raw_sample(torch, env, fields.field, 1, farthest, finals, row_env=np.arange(n).repeat(k))[0][:, 0].astype(np.float64).reshape(n, k)
    score = la.ret.cpu().numpy() - 5.0 * dist
    free = (la.reason.cpu().numpy() & _lib.DONE_COLLIDED) == 0
    best = np.zeros(n, dtype=np.int64)
    for i in range(n):
        order = sorted(range(k), key=lambda j: (-int(free[i, j]), -score[i, j], j))
        best[i] = order[0]
    assert (weighted.last_best.cpu().numpy() == best).all()
    assert torch.equal(chosen, weighted.library[0, torch.from_numpy(best).cuda()])
    assert (best != plain.last.best.cpu().numpy()).any()        # (the terminal cost changes some choices)
    env.step(chosen)

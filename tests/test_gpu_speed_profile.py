"""bcp_path_speed on the GPU (speed_kernel) against the contract restated in Python floats (tests/speed_profile_ref.py).
Every raw call writes into sentinel-filled buffers, and whole buffers are compared.  kappa and v_limit: bit for bit (they use
+ - * / and sqrt alone, each rounded on its own).  speed: within relative 2 (m + 1) 2^-52 of the sequential recurrence -- the
wave scans associate the sums of at most m non-negative terms in a tree (each association within m 2^-53 of exact, two passes
and two implementations: 4 m 2^-53 on the squared speed; the root halves that and adds a rounding; the factor 2 covers the
second-order terms).  The largest share of that bound seen is printed."""
import ctypes as C

import numpy as np
import pytest

import speed_profile_ref as SP
import test_gpu_goal_field as TG

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
WEAK = dict(SP.STOCK, a_dec=0.01, a_acc=0.01, v_start=0.0, v_end=0.0)   # both passes bind from one end of a 10 m row to the other


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from bc_gym_planning_env_amd import NativeOps
    return NativeOps()


def _params(p):
    from bc_gym_planning_env_amd import _lib
    c = _lib.BcpSpeedParams()
    for k, v in p.items():
        setattr(c, k, v)
    return c


def _buffers(torch, n, max_len):
    out = {k: torch.full((n, max_len), SENTINEL, dtype=torch.float64, device="cuda") for k in ("speed", "kappa", "v_limit")}
    out["status"] = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    return out


def _raw(torch, ops, paths, lens, p, optional=True):
    """one raw call into sentinel-filled buffers -> dict of host arrays"""
    pt, lt = torch.from_numpy(np.ascontiguousarray(paths)).cuda(), torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    n, max_len = paths.shape[:2]
    out = _buffers(torch, n, max_len)
    rc = ops._lib.bcp_path_speed(ops._h, pt.data_ptr(), lt.data_ptr(), max_len, n, C.byref(_params(p)), out["speed"].data_ptr(),
                                 out["kappa"].data_ptr() if optional else None, out["v_limit"].data_ptr() if optional else None,
                                 out["status"].data_ptr(), None)
    assert rc == 0, ops._lib.bcp_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, paths, lens, p, tag):
    """-> the largest share of the bound used"""
    want = SP.path_speed(paths, lens, p)
    np.testing.assert_array_equal(got["status"], want[3], err_msg=tag)
    np.testing.assert_array_equal(got["kappa"].view(np.uint64), want[1].view(np.uint64), err_msg=tag + " kappa")
    np.testing.assert_array_equal(got["v_limit"].view(np.uint64), want[2].view(np.uint64), err_msg=tag + " v_limit")
    worst = SP.assert_speed_close(got["speed"], want[0], lens, paths.shape[1])
    differ = int((got["speed"] != want[0]).sum())
    print("%s: %d of %d speeds differ from the recurrence, worst %.4f of the bound" % (tag, differ, int(np.minimum(lens, paths.shape[1]).clip(0).sum()), worst))
    return worst


def _corner_at(m, at, turn=np.pi / 2):
    """m way points 0.05 apart with one sharp corner at way point `at`"""
    j = np.arange(m)
    before, after = np.minimum(j, at) * 0.05, np.maximum(j - at, 0) * 0.05
    return np.column_stack([before + after * np.cos(turn), after * np.sin(turn), np.zeros(m)])


def test_lengths_where_the_scan_can_go_wrong_sixteen_rows_at_once(torch_cuda, ops):
    torch = torch_cuda
    rng = np.random.RandomState(5)
    rows = [SP.row_of_length(rng, m, sharp=(1,) if m % 2 else ()) for m in (1, 2, 3, 63, 64, 65, 127, 128, 129, 200)]
    rows.append(_corner_at(200, 195))             # the slowest point in the LAST trip of 64 (way points 192 .. 199)
    rows.append(_corner_at(200, 5))               # ... in the FIRST: the carries cross every trip, both ways
    rows.append(SP.row_of_length(rng, 260))       # lens > max_len: the first 200 count
    rows.append(SP.row_of_length(rng, 150))       # lens = 0
    rows.append(SP.row_of_length(rng, 150))       # a NaN among its way points
    rows.append(SP.row_of_length(rng, 97, blend=0.0))
    paths, lens = SP.stack(rows, 200, fill=3.25)
    lens[13] = 0
    paths[14, 77, 1] = np.nan
    assert len(rows) == 16 and lens[12] == 260
    for tag, p in (("stock", SP.STOCK), ("weak", WEAK), ("span 3, v_min", dict(WEAK, span=3, v_min=0.2, v_start=0.3))):
        got = _raw(torch, ops, paths, lens, p)
        _check(got, paths, lens, p, "16 rows, " + tag)
        assert got["status"].tolist() == [0] * 13 + [SP.NO_PATH, SP.NO_PATH, 0]
        for k in ("speed", "kappa", "v_limit"):
            assert (got[k][13:15].view(np.uint64) == 0).all(), k
    # under the weak limits the corner rows' passes bind across every trip: the speed changes at every way point, and
    # nearly everywhere a pass, not the way point's own limit, sets it
    got = _raw(torch, ops, paths, lens, WEAK)
    for r, at in ((10, 195), (11, 5)):
        s = got["speed"][r]
        assert s[at] == got["v_limit"][r, at] < 0.1 and (np.diff(s[1:at + 1]) != 0).all() and (np.diff(s[at:199]) != 0).all()
        assert (s[1:199] < got["v_limit"][r, 1:199]).sum() >= 190
    # without the optional outputs: the same speeds
    alone = _raw(torch, ops, paths, lens, WEAK, optional=False)
    assert (alone["speed"].view(np.uint64) == got["speed"].view(np.uint64)).all()
    assert (alone["kappa"] == SENTINEL).all() and (alone["v_limit"] == SENTINEL).all()
    # NativeOps.path_speed on host arrays: the same call behind the Python surface
    from bc_gym_planning_env_amd import SpeedProfile
    named = {k: v for k, v in WEAK.items() if k != "span"}
    prof = ops.path_speed(paths, lens, span=1, want=("v_limit",), **named)
    assert isinstance(prof, SpeedProfile) and prof.owner is None and prof.epoch is None and prof.kappa is None and prof.max_len == 200
    assert prof.params == WEAK
    for name, t in (("speed", prof.speed), ("v_limit", prof.v_limit), ("status", prof.status)):
        assert (t.cpu().numpy() == got[name]).all(), name


def test_max_len_one_and_4096(torch_cuda, ops):
    torch = torch_cuda
    rng = np.random.RandomState(6)
    one = np.array([[[0.5, -0.25, 0.1]], [[1.5, 2.0, 0.0]], [[np.inf, 0.0, 0.0]], [[0.0, 0.0, 0.0]]])
    lens = np.array([1, 7, 1, 0], np.int32)
    p = dict(SP.STOCK, v_start=0.3, v_end=0.2)
    got = _raw(torch, ops, one, lens, p)
    _check(got, one, lens, p, "max_len 1")
    assert got["speed"][:, 0].tolist() == [0.2, 0.2, 0.0, 0.0] and got["status"].tolist() == [0, 0, SP.NO_PATH, SP.NO_PATH]
    long_rows = [SP.blended_row(SP.random_vertices(rng, 260))[:4096], _corner_at(4096, 4090), _corner_at(4096, 3), SP.row_of_length(rng, 70)]
    assert len(long_rows[0]) == 4096
    paths, lens = SP.stack(long_rows, 4096)
    slow = dict(SP.STOCK, a_dec=0.0005, a_acc=0.0005, v_end=0.0)           # (200 m of row: the passes bind over all 64 trips)
    for tag, p in (("stock", SP.STOCK), ("slow", slow)):
        worst = _check(_raw(torch, ops, paths, lens, p), paths, lens, p, "max_len 4096, " + tag)
        assert worst <= 1.0


def test_properties_on_random_rows(torch_cuda, ops):
    torch = torch_cuda
    rng = np.random.RandomState(7)
    rows = [SP.row_of_length(rng, int(m), sharp=(2,) if k % 3 == 0 else ()) for k, m in enumerate(rng.randint(31, 295, 32))]
    paths, lens = SP.stack(rows, 300, fill=-1.0)
    p = dict(SP.STOCK, v_min=0.05, v_start=0.2, v_end=0.1)
    got = _raw(torch, ops, paths, lens, p)
    _check(got, paths, lens, p, "32 random rows")
    for i, r in enumerate(rows):
        m, b = len(r), SP.bound(len(r))
        s, cd, ca = got["speed"][i, :m], *SP.row(paths[i], m, 300, p)[4]
        assert (s <= got["v_limit"][i, :m]).all() and s[0] <= 0.2 and s[-1] <= 0.1
        assert (s[1:-1] >= 0.05).all()
        assert (s[:-1] ** 2 - s[1:] ** 2 <= cd * (1 + b)).all()
        assert (s[1:] ** 2 - s[:-1] ** 2 <= ca * (1 + b)).all()
        assert (got["speed"][i, m:].view(np.uint64) == 0).all()


def test_env_speed_profile_on_a_pool_after_route_paths_and_on_a_shared_path(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import SpeedProfile, _lib
    env = TG._mini(16, timeout=60)
    status = env.route_paths(max_len=400, smooth=dict(look=64, blend=0.3, delta=0.05, halvings=2, route_len=512))
    assert ((status.cpu().numpy() & ~_lib.SMOOTH_BLOCKED) == 0).sum() >= 8
    top = float(env.action_space.high[0])
    prof = env.speed_profile(a_lat=0.2, w_max=0.5, a_dec=0.4, a_acc=0.4, v_end=0.0, want=("kappa", "v_limit"))
    assert isinstance(prof, SpeedProfile) and prof.owner is env and prof.epoch == env._path_epoch and prof.max_len == 400
    assert prof.params == dict(span=1, v_max=top, v_min=0.0, a_lat=0.2, w_max=0.5, a_dec=0.4, a_acc=0.4, v_start=top, v_end=0.0)
    paths, lens = env._keep["path"].cpu().numpy(), env._keep["lens"].cpu().numpy()
    assert paths.shape == (16, 400, 3) and tuple(prof.speed.shape) == (16, 400)
    got = dict(speed=prof.speed.cpu().numpy(), kappa=prof.kappa.cpu().numpy(), v_limit=prof.v_limit.cpu().numpy(),
               status=prof.status.cpu().numpy())
    _check(got, paths, lens, prof.params, "the pool's routed, smoothed paths")
    assert (got["status"] == 0).all() and (got["kappa"].max(axis=1) > 0.5).sum() >= 8      # blended corners: radius < 2 m
    assert (got["speed"].min(axis=1, initial=1.0, where=np.arange(400)[None] < lens[:, None] - 1) < 0.9 * top).sum() >= 8
    # the raw form on the same tensors, and through a wrapper
    from bc_gym_planning_env_amd import wrappers
    raw = wrappers.BatchedObservationWrapper(env).path_speed(env._keep["path"], env._keep["lens"], top, 0.2, 0.5, 0.4, 0.4, v_end=0.0)
    assert torch.equal(raw.speed, prof.speed) and raw.owner is None and raw.kappa is None
    with pytest.raises(ValueError):
        env.speed_profile(want=("curvature",))
    # a shared path
    from util import GOLDEN, env_from_traj
    import os
    g = np.load(os.path.join(GOLDEN, "g8_traj_mini_00.npz"))
    shared = env_from_traj(g, "mini_nonoise", n_envs=3)
    prof = shared.speed_profile(a_lat=0.1, want=("kappa",))
    m = len(g["path"])
    assert tuple(prof.speed.shape) == (m,) and tuple(prof.kappa.shape) == (m,) and tuple(prof.status.shape) == (1,)
    want = SP.path_speed(np.asarray(g["path"], np.float64)[None], [m], prof.params)
    assert (prof.kappa.cpu().numpy().view(np.uint64) == want[1][0].view(np.uint64)).all()
    SP.assert_speed_close(prof.speed.cpu().numpy()[None], want[0], [m], m)
    # an endless pool is refused, as route_paths refuses it
    with pytest.raises(RuntimeError, match="endless"):
        TG._mini(8, timeout=60, endless=True).speed_profile()


def test_a_captured_call_replayed_twice(torch_cuda, ops):
    torch = torch_cuda
    rng = np.random.RandomState(8)
    paths, lens = SP.stack([SP.row_of_length(rng, m) for m in (150, 64, 1, 129)], 160)
    pt, lt = torch.from_numpy(paths).cuda(), torch.from_numpy(lens).cuda()
    p = _params(WEAK)
    out = _buffers(torch, 4, 160)

    def call():
        assert ops._lib.bcp_path_speed(ops._h, pt.data_ptr(), lt.data_ptr(), 160, 4, C.byref(p), out["speed"].data_ptr(),
                                       out["kappa"].data_ptr(), out["v_limit"].data_ptr(), out["status"].data_ptr(),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0

    call()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            call()
    torch.cuda.synchronize()
    for k, v in out.items():
        v.fill_(SENTINEL if v.dtype == torch.float64 else -77)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in out)
    pt[0, :, 0] *= 2.0                                         # the second replay reads the paths as they are now
    for k, v in out.items():
        v.fill_(SENTINEL if v.dtype == torch.float64 else -77)
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _check(got, pt.cpu().numpy(), lens, WEAK, "second replay")
    assert not torch.equal(out["speed"][0], eager["speed"][0]) and torch.equal(out["speed"][1:], eager["speed"][1:])


def test_refusals_write_nothing(torch_cuda, ops):
    torch = torch_cuda
    rng = np.random.RandomState(9)
    paths, lens = SP.stack([SP.row_of_length(rng, 40)] * 3, 48)
    pt, lt = torch.from_numpy(paths).cuda(), torch.from_numpy(lens).cuda()
    out = _buffers(torch, 3, 48)
    inf, nan = float("inf"), float("nan")

    def call(prm=None, **change):
        a = dict(h=ops._h, paths=pt.data_ptr(), lens=lt.data_ptr(), max_len=48, n=3, p=C.byref(_params(dict(SP.STOCK, **(prm or {})))),
                 speed=out["speed"].data_ptr(), kappa=out["kappa"].data_ptr(), v_limit=out["v_limit"].data_ptr(),
                 status=out["status"].data_ptr())
        a.update(change)
        rc = ops._lib.bcp_path_speed(a["h"], a["paths"], a["lens"], a["max_len"], a["n"], a["p"], a["speed"], a["kappa"], a["v_limit"],
                                     a["status"], None)
        return rc, ops._lib.bcp_last_error().decode()

    inside = pt.data_ptr() + 3 * 48 * 24 - 8                   # the last double of paths
    refused = [(dict(h=None), "null"), (dict(paths=None), "null"), (dict(lens=None), "null"), (dict(p=None), "null"),
               (dict(speed=None), "null"), (dict(status=None), "null"),
               (dict(max_len=0), "max_len"), (dict(max_len=4097), "max_len"), (dict(n=0), "n must"), (dict(n=-1), "n must"),
               (dict(prm=dict(span=0)), "span"), (dict(prm=dict(span=65)), "span"),
               (dict(prm=dict(v_max=0.0)), "v_max"), (dict(prm=dict(v_max=nan)), "v_max"), (dict(prm=dict(a_lat=inf)), "a_lat"),
               (dict(prm=dict(w_max=-1.0)), "w_max"), (dict(prm=dict(a_dec=0.0)), "a_dec"), (dict(prm=dict(a_acc=nan)), "a_acc"),
               (dict(prm=dict(v_min=-0.1)), "v_min"), (dict(prm=dict(v_start=nan)), "v_start"), (dict(prm=dict(v_end=inf)), "v_end"),
               (dict(prm=dict(v_min=0.6)), "v_min > v_max"),
               (dict(speed=pt.data_ptr()), "overlap"), (dict(kappa=inside), "overlap"), (dict(v_limit=pt.data_ptr() + 8), "overlap"),
               # the order: the first thing wrong is the one named
               (dict(max_len=0, n=0, prm=dict(span=0, v_max=nan)), "max_len"), (dict(n=0, prm=dict(span=0, v_max=nan)), "n must"),
               (dict(prm=dict(span=0, v_max=nan, v_min=nan)), "span"), (dict(prm=dict(a_acc=0.0, a_lat=0.0, v_end=-1.0)), "a_lat"),
               (dict(prm=dict(v_end=-1.0, v_min=0.6), speed=pt.data_ptr()), "v_end"), (dict(prm=dict(v_min=0.6), speed=pt.data_ptr()), "v_min > v_max")]
    for change, word in refused:
        rc, msg = call(**change)
        assert rc == -1 and msg.startswith("bcp_path_speed: ") and word in msg, (change, msg)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == (SENTINEL if v.dtype == torch.float64 else -77)).all(), k
    assert call()[0] == 0 and call(kappa=None, v_limit=None)[0] == 0     # the same call, unchanged, is taken
    torch.cuda.synchronize()
    assert (out["status"] == 0).all() and not (out["speed"] == SENTINEL).any()

"""GPU tests of bcp_smooth_route (smooth_kernel), GoalField.smooth and route_paths(smooth=...) against the restatement of
the contract (tests/smooth_route_ref.py) on fields that bcp_goal_field built.  Every raw call writes into sentinel-filled
outputs with a guard row before and behind, and whole buffers are compared: x, y, lens, status, info, target_idx and the
zero tails bit for bit, headings and min_spat_dist_so_far within 1e-9 (the project's bound on float64 state; atan2 and
hypot are the device's here, numpy's there).  target_idx is compared on rows away from the knife edges of
find_last_reached alone (goal_route_ref.away_from_knife_edges, decided in the reference); the hand-built cases have no such
row, the random ones at most one in ten.  The property tests at the end need no restatement."""
import numpy as np
import pytest

import goal_field_ref as GR
import goal_route_ref as RR
import smooth_route_ref as SR
import test_gpu_goal_field as TG

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
POISON_F, POISON_I = -7.5, -77
DEFAULT = dict(look=64, blend=0.3, delta=0.05, halvings=2)


def _env_params(**kw):
    from bc_gym_planning_env_amd import EnvParams
    return EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, resolution=SR.RES, refine_path=False, **kw)


class _Out(object):
    """sentinel-filled outputs of n rows with one guard row on either side"""

    def __init__(self, torch, n, max_len):
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")   # noqa: E731
        self.paths = full((n + 2, max_len, 3), POISON_F, torch.float64)
        self.lens, self.status = full((n + 2,), POISON_I, torch.int32), full((n + 2,), POISON_I, torch.int32)
        self.init, self.info = full((n + 2, 2), POISON_F, torch.float64), full((n + 2, 4), POISON_I, torch.int32)

    def tensors(self):
        return self.paths, self.lens, self.status, self.init, self.info

    def read(self, untouched=False):
        got = [t.cpu().numpy() for t in self.tensors()]
        for t, poison in zip(got, (POISON_F, POISON_I, POISON_I, POISON_F, POISON_I)):
            assert (t[0] == poison).all() and (t[-1] == poison).all()          # the guards are untouched
            assert not untouched or (t == poison).all()                        # a refused call writes nothing
        return tuple(t[1:-1] for t in got)


def _raw(torch, owner, field_t, paths_in, lens_in, max_len, row_env=None, entries=False, out=None, **prm):
    from bc_gym_planning_env_amd import _lib
    p = dict(DEFAULT, **prm)
    pt = torch.from_numpy(np.ascontiguousarray(paths_in, dtype=np.float64)).cuda()
    lt = torch.from_numpy(np.ascontiguousarray(lens_in, dtype=np.int32)).cuda()
    rt = None if row_env is None else torch.from_numpy(np.ascontiguousarray(row_env, dtype=np.int32)).cuda()
    n = len(paths_in)
    out = _Out(torch, n, max_len) if out is None else out
    f = field_t
    prm_c = _lib.BcpSmoothParams(p["look"], p["halvings"], p["blend"], p["delta"])
    _lib.check(owner._lib.bcp_smooth_route(owner._h, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2], pt.data_ptr(), lt.data_ptr(),
                                           pt.shape[1], n, None if rt is None else rt.data_ptr(), int(entries), prm_c, max_len,
                                           out.paths[1:].data_ptr(), out.lens[1:].data_ptr(), out.init[1:].data_ptr(),
                                           out.status[1:].data_ptr(), out.info[1:].data_ptr(), None))
    torch.cuda.synchronize()
    return out.read()


def _check(got, want, rp, what, may_skip=0):
    """got = (paths, lens, status, init, info) of the kernel, want = the restatement's -> the rows whose target_idx was skipped"""
    paths, lens, status, init, info = got
    on_edge = [i for i in range(len(lens)) if want[1][i] and not SR.away_from_knife_edges(want[0][i, :want[1][i]], rp)]
    print(what, "rows", len(lens), "with a path", int((want[1] > 0).sum()), "status", np.unique(want[2]).tolist(), "knife", on_edge,
          "max |heading - numpy| = %.3g, max |min_dist - numpy| = %.3g (bound 1e-9), max |xy - restatement| = %.3g"
          % (np.abs(paths[..., 2] - want[0][..., 2]).max(), np.abs(init[:, 0] - want[3][:, 0]).max(),
             np.abs(paths[..., :2] - want[0][..., :2]).max()))
    assert len(on_edge) <= may_skip, (what, on_edge)
    init = init.copy()
    init[on_edge, 1] = want[3][on_edge, 1]
    SR.compare(paths, lens, status, init, *want[:4])
    np.testing.assert_array_equal(info, want[4])
    return on_edge


# ---- the hand-built worlds: five private maps whose valid shapes are smaller than the padded 24 x 31 -----------------------
def hand_case():
    """everything of the hand-built case that needs no GPU: worlds, the fields Dijkstra gives, rows and their envs"""
    worlds = SR.hand_worlds()
    names = ["L", "U", "corridor", "diagonal"]
    corner = SR._world((24, 30), [(11, 12, 9, 10)], (3, 3), (20, 25), (0.05, -0.15))
    ws = [dict(worlds[k], d2=0) for k in names] + [corner]
    fields = np.stack([SR.padded(SR.world_field(w), fill=GR.NONE) for w in ws])
    valids = np.array([w["data"].shape for w in ws])
    origins = np.stack([w["origin"] for w in ws])
    ends = [(SR.pose_in(w, w["start_cell"], 0.3), SR.pose_in(w, w["goal_cell"], -1.0, off=(0.004, 0.003))) for w in ws]
    length = 61                                                           # world U's route fills every slot
    rows, lens_in, row_env = [], [], []

    def add(wp, k, env):
        slot = np.zeros((length, 3))
        slot[:min(len(wp), length)] = wp[:length]
        rows.append(slot)
        lens_in.append(k)
        row_env.append(env)

    for e, w in enumerate(ws):                                            # 0 .. 4: the stride-1 route of every world
        wp, k, st, _i, _c = RR.route_row(fields[e], valids[e], origins[e], SR.RES, ends[e][0], ends[e][1], 1, length)
        assert st == 0 and k <= length and (e != 1 or k == length)
        add(wp, k, e)
    o4 = origins[4]
    for off in ((0.003, 0.002), (-0.04, 0.04)):                          # 5, 6: the corner beside the blocked cell (11, 9)
        add(SR.corner_rows(o4, off), 3, 4)
    three = SR.corner_rows(origins[1] + np.array([0.6, 0.6]), (0.003, 0.002))   # in world U's free middle band: rows 9 .. 14
    three[:, 1] = origins[1][1] + 11 * SR.RES + 0.002
    three[:, 0] = origins[1][0] + np.array([10, 16, 22]) * SR.RES
    add(three[:2], 2, 1)                                                  # 7: two way points
    add(three, 3, 1)                                                      # 8: three on one line
    add(rows[1], 500, 1)                                                  # 9: lens_in above max_len_in
    nan = three.copy()
    nan[1, 2] = np.nan
    add(nan, 3, 1)                                                        # 10: NO_ROUTE
    outside = SR.corner_rows(o4, (0.003, 0.002))
    outside[2, 0] = o4[0] + 30.3 * SR.RES                                 # 11: beyond the valid shape's 30 columns: BLOCKED
    outside[2, 1] = outside[1, 1]
    add(outside, 3, 4)
    add(three, 1, 1)                                                      # 12: one way point
    add(three, 3, 7)                                                      # 13: an env out of range
    close = np.array([[three[0, 0], three[0, 1], 0.2], [three[0, 0] + 0.02, three[0, 1], 0.25]])
    add(close, 2, 1)                                                      # 14: TOO_CLOSE
    add(rows[3], lens_in[3], 3)                                           # 15: the diagonal world again, another lane's worth
    entry = np.array([e if 0 <= e < 5 else -1 for e in row_env])
    return dict(ws=ws, fields=fields, valids=valids, origins=origins, ends=ends, rows=np.stack(rows), lens_in=np.array(lens_in),
                row_env=np.array(row_env), entry=entry)


HAND_SWEEP = [dict(), dict(look=1), dict(look=200, blend=0.0), dict(look=7, blend=3.0), dict(halvings=0), dict(look=3, delta=0.021)]


def hand_want(case, rp, max_len=400, **prm):
    p = dict(DEFAULT, **prm)
    return SR.smooth(case["fields"], case["valids"], case["origins"], SR.RES, case["entry"], case["rows"], case["lens_in"],
                     p["look"], p["blend"], p["delta"], p["halvings"], max_len, reward_params=rp)


def _hand_env(torch, case, **kw):
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
    maps = [CostMap2D(w["data"].copy(), SR.RES, w["origin"]) for w in case["ws"]]
    env = BatchedPlanEnv(maps, [np.stack(e) for e in case["ends"]], _env_params(**kw), n_envs=5)
    fields = env.goal_field(clearance=0.0)
    got_f = fields.field.cpu().numpy()
    for e in range(5):                                                    # bcp_goal_field's planes are Dijkstra's, inside the valid shapes
        vr, vc = case["valids"][e]
        assert (got_f[e, :vr, :vc] == case["fields"][e, :vr, :vc]).all(), e
    return env, fields


def test_hand_built_worlds_rows_envs_and_parameters(torch_cuda):
    torch = torch_cuda
    case = hand_case()
    assert tuple(case["fields"].shape[1:]) == SR.PAD and (case["valids"] < np.array(SR.PAD)).any(axis=1).all()
    env, fields = _hand_env(torch, case)
    rp = env.params.reward_provider_params
    for prm in HAND_SWEEP:
        want = hand_want(case, rp, **prm)
        got = _raw(torch, env, fields.field, case["rows"], case["lens_in"], 400, row_env=case["row_env"], **prm)
        _check(got, want, rp, "hand-built %r" % (prm,))
        assert want[2].tolist()[9:15] == [0, SR.NO_ROUTE, SR.BLOCKED, SR.NO_ROUTE, SR.NO_ROUTE, SR.TOO_CLOSE]
        assert (want[2][:9] == 0).all() and (want[1][:10] >= 2).all()
        assert (want[0][9] == want[0][1]).all()                                              # lens_in above max_len_in counts as max_len_in
    want, keep_all = hand_want(case, rp), hand_want(case, rp, look=1)
    assert keep_all[4][5].tolist() == [3, 0, 1, 0] and keep_all[4][6].tolist() == [3, 0, 0, 1]   # halved; refused at every size
    assert want[4][7].tolist() == [2, 0, 0, 0] and want[4][8, 0] == 2                       # rows of 2 and of 3 way points
    assert want[4][0, 1] >= 1 and want[4][3, 0] >= 3                                        # the diagonal gap is not cut through
    assert hand_want(case, rp, look=1)[4][1, 0] == case["lens_in"][1]                       # look = 1 keeps everything
    assert hand_want(case, rp, look=1, blend=3.0)[4][8].tolist() == [3, 1, 0, 0]            # clipped by the legs' thirds
    _check(_raw(torch, env, fields.field, case["rows"], case["lens_in"], 400, row_env=case["row_env"], look=1, blend=3.0),
           hand_want(case, rp, look=1, blend=3.0), rp, "clipped blends")
    # max_len exactly the count, and one below it
    k = int(want[1][1])
    one = (case["rows"][1:2], case["lens_in"][1:2])
    fits = _raw(torch, env, fields.field, *one, k, row_env=[1])
    _check(fits, SR.smooth(case["fields"], case["valids"], case["origins"], SR.RES, [1], *one, 64, 0.3, 0.05, 2, k, reward_params=rp),
           rp, "max_len = the count")
    assert fits[1][0] == k and fits[2][0] == 0
    short = _raw(torch, env, fields.field, *one, k - 1, row_env=[1])
    assert short[1][0] == 0 and short[2][0] == SR.LONG and (short[0].view(np.uint64) == 0).all() and (short[3] == 0).all()
    assert short[4][0].tolist() == want[4][1].tolist()
    # GoalField.smooth: the same bytes, cached buffers, outputs on request
    p, l, s, i, info = fields.smooth(case["rows"], case["lens_in"], row_env=case["row_env"], max_len=400, want=("init", "info"))
    got = _raw(torch, env, fields.field, case["rows"], case["lens_in"], 400, row_env=case["row_env"])
    for a, b in zip((p, l, s, i, info), got):
        assert (np.ascontiguousarray(a.cpu().numpy()).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()
    assert fields.smooth(case["rows"], case["lens_in"], row_env=case["row_env"], max_len=400)[0].data_ptr() == p.data_ptr()
    assert fields.smooth(case["rows"], case["lens_in"], row_env=case["row_env"])[0].shape == (16, 61, 3)
    with pytest.raises(ValueError):
        fields.smooth(case["rows"], case["lens_in"], want=("nothing",))


def long_case():
    """one shared 64 x 200 map with a wall the route has to round: a row of more than 130 way points whose first anchor sees
    nothing in its farthest chunk of 64 candidates"""
    data = np.zeros((64, 200), dtype=np.uint8)
    data[0:50, 110:112] = 254
    origin = np.array([-2.0, 1.0])
    goal_cell, start_cell = (10, 190), (10, 5)
    field = GR.dijkstra(data, [goal_cell], 1)
    w = dict(origin=origin)
    start, goal = SR.pose_in(w, start_cell, 0.3), SR.pose_in(w, goal_cell, -1.0, off=(0.004, 0.003))
    wp, k, st, _i, _c = RR.route_row(field, field.shape, origin, SR.RES, start, goal, 1, 320)
    assert st == 0 and k >= 130
    return dict(data=data, origin=origin, field=field, rows=np.stack([wp, wp, wp]), lens_in=np.array([k, k, 140]), goal=goal, start=start)


def test_a_long_row_takes_more_than_one_chunk_of_candidates_and_one_field_serves_all(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
    c = long_case()
    env = BatchedPlanEnv(CostMap2D(c["data"].copy(), SR.RES, c["origin"]), np.stack([c["start"], c["goal"]]), _env_params(), n_envs=3)
    fields = env.goal_field(clearance=SR.RES)
    assert fields.field.shape == (1, 64, 200) and (fields.field.cpu().numpy()[0] == c["field"]).all()
    rp = env.params.reward_provider_params
    for prm in (dict(look=4096), dict(look=100), dict(look=64)):
        want = SR.smooth(c["field"][None], [c["field"].shape], [c["origin"]], SR.RES, np.zeros(3, dtype=np.int64), c["rows"],
                         c["lens_in"], prm["look"], 0.3, 0.05, 2, 600, reward_params=rp)
        got = _raw(torch, env, fields.field, c["rows"], c["lens_in"], 600, **prm)
        _check(got, want, rp, "64 x 200 %r" % (prm,))
        assert (want[2] == 0).all() and want[4][0, 0] < 12
    with pytest.raises(RuntimeError):
        env.route_paths(smooth={})


def test_a_pool_of_16_entries_rows_are_entries_and_a_diff_drive_handle(torch_cuda):
    torch = torch_cuda
    env = TG._mini(16, timeout=12)
    fields = env.goal_field()
    want_f = TG._ref_fields(env, 151)
    _data, valid, origins = TG._maps_of(env)
    rp = env.params.reward_provider_params
    cells, cell_lens, st = (t.cpu().numpy() for t in fields.route_bound(1, 200))
    assert (st == 0).all()
    want = SR.smooth(want_f, valid, origins, env.resolution, np.arange(16), cells, cell_lens, 64, 0.3, 0.05, 2, 160, reward_params=rp)
    got = _raw(torch, env, fields.field, cells, cell_lens, 160, entries=True)
    skipped = _check(got, want, rp, "16 pool entries, rows are entries", may_skip=1)
    assert (want[2] & ~SR.LONG == 0).all() and (want[1] > 0).sum() >= 12
    # rows through envs: 40 rows on the pool's current entries
    geom = env.geom_of_env.cpu().numpy()
    row_env = np.random.RandomState(5).randint(0, 16, 40)
    entry = geom[row_env].astype(np.int64)
    got = _raw(torch, env, fields.field, cells[entry], cell_lens[entry], 160, row_env=row_env)
    want40 = tuple(w[entry] for w in want)
    _check(got, want40, rp, "40 rows through row_env", may_skip=4 * max(len(skipped), 1))
    # a diff-drive handle on the hand-built worlds: the same paths, its own provider state
    case = hand_case()
    denv, dfields = _hand_env(torch, case, robot_name='industrial_diffdrive_v1')
    rp = denv.params.reward_provider_params
    got = _raw(torch, denv, dfields.field, case["rows"], case["lens_in"], 400, row_env=case["row_env"])
    _check(got, hand_want(case, rp), rp, "diff-drive")


def test_route_paths_smooth_on_pools_and_a_weighted_field(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import EnvParams, aisle_env, _lib
    ranges = aisle_env.TurnRanges(main_corridor_length=(3., 4.), turn_corridor_length=(2., 3.), main_corridor_width=(1.2, 1.8),
                                  turn_corridor_width=(1.2, 1.8), margin=0.5)
    aisle = lambda: aisle_env.BatchedRandomAisleTurnEnv(16, EnvParams(iteration_timeout=40, resolution=0.05), n_chains=2,   # noqa: E731
                                                        episodes=4, sampler="device_resident", auto_reset=True, ranges=ranges)
    smooth = dict(DEFAULT, route_len=512)
    for what, make, kw in (("mini pool", lambda: TG._mini(16, timeout=60), dict(clearance=None)),
                           ("mini pool, weighted", lambda: TG._mini(16, timeout=60), dict(cost_weight=2.0)),
                           ("aisle pool", aisle, dict(clearance=0.2))):
        env, twin = make(), make()
        if "cost_weight" in kw:
            env.inflate_costmaps(4.0)
            twin.inflate_costmaps(4.0)
        fields = env.goal_field(**kw)
        rp = env.params.reward_provider_params
        _data, valid, origins = TG._maps_of(env)
        starts = env._keep["path"].cpu().numpy()[:, 0].copy()
        lens0 = env._keep["lens"].cpu().numpy()
        ends = env._keep["path"].cpu().numpy()[np.arange(len(lens0)), lens0 - 1].copy()
        before = env._keep["path"].clone()
        n = len(lens0)
        max_len = 400
        plane = fields.field.cpu().numpy()
        cells = RR.route(plane, valid, origins, env.resolution, np.arange(n), starts, ends, 1, 512, reward_params=rp)
        want = SR.smooth(plane, valid, origins, env.resolution, np.arange(n), cells[0], cells[1], 64, 0.3, 0.05, 2, max_len,
                         reward_params=rp)
        status = env.route_paths(fields, max_len=max_len, smooth=smooth).cpu().numpy()
        assert (status == (want[2] | cells[2])).all() and (status & _lib.SMOOTH_BLOCKED == 0).all(), what
        ok = (status & ~_lib.SMOOTH_BLOCKED) == 0
        assert ok.sum() >= n // 2, (what, status)
        pts, lens = env._keep["path"].cpu().numpy(), env._keep["lens"].cpu().numpy()
        on_edge = [k for k in range(n) if ok[k] and not SR.away_from_knife_edges(want[0][k, :want[1][k]], rp)]
        print(what, "entries", n, "smoothed", int(ok.sum()), "knife", on_edge)
        first = env._initial_state
        for k in range(n):
            if not ok[k]:
                assert (pts[k, :before.shape[1]] == before[k].cpu().numpy()).all() and lens[k] == lens0[k]
                continue
            assert lens[k] == want[1][k] and (pts[k, :lens[k], :2] == want[0][k, :lens[k], :2]).all(), (what, k)
            assert np.abs(pts[k, :lens[k], 2] - want[0][k, :lens[k], 2]).max() <= 1e-9 and (pts[k, lens[k]:] == 0).all()
            assert abs(float(first.min_spat_dist_so_far[k]) - want[3][k, 0]) <= 1e-9
            assert k in on_edge or int(first.target_idx[k]) == want[3][k, 1]
        assert len(on_edge) * 10 <= n
        # the twin takes smooth=None: the function as it was
        old = RR.route(TG._ref_fields(twin, fields.clearance_d2) if "cost_weight" not in kw else plane, valid, origins, env.resolution,
                       np.arange(n), starts, ends, 2, max_len, reward_params=rp)
        twin_fields = twin.goal_field(**kw)
        st2 = twin.route_paths(twin_fields, stride=2, max_len=max_len, smooth=None).cpu().numpy()
        assert (st2 == old[2]).all()
        tp, tl = twin._keep["path"].cpu().numpy(), twin._keep["lens"].cpu().numpy()
        for k in range(n):
            if st2[k] == 0:
                assert tl[k] == old[1][k] and (tp[k, :tl[k], :2] == old[0][k, :tl[k], :2]).all()
    with pytest.raises(ValueError):
        env.route_paths(fields, smooth=dict(stride=2))


def test_one_captured_call_replayed_twice(torch_cuda):
    torch = torch_cuda
    case = hand_case()
    env, fields = _hand_env(torch, case)
    rows = torch.from_numpy(case["rows"]).cuda()
    lens_in = torch.from_numpy(case["lens_in"].astype(np.int32)).cuda()
    row_env = torch.from_numpy(case["row_env"].astype(np.int32)).cuda()
    names = ("paths", "lens", "status", "init", "info")

    def call():
        return dict(zip(names, fields.smooth(rows, lens_in, row_env=row_env, max_len=400, want=("init", "info"))))

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
    rows[0, 0, 1] += 0.004                                               # the input the captured launch reads changes
    graph.replay()
    torch.cuda.synchronize()
    replayed = {f: out[f].clone() for f in names}
    now = call()
    for f in names:
        assert torch.equal(now[f], replayed[f]), f
    assert not torch.equal(replayed["paths"], eager["paths"])


def test_refusals_write_nothing(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import _lib
    from bc_gym_planning_env_amd.ops import NativeOps
    case = hand_case()
    owner = NativeOps()
    L = owner._lib
    f = torch.from_numpy(case["fields"].copy()).cuda()
    rows = torch.from_numpy(case["rows"][:5].copy()).cuda()
    lens_in = torch.from_numpy(case["lens_in"][:5].astype(np.int32)).cuda()
    env_of = torch.zeros(5, dtype=torch.int32, device="cuda")
    out = _Out(torch, 5, 100)
    prm = _lib.BcpSmoothParams(64, 2, 0.3, 0.05)

    def call(h=owner._h, field=f.data_ptr(), nf=5, rows_=24, cols=31, pin=rows.data_ptr(), lin=lens_in.data_ptr(), mli=61, n=5,
             row_env=None, entries=0, p=prm, max_len=100, paths=out.paths[1:].data_ptr(), lens=out.lens[1:].data_ptr(),
             init=out.init[1:].data_ptr(), status=out.status[1:].data_ptr(), info=out.info[1:].data_ptr(), **kw):
        if kw:
            p = _lib.BcpSmoothParams(kw.get("look", 64), kw.get("halvings", 2), kw.get("blend", 0.3), kw.get("delta", 0.05))
        return L.bcp_smooth_route(h, field, nf, rows_, cols, pin, lin, mli, n, row_env, entries, p, max_len, paths, lens, init, status,
                                  info, None)

    assert call() == E_STATE and b"costmaps" in L.bcp_last_error()
    assert call(look=0) == E_INVALID                                       # (arguments before state)
    env, fields = _hand_env(torch, case)
    call_env = lambda **kw: call(h=env._h, **kw)                           # noqa: E731
    for name in ("field", "pin", "lin", "paths", "lens", "status", "p"):
        assert call_env(**{name: None}) == E_INVALID and b"null" in L.bcp_last_error(), name
    assert call(h=None) == E_INVALID
    for kw, word in ((dict(look=0), b"look"), (dict(look=4097), b"look"), (dict(halvings=-1), b"halvings"), (dict(halvings=9), b"halvings"),
                     (dict(blend=float("nan")), b"blend"), (dict(blend=-0.1), b"blend"), (dict(blend=float("inf")), b"blend"),
                     (dict(delta=float("nan")), b"delta"), (dict(delta=0.0), b"delta"), (dict(delta=float("inf")), b"delta"),
                     (dict(mli=1), b"max_len_in"), (dict(mli=4097), b"max_len_in"), (dict(max_len=1), b"max_len"),
                     (dict(max_len=4097), b"max_len"), (dict(n=0), b"n must"), (dict(n=-2), b"n must"),
                     (dict(entries=1, row_env=env_of.data_ptr()), b"row_env"), (dict(rows_=23), b"shape"), (dict(cols=32), b"shape"),
                     (dict(nf=2), b"n_fields"), (dict(nf=0), b"n_fields"), (dict(entries=1, nf=1), b"n_fields"),
                     (dict(entries=1, n=4), b"entries bound")):
        assert call_env(**kw) == E_INVALID and word in L.bcp_last_error(), kw
        assert L.bcp_last_error().startswith(b"bcp_smooth_route: ")
    assert call_env(look=0, halvings=9, mli=0) == E_INVALID and b"look" in L.bcp_last_error()          # the order
    assert call_env(halvings=9, blend=-1.0) == E_INVALID and b"halvings" in L.bcp_last_error()
    assert call_env(max_len=1, n=0) == E_INVALID and b"max_len" in L.bcp_last_error()
    # state: overlapping buffers, the bound paths' own arrays, a shared map with rows_are_entries
    assert call_env(paths=rows.data_ptr()) == E_STATE and b"overlap" in L.bcp_last_error()
    assert call_env(paths=rows[2:].data_ptr()) == E_STATE and call_env(lens=lens_in.data_ptr()) == E_STATE
    pts, blens = env._keep["path"], env._keep["lens"]
    assert call_env(paths=pts.data_ptr(), max_len=int(pts.shape[1])) == E_STATE and b"bound paths" in L.bcp_last_error()
    assert call_env(lens=blens.data_ptr()) == E_STATE
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
    c = long_case()
    shared = BatchedPlanEnv(CostMap2D(c["data"].copy(), SR.RES, c["origin"]), np.stack([c["start"], c["goal"]]), _env_params(), n_envs=5)
    f1 = torch.from_numpy(np.repeat(c["field"][None], 5, axis=0).copy()).cuda()
    assert call(h=shared._h, field=f1.data_ptr(), rows_=64, cols=200, entries=1) == E_STATE and b"shared" in L.bcp_last_error()
    torch.cuda.synchronize()
    out.read(untouched=True)
    assert call_env() == 0 and call_env(init=None, info=None) == 0 and call_env(row_env=env_of.data_ptr()) == 0
    assert call_env(entries=1) == 0
    torch.cuda.synchronize()


# ---- properties that need no restatement ---------------------------------------------------------------------------------
def random_worlds(n=32, seed=7):
    """n small box worlds with start and goal on cell centres -> (data list, origins, starts, goals)"""
    rng = np.random.RandomState(seed)
    datas, origins, starts, goals = [], [], [], []
    while len(datas) < n:
        shape = (int(rng.randint(26, 40)), int(rng.randint(26, 40)))
        data = np.zeros(shape, dtype=np.uint8)
        for _ in range(4):
            r, c, h, w = rng.randint(4, shape[0] - 8), rng.randint(4, shape[1] - 8), rng.randint(1, 7), rng.randint(1, 7)
            data[r:r + h, c:c + w] = 254
        free = np.argwhere(GR.free_mask(data, [], 1))
        a, b = free[rng.randint(len(free))], free[rng.randint(len(free))]
        if abs(a - b).sum() < 14:
            continue
        origin = np.round(rng.uniform(-1, 1, 2), 3)
        cell = lambda rc, th: np.array([origin[0] + np.float64(rc[1]) * SR.RES, origin[1] + np.float64(rc[0]) * SR.RES, th])   # noqa: E731
        datas.append(data)
        origins.append(origin)
        starts.append(cell(a, rng.uniform(-3, 3)))
        goals.append(cell(b, rng.uniform(-3, 3)))
    return datas, np.stack(origins), np.stack(starts), np.stack(goals)


def random_want(datas, origins, starts, goals, rp):
    n = len(datas)
    shape = (max(d.shape[0] for d in datas), max(d.shape[1] for d in datas))
    valids = np.array([d.shape for d in datas])
    cells_of = lambda k: (int(np.rint((goals[k, 1] - origins[k, 1]) / SR.RES)), int(np.rint((goals[k, 0] - origins[k, 0]) / SR.RES)))   # noqa: E731
    fields = np.stack([SR.padded(GR.dijkstra(d, [cells_of(k)], 1), shape, GR.NONE) for k, d in enumerate(datas)])
    cells = RR.route(fields, valids, origins, SR.RES, np.arange(n), starts, goals, 1, 128, reward_params=rp)
    want = SR.smooth(fields, valids, origins, SR.RES, np.arange(n), cells[0], cells[1], 64, 0.3, 0.05, 2, 200, reward_params=rp)
    return fields, valids, cells, want


def test_properties_on_32_random_worlds(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
    datas, origins, starts, goals = random_worlds()
    maps = [CostMap2D(d.copy(), SR.RES, o) for d, o in zip(datas, origins)]
    env = BatchedPlanEnv(maps, [np.stack([s, g]) for s, g in zip(starts, goals)], _env_params(), n_envs=32)
    rp = env.params.reward_provider_params
    fields = env.goal_field(clearance=SR.RES)
    want_f, valids, cells, want = random_want(datas, origins, starts, goals, rp)
    plane = fields.field.cpu().numpy()
    for k in range(32):
        assert (plane[k, :valids[k, 0], :valids[k, 1]] == want_f[k, :valids[k, 0], :valids[k, 1]]).all(), k
    rin, lin, st = fields.route_bound(1, 128)
    assert (st.cpu().numpy() == cells[2]).all()
    paths, lens, status = (t.cpu().numpy() for t in fields.smooth(rin, lin, entries=True, max_len=200))
    rin, lin = rin.cpu().numpy(), lin.cpu().numpy()
    routed = cells[2] == 0
    assert routed.sum() >= 24 and (status[routed] & ~SR.TOO_CLOSE == 0).all()      # a stride-1 route is never BLOCKED
    length = lambda a: np.hypot(np.diff(a[:, 0]), np.diff(a[:, 1])).sum()   # noqa: E731
    for k in np.nonzero(routed)[0]:
        p, q = paths[k, :lens[k]], rin[k, :lin[k]]
        cols = np.rint((p[:, 0] - origins[k, 0]) / SR.RES).astype(int)
        rows = np.rint((p[:, 1] - origins[k, 1]) / SR.RES).astype(int)
        assert (rows >= 0).all() and (rows < valids[k, 0]).all() and (cols >= 0).all() and (cols < valids[k, 1]).all()
        assert (plane[k][rows, cols] != GR.NONE).all(), k                           # every way point on a passable cell
        assert length(p) <= length(q) * (1 + 1e-12), k                              # the pull and the blends only shorten
        assert (p[0].view(np.uint64) == q[0].view(np.uint64)).all() and (p[-1].view(np.uint64) == q[-1].view(np.uint64)).all()
    # ... and against the restatement, at most one row in ten without its target_idx
    got = _raw(torch, env, fields.field, rin, lin, 200, entries=True)
    _check(got, want, rp, "32 random worlds", may_skip=3)

"""The weighted goal field's arithmetic (csrc/bcp_goal_cell.h: goal_relax_cell_cost, goal_cost_check_args, and the walk and the
route, unchanged, on weighted fields) as a stand-alone host program under AddressSanitizer and UBSan, bit for bit against the
contract restated in numpy / heapq (tests/goal_cost_ref.py).  tests/c_abi/goal_cost_main.cpp includes that header alone and
calls the very functions goal_field_kernel<.., kCost> calls; it reads every plane through a bounds-checked accessor and keeps
the map and the table in heap blocks of exactly their size.  The property the feature is for -- routes that keep to the
middle of free space -- is tested on the reference alone."""
import os

import numpy as np
import pytest

import host_program
import goal_cost_ref as CR
import goal_field_ref as GR
import goal_route_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bcp_goal_field_cost", "bcp_goal_field_cost_bound"]
ZERO = np.zeros(256, dtype=np.int64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "goal_cost_main.cpp")


def _run(exe, *args):
    return host_program.run(exe, args, "goal cost ok")


def _relax(exe, tmp_path, data, seeds, clearance_d2, table, valid=None, max_passes=0):
    """-> (field uint16 [rows, cols], sweeps, gave_up, reached) of the program"""
    data = np.asarray(data, dtype=np.uint8)
    rows, cols = data.shape
    valid = data.shape if valid is None else valid
    seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 2)
    path, out = str(tmp_path / "case.bin"), str(tmp_path / "field.bin")
    with open(path, "wb") as f:
        f.write(np.array([rows, cols, valid[0], valid[1], len(seeds), clearance_d2, max_passes, 0], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(data).tobytes())
        f.write(seeds.tobytes())
        f.write(np.asarray(table).astype(np.uint16).tobytes())
    words = _run(exe, "relax", path, out)[0].split()
    assert words[0::2] == ["sweeps", "gave_up", "reached", "lookups"]
    return np.fromfile(out, dtype=np.uint16).reshape(rows, cols), int(words[1]), int(words[3]), int(words[5])


def _table(**entries):
    t = ZERO.copy()
    for k, v in entries.items():
        t[int(k[1:])] = v
    return t


# ---- the rule -----------------------------------------------------------------------------------------------------------
def test_the_hand_case(program, tmp_path):
    data = np.array([[0, 7, 0, 9]], dtype=np.uint8)
    table = _table(c7=5, c9=3)
    want = [[0, 17, 29, 44]]
    assert CR.dijkstra(data, [(0, 0)], 0, table).tolist() == want
    assert CR.jacobi(data, [(0, 0)], 0, table)[0].tolist() == want
    got, _sweeps, gave_up, reached = _relax(program, tmp_path, data, [(0, 0)], 0, table)
    assert got.tolist() == want and gave_up == 0 and reached == 4


@pytest.mark.parametrize("clearance_d2", [0, 151])
@pytest.mark.parametrize("world", [0, 5, 17])
def test_zero_table_is_the_plain_field_on_the_worlds(program, tmp_path, world, clearance_d2):
    data, _origin, _res, goal, _start = GR.mini_world(world)
    want = GR.mini_field(world, clearance_d2)
    np.testing.assert_array_equal(CR.dijkstra(data, [goal], clearance_d2, ZERO), want)
    got, _sweeps, gave_up, reached = _relax(program, tmp_path, data, [goal], clearance_d2, ZERO)
    np.testing.assert_array_equal(got, want)
    assert gave_up == 0 and reached == (want != GR.NONE).sum()


def test_zero_table_is_the_plain_field_on_the_walls(program, tmp_path):
    for data in (GR.diagonal_wall(), GR.serpentine(33)):
        want = GR.dijkstra(data, [(0, 0)], 0)
        np.testing.assert_array_equal(CR.dijkstra(data, [(0, 0)], 0, ZERO), want)
        np.testing.assert_array_equal(CR.jacobi(data, [(0, 0)], 0, ZERO)[0], want)
        np.testing.assert_array_equal(_relax(program, tmp_path, data, [(0, 0)], 0, ZERO)[0], want)


@pytest.mark.parametrize("weight", [2, 8])
@pytest.mark.parametrize("world", [5, 9])
def test_dijkstra_equals_the_jacobi_fixed_point(program, tmp_path, world, weight):
    _data, _origin, _res, goal, start = GR.mini_world(world)
    cost = CR.inflated_world(world)
    want = CR.world_field(world, weight)
    got, passes, gave_up = CR.jacobi(cost, [goal], CR.CLEARANCE_D2, CR.cost_table(weight))
    np.testing.assert_array_equal(got, want)
    assert gave_up == 0 and 1 < passes < 183 * 183
    plain = GR.mini_field(world, CR.CLEARANCE_D2)
    assert ((want == GR.NONE) == (plain == GR.NONE)).all() and (want >= plain).all() and (want > plain).any()
    assert want[goal] == 0 and want[start] != GR.NONE and want[want != GR.NONE].max() < 6000     # far from saturation
    # ... and the program's in-place sweeps reach the same bytes
    field, _sweeps, gave_up, reached = _relax(program, tmp_path, cost, [goal], CR.CLEARANCE_D2, CR.cost_table(weight))
    np.testing.assert_array_equal(field, want)
    assert gave_up == 0 and reached == (want != GR.NONE).sum()


# ---- what the feature is for: on the reference alone ---------------------------------------------------------------------
@pytest.mark.parametrize("world", [5, 9])
def test_weighted_routes_keep_to_the_middle(world):
    """every interior route cell, leaving out the first and last three, lies more than 30 cells from the nearest lethal
    cell at weight 2 -- against 12.6 (just beyond sqrt(151)) on the plain field"""
    data, _origin, _res, _goal, start = GR.mini_world(world)
    plain = CR.min_clearance(data, CR.route_cells(GR.mini_field(world, CR.CLEARANCE_D2), start))
    weighted = CR.min_clearance(data, CR.route_cells(CR.world_field(world, 2), start))
    print("world", world, "smallest distance to a lethal cell: plain %.1f, weight 2 %.1f" % (plain, weighted))
    assert 12.2 < plain < 13.0
    assert weighted > 30.0


def test_a_costly_band_with_a_gap(program, tmp_path):
    data, table, seed, far = CR.banded(200)
    want = CR.dijkstra(data, [seed], 0, table)
    np.testing.assert_array_equal(_relax(program, tmp_path, data, [seed], 0, table)[0], want)
    cells = CR.route_cells(want, far)
    assert want[far] == 8 * 17 and (8, 4) in cells and not any(c == 4 and r < 8 for r, c in cells)      # through the gap
    assert want[4, 4] == 4 * 12 + 200                                                                 # entering the band costs
    data, table, seed, far = CR.banded(1)
    want = CR.dijkstra(data, [seed], 0, table)
    np.testing.assert_array_equal(_relax(program, tmp_path, data, [seed], 0, table)[0], want)
    assert want[far] == 8 * 12 + 1 and CR.route_cells(want, far) == [(4, c) for c in range(8, -1, -1)]    # straight
    # a seed on a costly cell: value 0, its own extra is never charged, leaving it costs the neighbour's
    data, table, seed, far = CR.banded(200)
    want = CR.dijkstra(data, [seed, (2, 4)], 0, table)
    got = _relax(program, tmp_path, data, [seed, (2, 4)], 0, table)[0]
    np.testing.assert_array_equal(got, want)
    assert got[2, 4] == 0 and got[2, 5] == 12 and got[1, 4] == 212 and got[far] == 2 * 17 + 2 * 12


# ---- shapes ------------------------------------------------------------------------------------------------------------
def test_padded_maps_show_nothing_of_the_padding(program, tmp_path):
    rng = np.random.RandomState(5)
    inner = np.where(rng.uniform(size=(40, 47)) < 0.2, 254, rng.randint(0, 100, size=(40, 47))).astype(np.uint8)
    valid = (36, 40)
    table = np.arange(256, dtype=np.int64) % 50
    table[200] = 4095
    seeds = [(20, 20), (38, 5), (-1, -1)]
    fields = []
    for junk in (200, 254, 0):
        data = inner.copy()
        data[:, 40:] = junk
        data[36:, :] = junk
        data[37, 41] = 254 if junk != 254 else 200
        for clearance_d2 in (0, 2):
            got = _relax(program, tmp_path, data, seeds, clearance_d2, table, valid=valid)[0]
            np.testing.assert_array_equal(got, CR.dijkstra(data, seeds, clearance_d2, table, valid=valid))
            assert (got[36:] == GR.NONE).all() and (got[:, 40:] == GR.NONE).all() and got[20, 20] == 0
            fields.append((clearance_d2, got))
    for clearance_d2, got in fields[2:]:
        np.testing.assert_array_equal(got, fields[clearance_d2 // 2][1])       # whatever the padding holds


def test_column_counts_31_to_65(program, tmp_path):
    rng = np.random.RandomState(6)
    table = (np.arange(256, dtype=np.int64) * 7) % 40
    for cols in range(31, 66):
        data = rng.randint(0, 253, size=(5, cols)).astype(np.uint8)
        data[1:4:2, 0] = 254
        data[0:5:3, cols - 1] = 254
        seeds = [(1, cols - 1)]
        got = _relax(program, tmp_path, data, seeds, 2, table)[0]
        np.testing.assert_array_equal(got, CR.dijkstra(data, seeds, 2, table))


def test_saturation_and_a_stuck_route(program, tmp_path):
    data = GR.serpentine(33)
    table = _table(c0=4095)
    want = CR.dijkstra(data, [(0, 0)], 0, table)
    got, _sweeps, gave_up, reached = _relax(program, tmp_path, data, [(0, 0)], 0, table)
    np.testing.assert_array_equal(got, want)
    assert gave_up == 0 and reached == 577 and (got == GR.FAR).sum() > 500 and got[got != GR.NONE].max() == GR.FAR
    assert got[0, 15] == 15 * (12 + 4095) and got[0, 16] == GR.FAR       # 16 * 4107 = 65 712: exactly FAR, never NONE
    # the route from the far end cannot descend a saturated stretch: STUCK, as the reference walk says
    far = (32, 32)
    assert got[far] == GR.FAR
    res = 0.05
    start, goal = [far[1] * res, far[0] * res, 0.0], [0.0, 0.0, 0.0]
    _wp, want_len, want_status, _init, _cells = RR.route_row(want, want.shape, (0.0, 0.0), res, start, goal, 1, 40, pure_pursuit=True)
    assert want_status & RR.STUCK
    path = str(tmp_path / "route.bin")
    with open(path, "wb") as f:
        f.write(np.array([33, 33, 1, 40], dtype=np.int32).tobytes())
        f.write(np.array([0.0, 0.0, res] + start + goal, dtype=np.float64).tobytes())
        f.write(got.tobytes())
    words = _run(program, "route", path)[0].split()
    assert words[0::2] == ["status", "len"] and int(words[1]) == want_status and int(words[3]) == want_len


def test_a_cap_that_ends_the_work(program, tmp_path):
    cost = CR.inflated_world(5)
    _data, _origin, _res, goal, _start = GR.mini_world(5)
    exact = CR.world_field(5, 8)
    capped, sweeps, gave_up, _reached = _relax(program, tmp_path, cost, [(182, 182), goal], CR.CLEARANCE_D2, CR.cost_table(8), max_passes=1)
    exact2 = CR.dijkstra(cost, [(182, 182), goal], CR.CLEARANCE_D2, CR.cost_table(8))
    assert sweeps == 1 and gave_up == 1
    assert (capped >= exact2).all() and (capped != exact2).any() and ((capped == GR.NONE) | (exact2 != GR.NONE)).all()
    assert (exact2 <= exact).all()
    ref, passes, ref_gave_up = CR.jacobi(cost, [goal], CR.CLEARANCE_D2, CR.cost_table(8), max_passes=20)
    assert passes == 20 and ref_gave_up == 1 and (ref >= exact).all() and (ref != exact).any()


def test_walk_steps_on_weighted_fields(program, tmp_path):
    rng = np.random.RandomState(3)
    for world, weight in ((5, 2), (9, 8)):
        field = CR.world_field(world, weight)
        cells = rng.randint(0, 183, size=(2000, 2)).astype(np.int32)
        path = str(tmp_path / "walk.bin")
        with open(path, "wb") as f:
            f.write(np.array([183, 183, 183, 183, len(cells), 0, 0, 0], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(field).tobytes())
            f.write(cells.tobytes())
        got = [int(ln) for ln in _run(program, "walk", path)[:len(cells)]]

        def look(r, c):
            return int(field[r, c]) if 0 <= r < 183 and 0 <= c < 183 else GR.NONE

        want = [RR.walk_step(look, int(r), int(c)) for r, c in cells]
        assert got == want and sum(k >= 0 for k in want) > 1000
        # the step is the true successor: from a cell with a value, the neighbour it names is strictly cheaper
        for (r, c), k in zip(cells, want):
            v = look(int(r), int(c))
            if v not in (GR.NONE, 0):
                assert k >= 0 and look(int(r) + GR.NBR[k][1], int(c) + GR.NBR[k][0]) < v


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_refusals_and_their_order(program, tmp_path):
    ok = (1, 4, 1, 1, 1, 183, 183, 1, 151, 0, 0, 0, 0)
    bad_everywhere = (0, -1, 0, 0, 0, 0, 0, 0, -1, -1, 1, 0, 1)
    table = [
        # the 13 arguments of the plain check, then the table: (-2,) none, (-1,) zeros, (i, value) -> (who refuses, number)
        (ok, (-1,), (0, 0)),
        (ok, (0, 4095), (0, 0)), (ok, (255, 4095), (0, 0)),
        ((1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0), (-1,), (0, 0)),            # n_maps == 0: nothing to point to
        (ok, (-2,), (2, 1)),
        (ok, (0, 4096), (2, 2)), (ok, (17, 65535), (2, 2)), (ok, (254, 4096), (2, 2)), (ok, (255, 4096), (2, 2)),
        ((1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0), (-2,), (2, 1)),            # the table is checked before n_maps == 0 returns
        ((0,) + ok[1:], (-2,), (1, 1)),                                      # the plain refusals come first, in their order
        ((1, -1) + ok[2:], (-2,), (1, 2)),
        (ok[:5] + (0, 183) + ok[7:], (3, 4096), (1, 3)),
        (ok[:7] + (0,) + ok[8:], (3, 4096), (1, 4)),
        (ok[:8] + (16130,) + ok[9:], (-2,), (1, 5)),
        (ok[:9] + (-1,) + ok[10:], (-2,), (1, 6)),
        (ok[:10] + (1, 0, 0), (-2,), (1, 7)),
        (ok[:10] + (1, 1, 1), (-2,), (1, 8)),
        ((1, 4, 0, 1, 1) + ok[5:], (-2,), (1, 9)),
        (bad_everywhere, (-2,), (1, 1)),
        ((1,) + bad_everywhere[1:], (-2,), (1, 2)),
    ]
    path = str(tmp_path / "args.txt")
    with open(path, "w") as f:
        for args, tab, _want in table:
            f.write(" ".join(str(a) for a in args + tab) + "\n")
    got = [tuple(int(w) for w in ln.split()) for ln in _run(program, "args", path)[:len(table)]]
    assert got == [want for _args, _tab, want in table]
    for args, tab, want in table:
        t = None if tab[0] == -2 else ZERO.copy()
        if tab[0] >= 0:
            t[tab[0]] = tab[1]
        assert CR.check_cost_args(GR.check_field_args(*args), t) == want


def test_cost_table():
    from bc_gym_planning_env_amd import _lib, goal_field
    assert _lib.GOAL_MAX_EXTRA == CR.MAX_EXTRA == 4095
    for w in (0, 2, 8, 341.25):
        t = goal_field.cost_table(w)
        assert t.dtype == np.uint16 and t.shape == (256,) and t.flags.c_contiguous
        np.testing.assert_array_equal(t, CR.cost_table(w))
        assert CR.check_cost_args(0, CR.cost_table(w)) == (0, 0)
    assert not goal_field.cost_table(0).any()
    t = goal_field.cost_table(2)
    assert t[252] == t[253] == 24 and t[254] == t[255] == 0 and t[0] == 0 and t[126] == 12 and t[21] == 2 and (np.diff(t[:253].astype(int)) >= 0).all()
    assert goal_field.cost_table(341.25)[252] == 4095                      # the largest weight: the last entry exactly
    above = 341.25 + 1.0 / 12.0                                            # one step of the last entry above it: 4096
    assert CR.cost_table(above)[252] == 4096 and CR.check_cost_args(0, CR.cost_table(above)) == (2, 2)
    for bad in (above, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            goal_field.cost_table(bad)
    with pytest.raises(ValueError):
        goal_field.checked_table(np.zeros(255))
    with pytest.raises(ValueError):
        goal_field.checked_table(np.full(256, 0.5))


def test_library_exports_the_two_symbols_and_lib_binds_them():
    import ctypes as C
    from bc_gym_planning_env_amd import _lib, build
    build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SYMBOLS, name
    lib = _lib.load()
    assert len(lib.bcp_goal_field_cost.argtypes) == 16 and len(lib.bcp_goal_field_cost_bound.argtypes) == 10
    assert lib.bcp_goal_field_cost.argtypes[:12] == lib.bcp_goal_field.argtypes[:12]
    assert lib.bcp_goal_field_cost_bound.argtypes[:6] == lib.bcp_goal_field_bound.argtypes[:6]
    assert _lib.ABI_VERSION == 2
    header = open(os.path.join(ROOT, "include", "bcplan.h")).read()
    assert "#define BCP_GOAL_MAX_EXTRA 4095" in header


def test_python_keywords_exist():
    import inspect
    from bc_gym_planning_env_amd import BatchedPlanEnv
    from bc_gym_planning_env_amd.goal_field import GoalField
    from bc_gym_planning_env_amd.ops import NativeOps
    assert list(inspect.signature(BatchedPlanEnv.goal_field).parameters)[1:] == [
        "clearance", "seeds", "max_passes", "follow_refresh", "cost_weight", "extra_of_cost"]
    assert "cost_weight" in inspect.signature(BatchedPlanEnv.route_paths).parameters
    assert inspect.signature(NativeOps.goal_field).parameters["extra_of_cost"].default is None
    assert inspect.signature(GoalField.__init__).parameters["extra_of_cost"].default is None

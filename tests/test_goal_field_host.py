"""The goal field's arithmetic (csrc/bcp_goal_cell.h: the pull relaxation of a cell, the widening of a mask word, the carrot
walk, the argument checks) as a stand-alone host program under AddressSanitizer and UBSan, bit for bit against the contract
restated in numpy / heapq (tests/goal_field_ref.py).  tests/c_abi/goal_field_main.cpp includes that header alone -- it has
no HIP in it -- and calls the very functions goal_field_kernel and goal_sample_kernel call; the program reads every plane
through a bounds-checked accessor, so a relaxation or a walk that left the map fails here, without a GPU."""
import os

import numpy as np
import pytest

import host_program
import goal_field_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bcp_goal_field", "bcp_goal_field_sample", "bcp_final_goal_field_sample"]
WORLDS = (0, 5, 17)
CLEARANCES = (0, 151)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "goal_field_main.cpp")


def _run(exe, *args):
    return host_program.run(exe, args, "goal field ok")


def _relax(exe, tmp_path, data, seeds, clearance_d2, valid=None, max_passes=0):
    """-> (field uint16 [rows, cols], sweeps, gave_up, reached) of the program"""
    rows, cols = data.shape
    valid = data.shape if valid is None else valid
    seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 2)
    path, out = str(tmp_path / "case.bin"), str(tmp_path / "field.bin")
    with open(path, "wb") as f:
        f.write(np.array([rows, cols, valid[0], valid[1], len(seeds), clearance_d2, max_passes, 0], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(data, dtype=np.uint8).tobytes())
        f.write(seeds.tobytes())
    words = _run(exe, "relax", path, out)[0].split()
    assert words[0::2] == ["sweeps", "gave_up", "reached"]
    return np.fromfile(out, dtype=np.uint16).reshape(rows, cols), int(words[1]), int(words[3]), int(words[5])


@pytest.mark.parametrize("clearance_d2", CLEARANCES)
@pytest.mark.parametrize("world", WORLDS)
def test_dijkstra_equals_the_jacobi_fixed_point(world, clearance_d2):
    data, _origin, _res, goal, start = GR.mini_world(world)
    want = GR.mini_field(world, clearance_d2)
    got, passes, gave_up = GR.jacobi(data, [goal], clearance_d2)
    np.testing.assert_array_equal(got, want)
    assert gave_up == 0 and 1 < passes <= 199
    assert want[goal] == 0 and want[start] != GR.NONE and want.max() == GR.NONE
    assert want[want != GR.NONE].max() <= 2914


@pytest.mark.parametrize("clearance_d2", CLEARANCES)
@pytest.mark.parametrize("world", WORLDS)
def test_relaxation_reaches_the_fixed_point_bit_for_bit(program, tmp_path, world, clearance_d2):
    data, _origin, _res, goal, _start = GR.mini_world(world)
    want = GR.mini_field(world, clearance_d2)
    got, sweeps, gave_up, reached = _relax(program, tmp_path, data, [goal], clearance_d2)
    np.testing.assert_array_equal(got, want)
    assert gave_up == 0 and reached == (want != GR.NONE).sum() and sweeps >= 2


def test_nothing_leaks_through_a_diagonal_wall(program, tmp_path):
    data = GR.diagonal_wall(9)
    want = GR.dijkstra(data, [(0, 0)], 0)
    got, _sweeps, gave_up, reached = _relax(program, tmp_path, data, [(0, 0)], 0)
    np.testing.assert_array_equal(got, want)
    rr, cc = np.indices(data.shape)
    far_side = rr + cc >= 8        # the wall itself and everything beyond it
    assert (got[far_side] == GR.NONE).all() and (got[~far_side] != GR.NONE).all() and gave_up == 0
    assert reached == 36 and got[0, 7] == 7 * 12 and got[3, 3] == 3 * 17


def test_serpentine_and_the_cap(program, tmp_path):
    data = GR.serpentine(33)
    want = GR.dijkstra(data, [(0, 0)], 0)
    got, _sweeps, gave_up, reached = _relax(program, tmp_path, data, [(0, 0)], 0)
    np.testing.assert_array_equal(got, want)
    assert reached == 577 and gave_up == 0 and got.max() == GR.NONE and got[32, 32 if 16 % 2 == 0 else 0] == 576 * 12
    # a cap that ends the work: every value is NONE or the length of some route, i.e. an upper bound (sweeps that run
    # against the corridor's direction gain one cell each)
    capped, sweeps, gave_up, _reached = _relax(program, tmp_path, data, [(32, 32)], 0, max_passes=5)
    exact = GR.dijkstra(data, [(32, 32)], 0)
    assert sweeps == 5 and gave_up == 1
    assert (capped >= exact).all() and (capped != exact).any()
    assert ((capped == GR.NONE) | (exact != GR.NONE)).all()


def test_ragged_shapes_clearances_and_seeds(program, tmp_path):
    rng = np.random.RandomState(5)
    for cols in (31, 32, 33, 63, 64, 65):
        data = np.zeros((7, cols), dtype=np.uint8)
        data[1:6:2, 0] = 254
        data[0:7:3, cols - 1] = 254
        seeds = [(1, cols - 1)]
        for clearance_d2 in (0, 2, 9):
            got = _relax(program, tmp_path, data, seeds, clearance_d2)[0]
            np.testing.assert_array_equal(got, GR.dijkstra(data, seeds, clearance_d2))
    data = np.where(rng.uniform(size=(40, 47)) < 0.2, 254, 0).astype(np.uint8)
    data[:, 40:] = 254          # (the padding's 254s are not obstacles)
    valid = (36, 40)
    blocked_seed = tuple(np.argwhere(data[:36, :40] == 254)[3])
    seeds = [blocked_seed, (38, 5), (-1, -1)]
    for clearance_d2 in (0, 1, 2, 9):
        got = _relax(program, tmp_path, data, seeds, clearance_d2, valid=valid)[0]
        want = GR.dijkstra(data, seeds, clearance_d2, valid=valid)
        np.testing.assert_array_equal(got, want)
        assert got[blocked_seed] == 0 and (got[36:] == GR.NONE).all() and (got[:, 40:] == GR.NONE).all()
    assert (_relax(program, tmp_path, data, [(38, 5), (-1, -1)], 0, valid=valid)[0] == GR.NONE).all()   # no usable seed
    # a large clearance: half-widths beyond a word
    data = np.zeros((90, 100), dtype=np.uint8)
    data[45, 50] = data[0, 99] = 254
    got = _relax(program, tmp_path, data, [(89, 0)], 40 * 40 + 3)[0]
    np.testing.assert_array_equal(got, GR.dijkstra(data, [(89, 0)], 40 * 40 + 3))


def _sample(exe, tmp_path, field, valid, origin, resolution, poses, carrot_cells, max_dist):
    rows, cols = field.shape
    with np.errstate(all="ignore"):
        cs = np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1)
    path = str(tmp_path / "sample.bin")
    with open(path, "wb") as f:
        f.write(np.array([rows, cols, valid[0], valid[1], len(poses), carrot_cells, 0, 0], dtype=np.int32).tobytes())
        f.write(np.array([origin[0], origin[1], resolution, max_dist], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(field, dtype=np.uint16).tobytes())
        f.write(np.concatenate([poses, cs], axis=1).tobytes())
    lines = [ln.split() for ln in _run(exe, "sample", path)[:len(poses)]]
    got3 = np.array([[int(w, 16) for w in ln[:3]] for ln in lines], dtype=np.uint32).view(np.float32)
    got_v = np.array([int(ln[3]) for ln in lines], dtype=np.int32)
    got_c = np.array([[int(ln[4]), int(ln[5])] for ln in lines], dtype=np.int32)
    want3, want_v, want_c = GR.sample(field[None], [valid], [origin], resolution, np.zeros(len(poses), dtype=np.int64), poses, cs,
                                      carrot_cells, max_dist)
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got3.view(np.uint32), want3.view(np.uint32))
    return got3, got_v, got_c


def test_walks_and_directions_bit_for_bit(program, tmp_path):
    data, origin, res, goal, _start = GR.mini_world(5)
    field = GR.mini_field(5, 151)
    poses = GR.edge_poses(np.random.RandomState(11), 2000, field, origin, res, goal)
    for carrot_cells, max_dist in ((1, np.inf), (8, 10.0), (256, 2.0)):
        out3, value, carrot = _sample(program, tmp_path, field, field.shape, origin, res, poses, carrot_cells, max_dist)
        has = value != GR.NONE
        assert has.sum() > 1000 and (~has).sum() > 100
        assert (out3[~has] == np.float32([max_dist, 0, 0])).all() and (carrot[~has] == -1).all()
        assert value[0] == 0 and (carrot[0] == goal).all() and (out3[0] == 0).all()          # on the seed: no walk
        assert (value[2:42] == GR.NONE).all() and (value[132:137] == GR.NONE).all() and value[138] == GR.NONE
        moved = has & (value != 0)
        norm = np.hypot(out3[moved, 1].astype(np.float64), out3[moved, 2].astype(np.float64))
        assert np.abs(norm - 1).max() < 1e-6
        # the walk descends the field: min over the admissible neighbours equals the cell's own value, step by step
        reached = field[carrot[moved, 0], carrot[moved, 1]].astype(np.int64)
        assert (reached < value[moved]).all()
        assert (out3[:, 0] <= np.float32(max_dist)).all()
        if carrot_cells == 256:
            assert (reached[value[moved] <= 256 * 12] == 0).all()       # every step gains at least 12
    # a valid shape smaller than the plane: the cells beyond it are never read as values
    sub = (100, 120)
    cut = field.copy()
    cut[sub[0]:, :] = 7
    cut[:, sub[1]:] = 7
    _out3, value, _carrot = _sample(program, tmp_path, cut, sub, origin, res, poses, 8, np.inf)
    cells = np.rint((poses[:, :2] - origin) / res)
    with np.errstate(invalid="ignore"):
        outside = ~((cells[:, 0] >= 0) & (cells[:, 0] < sub[1]) & (cells[:, 1] >= 0) & (cells[:, 1] < sub[0]))
    assert (value[outside] == GR.NONE).all()


def test_argument_checks(program, tmp_path):
    ok = (1, 4, 1, 1, 1, 183, 183, 1, 151, 0, 0, 0, 0)
    table = [
        # handle n_maps data seeds out rows cols n_seeds clearance_d2 max_passes valid_rows valid_cols shared -> refusal
        (ok, 0),
        ((1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0), 0),            # n_maps == 0: nothing to point to
        ((1, 4, 1, 1, 1, 2048, 2048, 4096, 16129, 7, 1, 1, 0), 0),
        ((1, 4, 1, 1, 1, 10, 10, 1, 0, 0, 0, 0, 1), 0),
        ((0,) + ok[1:], 1),
        ((1, -1) + ok[2:], 2),
        (ok[:5] + (0, 183) + ok[7:], 3), (ok[:5] + (183, 0) + ok[7:], 3),
        (ok[:5] + (2049, 183) + ok[7:], 3), (ok[:5] + (183, 2049) + ok[7:], 3),
        (ok[:7] + (0,) + ok[8:], 4), (ok[:7] + (4097,) + ok[8:], 4),
        (ok[:8] + (-1,) + ok[9:], 5), (ok[:8] + (16130,) + ok[9:], 5),
        (ok[:9] + (-1,) + ok[10:], 6),
        (ok[:10] + (1, 0, 0), 7), (ok[:10] + (0, 1, 0), 7),
        (ok[:10] + (1, 1, 1), 8),
        ((1, 4, 0, 1, 1) + ok[5:], 9), ((1, 4, 1, 0, 1) + ok[5:], 9), ((1, 4, 1, 1, 0) + ok[5:], 9),
        ((0, -1, 0, 0, 0, 0, 0, 0, -1, -1, 1, 0, 1), 1),          # the order: handle, maps, shape, seeds, ...
        ((1, -1, 0, 0, 0, 0, 0, 0, -1, -1, 1, 0, 1), 2),
        ((1, 1, 0, 0, 0, 0, 0, 0, -1, -1, 1, 0, 1), 3),
        ((1, 1, 0, 0, 0, 5, 5, 0, -1, -1, 1, 0, 1), 4),
        ((1, 1, 0, 0, 0, 5, 5, 1, -1, -1, 1, 0, 1), 5),
        ((1, 1, 0, 0, 0, 5, 5, 1, 0, -1, 1, 0, 1), 6),
        ((1, 1, 0, 0, 0, 5, 5, 1, 0, 0, 1, 0, 1), 7),
        ((1, 1, 0, 0, 0, 5, 5, 1, 0, 0, 1, 1, 1), 8),
        ((1, 1, 0, 0, 0, 5, 5, 1, 0, 0, 0, 0, 1), 9),
    ]
    path = str(tmp_path / "args.txt")
    with open(path, "w") as f:
        for args, _want in table:
            f.write(" ".join(str(a) for a in args) + "\n")
    got = [int(ln) for ln in _run(program, "args", path)[:len(table)]]
    assert got == [want for _args, want in table]
    assert [GR.check_field_args(*args) for args, _want in table] == got

    inf, nan = float("inf"), float("nan")
    ok = (1, 1, 1, 8, 10.0, 16, 16, 0, 0, 0, 183, 183, 183, 183, 1, 16)
    table = [
        # handle field out3 carrot max_dist n n_envs poses row_env final rows cols map_rows map_cols n_fields n_entries
        (ok, 0),
        (ok[:3] + (1, inf, 40, 16, 1, 1, 0) + ok[10:14] + (16, 16), 0),
        (ok[:3] + (256, 1e-300, 0, 16, 0, 0, 1) + ok[10:], 0),     # the final form: n is the record's
        (ok[:10] + (5, 5, 0, 0, 3, 0), 0),                          # no costmaps bound yet: that refusal is the caller's
        ((0,) + ok[1:], 1), ((1, 0) + ok[2:], 1), ((1, 1, 0) + ok[3:], 1),
        (ok[:3] + (0,) + ok[4:], 2), (ok[:3] + (257,) + ok[4:], 2),
        (ok[:4] + (0.0,) + ok[5:], 3), (ok[:4] + (-1.0,) + ok[5:], 3), (ok[:4] + (nan,) + ok[5:], 3), (ok[:4] + (-inf,) + ok[5:], 3),
        (ok[:5] + (0, 16, 1) + ok[8:], 4), (ok[:5] + (15, 16, 0) + ok[8:], 4), (ok[:5] + (-2, 16, 1) + ok[8:], 4),
        (ok[:7] + (0, 1) + ok[9:], 5),
        (ok[:10] + (183, 182) + ok[12:], 6), (ok[:10] + (184, 183) + ok[12:], 6),
        (ok[:14] + (0, 16), 7), (ok[:14] + (2, 16), 7), (ok[:14] + (17, 16), 7),
    ]
    path = str(tmp_path / "sargs.txt")
    with open(path, "w") as f:
        for args, _want in table:
            f.write(" ".join(float(a).hex() if isinstance(a, float) and np.isfinite(a) else str(a) for a in args) + "\n")
    got = [int(ln) for ln in _run(program, "sargs", path)[:len(table)]]
    assert got == [want for _args, want in table]
    assert [GR.check_sample_args(*args) for args, _want in table] == got


def test_widening_of_a_mask_word():
    """goal_widen_word restated: the dilation of a bit row by a half-width, word by word, against numpy's on the bits --
    through the program's relaxation it is only ever seen with the few half-widths of a test's clearance"""
    rng = np.random.RandomState(2)
    cols = 150
    for hw in (0, 1, 5, 31, 32, 33, 64, 127):
        row = rng.uniform(size=cols) < 0.03
        want = np.zeros(cols, dtype=bool)
        for c in np.nonzero(row)[0]:
            want[max(c - hw, 0):c + hw + 1] = True
        # a one-row map with clearance hw^2: blocked = the widened row
        data = (row * np.uint8(254)).astype(np.uint8)[None]
        free = GR.free_mask(data, [], hw * hw)
        np.testing.assert_array_equal(~free[0], want)


def test_library_exports_the_goal_field_symbols_and_lib_binds_them():
    import ctypes as C
    from bc_gym_planning_env_amd import _lib, build, robots
    build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SYMBOLS, name
    lib = _lib.load()
    assert len(lib.bcp_goal_field.argtypes) == 15 and len(lib.bcp_goal_field_sample.argtypes) == 14
    assert len(lib.bcp_final_goal_field_sample.argtypes) == 11
    assert lib.bcp_goal_field.argtypes[2] is C.c_int64 and lib.bcp_goal_field_sample.argtypes[8:10] == [C.c_int32, C.c_double]
    assert (_lib.GOAL_ORTHO, _lib.GOAL_DIAG, _lib.GOAL_FAR, _lib.GOAL_NONE, _lib.TUNE_GOAL_ROUTE) == (12, 17, 65534, 65535, 12)
    assert _lib.ABI_VERSION == 2
    # the tricycle's inscribed radius at 3 cm: clearance_d2 = 151
    radius = robots.inscribed_radius(robots.get_footprint(robots.INDUSTRIAL_TRICYCLE_V1))
    assert int(np.floor((np.float64(radius) / np.float64(0.03)) ** 2)) == 151

"""The box sampler's rule (csrc/bcp_boxes_cell.h: box_candidate, box_runs, box_accepted, scatter_entry and scatter_check_args,
with bcp_philox.h and bcp_outline.h) as a stand-alone host program under AddressSanitizer and UBSan, against the contract
restated in numpy (tests/scatter_boxes_ref.py, the fill by oracle.fill_poly).  tests/c_abi/scatter_boxes_main.cpp includes
that header alone -- it has no HIP in it -- and calls the very functions scatter_boxes_kernel calls; every array is a heap
block of exactly its stated size and every cell is written through a sink that refuses one outside the valid shape, so a
run that left the map fails here, without a GPU.  Everything is compared byte for byte: maps, boxes and counts."""
import os

import numpy as np
import pytest

import host_program
import scatter_boxes_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "scatter_boxes_main.cpp")


def _run(exe, *args):
    return host_program.run(exe, args, "scatter boxes ok")


def _scatter(exe, tmp_path, data, valid, origins, resolution, frame, keep, yaw_cs, n_boxes, max_attempts, seed, along, half_size,
             first_entry=0, want=None):
    """runs the program and the reference on the same batch, compares every byte -> (maps, boxes, counts)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n, rows, cols = data.shape
    valid = np.tile([rows, cols], (n, 1)) if valid is None else np.asarray(valid)
    keep = np.zeros((n, 0, 3), dtype=np.int32) if keep is None else np.asarray(keep, dtype=np.int32)
    yaw_cs = np.asarray(yaw_cs, dtype=np.float64)
    n_yaws, n_keep = len(yaw_cs), keep.shape[1]
    path, out = str(tmp_path / "case.bin"), str(tmp_path / "case.out")
    with open(path, "wb") as f:
        f.write(np.array([n, rows, cols, n_boxes, max_attempts, n_yaws, n_keep, 0], dtype=np.int32).tobytes())
        f.write(np.array([seed, first_entry], dtype=np.uint64).tobytes())
        f.write(np.array([resolution, along[0], along[1], half_size[0], half_size[1]], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(valid, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(origins, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(frame, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(keep, dtype=np.int32).tobytes())
        f.write(yaw_cs.tobytes())
        f.write(data.tobytes())
    _run(exe, "scatter", path, out)
    raw = np.fromfile(out, dtype=np.uint8)
    n_d, n_b = data.size, n * n_boxes * SR.WORDS * 4
    assert len(raw) == n_d + n_b + 4 * n
    maps = raw[:n_d].reshape(data.shape)
    boxes = raw[n_d:n_d + n_b].view(np.int32).reshape(n, n_boxes, SR.WORDS)
    counts = raw[n_d + n_b:].view(np.int32)
    if want is None:
        want = SR.scatter(data, valid, origins, resolution, n_boxes, max_attempts, n_yaws, seed, along, half_size, frame, keep,
                          yaw_cs, first_entry)
    assert (counts == want[2]).all(), (counts, want[2])
    assert (boxes == want[1]).all()
    assert (maps == want[0]).all()
    changed = maps != data
    assert (maps[changed] == SR.LETHAL).all()
    return maps, boxes, counts


def small_batch(n=5, side=9, seed=3):
    """n maps of side x side at 1 m with a wall each, frames along the diagonal"""
    rng = np.random.RandomState(seed)
    data = np.zeros((n, side, side), dtype=np.uint8)
    for i in range(n):
        data[i, rng.randint(side), :] = SR.LETHAL
    origins = rng.uniform(-1.0, 1.0, (n, 2))
    starts = origins + rng.uniform(0.0, 1.5, (n, 2))
    goals = origins + side - 1 - rng.uniform(0.0, 1.5, (n, 2))
    return data, origins, SR.frames(starts, goals, 2.5), starts, goals


def test_philox_against_the_published_vectors(program):
    lines = _run(program, "philox")
    assert lines[0] == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert lines[1] == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    zero = SR.philox4x32_10(np.zeros(4, dtype=np.uint32), (0, 0))
    ones = SR.philox4x32_10(np.full(4, 0xFFFFFFFF, dtype=np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))
    assert " ".join("%08x" % w for w in zero) == lines[0] and " ".join("%08x" % w for w in ones) == lines[1]


def test_the_golden_worlds_dense(program, tmp_path):
    maps, origins, res, _starts, _goals = SR.golden()
    want_maps, want_boxes, want_counts, frame, keep, yaw_cs = SR.dense_golden()
    assert len(maps) == 48
    d = SR.DENSE
    _scatter(program, tmp_path, maps, None, origins, res, frame, keep, yaw_cs, d["n_boxes"], d["max_attempts"], d["seed"],
             d["along"], d["half_size"], want=(want_maps, want_boxes, want_counts))
    assert want_counts.min() < d["n_boxes"] and want_counts.max() > 0
    # every kind of verdict occurs: the comparison above covers both rejections
    seen = set()
    for k in range(48):
        seen |= set(SR.scatter_entry(maps[k], maps[k].shape, origins[k], res, k, frame=frame[k], keep=keep[k], yaw_cs=yaw_cs,
                                     **d)[3])
        if seen == {"ok", "out", "keep"}:
            break
    assert seen == {"ok", "out", "keep"}


@pytest.mark.parametrize("max_attempts", [1, 31, 256, 257])
def test_nine_by_nine(program, tmp_path, max_attempts):
    data, origins, frame, starts, goals = small_batch()
    keep = SR.keep_outs(starts, goals, origins, 1.0, 1)
    _maps, _boxes, counts = _scatter(program, tmp_path, data, None, origins, 1.0, frame, keep, SR.yaw_table(16), 64, max_attempts,
                                     11, (0.1, 0.9), (0.3, 1.6))
    assert (counts <= min(max_attempts, 64)).all() and counts.max() >= 1
    if max_attempts == 257:   # beyond the chunk boundary, more boxes wanted than the attempts yield or exactly as many
        assert counts.max() == 64


def test_the_attempt_behind_the_chunk_boundary_counts(program, tmp_path):
    """n_boxes so large that attempt 256 is the one that fills the last slot of some entry, or is needed at all"""
    data, origins, frame, starts, goals = small_batch(n=24, seed=5)
    keep = SR.keep_outs(starts, goals, origins, 1.0, 14)   # (most attempts are rejected: the counts stay low)
    args = (data, None, origins, 1.0, frame, keep, SR.yaw_table(16), 64)
    _m, b256, c256 = _scatter(program, tmp_path, *args, 256, 11, (0.0, 1.0), (0.3, 1.0))
    _m, b257, c257 = _scatter(program, tmp_path, *args, 257, 11, (0.0, 1.0), (0.3, 1.0))
    assert (c256 < 64).all()
    grew = c257 > c256
    assert grew.any() and (b257[grew, c257[grew] - 1, 0] == 256).all()


def test_padded_entries_and_the_last_valid_row_and_column(program, tmp_path):
    """half sizes 0 and a frame without extent: attempt 0 is the single cell of the anchor"""
    rows, cols = 12, 14
    valid = np.array([[12, 14], [7, 9], [10, 5]])
    origins = np.array([[0.5, -0.25], [0.0, 0.0], [-3.0, 2.0]])
    data = np.full((3, rows, cols), 77, dtype=np.uint8)   # (the padding holds a sentinel that must survive)
    for i, (vr, vc) in enumerate(valid):
        data[i, :vr, :vc] = 0
    res = 0.5

    def anchors(dr, dc):
        f = np.zeros((3, 6))
        f[:, 0] = origins[:, 0] + (valid[:, 1] - 1 + dc) * res
        f[:, 1] = origins[:, 1] + (valid[:, 0] - 1 + dr) * res
        return f

    yaw = SR.yaw_table(4)
    maps, boxes, counts = _scatter(program, tmp_path, data, valid, origins, res, anchors(0, 0), None, yaw, 2, 1, 1, (0, 1), (0, 0))
    assert list(counts) == [1, 1, 1]
    for i, (vr, vc) in enumerate(valid):
        assert list(boxes[i, 0]) == [0] + [vc - 1, vr - 1] * 4
        assert maps[i, vr - 1, vc - 1] == SR.LETHAL and (maps[i] != data[i]).sum() == 1
    for dr, dc in ((1, 0), (0, 1)):
        maps, boxes, counts = _scatter(program, tmp_path, data, valid, origins, res, anchors(dr, dc), None, yaw, 2, 1, 1, (0, 1),
                                       (0, 0))
        assert list(counts) == [0, 0, 0] and (maps == data).all() and (boxes == 0).all()
    # boxes with extent on the padded entries: everything stays inside the valid shapes
    frame = SR.frames(origins + 0.5, origins + (valid[:, ::-1] - 2) * res, 1.5)
    maps, _b, counts = _scatter(program, tmp_path, data, valid, origins, res, frame, None, SR.yaw_table(16), 6, 40, 2, (0, 1),
                                (0.2, 1.2))
    assert counts.min() >= 1
    for i, (vr, vc) in enumerate(valid):
        assert (maps[i, vr:] == 77).all() and (maps[i, :, vc:] == 77).all()


def test_degenerate_boxes_a_pixel_and_lines(program, tmp_path):
    data, origins, frame, _s, _g = small_batch(n=4, seed=9)
    # half sizes below half a cell: pixels, lines of two cells and squares of four, as the rounding falls
    _maps, boxes, counts = _scatter(program, tmp_path, data, None, origins, 1.0, frame, None, SR.yaw_table(16), 40, 60, 5, (0, 1),
                                    (0.0, 0.7))
    kinds = set()
    for i in range(4):
        for b in boxes[i, :counts[i]]:
            v = b[1:].reshape(4, 2)
            kinds.add((len(set(v[:, 0])), len(set(v[:, 1]))))
    assert (1, 1) in kinds and ((1, 2) in kinds or (2, 1) in kinds)
    # half sizes of exactly 0: one cell per box
    maps, boxes, counts = _scatter(program, tmp_path, data, None, origins, 1.0, frame, None, SR.yaw_table(16), 5, 60, 5, (0, 1),
                                   (0.0, 0.0))
    assert (counts == 5).all() and ((maps != data).sum(axis=(1, 2)) <= 5).all()
    assert (boxes[:, :, 1:3] == boxes[:, :, 7:9]).all()


def test_keep_outs_on_the_boundary_and_unused_slots(program, tmp_path):
    origins = np.zeros((1, 2))
    data = np.zeros((1, 20, 20), dtype=np.uint8)
    frame = np.zeros((1, 6))
    frame[0, :2] = [12.0, 9.0]   # the cell (row 9, col 12)
    yaw = SR.yaw_table(1)

    def one(keep):
        return _scatter(program, tmp_path, data, None, origins, 1.0, frame, np.array([keep], dtype=np.int32), yaw, 1, 1, 0, (0, 1),
                        (0, 0))[2][0]

    d2 = 3 * 3 + 4 * 4                               # keep-out at (row 6, col 8): distance squared exactly 25
    assert one([[6, 8, d2]]) == 0                    # at distance d2: rejected
    assert one([[6, 8, d2 - 1]]) == 1                # at distance d2 + 1 of a keep-out one smaller: accepted
    assert one([[6, 8, -1]]) == 1                    # an unused slot
    assert one([[9, 12, -5], [6, 8, d2 - 1], [9, 12, -1]]) == 1
    assert one([[9, 12, -5], [6, 8, d2 - 1], [9, 12, 0]]) == 0
    assert one([[-300000, 70000, 5], [2000000000, -2000000000, 2000000000]]) == 1   # far keep-outs: no overflow
    # a box with extent: the nearest cell of a run decides, not its ends
    frame[0, 2:] = [0.0, 0.0, 0.0, 0.0]
    wide = lambda keep: _scatter(program, tmp_path, data, None, origins, 1.0, frame, np.array([keep], dtype=np.int32), yaw, 1, 1, 0,
                                 (0, 1), (3.0, 3.0))[2][0]
    # (rows 6 .. 12, columns 9 .. 15)
    assert wide([[2, 12, 15]]) == 1 and wide([[2, 12, 16]]) == 0 and wide([[1, 12, 24]]) == 1 and wide([[1, 12, 25]]) == 0
    assert wide([[3, 18, 17]]) == 1 and wide([[3, 18, 18]]) == 0 and wide([[9, 12, 0]]) == 0


def test_one_yaw_a_high_seed_word_and_entries_beyond_32_bits(program, tmp_path):
    data, origins, frame, starts, goals = small_batch(n=3, seed=21)
    keep = SR.keep_outs(starts, goals, origins, 1.0, 2)
    tilted = np.array([[np.cos(0.4), np.sin(0.4)]])
    base = _scatter(program, tmp_path, data, None, origins, 1.0, frame, keep, tilted, 8, 32, 7, (0.1, 0.9), (0.3, 1.6))
    high = _scatter(program, tmp_path, data, None, origins, 1.0, frame, keep, tilted, 8, 32, 7 + (5 << 32), (0.1, 0.9), (0.3, 1.6))
    assert not (base[1] == high[1]).all()
    far = _scatter(program, tmp_path, data, None, origins, 1.0, frame, keep, tilted, 8, 32, 7, (0.1, 0.9), (0.3, 1.6),
                   first_entry=(3 << 32) + 1)
    assert not (base[1] == far[1]).all()
    full = _scatter(program, tmp_path, data, None, origins, 1.0, frame, keep, SR.yaw_table(4096), 8, 32, 2 ** 64 - 1, (0.1, 0.9),
                    (0.3, 1.6))
    assert full[2].max() >= 1


def test_argument_checks_and_their_order(program, tmp_path):
    ok = (1, 1, 48, 183, 183, 0.03, 12, 32, 16, 2, 0.2, 0.8, 0.2, 0.5, 1, 1, 1, 1)
    nan, inf = float("nan"), float("inf")

    def put(i, v, base=ok):
        return base[:i] + (v,) + base[i + 1:]

    table = [
        (ok, 0), (put(2, 0), 0), (put(9, 0, put(17, 0)), 0), (put(14, 0, put(15, 0)), 0),
        (put(3, 2048, put(4, 1, put(13, 0.0, put(12, 0.0)))), 12),    # a map of one column holds no box at all ...
        (put(3, 2048, put(4, 3, put(13, 0.0, put(12, 0.0)))), 0),     # ... one of three columns holds a cell
        (put(0, 0), 1), (put(1, 0), 2), (put(2, -1), 3),
        (put(3, 0), 4), (put(3, 2049), 4), (put(4, 0), 4), (put(4, 2049), 4),
        (put(5, 0.0), 5), (put(5, -1.0), 5), (put(5, nan), 5), (put(5, inf), 5),
        (put(6, 0), 6), (put(6, 65), 6), (put(7, 0), 7), (put(7, 4097), 7), (put(8, 0), 8), (put(8, 4097), 8),
        (put(9, -1), 9), (put(9, 17), 9),
        (put(10, 0.9), 10), (put(10, nan), 10), (put(11, inf), 10),
        (put(12, -0.1), 11), (put(12, 0.6), 11), (put(13, nan), 11), (put(13, inf), 11), (put(12, nan), 11),
        (put(13, 1.36), 12), (put(13, 1.35), 0), (put(3, 60), 12), (put(4, 68), 12), (put(4, 69), 0),
        (put(14, 0), 13), (put(15, 0), 13),
        (put(16, 0), 14), (put(17, 0), 14), (put(16, 0, put(2, 0)), 0),
        # the order: everything wrong at once, then one fewer each time
        ((0, 0, -1, 0, 0, 0.0, 0, 0, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 1),
        ((1, 0, -1, 0, 0, 0.0, 0, 0, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 2),
        ((1, 1, -1, 0, 0, 0.0, 0, 0, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 3),
        ((1, 1, 5, 0, 0, 0.0, 0, 0, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 4),
        ((1, 1, 5, 50, 50, 0.0, 0, 0, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 5),
        ((1, 1, 5, 50, 50, 0.1, 0, 0, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 6),
        ((1, 1, 5, 50, 50, 0.1, 1, 0, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 7),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 0, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 8),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, -1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 9),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, 1, 1.0, 0.0, -1.0, 9.0, 1, 0, 0, 0), 10),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, 1, 0.0, 1.0, -1.0, 9.0, 1, 0, 0, 0), 11),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, 1, 0.0, 1.0, 1.0, 9.0, 1, 0, 0, 0), 12),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, 1, 0.0, 1.0, 1.0, 1.0, 1, 0, 0, 0), 13),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, 1, 0.0, 1.0, 1.0, 1.0, 1, 1, 0, 0), 14),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, 1, 0.0, 1.0, 1.0, 1.0, 1, 1, 1, 0), 14),
        ((1, 1, 5, 50, 50, 0.1, 1, 1, 1, 1, 0.0, 1.0, 1.0, 1.0, 1, 1, 1, 1), 0),
    ]
    path = str(tmp_path / "args.txt")
    with open(path, "w") as f:
        for args, _want in table:
            f.write(" ".join(repr(a) for a in args) + "\n")
    got = [int(ln) for ln in _run(program, "args", path)[:len(table)]]
    assert [SR.check_args(*args) for args, _want in table] == [want for _args, want in table]
    assert got == [want for _args, want in table]


def test_header_library_and_binding_agree_and_the_abi_stays():
    import ctypes as C
    from bc_gym_planning_env_amd import _lib, build
    build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "bcplan.h")).read()
    assert hasattr(raw, "bcp_scatter_boxes") and "bcp_scatter_boxes" in _lib.SYMBOLS
    assert "int bcp_scatter_boxes(bcp_handle *h" in header and "typedef struct bcp_scatter_params" in header
    lib = _lib.load()
    args = lib.bcp_scatter_boxes.argtypes
    assert len(args) == 17 and args[2] is C.c_int64 and args[8] is C.c_double and args[12] is C.c_int32
    assert C.sizeof(_lib.BcpScatterParams) == 56
    assert (_lib.SCATTER_SHORT, _lib.SCATTER_REVERTED) == (SR.SHORT, SR.REVERTED) == (1, 2)
    assert _lib.ABI_VERSION == 2 and raw.bcp_abi_version() == 2
    assert "#define BCP_ABI_VERSION 2" in header.replace("  ", " ")

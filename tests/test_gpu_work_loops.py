"""The work loops: kernels whose host side caps the grid and whose device side loops over what is left, at batches large enough
to take the loop a second time.  Every other GPU module stays below these caps (at most 192 images, 16 maps, 26 000 rays, a few
dozen pool entries), so there a wave or a workgroup draws exactly one item; bench.py runs the second trips at 65 536 envs but
compares nothing.

Sizes are derived, not guessed.  A CU holds at most 32 waves, so 32 * CU bounds the resident waves of any kernel, and with them
gridDim.x * waves of every launch_persistent grid whatever the occupancy API answers:
  N_MID = 3 * 32 * CU + 37    every wave draws at least 3 images (k = 0, 1, 2 of ego_broadcast), the last batch is ragged, and
                              a 256-thread workgroup (at most 8 per CU) takes at least 12
  N_BIG = 64 * 32 * CU + 37   some wave draws more than 64 images: the outer `base += 64 * stride` loop runs twice; 6 x 5 px only
The fixed caps (16 384 and 512 maps, 2 048 chunks of rays, 8 192 pool entries) are restated here and looked up in the shipped
headers, so that a raised cap fails a test instead of silently keeping it on the first trip.

References stay cheap: a batch is drawn, shuffled and with repetition, from a small table of distinct items (256 poses, 1 024
map patterns); the reference is computed once per table entry and `got` is compared with ref[idx].  Neighbouring lanes, waves and
trips still hold different items, so an index mixed up between them shows.  Where only a few items take the second trip (37 maps
beyond a cap of 16 384) those items and the first-trip items of the same workgroups are chosen on purpose.  Everything is compared
bit for bit; the range scan is walked from the call's own heading_cs_out, as in test_gpu_range_scan.  Every "this really got
there" condition is asserted on the inputs, on the host.

What stays uncovered, and why:
  * range_scan_kernel<false> (maps beyond LDS, private maps) loops only beyond 2^20 chunks of 256 rays: about 1 GB of ranges.
  * the scratch-bounded `fit` grid of the global goal-field and inflation routes needs 2048 x 2048 maps to bite.
  * ego_sparse_kernel, ego_pooled_sparse_kernel and ego_pooled_sampled_kernel are launched one image per wave: they have no stride
    loop that could run twice.
  * the caps are multiples of four, so the `head` of the aligned dword run is the same for both maps of one workgroup; it still
    cycles through all four values across the batch (cells % 4 == 1)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import goal_field_ref as GR
import inflate_ref as IR
import range_scan_ref as RR
from test_gpu_egocentric import _route
from test_gpu_goal_field import SENTINEL as FIELD_SENTINEL, _raw_fields, _ref, _same
from test_gpu_inflate import FACTOR, RADIUS, RES, _raw
from test_gpu_range_scan import _Out, _same_bits, _sprinkled

pytestmark = pytest.mark.gpu

WAVES_PER_CU = 32           # MI355X: "Max waves per CU"
LDS_PER_CU = 160 * 1024     # ... and its LDS
GOAL_LDS_GRID = INFLATE_LDS_GRID = 16384
GOAL_GLOBAL_GRID = INFLATE_GLOBAL_GRID = 512
SCAN_STAGED_GRID, SCAN_BLOCK = 2048, 256
CELLS_GRID = 8192
TAIL = 37                   # items beyond a cap: the second trip of workgroups 0 .. 36
N_POSES, N_PATTERNS = 256, 1024
PIXEL_SENTINEL, GUARD = 123, 4096
PATH = np.array([[0., 0., 0.], [1., 0., 0.], [2., 0., 0.]])
WIN_40, WIN_6X5, WIN_250X6 = ((-1.0, -1.0), (2.0, 2.0)), ((-0.1, -0.15), (0.3, 0.25)), ((-0.15, -6.0), (0.3, 12.5))


# ---- the caps, as the shipped headers state them ----------------------------------------------------------------------------
def _header(name):
    import bc_gym_planning_env_amd
    with open(os.path.join(os.path.dirname(bc_gym_planning_env_amd.__file__), "csrc", name)) as f:
        return f.read()


@pytest.mark.parametrize("name,pattern,value", [
    ("bcp_goal_plan.h", r"kGoalLdsGrid\s*=\s*(\d+)\s*;", GOAL_LDS_GRID),
    ("bcp_goal_plan.h", r"kGoalGlobalGrid\s*=\s*(\d+)\s*;", GOAL_GLOBAL_GRID),
    ("bcp_inflate_host.h", r"std::min<int64_t>\(n_maps,\s*(\d+)\)", INFLATE_LDS_GRID),
    ("bcp_inflate_host.h", r"kInflateGlobalGrid\s*=\s*(\d+)\s*;", INFLATE_GLOBAL_GRID),
    ("bcp_scan_host.h", r"std::min<int64_t>\(chunks,\s*staged\s*\?\s*(\d+)\s*:", SCAN_STAGED_GRID),
    ("bcp_scan.h", r"kScanBlock\s*=\s*(\d+)\s*;", SCAN_BLOCK),
    ("bcp_host.h", r"std::min<int64_t>\(max_entries,\s*(\d+)\)", CELLS_GRID),
    ("bcp_ego.h", r"base \+= (\d+) \* stride", 64),      # ego_costmap_kernel and ego_costmap_window_kernel
    ("bcp_ego.h", r"base < whole; base \+= (\d+)\)", 256),   # ego_costmap_binned_kernel
    ("bcp_ego_route.h", r"kEgoWaves\s*=\s*(\d+)\s*;", 8),
], ids=["goal-lds", "goal-global", "inflate-lds", "inflate-global", "scan-staged", "scan-block", "cells", "ego-batch", "binned-batch",
        "ego-waves"])
def test_headers_still_state_the_caps(name, pattern, value):
    """the sizes below are derived from these numbers: if one of them moves, the second trips move with it"""
    found = re.findall(pattern, _header(name))
    assert found and all(int(v) == value for v in found), (name, pattern, found, value)


@pytest.fixture(scope="module")
def sizes(torch_cuda):
    """(CU, N_MID, N_BIG)"""
    cu = int(torch_cuda.cuda.get_device_properties(0).multi_processor_count)
    waves = WAVES_PER_CU * cu
    n_mid, n_big = 3 * waves + TAIL, 64 * waves + TAIL
    # every strided worker of at most `waves` (waves) or `waves / 4` (256-thread workgroups) draws this many at least ...
    assert n_mid // waves >= 3 and n_mid // (waves // 4) >= 12 and n_big // waves >= 64 and n_big > 64 * waves
    # ... and no grid of k workgroups per CU divides the batches: the last batch is ragged
    assert all(n % (k * cu) for n in (n_mid, n_big) for k in range(1, WAVES_PER_CU + 1))
    return cu, n_mid, n_big


# ---- egocentric views ---------------------------------------------------------------------------------------------------------
def _dense_map(rng, shape):
    m = rng.randint(0, 256, shape).astype(np.uint8)
    m[m == PIXEL_SENTINEL] = PIXEL_SENTINEL + 1     # (no source cell and no border value equals the sentinel `out` is filled with)
    return m


def _pose_table(rng, hi, extent):
    """N_POSES poses of the kind test_random_poses_vs_oracle draws: inside and far outside the map, headings beyond 4 pi; the
    second half lies within `extent` metres of the origin's corner, so that small windows see the map too"""
    poses = np.stack([rng.uniform(-4, hi, N_POSES), rng.uniform(-4, hi, N_POSES), rng.uniform(-7, 7, N_POSES)], axis=1)
    half = N_POSES // 2
    poses[half:, 0] = rng.uniform(-1.0, extent[0] - 1.0, half)
    poses[half:, 1] = rng.uniform(-1.0, extent[1] - 1.0, half)
    poses[0] = (0., 0., 0.)
    poses[1] = (1.0, 1.0, np.pi)
    poses[2:6, 2] = (15.0, -15.0, 40 * np.pi + 0.3, -1000.7)
    poses[6] = (1e4, -1e4, 0.3)
    poses[7] = (-300.0, 200.0, -2.0)
    return poses


def _draw(torch, env, poses, window, border):
    """bcp_egocentric_costmaps of poses [n, 3] into a sentinel-filled buffer with a guard behind it -> uint8 [n, rows, cols]"""
    from bc_gym_planning_env_amd import _lib
    f64p = C.POINTER(C.c_double)
    o, s = np.array(window[0], dtype=np.float64), np.array(window[1], dtype=np.float64)
    shape = (C.c_int32 * 2)()
    _lib.check(env._lib.bcp_egocentric_shape(env._h, s.ctypes.data_as(f64p), shape))
    n, pixels = len(poses), shape[0] * shape[1]
    pt = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).cuda()
    buf = torch.full((n * pixels + GUARD,), PIXEL_SENTINEL, dtype=torch.uint8, device="cuda")
    _lib.check(env._lib.bcp_egocentric_costmaps(env._h, pt.data_ptr(), n, o.ctypes.data_as(f64p), s.ctypes.data_as(f64p), border,
                                                buf.data_ptr(), None))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[n * pixels:] == PIXEL_SENTINEL).all(), "guard overwritten"
    return got[:n * pixels].reshape(n, shape[0], shape[1])


def _ego_refs(oracle, data, origin, res, poses, window, border):
    return np.stack([oracle.extract_egocentric(data, origin, res, p, np.array(window[0]), np.array(window[1]), border) for p in poses])


def _same_images(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    print(what, "images", len(got), "different:", len(bad), bad[:8].tolist())
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())
    assert not (got == PIXEL_SENTINEL).any(), what       # no pixel kept the fill


def test_shared_map_staged(torch_cuda, oracle, sizes):
    """ego_costmap_kernel<staged>: lanes k > 0 of ego_broadcast, the row table rewritten between a wave's images, the outer loop
    twice; 8 pixels per lane (40 x 40, border 255) and 4 (6 x 5, border 9)"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    cu, n_mid, n_big = sizes
    rng = np.random.RandomState(41)
    res = 0.05
    data, org = _dense_map(rng, (90, 70)), rng.uniform(-2, 0, 2)
    env = BatchedPlanEnv(CostMap2D(data, res, org), PATH, EnvParams(resolution=res, refine_path=False), n_envs=4)
    table = _pose_table(rng, 6, (3.5, 4.5))
    for window, border, n in ((WIN_40, 255, n_mid), (WIN_6X5, 9, n_mid), (WIN_6X5, 9, n_big)):
        refs = _ego_refs(oracle, data, org, res, table, window, border)
        assert len({r.tobytes() for r in refs}) > N_POSES // 3
        idx = rng.randint(N_POSES, size=n)
        got = _draw(torch, env, table[idx], window, border)
        assert _route(env)[0] == "ego_costmap_kernel<staged>", _route(env)
        _same_images(got, refs[idx], "staged %s x %d" % (refs.shape[1:], n))


def test_shared_map_global_and_window(torch_cuda, oracle, sizes):
    """a 420 x 400 map, beyond LDS: ego_costmap_window_kernel re-stages the window's part of the map for every image of a
    workgroup -- also right after an image whose window misses the map (w = h = 0) --, ego_costmap_kernel<global> reads the map
    itself"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    cu, n_mid, n_big = sizes
    rng = np.random.RandomState(42)
    res = 0.05
    data, org = _dense_map(rng, (420, 400)), rng.uniform(-2, 0, 2)
    env = BatchedPlanEnv(CostMap2D(data, res, org), PATH, EnvParams(resolution=res, refine_path=False), n_envs=4)
    table = _pose_table(rng, 23, (20.0, 21.0))
    far = np.arange(16, 80, 2)          # every second of these entries looks at nothing
    table[far, 0] = 1e3 + far
    table[far, 1] = -2e3
    cases = ((WIN_40, 31, n_mid, "ego_costmap_window_kernel"), (WIN_250X6, 31, n_mid, "ego_costmap_kernel<global>"),
             (WIN_6X5, 31, n_big, "ego_costmap_window_kernel"))
    for window, border, n, kernel in cases:
        refs = _ego_refs(oracle, data, org, res, table, window, border)
        sees = (refs != border).reshape(N_POSES, -1).any(axis=1)
        assert not sees[far].any() and sees.sum() > N_POSES // 3
        idx = rng.randint(N_POSES, size=n)
        # whatever the grid (k workgroups per CU, strided by the grid), some workgroup draws a window off the map and then one on it
        for k in range(1, 9):
            assert (~sees[idx[:-k * cu]] & sees[idx[k * cu:]]).any(), k
        got = _draw(torch, env, table[idx], window, border)
        assert _route(env)[0] == kernel, (window, _route(env))
        _same_images(got, refs[idx], "%s %s x %d" % (kernel, refs.shape[1:], n))


def _binned_runs(entry_of_image, n_entries, grid):
    """ego_costmap_binned_kernel's partition restated: images grouped by map entry, cut into `grid` equal chunks; a run is what
    one chunk holds of one entry.  -> (run lengths, a run is cut by a chunk end, a chunk holds two entries)"""
    n = len(entry_of_image)
    counts = np.bincount(entry_of_image, minlength=n_entries)
    starts = (np.cumsum(counts) - counts)[counts > 0]
    chunk = -(-n // grid)
    cuts = np.arange(0, n, chunk)
    runs = np.diff(np.unique(np.concatenate([cuts, starts, [n]])))
    return runs, np.setdiff1d(cuts, starts).size > 0, np.setdiff1d(starts, cuts).size > 0


BINNED_SHAPES = [(90, 70), (64, 101), (300, 260)]     # (the 300 x 260 map needs more than 64 KB of LDS)


@pytest.fixture(scope="module")
def binned_world(oracle):
    """3 dense maps, N_POSES poses and, per window, the oracle's image of every (pose, map): shared by the two binned tests"""
    rng = np.random.RandomState(43)
    res = 0.05
    maps = [_dense_map(rng, s) for s in BINNED_SHAPES]
    orgs = [rng.uniform(-2, 0, 2) for _ in BINNED_SHAPES]
    table = _pose_table(rng, 6, (3.5, 3.2))
    refs = {w: np.stack([_ego_refs(oracle, maps[k], orgs[k], res, table, w, b) for k in range(3)], axis=1)
            for w, b in ((WIN_40, 255), (WIN_6X5, 9))}
    for r in refs.values():
        r.setflags(write=False)
    return maps, orgs, table, refs


@pytest.mark.parametrize("kind", ["private", "pool"])
def test_binned_route(torch_cuda, binned_world, sizes, kind):
    """ego_costmap_binned_kernel with chunk > 1: runs of several images (one per wavefront, lanes k > 0, `base += 256` twice),
    a second map staged by the same workgroup, runs cut by a chunk end and runs that end where the next entry begins"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    cu, n_mid, n_big = sizes
    maps, orgs, table, refs = binned_world
    res, n_envs = 0.05, 96
    params = EnvParams(resolution=res, refine_path=False)
    if kind == "private":
        env = BatchedPlanEnv([CostMap2D(maps[i % 3], res, orgs[i % 3]) for i in range(n_envs)], [PATH] * n_envs, params, n_envs=n_envs)
        entry_of_env, n_entries = np.arange(n_envs), n_envs
        map_of_env = entry_of_env % 3
    else:
        geom = (np.arange(n_envs) * 7 % 3).astype(np.int32)
        env = BatchedPlanEnv([CostMap2D(m, res, o) for m, o in zip(maps, orgs)], [PATH] * 3, params, n_envs=n_envs, geom_of_env=geom)
        entry_of_env, n_entries = env.geom_of_env.cpu().numpy().astype(np.int64), 3
        assert (entry_of_env == geom).all()
        map_of_env = entry_of_env
    # the staged map alone takes (rows + 2) * (cols + 2) bytes of a workgroup's LDS: no more workgroups per CU than fit
    by_lds = LDS_PER_CU // ((BINNED_SHAPES[2][0] + 2) * (BINNED_SHAPES[2][1] + 2))
    assert 1 <= by_lds < WAVES_PER_CU // 4
    rng = np.random.RandomState(44)
    for window, border, n in ((WIN_40, 255, n_mid), (WIN_6X5, 9, n_big)):
        idx = rng.randint(N_POSES, size=n)
        image_env = np.arange(n) % n_envs            # image i shows the costmap of env i % n_envs
        for k in range(1, WAVES_PER_CU // 4 + 1):    # every grid of k 256-thread workgroups per CU
            runs, cut, two = _binned_runs(entry_of_env[image_env], n_entries, k * cu)
            assert runs.max() >= 4 and cut and two, (kind, n, k)
            if n == n_big:
                assert runs.max() > 256, (kind, k)
                if k <= by_lds:                      # ... and every wave of some workgroup goes round `base += 256` again
                    assert (runs.max() & ~3) >= 256 + 4, (kind, k)
        got = _draw(torch, env, table[idx], window, border)
        assert _route(env)[0] == "ego_costmap_binned_kernel", _route(env)
        _same_images(got, refs[window][idx, map_of_env[image_env]], "binned %s %s x %d" % (kind, refs[window].shape[2:], n))


def test_cell_lists_beyond_the_grid(torch_cuda, oracle):
    """ego_cells_kernel over a pool of 8 192 + 37 entries: workgroups 0 .. 36 count and list a second entry.  Entry 5 is all
    non-zero and the same workgroup's second entry holds 12 cells: a count carried over would pass the largest one.  Entry 6 holds
    12 cells and that workgroup's second entry is empty."""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    rng = np.random.RandomState(45)
    res, rows, cols, n_envs = 0.05, 24, 20, 48
    n_entries = CELLS_GRID + TAIL
    maps = np.zeros((n_entries, rows * cols), dtype=np.uint8)
    for e, k in enumerate(rng.randint(0, 13, n_entries)):
        maps[e, rng.choice(rows * cols, k, replace=False)] = rng.randint(1, 256, k)
    maps[5] = rng.randint(1, 256, rows * cols)
    maps[CELLS_GRID + 6] = 0
    for e in (CELLS_GRID + 5, 6):
        maps[e] = 0
        maps[e, rng.choice(rows * cols, 12, replace=False)] = rng.randint(1, 256, 12)
    maps = maps.reshape(n_entries, rows, cols)
    orgs = rng.uniform(-1, 0, (n_entries, 2))
    per_entry = (maps != 0).reshape(n_entries, -1).sum(axis=1)
    assert per_entry.max() == rows * cols == per_entry[5] and (per_entry == rows * cols).sum() == 1
    assert per_entry[CELLS_GRID + 5] == per_entry[6] == 12 and per_entry[CELLS_GRID + 6] == 0
    geom = np.concatenate([[0, CELLS_GRID - 1, CELLS_GRID, n_entries - 1, 5, CELLS_GRID + 6, CELLS_GRID + 5, 6],
                           rng.randint(0, CELLS_GRID, 16), rng.randint(CELLS_GRID, n_entries, 24)]).astype(np.int32)
    assert len(geom) == n_envs and (geom >= CELLS_GRID).sum() >= 24
    env = BatchedPlanEnv([CostMap2D(maps[e], res, orgs[e]) for e in range(n_entries)], [PATH] * n_entries,
                         EnvParams(resolution=res, refine_path=False), n_envs=n_envs, geom_of_env=geom)
    assert (env.geom_of_env.cpu().numpy() == geom).all()
    poses = np.concatenate([orgs[geom] + rng.uniform(0.0, 1.0, (n_envs, 2)), rng.uniform(-7, 7, (n_envs, 1))], axis=1)
    poses[4] = (orgs[5, 0] + 0.5, orgs[5, 1] + 0.6, 0.3)                              # over the entry that is all non-zero
    poses[5] = (orgs[CELLS_GRID + 6, 0] + 0.5, orgs[CELLS_GRID + 6, 1] + 0.6, 0.3)    # ... and over the empty one
    window = ((-0.5, -0.5), (1.0, 1.0))
    env.set_tuning(ego_sparse=4096)
    got = _draw(torch, env, poses, window, 0)
    kernel, counted, stride, limit = _route(env)
    print("route", kernel, "counted", counted, "stride", stride, "limit", limit)
    assert kernel == "ego_sparse_kernel" and limit == 4096
    assert counted == per_entry.max()
    lit = 0
    for i in range(n_envs):
        ref = oracle.extract_egocentric(maps[geom[i]], orgs[geom[i]], res, poses[i], np.array(window[0]), np.array(window[1]), 0)
        assert (ref == got[i]).all(), (i, int(geom[i]), int((ref != got[i]).sum()))
        lit += int((ref != 0).any()) if geom[i] >= CELLS_GRID else 0
    assert lit >= 8      # second-trip entries whose cells are in sight
    assert (got[4] != 0).sum() > 100 and not got[5].any()
    env.set_tuning(ego_sparse=0)
    sampled = _draw(torch, env, poses, window, 0)
    assert _route(env)[0] != "ego_sparse_kernel" and (sampled == got).all()


# ---- goal fields --------------------------------------------------------------------------------------------------------------
def _valid_shapes(rng, rows, cols, n):
    """valid shapes of n patterns: mostly full, some (0, .), (., 0), tiny and ragged"""
    valid = np.tile(np.array([rows, cols], dtype=np.int32), (n, 1))
    valid[0::16] = (0, cols // 2)
    valid[1::16] = (rows // 2, 0)
    valid[2::16] = np.stack([rng.randint(1, 4, len(valid[2::16])), rng.randint(1, 4, len(valid[2::16]))], axis=1)
    valid[3::16] = np.stack([rng.randint(1, rows + 1, len(valid[3::16])), rng.randint(1, cols + 1, len(valid[3::16]))], axis=1)
    return valid


def _goal_patterns(rng, rows, cols):
    """N_PATTERNS distinct (map, two seeds, valid shape) at about 15 % obstacles -- 3, 8, 15 and 34 % in turn, so that with a
    clearance some fields still span their map --, 254s in the padding; the second seed is unusable in some, both in a few"""
    n = N_PATTERNS
    valid = _valid_shapes(rng, rows, cols, n)
    density = np.array([0.03, 0.08, 0.15, 0.34])[np.arange(n) // 16 % 4]
    data = np.where(rng.uniform(size=(n, rows, cols)) < density[:, None, None], 254, 0).astype(np.uint8)
    seeds = np.zeros((n, 2, 2), dtype=np.int32)
    for k, (vr, vc) in enumerate(valid):
        padding = np.ones((rows, cols), dtype=bool)
        padding[:vr, :vc] = False
        data[k][padding] = rng.choice(np.array([254, 254, 0, 100], dtype=np.uint8), int(padding.sum()))
        seeds[k, 0] = (rng.randint(max(vr, 1)), rng.randint(max(vc, 1)))
        seeds[k, 1] = (rng.randint(rows), rng.randint(cols))
    seeds[4::8, 1] = (-1, -1)
    seeds[6::8, 1] = (rows, 3)
    seeds[5::32, 0] = (-1, -1)
    seeds[5::32, 1] = (2, cols)
    assert len({data[k].tobytes() + seeds[k].tobytes() + valid[k].tobytes() for k in range(n)}) == n
    return data, seeds, valid


def _goal_classes(data, seeds, valid, fields):
    """what max_passes = 2 must do to a pattern, from the inputs alone.  A pass relaxes every row once, the (at most 64) cells
    of a row at the same time, so a value moves at most `rows` columns per pass.  `needs_more` -- some cell with a value lies more
    than 2 * rows columns from every usable seed -- is therefore unfinished after two passes, and the second pass still lowered
    a cell (else the field were a fixed point of the relaxation, i.e. finished): gave_up = 1.  `trivial` -- no usable seed --
    lowers nothing in its first pass: gave_up = 0."""
    n, rows, cols = data.shape
    trivial, needs_more = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for k in range(n):
        usable = GR.usable_seeds(seeds[k], (rows, cols), valid[k])
        trivial[k] = not usable
        if usable:
            reached = np.nonzero((fields[k] != GR.NONE).any(axis=0))[0]      # columns that hold a value
            nearest = np.abs(reached[:, None] - np.array([c for _r, c in usable])[None, :]).min(axis=1)
            needs_more[k] = nearest.max() > 2 * rows
    return trivial, needs_more


def _batch_indices(rng, n, cap, kinds):
    """n draws from N_PATTERNS.  The workgroups whose second map lies beyond `cap` get chosen pairs instead: workgroup m draws
    its first map from kinds[m % len(kinds)][0] and its second from kinds[m % len(kinds)][1], never the same pattern twice"""
    idx = rng.randint(N_PATTERNS, size=n)
    assert n - cap == TAIL
    for m in range(TAIL):
        first, second = kinds[m % len(kinds)]
        assert len(first) > m and len(second) > m
        idx[m], idx[cap + m] = first[m], second[-1 - m]
        assert idx[m] != idx[cap + m]
    return idx


def _fields_without_info(torch, ops, data, seeds, clearance_d2, valid):
    """_raw_fields with info = NULL: phase 5 of the kernel then has no barrier"""
    n, rows, cols = data.shape
    cells = rows * cols
    d, s = torch.from_numpy(data).cuda(), torch.from_numpy(seeds).cuda()
    vr, vc = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).cuda() for v in valid)
    out = torch.from_numpy(np.full((n + 2) * cells, FIELD_SENTINEL, dtype=np.uint16)).cuda()
    rc = ops._lib.bcp_goal_field(ops._h, d.data_ptr(), n, rows, cols, 0, vr.data_ptr(), vc.data_ptr(), s.data_ptr(), seeds.shape[1],
                                 int(clearance_d2), 0, out.data_ptr() + 2 * cells, None, None)
    assert rc == 0, ops._lib.bcp_last_error()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:cells] == FIELD_SENTINEL).all() and (o[(n + 1) * cells:] == FIELD_SENTINEL).all(), "guard overwritten"
    return o[cells:(n + 1) * cells].reshape(n, rows, cols)


def _check_goal_fields(torch, ops, rows, cols, cap, seed):
    rng = np.random.RandomState(seed)
    n = cap + TAIL
    data, seeds, valid = _goal_patterns(rng, rows, cols)
    for clearance_d2 in (0, 2):
        want = np.stack([_ref(data[k], seeds[k], clearance_d2, valid[k]) for k in range(N_PATTERNS)])
        count = (want != GR.NONE).reshape(N_PATTERNS, -1).sum(axis=1)
        trivial, needs_more = _goal_classes(data, seeds, valid, want)
        assert trivial.sum() >= TAIL and needs_more.sum() >= 2 * TAIL
        assert (count == 0).sum() >= N_PATTERNS // 16 and (count > 100).sum() > 200
        # a workgroup's two maps: gave_up = 0 right after a 1 and the reverse, and two unlike fields that both take many passes
        # (a mask, a plane or a list of the first map that survived into the second shows against Dijkstra)
        hard, easy = np.nonzero(needs_more)[0], np.nonzero(trivial)[0]
        idx = _batch_indices(rng, n, cap, [(hard, easy), (easy, hard), (hard, hard)])
        batch = (data[idx], seeds[idx], clearance_d2, (valid[idx, 0], valid[idx, 1]))
        what = "%d maps of %d x %d, clearance_d2 %d" % (n, rows, cols, clearance_d2)
        # 1. every map equals Dijkstra, info = {count, 0}; _raw_fields checks the guards around out and info
        got, info = _raw_fields(torch, ops, *batch)
        bad = np.nonzero((got != want[idx]).reshape(n, -1).any(axis=1))[0]
        print(what, "different maps:", len(bad), bad[:8].tolist())
        assert len(bad) == 0, (what, len(bad), bad[:8].tolist())
        assert (info[:, 0] == count[idx]).all() and (info[:, 1] == 0).all(), what
        for m in (0, 1, cap - 1, cap, cap + 1, n - 1):
            _same(got[m], want[idx[m]], info[m], "map %d of %s" % (m, what))
        # 2. info = NULL: the same fields
        assert (_fields_without_info(torch, ops, data[idx], seeds[idx], clearance_d2, (valid[idx, 0], valid[idx, 1])) == got).all(), what
        # 3. max_passes = 2: an upper bound where the kernel gave up, the finished field where it did not
        capped, info2 = _raw_fields(torch, ops, *batch, max_passes=2)
        gave_up = info2[:, 1] == 1
        print(what, "max_passes 2: gave up", int(gave_up.sum()), "finished", int((~gave_up).sum()))
        assert set(np.unique(info2[:, 1]).tolist()) == {0, 1}
        assert (gave_up[needs_more[idx]]).all() and not gave_up[trivial[idx]].any(), what      # no flag leaks from the map before
        assert (capped[~gave_up] == got[~gave_up]).all(), what
        assert (capped[gave_up] >= got[gave_up]).all() and (capped[gave_up][got[gave_up] == GR.NONE] == GR.NONE).all(), what
        assert (info2[:, 0] == (capped != GR.NONE).reshape(n, -1).sum(axis=1)).all(), what


def test_goal_field_lds_route_beyond_its_grid(torch_cuda):
    """16 384 + 37 maps of 9 x 37 (cells % 4 == 1): the masks, the plane, the counter and the pass flags are reused by a
    workgroup's second map without a barrier in between"""
    from bc_gym_planning_env_amd.ops import NativeOps
    assert (9 * 37) % 4 == 1
    ops = NativeOps()
    _check_goal_fields(torch_cuda, ops, 9, 37, GOAL_LDS_GRID, 46)
    ops.close()


def test_goal_field_global_route_beyond_its_grid(torch_cuda):
    """512 + 37 maps of 12 x 40 with BCP_TUNE_GOAL_ROUTE = 2: the plane is each map's own slab of `out`, the masks are the
    workgroup's reused slice of scratch"""
    from bc_gym_planning_env_amd import _lib
    from bc_gym_planning_env_amd.ops import NativeOps
    forced = NativeOps()
    _lib.check(forced._lib.bcp_set_tuning(forced._h, _lib.TUNE_GOAL_ROUTE, 2))
    _check_goal_fields(torch_cuda, forced, 12, 40, GOAL_GLOBAL_GRID, 47)
    forced.close()


# ---- inflation ------------------------------------------------------------------------------------------------------------------
INFLATE_SENTINEL, POISON_F = 0x5A, -7.5


def _inflate_patterns(rng, rows, cols):
    """N_PATTERNS distinct maps of arbitrary bytes whose 254s come at densities from none to 30 %, with valid shapes; `long`:
    every row holds an obstacle, `none`: no obstacle in the valid shape"""
    n = N_PATTERNS
    valid = _valid_shapes(rng, rows, cols, n)
    data = rng.randint(0, 256, (n, rows, cols)).astype(np.uint8)
    data[data == 254] = 253
    density = np.array([0.0, 0.01, 0.05, 0.3])[np.arange(n) // 16 % 4]
    data[rng.uniform(size=data.shape) < density[:, None, None]] = 254
    full = np.nonzero((valid == (rows, cols)).all(axis=1) & (density == 0.3))[0][:2 * TAIL]
    data[full[:, None], np.arange(rows)[None, :], rng.randint(0, cols, (len(full), rows))] = 254
    inside = np.zeros(data.shape, dtype=bool)
    for k, (vr, vc) in enumerate(valid):
        inside[k, :vr, :vc] = True
    lethal_rows = ((data == 254) & inside).any(axis=2).sum(axis=1)
    long, none = np.nonzero(lethal_rows == rows)[0], np.nonzero(lethal_rows == 0)[0]
    assert len({d.tobytes() + v.tobytes() for d, v in zip(data, valid)}) == n
    return data, valid, long, none


def _check_inflate(torch, ops, rows, cols, cap, seed):
    rng = np.random.RandomState(seed)
    n, cells = cap + TAIL, rows * cols
    data, valid, long, none = _inflate_patterns(rng, rows, cols)
    assert len(long) >= 2 * TAIL and len(none) >= TAIL
    refs = [IR.inflate_and_margin(data[k], RES, RADIUS, FACTOR, valid=valid[k]) for k in range(N_PATTERNS)]
    assert min(r[2] for r in refs) > 1e-9        # (no pre-truncation value near an integer: exp()'s last bits change no byte)
    want, want_d = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    # a workgroup's two maps: n_list == 0 directly after a long list, the reverse, and two unlike maps with obstacles in every row
    idx = _batch_indices(rng, n, cap, [(long, none), (none, long), (long, long)])
    batch = np.ascontiguousarray(data[idx])
    vr, vc = (torch.from_numpy(np.ascontiguousarray(valid[idx, j], dtype=np.int32)).cuda() for j in (0, 1))
    what = "%d maps of %d x %d" % (n, rows, cols)

    def guarded(fill, dtype):
        return torch.from_numpy(np.full((n + 2) * cells, fill, dtype=dtype)).cuda()

    def read(buf, fill):
        b = buf.cpu().numpy()
        assert (b[:cells] == fill).all() and (b[(n + 1) * cells:] == fill).all(), "guard overwritten"
        return b[cells:(n + 1) * cells].reshape(n, rows, cols)

    def compare(cost, dist, how):
        bad = np.nonzero((cost != want[idx]).reshape(n, -1).any(axis=1))[0]
        bad_d = np.nonzero((dist.view(np.uint32) != want_d[idx].view(np.uint32)).reshape(n, -1).any(axis=1))[0]
        print(what, how, "maps with a different cost:", len(bad), bad[:8].tolist(), "distance:", len(bad_d), bad_d[:8].tolist())
        assert len(bad) == 0 and len(bad_d) == 0, (what, how, bad[:8].tolist(), bad_d[:8].tolist())

    src = torch.from_numpy(batch).cuda()
    out, dist = guarded(INFLATE_SENTINEL, np.uint8), guarded(POISON_F, np.float32)
    assert _raw(ops, src.data_ptr(), out.data_ptr() + cells, n, rows, cols, vr=vr.data_ptr(), vc=vc.data_ptr(),
                dist=dist.data_ptr() + 4 * cells) == 0, ops._lib.bcp_last_error()
    torch.cuda.synchronize()
    assert (src.cpu().numpy() == batch).all()
    cost = read(out, INFLATE_SENTINEL)
    compare(cost, read(dist, POISON_F), "out of place")
    # in place: out == data
    buf, dist = guarded(INFLATE_SENTINEL, np.uint8), guarded(POISON_F, np.float32)
    buf[cells:(n + 1) * cells] = src.reshape(-1)
    at = buf.data_ptr() + cells
    assert _raw(ops, at, at, n, rows, cols, vr=vr.data_ptr(), vc=vc.data_ptr(), dist=dist.data_ptr() + 4 * cells) == 0
    torch.cuda.synchronize()
    in_place = read(buf, INFLATE_SENTINEL)
    assert (in_place == cost).all(), what
    compare(in_place, read(dist, POISON_F), "in place")


def test_inflate_lds_route_beyond_its_grid(torch_cuda):
    """16 384 + 37 maps of 9 x 37: the mask, list, pos and the plane reused by a workgroup's second map without a barrier between"""
    from bc_gym_planning_env_amd import NativeOps
    ops = NativeOps()
    _check_inflate(torch_cuda, ops, 9, 37, INFLATE_LDS_GRID, 48)
    ops.close()


def test_inflate_global_route_beyond_its_grid(torch_cuda):
    """512 + 37 maps of 12 x 40 with BCP_TUNE_INFLATE_ROUTE = 2: the plane is the workgroup's reused slice of scratch"""
    from bc_gym_planning_env_amd import NativeOps, _lib
    ops = NativeOps()
    _lib.check(ops._lib.bcp_set_tuning(ops._h, _lib.TUNE_INFLATE_ROUTE, 2))
    _check_inflate(torch_cuda, ops, 12, 40, INFLATE_GLOBAL_GRID, 49)
    ops.close()


# ---- range scan -----------------------------------------------------------------------------------------------------------------
def test_range_scan_staged_second_trip(torch_cuda):
    """range_scan_kernel<true>: 2 100 rows x 251 beams = 527 100 rays > 2 048 x 256.  Workgroups 0 .. 10 rewrite their row records
    for a second chunk behind the barrier at the top of the loop while the staged mask stays; row 2 088 straddles the boundary
    between the two trips"""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams, _lib
    rng = np.random.RandomState(50)
    res, n_rows, n_beams, max_range = 0.05, 2100, 251, 3.0
    first_trip = SCAN_STAGED_GRID * SCAN_BLOCK
    total = n_rows * n_beams
    assert total > first_trip and n_beams % SCAN_BLOCK and SCAN_BLOCK % n_beams and first_trip % n_beams
    row_cut = first_trip // n_beams              # the row whose beams lie on both sides of the trip boundary
    late = np.arange(row_cut, n_rows)            # rows with rays in the second trip
    data = _sprinkled(rng, (64, 64), 0.05)
    org = rng.uniform(-2, 0, 2)
    env = BatchedPlanEnv(CostMap2D(data, res, org), PATH, EnvParams(resolution=res, refine_path=False), n_envs=4)
    table = RR.edge_rows(rng, data, data.shape, org, res, n_inside=N_POSES - 16)
    assert len(table) == N_POSES
    idx = rng.randint(N_POSES, size=n_rows)
    # the second trip sees a row in a lethal cell, rows outside the map, non-finite rows and rows inside; the rows the same
    # workgroups walked on their first trip (the first chunks) are others
    late_chunks = -(-(total - first_trip) // SCAN_BLOCK)
    early = np.arange((late_chunks * SCAN_BLOCK - 1) // n_beams + 1)
    idx[early] = 100 + np.arange(len(early))
    others = [e for e in 16 + rng.permutation(N_POSES - 16) if e != 20 and not 100 <= e < 100 + len(early)]
    idx[late] = np.concatenate([[20, 0, 4, 10, 12, 7], others[:len(late) - 6]])
    assert len(late) == 12 and len(early) == 12 and not set(idx[late].tolist()) & set(idx[early].tolist())
    poses = table[idx]
    beams = RR.beam_table(RR.wrapper_angles(n_beams, 2 * np.pi))
    beams_dev = torch.from_numpy(beams).cuda()
    pt = torch.from_numpy(np.ascontiguousarray(poses)).cuda()
    out = _Out(torch, n_rows, n_beams)
    _lib.check(env._lib.bcp_range_scan(env._h, pt.data_ptr(), n_rows, beams_dev.data_ptr(), n_beams, max_range, out.ranges.data_ptr(),
                                       out.hit.data_ptr(), out.cs.data_ptr(), None))
    torch.cuda.synchronize()
    ranges, hit, cs = out.read()                 # (checks the guards behind all three)
    # rows of one table entry got the same heading_cs_out, bit for bit; the reference walks each entry once from it
    used, first = np.unique(idx, return_index=True)
    at = np.searchsorted(used, idx)
    assert (cs.view(np.uint64) == cs[first][at].view(np.uint64)).all()
    want_r, want_h, trips, bound = RR.range_scan(data[None], [64], [64], org[None], res, np.zeros(len(used), dtype=np.int64), table[used],
                                                 cs[first], beams, max_range)
    assert trips.max() < bound
    _same_bits((ranges, hit), (want_r[at], want_h[at]), "staged, %d rays" % total)
    _same_bits((ranges[late], hit[late]), (want_r[at[late]], want_h[at[late]]), "the second trip's rows")
    assert (want_h[at[late]] >= 0).any() and (want_h[at[late]] == -1).any()

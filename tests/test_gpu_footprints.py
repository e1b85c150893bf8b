"""The footprint zoo (tests/footprints.py) through every execution path of the library: shapes the two stock footprints
never send there -- concave and self-intersecting contours (general even-odd path), images wider than 96 px (8-word row
masks, WIDE step variants), 3 .. 32 vertices (16 / 32 lanes per cell with and without inert lanes), footprints beside
the robot origin, classification geometry with one sample / skipped inner discs / no inner disc, and images at the
255-px size limit.

Expectations come from the CPU oracle (float64, the reference's operation order), from the genuine reference (golden
g15) and, for the masks, from geometry alone (footprints.fill_bounds).  Discrete outputs bit for bit, float state and
reward within util.ATOL.  Every "this case really gets there" condition is asserted on the inputs, on the host."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import footprints as F
import lookahead_ref as LR
from test_gpu_parity import MODES
from util import ATOL, GOLDEN, z_in

pytestmark = pytest.mark.gpu

NAMES = sorted(F.ZOO)
N_RANDOM = 400
E_INVALID = -1
TRICYCLE_NAME = "industrial_tricycle_v1"


def _ids(m):
    return "-".join("%s%d" % (k[:4], v) for k, v in sorted(m.items())) or "default"


@contextlib.contextmanager
def zoo_ops(name, **tuning):
    """NativeOps with zoo member `name` as its footprint"""
    from bc_gym_planning_env_amd import NativeOps
    with F.registered(F.registered_name(name), F.ZOO[name]) as robot:
        ops = NativeOps(robot)
        try:
            ops.set_tuning(**tuning)
            yield ops
        finally:
            ops.close()


@pytest.fixture(scope="module")
def g15():
    return np.load(os.path.join(GOLDEN, "g15_footprint_zoo.npz"))


@pytest.fixture(scope="module")
def g6():
    return np.load(os.path.join(GOLDEN, "g6_pose_collides.npz"))


_CASES = {}


def _case(oracle, g6, name, res, kind):
    """pose_case, computed once per (footprint, resolution, map): the eight modes share the oracle's verdicts.  The
    conditions that keep a case from being vacuous are asserted here, on the oracle's verdicts and the inputs alone."""
    key = (name, res, kind)
    if key in _CASES:
        return _CASES[key]
    c = F.pose_case(oracle, name, res, kind, g6=g6)
    share = c["exp"].mean()
    assert 0.05 <= share <= 0.95, (key, share)
    verts = F.ZOO[name]
    if kind == "speckle" and name in F.CONCAVE:
        hull = F.oracle_verdicts(oracle, F.convex_hull(verts), c["cm"], c["origin"], res, c["poses"])
        n_notch = int(((hull == 1) & (c["exp"] == 0)).sum())
        assert n_notch >= 100, "%s: only %d poses where the hull collides and the footprint does not" % (key, n_notch)
    if kind == "slab":
        large_enough = (c["box_area"] // 2 > F.SPARSE_CAP).mean() >= 0.9
        c["too_many"] = int((c["lethal_under_box"] > F.SPARSE_CAP).sum())
        if large_enough:
            assert c["too_many"] >= 1000, (key, c["too_many"])
    if name == "offcentre":
        assert (c["image_on_map"] & ~c["box_on_map"]).sum() >= 100 and (~c["origin_on_map"] & c["box_on_map"]).sum() >= 100
        assert (~c["image_on_map"]).sum() >= 100
    _CASES[key] = c
    return c


def _report(got, c):
    bad = np.nonzero(got != c["exp"])[0]
    return "%s at %g on %s: %d of %d verdicts differ from the oracle; first poses %s library %s oracle %s" % (
        c["name"], c["res"], c["kind"], len(bad), len(got), c["poses"][bad[:4]].tolist(), got[bad[:4]], c["exp"][bad[:4]])


# ---------------------------------------------------------------------------------------------------- 1. masks
def test_the_zoo_reaches_every_grouping_and_the_wide_masks():
    """K = 3 .. 15 (inert lanes in a 16-lane group), 16 (none), 17 .. 31 (32 lanes, inert ones), 32 (none); every member
    that can be wide has a wide resolution, and three members are also taken to the 255-px limit."""
    ks = sorted(set(len(v) for v in F.ZOO.values()))
    assert {3, 4, 15, 16, 17, 24, 32} <= set(ks) and min(ks) == 3 and max(ks) == F.MAX_VERTS
    for name in NAMES:
        v = F.ZOO[name]
        rs = F.gpu_resolutions(name)
        assert all(F.check_kernel_size(v, r) for r in rs)
        if F.has_wide_resolution(v):
            assert any(F.footprint_is_wide(v, r) for r in rs) and not F.footprint_is_wide(v, rs[0]) or name == "tricycle_x3"
        if name in F.LIMIT_MEMBERS:
            assert F.radius(v) / rs[-1] + 2.0 > F.MAX_KERNEL_HALF - 0.02 and 2 * int(np.ceil(F.radius(v) / rs[-1])) + 1 >= 251


@pytest.mark.parametrize("name", NAMES)
def test_masks_bit_exact_and_within_geometric_bounds(torch_cuda, oracle, g15, name):
    """get_pixel_footprint, cooperative and per-thread rasteriser, zoo x resolutions x (the reference's own angles of g15
    + 400 random + k pi / 8 + awkward ones): the shapes of the genuine reference, the oracle's pixels bit for bit, nothing
    outside [:h, :w], and -- independently of the oracle -- must <= mask <= may."""
    verts = F.ZOO[name]
    n_golden = len(F.resolutions(name))
    for ri, res in enumerate(F.gpu_resolutions(name)):
        angles = F.angle_set(N_RANDOM, seed=77 + ri)
        n_own = len(angles)
        if ri < n_golden:
            key = "%s_r%d" % (name, ri)
            assert float(g15[name + "_res"][ri]) == res
            angles = np.concatenate([angles, g15[key + "_angles"]])
        if ri == n_golden - 1 and F.has_wide_resolution(verts):
            assert F.footprint_is_wide(verts, res) and F.check_kernel_size(verts, res), (name, res)
        ivs, oshapes, omasks = F.oracle_masks(oracle, verts, res, angles)
        if name in F.CONCAVE:
            cc = [F.chain_changes(iv) for iv in ivs[:N_RANDOM]]
            n_general = sum(1 for ch, ne in cc if ne >= 2 and ch != 2)
            assert n_general >= 50, (name, res, n_general)
            if name == "bowtie":   # (two monotone chains that cross: the fast path with a self-intersecting contour)
                assert sum(1 for ch, ne in cc if ch == 2) >= 200
        must, may = F.fill_bounds_batch(ivs, oshapes)
        H, W = omasks.shape[1:]
        for exact_mode, what in ((1, "cooperative"), (2, "per-thread")):
            with zoo_ops(name, exact_mode=exact_mode) as ops:
                masks, shapes = ops.get_pixel_footprint(angles, res)
                masks, shapes = masks.cpu().numpy(), shapes.cpu().numpy()
            tag = "%s at %g, %s rasteriser" % (name, res, what)
            np.testing.assert_array_equal(shapes, oshapes, err_msg=tag)
            if ri < n_golden:
                np.testing.assert_array_equal(shapes[n_own:], g15[key + "_shape"], err_msg=tag)
            side = masks.shape[1]
            assert side >= H and side >= W
            inside = (np.arange(side)[None, :, None] < shapes[:, 0, None, None]) & \
                     (np.arange(side)[None, None, :] < shapes[:, 1, None, None])
            assert not (masks[~inside] != 0).any(), tag + ": pixels set outside [:h, :w]"
            got = masks[:, :H, :W]
            diff = np.nonzero((got != omasks).any(axis=(1, 2)))[0]
            assert len(diff) == 0, "%s: %d of %d masks differ from the oracle's, first at angle %r (%d pixels)" % (
                tag, len(diff), len(angles), angles[diff[0]], (got[diff[0]] != omasks[diff[0]]).sum())
            assert set(np.unique(got)) <= {0, 255}
            miss, far = F.fill_violations(got, must, may)
            assert miss.sum() == 0 and far.sum() == 0, (tag, int(miss.sum()), int(far.sum()))


# ---------------------------------------------------------------------------------------------------- 2. pose_collides
@pytest.mark.parametrize("mode", MODES, ids=_ids)
@pytest.mark.parametrize("name", NAMES)
def test_pose_collides_every_path_vs_oracle(torch_cuda, oracle, g6, name, mode):
    """20 000 poses per (footprint, resolution, map) through every execution path of the library, against the oracle:
    a mini-env map, a speckle map (a lethal cell in a notch must be free) and a slab map (more than kSparseCap lethal
    cells under the footprint: the too-many fallback)."""
    for res in F.gpu_resolutions(name):
        with zoo_ops(name, **mode) as ops:
            for kind in F.MAP_KINDS:
                c = _case(oracle, g6, name, res, kind)
                ops.set_costmap(c["cm"], c["origin"], res)
                got = ops.pose_collides(c["poses"]).cpu().numpy()
                assert (got == c["exp"]).all(), _report(got, c)


@pytest.mark.parametrize("name", NAMES)
def test_pose_collides_vs_reference(torch_cuda, g15, g6, name):
    """The verdicts of the genuine envs.base.env.pose_collides (golden g15) on the default path; where the footprint is
    too large for a map's resolution the library refuses the map."""
    from bc_gym_planning_env_amd import _lib
    for tag in ("mini0", "mini3", "mini64"):
        cm, origin, res = g6[tag + "_map"], g6[tag + "_origin"], float(g6[tag + "_res"])
        poses = g15[tag + "_poses"]
        want = np.unpackbits(g15["%s_%s_collides" % (name, tag)])[:len(poses)]
        with zoo_ops(name) as ops:
            if not F.check_kernel_size(F.ZOO[name], res):
                assert name == "tricycle_x3"
                with pytest.raises(_lib.BcpError):
                    ops.set_costmap(cm, origin, res)
                continue
            ops.set_costmap(cm, origin, res)
            got = ops.pose_collides(poses).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg="%s on %s" % (name, tag))


# ---------------------------------------------------------------------------------------------------- 3. classification
@pytest.mark.parametrize("name", NAMES)
def test_classification_on_equals_classification_off(torch_cuda, oracle, g6, name):
    """The distance-field pre-classification must never change a verdict: cull = 1 against cull = 0 (and both against
    the oracle) on the speckle and slab maps.  A difference here convicts build_cull_geometry or the field, not a
    rasteriser."""
    for res in F.gpu_resolutions(name):
        geo = F.cull_geometry(F.ZOO[name], res)
        for kind in ("speckle", "slab"):
            c = _case(oracle, g6, name, res, kind)
            got = {}
            for cull in (0, 1):
                with zoo_ops(name, cull=cull) as ops:
                    ops.set_costmap(c["cm"], c["origin"], res)
                    got[cull] = ops.pose_collides(c["poses"]).cpu().numpy()
            bad = np.nonzero(got[0] != got[1])[0]
            assert len(bad) == 0, "%s at %g on %s: the pre-classification changes %d verdicts (n_out %d t_out %d, %d inner " \
                "discs, %d axis samples outside the polygon); first poses %s: with %s, without %s, oracle %s" % (
                    name, res, kind, len(bad), geo["n_out"], geo["t_out"], len(geo["inner"]), geo["skipped_outside"],
                    c["poses"][bad[:4]].tolist(), got[1][bad[:4]], got[0][bad[:4]], c["exp"][bad[:4]])
            assert (got[0] == c["exp"]).all(), _report(got[0], c)


def _outer_sample_distance(geo, cells, u, v, ang):
    """distance (px) from the nearest lethal cell to the nearest outer sample pixel of poses at pixel (u, v)"""
    px, py = np.rint(u), np.rint(v)
    best = np.full(len(u), np.inf)
    for ox in geo["out_x"]:
        sx = px + np.rint(ox * np.cos(ang) - geo["axis_y"] * np.sin(ang))
        sy = py + np.rint(ox * np.sin(ang) + geo["axis_y"] * np.cos(ang))
        d = np.hypot(sx[:, None] - cells[None, :, 0], sy[:, None] - cells[None, :, 1]).min(axis=1)
        best = np.minimum(best, d)
    return best


@pytest.mark.parametrize("name", ["U", "star32", "broad", "offcentre", "triangle", "tricycle_x1.7", "collinear"])
def test_parked_poses_follow_the_restated_outer_samples(torch_cuda, name):
    """The library's sample geometry agrees with footprints.cull_geometry, shown through behaviour (default step form):
    envs standing (noise off, zero command) where every outer sample is farther than t_out from any lethal cell leave
    bcp_parked_poses unchanged over a step; envs standing where one is closer are all handed to the exact test.  The
    margins (8 px beyond, 3 px within) cover the floor of the field and the float32 sample offsets of the step."""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    verts, res = F.ZOO[name], 0.05
    geo = F.cull_geometry(verts, res)
    side = 400
    rng = np.random.RandomState(5)
    cells = rng.randint(40, side - 40, (10, 2))          # (x, y) of ten isolated lethal cells
    cm = np.zeros((side, side), dtype=np.uint8)
    cm[cells[:, 1], cells[:, 0]] = 254
    origin = np.array([-0.5 * side * res, -0.5 * side * res])
    m = 60000
    u, v, ang = rng.uniform(0, side, m), rng.uniform(0, side, m), rng.uniform(-np.pi, np.pi, m)
    # every sixth candidate is aimed: one of its outer samples lands within t_out - 3 of a lethal cell
    aimed = np.arange(0, m, 6)
    ox = np.array(geo["out_x"])[rng.randint(0, geo["n_out"], len(aimed))]
    cell = cells[rng.randint(0, len(cells), len(aimed))]
    rad, phi = max(geo["t_out"] - 4.0, 0.0) * np.sqrt(rng.uniform(0, 1, len(aimed))), rng.uniform(-np.pi, np.pi, len(aimed))
    u[aimed] = cell[:, 0] - (ox * np.cos(ang[aimed]) - geo["axis_y"] * np.sin(ang[aimed])) + rad * np.cos(phi)
    v[aimed] = cell[:, 1] - (ox * np.sin(ang[aimed]) + geo["axis_y"] * np.cos(ang[aimed])) + rad * np.sin(phi)
    keep = (u >= 0) & (u < side) & (v >= 0) & (v < side)
    u, v, ang = u[keep], v[keep], ang[keep]
    d = _outer_sample_distance(geo, cells, u, v, ang)
    far, close = np.nonzero(d >= geo["t_out"] + 8)[0], np.nonzero(d <= geo["t_out"] - 3)[0]
    n = 2048
    assert len(far) >= n and len(close) >= n, (len(far), len(close))
    path = np.array([[-8.0, -8.0, 0.0], [8.0, 8.0, 1.0]])
    with F.registered(F.registered_name(name), verts, model=0) as robot:
        env = BatchedPlanEnv(CostMap2D(cm, res, origin), path, EnvParams(resolution=res, refine_path=False), n_envs=n,
                             robot_name=robot, noise_parameters=None)
        zero = np.zeros((n, 2))
        for pick, expect_parked in ((far[:n], 0), (close[:n], n)):
            env.reset()
            st = np.zeros((7, n))
            st[0], st[1], st[2] = origin[0] + u[pick] * res, origin[1] + v[pick] * res, ang[pick]
            env.state.robot.copy_(torch.from_numpy(st))
            before = env.parked_poses()
            env.step(zero)
            parked = env.parked_poses() - before
            np.testing.assert_array_equal(env.state.robot.cpu().numpy()[:3], st[:3])    # (nobody moved)
            print("%s: %d envs, %d parked, %d expected" % (name, n, parked, expect_parked))
            assert parked == expect_parked, (name, parked, expect_parked)
        env.check_errors()


# ---------------------------------------------------------------------------------------------------- 4. whole steps
STEP_CASES = {   # zoo member -> (base footprint, footprint_scale, resolution)
    "L": (F.ZOO["L"], 1.0, 0.05), "U": (F.ZOO["U"], 1.0, 0.05), "star32": (F.ZOO["star32"], 1.0, 0.05),
    "offcentre": (F.ZOO["offcentre"], 1.0, 0.05), "triangle": (F.ZOO["triangle"], 1.0, 0.05),
    "tricycle_x0.5": (F.TRICYCLE, 0.5, 0.05), "tricycle_x1.7": (F.TRICYCLE, 1.7, 0.03),
}
STEP_FORMS = [dict(), dict(local_pairs=2), dict(local_pairs=1), dict(fused=0), dict(defer=0)]
SP, AP, TIMEOUT = 0.2, np.pi / 8, 60


def _scatter(rng, n, cm, origin, res, path, r):
    """start states: near the path, a third next to a lethal cell of the interior; random progress and age"""
    idx = rng.randint(0, len(path), n)
    st = np.zeros((7, n))
    st[0] = path[idx, 0] + rng.normal(0, 0.15, n)
    st[1] = path[idx, 1] + rng.normal(0, 0.15, n)
    st[2] = path[idx, 2] + rng.normal(0, 0.4, n)
    st[3] = rng.uniform(0, 0.5, n)
    st[4] = rng.uniform(-0.5, 0.5, n)
    st[6] = rng.uniform(-1.0, 1.0, n)
    ly, lx = np.nonzero(cm[1:-1, 1:-1] == 254)
    near = rng.rand(n) < 0.33
    pick = rng.randint(0, len(ly), n)
    ang, rad = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.3, 1.0, n) * (r + 0.3)
    st[0] = np.where(near, origin[0] + (lx[pick] + 1) * res + rad * np.cos(ang), st[0])
    st[1] = np.where(near, origin[1] + (ly[pick] + 1) * res + rad * np.sin(ang), st[1])
    tgt = np.clip(idx + rng.randint(-3, 4, n), 1, len(path) - 1).astype(np.int32)
    md = np.hypot(path[tgt, 0] - st[0], path[tgt, 1] - st[1]) + rng.uniform(-0.01, 0.05, n)
    it = rng.randint(0, TIMEOUT, n).astype(np.int32)
    it[:8] = TIMEOUT - 1
    return st, md, tgt, it


@contextlib.contextmanager
def _robot(case):
    """(robot_name, footprint_scale, noise) that give BatchedPlanEnv the case's footprint on a tricycle model"""
    from bc_gym_planning_env_amd import robots
    base, scale, _ = STEP_CASES[case]
    if base is F.TRICYCLE:
        yield TRICYCLE_NAME, scale, 'planenv'
    else:
        with F.registered(F.registered_name(case), base, model=0) as robot:
            yield robot, scale, dict(robots.PLANENV_NOISE)


def _oracle_params(oracle, case, **kw):
    base, scale, _ = STEP_CASES[case]
    return oracle.make_params("tricycle", noise=oracle.PLANENV_NOISE, spatial_precision=SP, angular_precision=AP,
                              footprint=base, footprint_scale=scale, **kw)


def _step_and_compare(torch, env, ref, steps, rng, speed=3.0, tag=""):
    n = env.n_envs
    zout = torch.zeros(n, 3, dtype=torch.float64, device="cuda")
    n_coll = n_done = 0
    env.worlds_seen = set()
    for t in range(steps):
        a = env.action_space.sample_batch(n, rng)
        a[:, 0] *= speed
        env.step(a, noise_z_out=zout)
        ref.step(a.astype(np.float64), z_in(zout.cpu().numpy()), auto_reset=True, threads=16)
        msg = "%s step %d" % (tag, t)
        np.testing.assert_array_equal(env.done.cpu().numpy(), ref.done, err_msg=msg + " done")
        np.testing.assert_array_equal(env.collided_now.cpu().numpy(), ref.collided_now, err_msg=msg + " collided_now")
        np.testing.assert_array_equal(env.state.target_idx.cpu().numpy(), ref.target_idx, err_msg=msg + " target_idx")
        np.testing.assert_array_equal(env.state.current_iter.cpu().numpy(), ref.cur_iter, err_msg=msg + " current_iter")
        np.testing.assert_array_equal(env.state.robot_collided.cpu().numpy(), ref.collided, err_msg=msg + " robot_collided")
        if env.geom_of_env is not None:
            np.testing.assert_array_equal(env.geom_of_env.cpu().numpy(), ref.geom, err_msg=msg + " pool entry")
            env.worlds_seen.update(np.unique(ref.geom).tolist())
        np.testing.assert_allclose(env.state.robot.cpu().numpy(), np.stack(ref.st), rtol=0, atol=ATOL, err_msg=msg)
        np.testing.assert_allclose(env.reward.cpu().numpy(), ref.reward, rtol=0, atol=ATOL, err_msg=msg)
        np.testing.assert_allclose(env.state.min_spat_dist_so_far.cpu().numpy(), ref.min_dist, rtol=0, atol=ATOL, err_msg=msg)
        n_coll += int(ref.collided_now.sum())
        n_done += int(ref.done.sum())
    env.check_errors()
    return n_coll, n_done


def _put(torch, env, ref, st, md, tgt, it):
    for f in range(7):
        ref.st[f][:] = st[f]
    ref.min_dist[:], ref.target_idx[:], ref.cur_iter[:] = md, tgt, it
    env.state.robot.copy_(torch.from_numpy(st))
    env.state.min_spat_dist_so_far.copy_(torch.from_numpy(md))
    env.state.target_idx.copy_(torch.from_numpy(tgt))
    env.state.current_iter.copy_(torch.from_numpy(it))


def _env_params(res, timeout=TIMEOUT, refine_path=False, **kw):
    from bc_gym_planning_env_amd import EnvParams
    return EnvParams(goal_spat_dist=SP, goal_ang_dist=AP, resolution=res, refine_path=refine_path, iteration_timeout=timeout, **kw)


@pytest.mark.parametrize("form", STEP_FORMS, ids=_ids)
@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_steps_shared_map_vs_oracle(torch_cuda, oracle, case, form):
    """4096 envs x 200 steps on one shared map and path, auto-reset, on-device noise replayed through the oracle."""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
    base, scale, res = STEP_CASES[case]
    verts = base * scale
    if case == "tricycle_x1.7":
        assert F.footprint_is_wide(verts, res) and F.check_kernel_size(verts, res)
    n, steps = 4096, 200
    cm, origin, path = F.speckle_world(oracle, verts, res, seed=3)
    rng = np.random.RandomState(7)
    with _robot(case) as (robot, fscale, noise):
        env = BatchedPlanEnv(CostMap2D(cm, res, origin), path, _env_params(res), n_envs=n, robot_name=robot,
                             noise_parameters=noise, footprint_scale=fscale, auto_reset=True, seed=123)
        env.set_tuning(**form)
        ref = oracle.OracleBatch(_oracle_params(oracle, case, iteration_timeout=TIMEOUT), n, cm, origin, res, path)
        ref.reset_from_paths()
        _put(torch, env, ref, *_scatter(rng, n, cm, origin, res, path, F.radius(verts)))
        n_coll, n_done = _step_and_compare(torch, env, ref, steps, rng, tag="%s %s" % (case, _ids(form)))
    assert n_coll >= 1000 and n_done >= 1000, (n_coll, n_done)


@pytest.mark.parametrize("form", STEP_FORMS, ids=_ids)
@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_steps_private_maps_and_paths_vs_oracle(torch_cuda, oracle, case, form):
    """4096 envs x 200 steps, every env on a private copy of one of four maps (own lethal cells) and paths (own length)."""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
    base, scale, res = STEP_CASES[case]
    verts = base * scale
    n, steps, n_templates = 4096, 200, 4
    worlds = [F.speckle_world(oracle, verts, res, seed=20 + k) for k in range(n_templates)]
    assert len(set(len(w[2]) for w in worlds)) > 1
    template = np.arange(n) % n_templates
    rng = np.random.RandomState(9)
    with _robot(case) as (robot, fscale, noise):
        env = BatchedPlanEnv([CostMap2D(w[0], res, w[1]) for w in worlds], [w[2] for w in worlds], _env_params(res),
                             n_envs=n, robot_name=robot, noise_parameters=noise, footprint_scale=fscale, auto_reset=True,
                             seed=5, template_of_env=template)
        env.set_tuning(**form)
        max_len = max(len(w[2]) for w in worlds)
        pbuf = np.zeros((n_templates, max_len, 3))
        for k, w in enumerate(worlds):
            pbuf[k, :len(w[2])] = w[2]
        ref = oracle.OracleBatch(_oracle_params(oracle, case, iteration_timeout=TIMEOUT), n, np.stack([w[0] for w in worlds]),
                                 np.stack([w[1] for w in worlds]), res, pbuf, lens=[len(w[2]) for w in worlds],
                                 geom=template.astype(np.int32))
        ref.reset_from_paths()
        np.testing.assert_array_equal(env.state.target_idx.cpu().numpy(), ref.target_idx)
        parts = [_scatter(rng, n, w[0], w[1], res, w[2], F.radius(verts)) for w in worlds]
        pick = lambda j: np.choose(template, [p[j] for p in parts])   # (env i takes the start state drawn for its template)
        _put(torch, env, ref, pick(0), pick(1), pick(2).astype(np.int32), pick(3).astype(np.int32))
        n_coll, n_done = _step_and_compare(torch, env, ref, steps, rng, tag="%s %s" % (case, _ids(form)))
    assert n_coll >= 1000 and n_done >= 1000, (n_coll, n_done)


@pytest.mark.parametrize("form", STEP_FORMS, ids=_ids)
@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_steps_mini_env_pool_vs_oracle(torch_cuda, oracle, case, form):
    """4096 envs x 200 steps over a BatchedRandomMiniEnv pool (16 chains x 3 worlds): every reset moves an env to its next
    world.  The sampler accepts start poses with the footprint of env_params.robot_name at scale 1; the steps use the
    case's own scale.  Episodes of up to 100 steps: with 25 the robots hardly leave their (collision-free) start poses --
    the oracle alone, fed numpy normals, counts 0 collisions for the half-size tricycle and 850 for the triangle; with
    100 it counts 1905 (offcentre) to 60 391 (tricycle x 1.7) and 8431 or more resets per case."""
    torch = torch_cuda
    from bc_gym_planning_env_amd import mini_env
    base, scale, _ = STEP_CASES[case]
    n, steps, n_chains, episodes, timeout = 4096, 200, 16, 3, 100
    rng = np.random.RandomState(4)
    with _robot(case) as (robot, fscale, noise):
        params = mini_env.RandomMiniEnvParams(env_params=_env_params(0.03, timeout=timeout, refine_path=True, robot_name=robot))
        res = float(params.env_params.resolution)
        if case == "tricycle_x1.7":
            assert F.footprint_is_wide(base * scale, res)
        pool = mini_env.sample_pool(params, list(range(100, 100 + n_chains)), episodes)
        env = mini_env.BatchedRandomMiniEnv(n, params, pool=pool, auto_reset=True, seed=11, noise_parameters=noise,
                                            footprint_scale=fscale)
        env.set_tuning(**form)
        maps = np.stack([c.get_data() for c in pool.costmaps])
        origins = np.stack([c.get_origin() for c in pool.costmaps])
        paths = env._paths
        pbuf = np.zeros((len(paths), max(len(p) for p in paths), 3))
        for k, p in enumerate(paths):
            pbuf[k, :len(p)] = p
        i = np.arange(n)
        geom0 = (i % n_chains) * episodes + (i // n_chains) % episodes
        ref = oracle.OracleBatch(_oracle_params(oracle, case, iteration_timeout=timeout), n, maps, origins, res, pbuf,
                                 lens=[len(q) for q in paths], geom=geom0, next_geom=pool.next_geom)
        ref.reset_from_paths()
        ref.reset_all_to_geom(advance=True)    # (the constructor's reset() moves every env to world 1 of its chain)
        n_coll, n_done = _step_and_compare(torch, env, ref, steps, rng, tag="%s %s" % (case, _ids(form)))
    assert n_coll >= 1000 and n_done >= 1000, (n_coll, n_done)
    assert len(env.worlds_seen) == len(pool)       # every world of the pool was in use at some step


def _wide_u_world(oracle):
    verts = F.ZOO["U"]
    res = F.wide_resolution(verts)
    assert F.footprint_is_wide(verts, res) and F.check_kernel_size(verts, res)
    return (verts, res) + F.speckle_world(oracle, verts, res, seed=3)


def test_rollout_with_a_wide_concave_footprint_vs_oracle(torch_cuda, oracle):
    """bcp_rollout carries `wide` and n_verts: U at its wide resolution, 8 steps per call, against the oracle stepped 8
    times with the normals the rollout drew."""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, robots
    verts, res, cm, origin, path = _wide_u_world(oracle)
    n, k_steps, rounds = 2048, 8, 8
    rng = np.random.RandomState(12)
    with F.registered(F.registered_name("U"), verts, model=0) as robot:
        env = BatchedPlanEnv(CostMap2D(cm, res, origin), path, _env_params(res), n_envs=n, robot_name=robot,
                             noise_parameters=dict(robots.PLANENV_NOISE), auto_reset=True, seed=77)
        p = oracle.make_params("tricycle", noise=oracle.PLANENV_NOISE, spatial_precision=SP, angular_precision=AP,
                               footprint=verts, iteration_timeout=TIMEOUT)
        ref = oracle.OracleBatch(p, n, cm, origin, res, path)
        ref.reset_from_paths()
        _put(torch, env, ref, *_scatter(rng, n, cm, origin, res, path, F.radius(verts)))
        hits = dones = 0
        for r in range(rounds):
            acts = np.stack([env.action_space.sample_batch(n, rng) for _ in range(k_steps)])
            acts[..., 0] *= 3.0
            zout = torch.zeros(k_steps, n, 3, dtype=torch.float64, device="cuda")
            coll = torch.zeros(k_steps, n, dtype=torch.uint8, device="cuda")
            rew, done = env.rollout(torch.from_numpy(acts).cuda(), noise_z_out=zout, collided_out=coll)
            z = zout.cpu().numpy()
            for k in range(k_steps):
                ref.step(acts[k].astype(np.float64), z_in(z[k]), auto_reset=True, threads=16)
                np.testing.assert_array_equal(done[k].cpu().numpy(), ref.done, err_msg="round %d step %d" % (r, k))
                np.testing.assert_array_equal(coll[k].cpu().numpy(), ref.collided_now, err_msg="round %d step %d" % (r, k))
                np.testing.assert_allclose(rew[k].cpu().numpy(), ref.reward, rtol=0, atol=ATOL)
                hits += int(ref.collided_now.sum())
                dones += int(ref.done.sum())
            np.testing.assert_allclose(env.state.robot.cpu().numpy(), np.stack(ref.st), rtol=0, atol=ATOL)
            np.testing.assert_array_equal(env.state.target_idx.cpu().numpy(), ref.target_idx)
            np.testing.assert_array_equal(env.state.current_iter.cpu().numpy(), ref.cur_iter)
        env.check_errors()
    assert hits >= 100 and dones >= 300, (hits, dones)


def test_lookahead_with_a_wide_concave_footprint_vs_oracle(torch_cuda, oracle):
    """bcp_lookahead carries `wide` and n_verts: U at its wide resolution, 16 candidates x 40 steps per env."""
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
    from test_gpu_lookahead import ALL, _check, _set_start
    verts, res, cm, origin, path = _wide_u_world(oracle)
    n, k, horizon = 512, 16, 40
    rng = np.random.RandomState(13)
    st, md, tgt, it = _scatter(rng, n, cm, origin, res, path, F.radius(verts))
    start = LR.StartState(st, md, tgt, it)
    library = LR.random_library(np.random.RandomState(11), k, horizon)
    p = oracle.make_params("tricycle", noise=None, spatial_precision=SP, angular_precision=AP, footprint=verts,
                           iteration_timeout=TIMEOUT)
    exp = LR.oracle_lookahead(oracle, p, dict(costmaps=cm, origins=origin, resolution=res, paths=path), start, library,
                              threads=16)
    with F.registered(F.registered_name("U"), verts, model=0) as robot:
        env = BatchedPlanEnv(CostMap2D(cm, res, origin), path, _env_params(res), n_envs=n, robot_name=robot,
                             noise_parameters=None)
        _set_start(torch, env, start)
        la = env.lookahead(torch.from_numpy(library).cuda(), want=ALL)
        got = _check(la, exp, horizon, tag="wide U")
        env.check_errors()
    assert ((got["reason"] & LR.DONE_COLLIDED) != 0).sum() >= 500 and (got["reason"] == 0).sum() >= 500


@pytest.mark.parametrize("name", ["L", "U"])
def test_device_sampler_with_a_concave_footprint_matches_host(torch_cuda, name):
    """bcp_sample_mini_worlds tests start poses with the footprint of env_params.robot_name: with a registered concave
    footprint the device sampler's worlds must be the host sampler's (as test_device_sampler_matches_host_and_reference
    shows for the tricycle), and must differ from the tricycle's worlds somewhere -- the footprint really is used."""
    from bc_gym_planning_env_amd import EnvParams, mini_env
    seeds = list(range(500, 564))
    with F.registered(F.registered_name(name), F.ZOO[name], model=0) as robot:
        params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, robot_name=robot))
        a = mini_env.sample_pool(params, seeds, 6)
        b = mini_env.sample_pool_device(params, seeds, 6)
    same_maps = 0
    for wa, wb, ca, cb in zip(a.worlds, b.worlds, a.costmaps, b.costmaps):
        for fa, fb in ((wa.start_pos, wb.start_pos), (wa.end_pos, wb.end_pos), (wa.obstacle_o, wb.obstacle_o),
                       (wa.obstacle_a, wb.obstacle_a), (wa.obstacle_b, wb.obstacle_b)):
            np.testing.assert_allclose(fa, fb, rtol=0, atol=1e-12)
        same_maps += int((ca.get_data() == cb.get_data()).all())
    assert same_maps >= len(a.worlds) - 1
    tri = mini_env.sample_pool(mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2)),
                               seeds, 6)
    assert any(not np.array_equal(wa.start_pos, wt.start_pos) for wa, wt in zip(a.worlds, tri.worlds))


# ---------------------------------------------------------------------------------------------------- 5. refusals
def _create(L, p, n=8):
    h = C.c_void_p()
    return L.bcp_create(C.byref(p), n, 0, 0, C.byref(h)), h


def test_create_refuses_vertex_counts_and_non_finite_vertices(torch_cuda):
    from bc_gym_planning_env_amd import EnvParams, _lib, robots
    L = _lib.load()
    for n_verts in (2, 33, 0, -1):
        p = robots.make_bcp_params(EnvParams(), TRICYCLE_NAME, None)
        p.n_verts = n_verts
        rc, h = _create(L, p)
        assert rc == E_INVALID and not h.value and b"n_verts" in L.bcp_last_error(), n_verts
    for n_verts in (3, 32):
        with F.registered("zoo_count", F.ZOO["star32"][:n_verts]) as robot:
            rc, h = _create(L, robots.make_bcp_params(EnvParams(), robot, None))
            assert rc == 0 and L.bcp_destroy(h) == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k, axis in ((0, 0), (15, 1)):
            p = robots.make_bcp_params(EnvParams(), TRICYCLE_NAME, None)
            p.verts[k][axis] = bad
            rc, h = _create(L, p)
            assert rc == E_INVALID and not h.value and b"finite" in L.bcp_last_error(), (bad, k)
    p = robots.make_bcp_params(EnvParams(), TRICYCLE_NAME, None)
    p.verts[20][0] = float("nan")      # (beyond n_verts: not part of the footprint)
    rc, h = _create(L, p)
    assert rc == 0 and L.bcp_destroy(h) == 0


@pytest.mark.parametrize("name", F.LIMIT_MEMBERS)
def test_size_limit_is_where_the_header_says(torch_cuda, name):
    """radius / resolution + 2 just above BCP_MAX_KERNEL_HALF is refused by bcp_set_costmaps, bcp_pixel_footprint and the
    mini-world sampler; just below it is accepted (and tested at that size by the mask and pose tests above)."""
    from bc_gym_planning_env_amd import EnvParams, _lib, mini_env
    verts = F.ZOO[name]
    inside, outside = F.limit_resolution(verts, True), F.limit_resolution(verts, False)
    assert F.check_kernel_size(verts, inside) and not F.check_kernel_size(verts, outside)
    assert inside in F.gpu_resolutions(name)
    cm = np.zeros((64, 64), dtype=np.uint8)
    with zoo_ops(name) as ops:
        for call in (lambda: ops.set_costmap(cm, np.zeros(2), outside), lambda: ops.get_pixel_footprint(np.zeros(3), outside)):
            with pytest.raises(_lib.BcpError) as err:
                call()
            assert "exceeds" in str(err.value)
        ops.set_costmap(cm, np.zeros(2), inside)
        masks, shapes = ops.get_pixel_footprint(np.array([0.0, 0.7]), inside)
        assert int(shapes.max()) >= 240 and bool((masks[0] != 0).any())
    # the sampler: a footprint too large for the mini world's resolution (0.03 m)
    big = verts * (F.radius(F.TRICYCLE * 3.0) / F.radius(verts))
    assert not F.check_kernel_size(big, 0.03)
    with F.registered("zoo_big", big, model=0) as robot:
        params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2, robot_name=robot))
        with pytest.raises(_lib.BcpError):
            mini_env.sample_pool_device(params, [1, 2], 2)

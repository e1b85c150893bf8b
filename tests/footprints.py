"""The footprint zoo and its helpers: shapes that send the collision code down the paths the two stock footprints never
reach (general even-odd contour, wide row masks, every lanes-per-cell grouping, degenerate classification geometry),
a geometry check of a polygon fill in exact integer arithmetic, and host restatements of the library's predicates.

Plain module (no fixtures): imported by test_footprints_host.py, test_gpu_footprints.py, test_oracle_golden.py and
oracle/gen_golden.py.  Nothing here imports the GPU package at module level.
"""
import contextlib

import numpy as np

# ---- constants restated from the native headers (include/bcplan.h, csrc/bcp_desc.h, csrc/bcp_field_plan.h) --------------
MAX_VERTS = 32               # BCP_MAX_VERTS
MAX_KERNEL_HALF = 127        # BCP_MAX_KERNEL_HALF
MAX_SAMPLES = 8              # kMaxSamples
SPARSE_CAP = 256             # kSparseCap
SLACK_OUTER = 0.7072 + 0.5 + 0.01 + 0.7072   # kSlackOuter
SLACK_INNER = 0.7072 + 0.7072 + 0.05         # kSlackInner
NARROW_MASK_PX = 96          # three 32-bit words per row of the cooperative rasteriser (footprint_is_wide)

TRICYCLE = np.array([
    [1348.35, 0.], [1338.56, 139.75], [1306.71, 280.12], [1224.36, 338.62], [1093.81, 374.64], [-214.37, 374.64],
    [-313.62, 308.56], [-366.36, 117.44], [-374.01, -135.75], [-227.96, -459.13], [-156.72, -458.78],
    [759.8, -442.96], [849.69, -426.4], [1171.05, -353.74], [1303.15, -286.54], [1341.34, -118.37]]) / 1000.
DIFFDRIVE = np.array([
    [644.5, 0], [634.86, 61], [571.935, 130.54], [553.38, 161], [360.36, 186], [250, 186], [250, 186], [100, 186],
    [100, 186], [0, 196], [-119.21, 190.5], [-173.4, 146], [-193, 0], [-173.4, -143], [-111.65, -246],
    [-71.57, -246], [100, -246], [100, -246], [250, -246], [250, -246], [413.085, -223], [491.5, -204.5],
    [553, -161], [634.86, -62]]) / 1000.
STOCK = {"tricycle": ("industrial_tricycle_v1", TRICYCLE), "diffdrive": ("industrial_diffdrive_v1", DIFFDRIVE)}
SCALES = (0.5, 1.7, 3.0)


def _ngon(n, rx, ry, phase):
    a = phase + np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([rx * np.cos(a), ry * np.sin(a)], 1)


def _star(n, r0, r1):
    a = np.linspace(0, 2 * np.pi, 2 * n, endpoint=False)
    r = np.where(np.arange(2 * n) % 2 == 0, r0, r1)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1)


_L = np.array([[-0.5, -0.4], [1.0, -0.4], [1.0, 0.0], [0.1, 0.0], [0.1, 0.6], [-0.5, 0.6]])

ZOO = {
    # K = 3: the smallest footprint the C ABI takes; 13 inert lanes in a 16-lane group
    "triangle": np.array([[1.0, 0.0], [-0.5, 0.5], [-0.5, -0.5]]),
    # K = 4: the reference's own known-answer rectangle (utilities/test_costmap_utils.py:242-248)
    "kat_rect": np.array([[-0.77, -0.385], [-0.77, 0.385], [0.67, 0.385], [0.67, -0.385]]),
    # K = 15 / 16 / 17: one inert lane of a 16-lane group, none, and the switch to 32 lanes per cell with 15 inert
    "ngon15": _ngon(15, 1.0, 0.6, 0.1),
    "ngon16": _ngon(16, 1.0, 0.6, 0.1),
    "ngon17": _ngon(17, 1.0, 0.6, 0.1),
    # K = 32, alternating radii: concave all round (up to 30 chain changes), every lane of the group owns an edge
    "star32": _star(16, 1.0, 0.45),
    # concave with one inner corner: about half of all angles leave the two-chain fast path
    "L": _L,
    # concave, the notch opens along +x: the classification axis (y = 0) runs through the notch, so axis samples lie
    # OUTSIDE the polygon and nearly every angle needs the general contour path
    "U": np.array([[-0.6, -0.5], [0.9, -0.5], [0.9, -0.25], [-0.2, -0.25], [-0.2, 0.25], [0.9, 0.25], [0.9, 0.5],
                   [-0.6, 0.5]]),
    # self-intersecting, 4 vertices: even-odd fill; most angles are two monotone chains that CROSS (fast path)
    "bowtie": np.array([[-0.8, -0.4], [0.8, 0.4], [0.8, -0.4], [-0.8, 0.4]]),
    # thinner than a pixel at every tested resolution: outline only, fewer than two non-horizontal edges at some angles
    "sliver": np.array([[-1.0, 0.0], [1.0, 0.004], [1.0, -0.004]]),
    # three vertices on one line: zero area, the fill is the outline
    "collinear": np.array([[-0.8, 0.0], [0.1, 0.0], [0.9, 0.0]]),
    # three identical vertices: one pixel, no edge at all
    "point3": np.array([[0.3, 0.2], [0.3, 0.2], [0.3, 0.2]]),
    # concave with doubled vertices, as the diff-drive mock has: zero-length edges inside a general contour
    "repeated": np.repeat(_L, 2, axis=0),
    # the robot origin lies outside the polygon: the kernel image is far bigger than the polygon in it
    "offcentre": np.array([[2.0, 1.0], [2.6, 1.0], [2.6, 1.5], [2.0, 1.5]]),
    # ymax - ymin > 4 (xmax - xmin): the classification axis degenerates to one sample (a0 > a1)
    "broad": np.array([[-0.15, -0.9], [0.15, -0.9], [0.2, 0.0], [0.15, 0.9], [-0.15, 0.9], [-0.2, 0.0]]),
}
for _name, (_robot, _fp) in STOCK.items():
    for _s in SCALES:
        # the stock footprints through footprint_scale: 0.5 = small images, 1.7 / 3.0 = long axis (n_out at kMaxSamples)
        ZOO["%s_x%g" % (_name, _s)] = _fp * _s

CONCAVE = ("L", "U", "star32", "bowtie", "repeated")   # members asserted to leave the two-chain fast path
COARSE_RES = (0.05, 0.03)


def registered_name(name):
    return "zoo_" + name


@contextlib.contextmanager
def registered(name, verts, model=1):
    """Make `name` a robot of the GPU package for the duration of the block: NativeOps(name) and
    BatchedPlanEnv(..., robot_name=name) then take `verts` as the footprint and `model` (0 tricycle, 1 diff-drive) as
    the motion model.  Removed again on exit."""
    from bc_gym_planning_env_amd import robots
    assert name not in robots.FOOTPRINTS and name not in robots.MODELS, name
    robots.FOOTPRINTS[name] = np.array(verts, dtype=np.float64)
    robots.MODELS[name] = model
    try:
        yield name
    finally:
        del robots.FOOTPRINTS[name], robots.MODELS[name]


# ---- host restatements of the library's predicates ----------------------------------------------------------------
def radius(verts):
    return float(np.sqrt((np.asarray(verts) ** 2).sum(1).max()))


def diameter(verts):
    v = np.asarray(verts, dtype=np.float64)
    d = v[:, None, :] - v[None, :, :]
    return float(np.sqrt((d ** 2).sum(2).max()))


def footprint_is_wide(verts, res):
    """footprint_is_wide (bcp_field_plan.h): the cooperative rasteriser's row masks need more than three words"""
    return diameter(verts) / res + 3.0 > NARROW_MASK_PX


def check_kernel_size(verts, res):
    """check_kernel_size (bcp_field_plan.h): the rotated image stays within 255 x 255 px"""
    return radius(verts) / res + 2.0 <= MAX_KERNEL_HALF


def wide_resolution(verts):
    """A resolution at which the footprint is wide and still accepted (radius / res + 2 = 120), or None where no
    resolution can give both (diameter / radius too small: the image grows faster than the polygon in it)."""
    r = radius(verts)
    if r == 0:
        return None
    res = r / 118.0
    return res if footprint_is_wide(verts, res) and check_kernel_size(verts, res) else None


def has_wide_resolution(verts):
    """wide needs diameter / res > 93, the size check radius / res <= 125: both hold for some res iff
    diameter / radius > 93 / 125"""
    r = radius(verts)
    return r > 0 and diameter(verts) / r > (NARROW_MASK_PX - 3.0) / (MAX_KERNEL_HALF - 2.0)


def limit_resolution(verts, accepted=True):
    """A resolution just inside (radius / res + 2 = 126.99: 255-px images) or just outside (127.01) the size check"""
    return radius(verts) / ((MAX_KERNEL_HALF - 2.0) + (-0.01 if accepted else 0.01))


def resolutions(name):
    """The resolutions a zoo member is tested at: the two coarse ones where the size check accepts them, and its wide one"""
    v = ZOO[name]
    out = [r for r in COARSE_RES if check_kernel_size(v, r)]
    w = wide_resolution(v)
    if w is not None:
        out.append(w)
    return out


def chain_changes(iv):
    """raster_runs' count (bcp_raster.h): sign changes of dy around the integer contour, horizontal edges skipped, the
    wrap-around included.  2 = two y-monotone chains = fast path; anything else with >= 2 edges = general contour.
    -> (changes, n_edges)"""
    iv = np.asarray(iv)
    dy = iv[:, 1] - np.roll(iv[:, 1], 1)
    s = np.sign(dy[dy != 0])
    if len(s) == 0:
        return 0, 0
    return int((s != np.roll(s, 1)).sum()), len(s)


def angle_set(n_random, seed):
    """n_random uniform angles + k pi / 8 + the awkward ones (tiny, -pi, beyond +-2 pi)"""
    rng = np.random.RandomState(seed)
    fixed = [k * np.pi / 8 for k in range(-8, 9)] + [1e-9, -1e-9, -np.pi, 7.0, -9.5, 2 * np.pi + 0.3, -4 * np.pi - 1.1]
    return np.concatenate([rng.uniform(-np.pi, np.pi, n_random), fixed])


def convex_hull(verts):
    """Andrew's monotone chain -> hull vertices, counter-clockwise"""
    pts = sorted(set(map(tuple, np.asarray(verts, dtype=np.float64))))
    if len(pts) < 3:
        return np.array(pts)

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) -
                                     (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(p)
        return out[:-1]
    return np.array(half(pts) + half(pts[::-1]))


# ---- the geometry check of a polygon fill, in exact integer arithmetic ---------------------------------------------
def fill_bounds_batch(ivs, shapes, chunk=48):
    """fill_bounds for A polygons at once (worked through in chunks to bound the memory; see _fill_bounds_chunk)."""
    ivs, shapes = np.asarray(ivs, dtype=np.int64), np.asarray(shapes, dtype=np.int64)
    H, W = int(shapes[:, 0].max()), int(shapes[:, 1].max())
    parts = [_fill_bounds_chunk(ivs[i:i + chunk], shapes[i:i + chunk], H, W) for i in range(0, len(ivs), chunk)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _fill_bounds_chunk(ivs, shapes, H, W):
    """fill_bounds for A polygons at once.  ivs int [A, K, 2] (x, y), shapes int [A, 2] (h, w) ->
    (must, may) bool [A, H, W], H and W at least the largest shape; pixels outside a polygon's own [:h, :w] are False in both.

    For a pixel (u, v) and every edge with y0 != y1 and min(y0, y1) <= v < max(y0, y1) let
    x_e = x0 + (v - y0)(x1 - x0) / (y1 - y0), exactly (all comparisons are cross-multiplied int64).
      must: an odd number of x_e < u, or some x_e within 1 / 64 of u, or (u, v) is a vertex.
      may:  must, or the Euclidean distance from (u, v) to the closed contour is <= 1.
    A correct cv2.fillPoly restatement has must <= mask <= may: fillPoly's 16.16 slope is truncated, an error < 2^-16 per
    row and < 2^-8 over the <= 255 rows an image can have, so a centre further than 1 / 64 from every crossing is on the
    same side for fillPoly as for exact arithmetic, a centre within 1 / 64 of an edge is a pixel of that edge's
    8-connected line, and a line's end points are always drawn; an outline pixel is within half a pixel per axis of its
    edge and a span pixel inside up to the 2^-8 above."""
    A, K, _ = ivs.shape
    assert (ivs >= 0).all() and (ivs[:, :, 0] < shapes[:, None, 1]).all() and (ivs[:, :, 1] < shapes[:, None, 0]).all()
    x1, y1 = ivs[:, :, 0], ivs[:, :, 1]
    x0, y0 = np.roll(x1, 1, axis=1), np.roll(y1, 1, axis=1)
    v = np.arange(H, dtype=np.int64)[None, :, None]                      # [1, H, 1] against edges [A, 1, K]
    X0, Y0, X1, Y1 = x0[:, None, :], y0[:, None, :], x1[:, None, :], y1[:, None, :]
    active = (np.minimum(Y0, Y1) <= v) & (v < np.maximum(Y0, Y1))        # [A, H, K]
    den = Y1 - Y0
    num = X0 * den + (v - Y0) * (X1 - X0)                                # x_e = num / den
    neg = den < 0
    num, den = np.where(neg, -num, num), np.where(neg, -den, den)
    den = np.where(active, den, 1)
    a_idx, v_idx, _ = np.nonzero(active)
    num_a, den_a = num[active], den[active]
    # parity: x_e < u  <=>  u >= floor(x_e) + 1 : toggle the row from there on
    first = np.clip(num_a // den_a + 1, 0, W)
    toggles = np.bincount((a_idx * H + v_idx) * (W + 1) + first, minlength=A * H * (W + 1)).reshape(A, H, W + 1)
    must = (np.cumsum(toggles[:, :, :W], axis=2) & 1).astype(bool)
    # crossings within 1 / 64 of a pixel centre: only the nearest integer can be
    u0 = (2 * num_a + den_a) // (2 * den_a)
    near = (64 * np.abs(num_a - u0 * den_a) <= den_a) & (u0 >= 0) & (u0 < W)
    must[a_idx[near], v_idx[near], u0[near]] = True
    # vertices
    must[np.repeat(np.arange(A), K), y1.reshape(-1), x1.reshape(-1)] = True
    # may: candidates = pixels of rows ymin - 1 .. ymax + 1 of each edge whose x lies within 2 of the part of the edge
    # between rows v - 1 and v + 1 (a float bound, padded); the distance test itself is exact
    may = must.copy()
    vv = np.arange(-1, H + 1, dtype=np.int64)[None, :, None]
    ylo, yhi = np.minimum(Y0, Y1), np.maximum(Y0, Y1)
    rows_on = (vv >= ylo - 1) & (vv <= yhi + 1) & (vv >= 0) & (vv < H)
    dyf = (Y1 - Y0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta = np.clip(np.where(dyf != 0, (vv - 1 - Y0) / dyf, 0.0), 0.0, 1.0)
        tb = np.clip(np.where(dyf != 0, (vv + 1 - Y0) / dyf, 1.0), 0.0, 1.0)
    xa, xb = X0 + ta * (X1 - X0), X0 + tb * (X1 - X0)
    lo = np.maximum(np.floor(np.minimum(xa, xb)).astype(np.int64) - 2, 0)
    hi = np.minimum(np.ceil(np.maximum(xa, xb)).astype(np.int64) + 2, W - 1)
    cnt = np.where(rows_on & (hi >= lo), hi - lo + 1, 0)
    a_i, r_i, e_i = np.nonzero(cnt)
    n = cnt[a_i, r_i, e_i]
    total = int(n.sum())
    start = np.cumsum(n) - n
    rep = np.repeat(np.arange(len(n)), n)
    pu = lo[a_i, r_i, e_i][rep] + (np.arange(total) - start[rep])
    pa, pe = a_i[rep], e_i[rep]
    pv = r_i[rep] - 1                                                   # (vv starts at -1)
    ax, ay, bx, by = x0[pa, pe], y0[pa, pe], x1[pa, pe], y1[pa, pe]
    ex, ey, wx, wy = bx - ax, by - ay, pu - ax, pv - ay
    ee, dot = ex * ex + ey * ey, wx * ex + wy * ey
    cross = wx * ey - wy * ex
    close = np.where(dot <= 0, wx * wx + wy * wy <= 1,
                     np.where(dot >= ee, (pu - bx) ** 2 + (pv - by) ** 2 <= 1, cross * cross <= ee))
    may[pa[close], pv[close], pu[close]] = True
    inside = (np.arange(H)[None, :, None] < shapes[:, 0, None, None]) & (np.arange(W)[None, None, :] < shapes[:, 1, None, None])
    return must & inside, may & inside


def fill_bounds(int_vertices, shape):
    """(must, may) for one polygon: bool images of `shape` (h, w); see fill_bounds_batch."""
    must, may = fill_bounds_batch(np.asarray(int_vertices)[None], np.asarray(shape)[None])
    return must[0], may[0]


def fill_violations(masks, must, may):
    """-> (pixels that had to be set and are not, pixels set outside the allowed band), per polygon [A]"""
    m = np.asarray(masks) != 0
    return (must & ~m).sum(axis=(1, 2)), (m & ~may).sum(axis=(1, 2))


def oracle_masks(oracle, verts, res, angles):
    """The oracle's integer polygons, shapes and masks for `angles`, masks padded to the largest shape ->
    (ivs [A, K, 2], shapes [A, 2], masks uint8 [A, H, W])"""
    ivs, shapes, imgs = [], [], []
    for a in angles:
        iv, half = oracle.footprint_vertices(a, verts, res)
        ivs.append(iv)
        shapes.append((2 * half[1] + 1, 2 * half[0] + 1))
        imgs.append(oracle.pixel_footprint(a, verts, res))
    shapes = np.array(shapes)
    masks = np.zeros((len(imgs), shapes[:, 0].max(), shapes[:, 1].max()), dtype=np.uint8)
    for i, m in enumerate(imgs):
        masks[i, :m.shape[0], :m.shape[1]] = m
    return np.array(ivs), shapes, masks


# ---- host restatement of build_cull_geometry (bcp_field_plan.h) ----------------------------------------------------------
def _seg_dist(px, py, ax, ay, bx, by):
    vx, vy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    vv = vx * vx + vy * vy
    t = (wx * vx + wy * vy) / vv if vv > 0 else 0.0
    t = min(max(t, 0.0), 1.0)
    return float(np.hypot(px - (ax + t * vx), py - (ay + t * vy)))


def point_in_polygon(px, py, v):
    inside = False
    k = len(v)
    for i in range(k):
        j = (i - 1) % k
        if (v[i][1] > py) != (v[j][1] > py) and \
                px < (v[j][0] - v[i][0]) * (py - v[i][1]) / (v[j][1] - v[i][1]) + v[i][0]:
            inside = not inside
    return inside


def cull_geometry(verts, res):
    """The sample geometry of the distance-field pre-classification, as build_cull_geometry derives it: a dict with the
    axis (a0, a1, ay, metres), rho, the outer samples out_x (pixels) with their threshold t_out, and the accepted inner
    discs as (bx metres, rin metres, t_in) triples."""
    v = np.asarray(verts, dtype=np.float64)
    K = len(v)
    xmin, xmax, ymin, ymax = v[:, 0].min(), v[:, 0].max(), v[:, 1].min(), v[:, 1].max()
    rmax = radius(v)
    reach = int(np.ceil(rmax / res)) + 2
    ay, half_w = 0.5 * (ymin + ymax), 0.5 * (ymax - ymin)
    a0, a1 = xmin + 0.25 * half_w, xmax - 0.25 * half_w
    degenerate = bool(a0 > a1)
    if degenerate:
        a0 = a1 = 0.5 * (xmin + xmax)
    rho = max(_seg_dist(v[k, 0], v[k, 1], a0, ay, a1, ay) for k in range(K))
    n_unclamped = max(2, int(np.ceil((a1 - a0) / (0.5 * rho))) + 1) if a1 > a0 and rho > 0 else (MAX_SAMPLES + 1 if a1 > a0 else 1)
    n_out = min(MAX_SAMPLES, n_unclamped) if a1 > a0 else 1
    h = (a1 - a0) / (n_out - 1) if n_out > 1 else 0.0
    r_out = np.sqrt(rho * rho + 0.25 * h * h) / res + SLACK_OUTER
    inner, skipped_outside = [], 0
    for j in range(MAX_SAMPLES):
        bx = a0 + (a1 - a0) * j / (MAX_SAMPLES - 1)
        if not point_in_polygon(bx, ay, v):
            skipped_outside += 1
            continue
        rin = min(_seg_dist(bx, ay, v[k, 0], v[k, 1], v[(k + 1) % K, 0], v[(k + 1) % K, 1]) for k in range(K))
        t = int(np.floor(rin / res - SLACK_INNER)) - 1
        if t < 0:
            continue
        inner.append((bx, rin, t))
        if a1 <= a0:
            break
    return dict(a0=a0, a1=a1, ay=ay, rho=rho, degenerate=degenerate, n_out=n_out, clamped=n_unclamped > MAX_SAMPLES,
                h=h, out_x=[(a0 + i * h) / res for i in range(n_out)], axis_y=ay / res,
                t_out=int(np.floor(r_out)) + 1, r_out=r_out, inner=inner, skipped_outside=skipped_outside,
                reach=reach, pad=2 * reach + 4)


# ---- maps and poses of the pose_collides tests ---------------------------------------------------------------------
N_POSES = 20000
LIMIT_MEMBERS = ("tricycle_x1.7", "star32", "U")   # also tested just inside the size limit (255-px images)
MAP_KINDS = ("g6", "speckle", "slab")


def gpu_resolutions(name):
    rs = resolutions(name)
    return rs + [limit_resolution(ZOO[name], True)] if name in LIMIT_MEMBERS else rs


def oracle_verdicts(oracle, verts, cm, origin, res, poses, threads=8):
    """oracle.pose_collides over many poses: the same C call, without the per-call conversions, on a few threads
    (ctypes drops the GIL during the call)"""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    lib = oracle.lib()
    v = np.ascontiguousarray(verts, dtype=np.float64)
    m = np.ascontiguousarray(cm, dtype=np.uint8)
    o = np.ascontiguousarray(origin, dtype=np.float64)
    f64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    vp, mp, op = v.ctypes.data_as(f64p), m.ctypes.data_as(u8p), o.ctypes.data_as(f64p)
    k, rows, cols, res = len(v), m.shape[0], m.shape[1], float(res)
    out = np.zeros(len(poses), dtype=np.uint8)
    P = np.asarray(poses, dtype=np.float64).tolist()

    def work(lo, hi):
        fn = lib.bco_pose_collides
        for i in range(lo, hi):
            x, y, a = P[i]
            r = fn(x, y, a, vp, k, mp, rows, cols, op, res)
            assert r >= 0
            out[i] = r
    edges = np.linspace(0, len(P), threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        for f in [ex.submit(work, edges[t], edges[t + 1]) for t in range(threads)]:
            f.result()
    return out


def _pixel_polygons(verts, res, angles):
    """rotated footprint in pixels (float, unrounded) for many angles -> [n, K, 2]; numpy's own arithmetic: good to a
    fraction of a pixel, which is all the pose generators and the counts below need"""
    q = np.asarray(verts, dtype=np.float64) / res
    c, s = np.cos(angles)[:, None], np.sin(angles)[:, None]
    return np.stack([q[None, :, 0] * c - q[None, :, 1] * s, q[None, :, 0] * s + q[None, :, 1] * c], axis=2)


def pose_case(oracle, name, res, kind, seed=0, n=N_POSES, g6=None):
    """A map of `kind` at `res` and n poses for zoo member `name`, with the oracle's verdicts and what the tests assert
    about the inputs.  Everything is derived from the footprint's geometry and the oracle alone.
      g6      the cells of a mini-env map of the reference (g6 `mini0`), read at `res`
      speckle isolated lethal cells at a density of 0.7 / (pixels of the footprint): about half of the poses on the map
              have a lethal cell under the footprint; a lethal cell in a notch or between two points must be free
      slab    the right half of the map lethal: more than kSparseCap lethal cells under every large image that lies in it
    A third of the poses hug lethal cells (a vertex of the footprint within a pixel or two of one), the rest are uniform
    over the map and a rim wide enough for an image to lie wholly off the map."""
    verts = ZOO[name]
    rng = np.random.RandomState(1000 * sorted(ZOO).index(name) + 10 * MAP_KINDS.index(kind) + seed)
    r_px = radius(verts) / res
    image = 2 * int(np.ceil(r_px)) + 1
    area = int(np.count_nonzero(oracle.pixel_footprint(0.3, verts, res)))
    if kind == "g6":
        cm = np.ascontiguousarray(g6["mini0_map"])
        side_r, side_c = cm.shape
        origin = np.asarray(g6["mini0_origin"], dtype=np.float64) * (res / float(g6["mini0_res"]))
    else:
        side_r = side_c = int(max(200, 2.2 * image))
        origin = np.array([-0.5 * side_c * res, -0.5 * side_r * res])
        cm = np.zeros((side_r, side_c), dtype=np.uint8)
        if kind == "speckle":
            cm[rng.rand(side_r, side_c) < min(0.3, 0.7 / area)] = 254
        else:
            cm[:, side_c // 2:] = 254
    rim = 0.5 * image + 6
    ang = rng.uniform(-np.pi, np.pi, n)
    u, v = rng.uniform(-rim, side_c + rim, n), rng.uniform(-rim, side_r + rim, n)
    # the hugging third: a vertex of the rotated footprint lands on or next to a lethal cell
    k = n // 3
    if kind == "slab":
        ly, lx = np.arange(side_r), np.full(side_r, side_c // 2)      # the cells of the slab's edge
    else:
        ly, lx = np.nonzero(cm == 254)
    pick = rng.randint(0, len(ly), k)
    poly = _pixel_polygons(verts, res, ang[:k])
    vert = poly[np.arange(k), rng.randint(0, len(verts), k)]
    jitter = rng.normal(0, 1.0, (k, 2)) * rng.choice([0.5, 2.0], (k, 1))
    u[:k], v[:k] = lx[pick] - vert[:, 0] + jitter[:, 0], ly[pick] - vert[:, 1] + jitter[:, 1]
    poses = np.stack([origin[0] + u * res, origin[1] + v * res, ang], axis=1)
    exp = oracle_verdicts(oracle, verts, cm, origin, res, poses)
    # what lies under each pose: the polygon's pixel box (what coop_collides_sparse lists the lethal cells of)
    px, py = np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)
    poly = _pixel_polygons(verts, res, ang)
    bx0, bx1 = px + np.floor(poly[:, :, 0].min(1)).astype(np.int64), px + np.ceil(poly[:, :, 0].max(1)).astype(np.int64)
    by0, by1 = py + np.floor(poly[:, :, 1].min(1)).astype(np.int64), py + np.ceil(poly[:, :, 1].max(1)).astype(np.int64)
    integral = np.zeros((side_r + 1, side_c + 1), dtype=np.int64)
    integral[1:, 1:] = np.cumsum(np.cumsum(cm == 254, axis=0), axis=1)

    def count(x0, x1, y0, y1):   # lethal cells in columns x0..x1, rows y0..y1 (inclusive), clipped to the map
        x0, x1 = np.clip(x0, 0, side_c), np.clip(x1 + 1, 0, side_c)
        y0, y1 = np.clip(y0, 0, side_r), np.clip(y1 + 1, 0, side_r)
        ok = (x1 > x0) & (y1 > y0)
        return np.where(ok, integral[y1, x1] - integral[y0, x1] - integral[y1, x0] + integral[y0, x0], 0)
    # (one pixel in from the float box on every side: a lower bound whatever the rounding of the vertices does)
    lethal_under_box = count(bx0 + 1, bx1 - 1, by0 + 1, by1 - 1)
    box_area = np.maximum(bx1 - bx0 - 1, 0) * np.maximum(by1 - by0 - 1, 0)
    half = int(np.ceil(r_px))
    image_on_map = (px + half >= 0) & (px - half < side_c) & (py + half >= 0) & (py - half < side_r)
    box_on_map = (bx1 >= 0) & (bx0 < side_c) & (by1 >= 0) & (by0 < side_r)
    origin_on_map = (px >= 0) & (px < side_c) & (py >= 0) & (py < side_r)
    return dict(name=name, kind=kind, res=res, cm=cm, origin=origin, poses=poses, exp=exp, area=area, image=image,
                lethal_under_box=lethal_under_box, box_area=box_area, image_on_map=image_on_map, box_on_map=box_on_map,
                origin_on_map=origin_on_map)


# ---- a world for whole-step tests ------------------------------------------------------------------------------
def speckle_world(oracle, verts, res, seed, n_way=40):
    """A square world with a lethal border and isolated lethal cells (about one under every second footprint), a straight
    path across it, and no lethal cell near the path's first pose -> (costmap data, origin, path)"""
    rng = np.random.RandomState(seed)
    r = radius(verts)
    side_m = max(6.0, 4.0 * r)
    side = int(round(side_m / res))
    area = int(np.count_nonzero(oracle.pixel_footprint(0.3, verts, res)))
    cm = np.zeros((side, side), dtype=np.uint8)
    cm[rng.rand(side, side) < 0.7 / area] = 254
    origin = np.array([-0.5 * side_m, -0.5 * side_m])
    a, b = np.array([-0.28 * side_m, -0.2 * side_m]), np.array([0.28 * side_m, 0.2 * side_m])
    t = np.linspace(0.0, 1.0, n_way + seed % 3)[:, None]
    xy = a + t * (b - a)
    path = np.concatenate([xy, np.full((len(xy), 1), np.arctan2(b[1] - a[1], b[0] - a[0]))], axis=1)
    yy, xx = np.mgrid[0:side, 0:side]
    cm[np.hypot(origin[0] + xx * res - a[0], origin[1] + yy * res - a[1]) < r + 0.4] = 0
    cm[0, :] = cm[-1, :] = cm[:, 0] = cm[:, -1] = 254
    assert not oracle.pose_collides(path[0, 0], path[0, 1], path[0, 2], verts, cm, origin, res)
    return cm, origin, path

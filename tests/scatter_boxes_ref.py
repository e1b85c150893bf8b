"""numpy restatement of bcp_scatter_boxes as include/bcplan.h specifies it: Philox4x32-10 written out for arrays of
counters, the candidate box in float64 (every product and sum a numpy operation of its own), the pixel set by
oracle.fill_poly (the CPU's cv2.fillPoly), the two rejections, the first n_boxes accepted attempts in attempt order, and the
argument checks in their order.  Nothing here reads the library under test."""
import functools
import os

import numpy as np

import oracle

M32 = np.uint64(0xFFFFFFFF)
MAX_BOXES, MAX_ATTEMPTS, MAX_YAWS, MAX_KEEP, MAX_SIDE = 64, 4096, 4096, 16, 2048
WORDS = 9
LETHAL = 254
SHORT, REVERTED = 1, 2


def philox4x32_10(counter, key):
    """counter uint32 [..., 4], key (k0, k1) -> uint32 [..., 4] (Salmon et al., SC'11)"""
    c = [np.asarray(counter, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _round in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def yaw_table(n_yaws):
    """(cos, sin) of the multiples of 2 pi / n_yaws, float64 [n_yaws, 2]: a caller's table, any other would do"""
    ang = np.arange(n_yaws, dtype=np.float64) * (2.0 * np.pi / n_yaws)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


def uniform(w):
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def candidates(m, max_attempts, n_yaws, seed, along, half_size, frame, yaw_cs, origin, resolution):
    """-> (float64 [max_attempts, 4, 2] rounded (px, py) of the four corners, still float64: nothing is converted before the
    range test)"""
    a = np.arange(max_attempts, dtype=np.uint32)
    ctr = np.zeros((max_attempts, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.uint32(m & 0xFFFFFFFF), np.uint32((m >> 32) & 0xFFFFFFFF), a
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = philox4x32_10(ctr, key)
    ctr[:, 3] = 1
    v0 = philox4x32_10(ctr, key)[:, 0]
    f64 = np.float64
    t_lo, t_hi, h_lo, h_hi = f64(along[0]), f64(along[1]), f64(half_size[0]), f64(half_size[1])
    t = t_lo + uniform(w[:, 0]) * (t_hi - t_lo)
    l = 2.0 * uniform(w[:, 1]) - 1.0
    hx = h_lo + uniform(w[:, 2]) * (h_hi - h_lo)
    hy = h_lo + uniform(w[:, 3]) * (h_hi - h_lo)
    k = ((v0.astype(np.uint64) * np.uint64(n_yaws)) >> np.uint64(32)).astype(np.int64)
    yaw_cs = np.asarray(yaw_cs, dtype=np.float64)
    c, s = yaw_cs[k, 0], yaw_cs[k, 1]
    ax, ay, dx, dy, nx, ny = (f64(x) for x in frame)
    cx = (ax + t * dx) + l * nx
    cy = (ay + t * dy) + l * ny
    inv_res = f64(1.0) / f64(resolution)
    out = np.empty((max_attempts, 4, 2), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q, (sx, sy) in enumerate(((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))):
            wx = (cx + (sx * hx) * c) - (sy * hy) * s
            wy = (cy + (sx * hx) * s) + (sy * hy) * c
            out[:, q, 0] = np.rint((wx - f64(origin[0])) * inv_res)
            out[:, q, 1] = np.rint((wy - f64(origin[1])) * inv_res)
    return out


def pixel_set(shape, verts):
    """bool [rows, cols]: what cv2.fillPoly writes for the int contour verts [4, 2] of (x, y)"""
    img = np.zeros(shape, dtype=np.uint8)
    oracle.fill_poly(img, np.asarray(verts, dtype=np.int32), LETHAL)
    return img == LETHAL


def scatter_entry(data, valid, origin, resolution, m, n_boxes, max_attempts, n_yaws, seed, along, half_size, frame, keep,
                  yaw_cs):
    """One entry -> (new map, boxes int32 [n_boxes, 9], count, verdicts: per attempt tried 'out' / 'keep' / 'ok')"""
    data = np.array(data, dtype=np.uint8)
    rows, cols = data.shape
    vr = min(max(int(valid[0]), 0), rows)
    vc = min(max(int(valid[1]), 0), cols)
    cand = candidates(m, max_attempts, n_yaws, seed, along, half_size, frame, yaw_cs, origin, resolution)
    boxes = np.zeros((n_boxes, WORDS), dtype=np.int32)
    keep = np.asarray(keep, dtype=np.int64).reshape(-1, 3)
    count, verdicts = 0, []
    for a in range(max_attempts):
        if count == n_boxes:
            break
        p = cand[a]
        with np.errstate(invalid="ignore"):
            inside = bool(((p[:, 0] >= 0) & (p[:, 0] < vc) & (p[:, 1] >= 0) & (p[:, 1] < vr)).all())
        if not inside:
            verdicts.append("out")
            continue
        verts = p.astype(np.int32)
        cells = pixel_set((rows, cols), verts)
        rr, cc = np.nonzero(cells)
        hit = False
        for kr, kc, d2 in keep:
            if d2 >= 0 and ((rr - kr) ** 2 + (cc - kc) ** 2 <= d2).any():
                hit = True
        if hit:
            verdicts.append("keep")
            continue
        verdicts.append("ok")
        boxes[count, 0] = a
        boxes[count, 1:] = verts.reshape(8)
        count += 1
        data[cells] = LETHAL
    return data, boxes, count, verdicts


def scatter(data, valid, origins, resolution, n_boxes, max_attempts, n_yaws, seed, along, half_size, frame, keep, yaw_cs,
            first_entry=0):
    """The batch: data uint8 [n, rows, cols], valid [n, 2] or None, origins [n, 2], frame [n, 6], keep [n, K, 3] or None
    -> (maps, boxes int32 [n, n_boxes, 9], counts int32 [n])"""
    data = np.asarray(data, dtype=np.uint8)
    n = data.shape[0]
    out = np.empty_like(data)
    boxes = np.zeros((n, n_boxes, WORDS), dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    for i in range(n):
        v = data.shape[1:] if valid is None else valid[i]
        k = np.zeros((0, 3), dtype=np.int64) if keep is None else keep[i]
        out[i], boxes[i], counts[i], _ = scatter_entry(data[i], v, origins[i], resolution, first_entry + i, n_boxes,
                                                       max_attempts, n_yaws, seed, along, half_size, frame[i], k, yaw_cs)
    return out, boxes, counts


def check_args(have_handle, have_params, n_maps, rows, cols, resolution, n_boxes, max_attempts, n_yaws, n_keep, t_lo, t_hi,
               h_lo, h_hi, have_valid_rows, have_valid_cols, have_arrays, have_keep):
    """what bcp_scatter_boxes refuses, by number, in the order it looks (0 = accepted)"""
    fin = np.isfinite
    if not have_handle:
        return 1
    if not have_params:
        return 2
    if n_maps < 0:
        return 3
    if not (1 <= rows <= MAX_SIDE and 1 <= cols <= MAX_SIDE):
        return 4
    if not (resolution > 0 and fin(resolution)):
        return 5
    if not 1 <= n_boxes <= MAX_BOXES:
        return 6
    if not 1 <= max_attempts <= MAX_ATTEMPTS:
        return 7
    if not 1 <= n_yaws <= MAX_YAWS:
        return 8
    if not 0 <= n_keep <= MAX_KEEP:
        return 9
    if not (fin(t_lo) and fin(t_hi) and t_lo <= t_hi):
        return 10
    if not (fin(h_hi) and h_lo >= 0 and h_lo <= h_hi):
        return 11
    if not (np.float64(4.0) * np.float64(h_hi)) * (np.float64(1.0) / np.float64(resolution)) + 2.0 <= min(rows, cols):
        return 12
    if bool(have_valid_rows) != bool(have_valid_cols):
        return 13
    if n_maps > 0 and (not have_arrays or (n_keep > 0 and not have_keep)):
        return 14
    return 0


# ---- the reference worlds (tests/golden/g9_mini_geometry.npz) and their frames, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def golden():
    """-> (maps uint8 [48, 183, 183], origins [48, 2], resolution, starts [48, 3], goals [48, 3])"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_mini_geometry.npz"))
    cols = int(g["map_shape"][1])
    n = len(g["lens"])
    maps = (np.unpackbits(g["maps"][:n], axis=2)[:, :, :cols].astype(bool) * np.uint8(LETHAL)).astype(np.uint8)
    ends = np.concatenate([[0], np.cumsum(g["lens"])]).astype(np.int64)
    paths = g["paths"].astype(np.float64)
    starts = np.stack([paths[ends[k]] for k in range(n)])
    goals = np.stack([paths[ends[k + 1] - 1] for k in range(n)])
    origins = np.tile(g["origin"].astype(np.float64), (n, 1))
    for arr in (maps, origins, starts, goals):
        arr.setflags(write=False)
    return maps, origins, float(g["resolution"]), starts, goals


def frames(starts, goals, lateral):
    """frame [n, 6] = (start, goal - start, lateral * unit normal) of straight paths: what scatter_obstacles derives"""
    starts, goals = np.asarray(starts, dtype=np.float64), np.asarray(goals, dtype=np.float64)
    d = goals[:, :2] - starts[:, :2]
    norm = np.hypot(d[:, 0], d[:, 1])
    norm = np.where(norm > 0, norm, 1.0)
    normal = np.stack([-d[:, 1], d[:, 0]], axis=1) / norm[:, None]
    return np.ascontiguousarray(np.concatenate([starts[:, :2], d, lateral * normal], axis=1))


def cells_of(points, origins, resolution):
    """(row, col) int64 [n, 2] of world points [n, >= 2], world_to_pixel's expression"""
    inv = np.float64(1.0) / np.float64(resolution)
    col = np.rint((points[:, 0] - origins[:, 0]) * inv)
    row = np.rint((points[:, 1] - origins[:, 1]) * inv)
    return np.stack([row, col], axis=1).astype(np.int64)


def keep_outs(starts, goals, origins, resolution, d2):
    """keep int32 [n, 2, 3]: the start and goal cells with squared radius d2"""
    s, g = cells_of(starts, origins, resolution), cells_of(goals, origins, resolution)
    keep = np.zeros((len(s), 2, 3), dtype=np.int32)
    keep[:, 0, :2], keep[:, 1, :2], keep[:, :, 2] = s, g, d2
    return keep


# the dense configuration of the issue: 12 boxes of half sizes 0.2 .. 0.5 m, along (0.2, 0.8), 2 m to either side, a keep-out
# of 0.9 m about start and goal, 16 yaws at multiples of pi / 8, seed 7, 32 attempts
DENSE = dict(n_boxes=12, max_attempts=32, n_yaws=16, seed=7, along=(0.2, 0.8), half_size=(0.2, 0.5))
DENSE_LATERAL, DENSE_KEEP_M = 2.0, 0.9


@functools.lru_cache(maxsize=None)
def dense_golden():
    """-> (maps, boxes, counts, frame, keep, yaw_cs) of the dense configuration on the 48 golden worlds"""
    maps, origins, res, starts, goals = golden()
    frame = frames(starts, goals, DENSE_LATERAL)
    d2 = int(np.ceil(DENSE_KEEP_M / res)) ** 2
    keep = keep_outs(starts, goals, origins, res, d2)
    yaw_cs = yaw_table(DENSE["n_yaws"])
    out, boxes, counts = scatter(maps, None, origins, res, frame=frame, keep=keep, yaw_cs=yaw_cs, **DENSE)
    for arr in (out, boxes, counts, frame, keep, yaw_cs):
        arr.setflags(write=False)
    return out, boxes, counts, frame, keep, yaw_cs


# ---- is the goal still reachable?  (what ensure_route asks of bcp_goal_field, restated without a field)
def free_mask(data, valid, clearance_d2, seed_cell):
    """bool [rows, cols]: inside the valid shape and farther than clearance_d2 (squared, in cells) from every cell == 254 of
    the valid shape, plus the seed cell: bcp_goal_field's free cells, by shifting the obstacle mask over the disc"""
    data = np.asarray(data, dtype=np.uint8)
    rows, cols = data.shape
    vr, vc = min(max(int(valid[0]), 0), rows), min(max(int(valid[1]), 0), cols)
    reach = int(np.floor(np.sqrt(clearance_d2)))
    pad = np.zeros((rows + 2 * reach, cols + 2 * reach), dtype=bool)
    pad[reach:reach + vr, reach:reach + vc] = data[:vr, :vc] == LETHAL
    blocked = np.zeros((rows, cols), dtype=bool)
    for dr in range(-reach, reach + 1):
        for dc in range(-reach, reach + 1):
            if dr * dr + dc * dc <= clearance_d2:
                blocked |= pad[reach + dr:reach + dr + rows, reach + dc:reach + dc + cols]
    free = np.zeros((rows, cols), dtype=bool)
    free[:vr, :vc] = ~blocked[:vr, :vc]
    if 0 <= seed_cell[0] < vr and 0 <= seed_cell[1] < vc:
        free[seed_cell[0], seed_cell[1]] = True
    return free


def routable(data, valid, clearance_d2, start_cell, goal_cell):
    """True iff bcp_goal_field seeded at goal_cell gives start_cell a value.  A corner step needs both edge cells it passes
    between, so it never reaches what two edge steps do not: the cells with a value are the 4-connected component of the
    seed in the free mask."""
    free = free_mask(data, valid, clearance_d2, goal_cell)
    rows, cols = free.shape
    sr, sc = int(start_cell[0]), int(start_cell[1])
    gr, gc = int(goal_cell[0]), int(goal_cell[1])
    if not (0 <= sr < rows and 0 <= sc < cols and 0 <= gr < rows and 0 <= gc < cols and free[gr, gc] and free[sr, sc]):
        return False
    seen = np.zeros_like(free)
    seen[gr, gc] = True
    front = [(gr, gc)]
    fr = free.tolist()
    sn = seen.tolist()
    while front:
        nxt = []
        for r, c in front:
            for rr, cc in ((r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)):
                if 0 <= rr < rows and 0 <= cc < cols and fr[rr][cc] and not sn[rr][cc]:
                    sn[rr][cc] = True
                    nxt.append((rr, cc))
        if sn[sr][sc]:
            return True
        front = nxt
    return bool(sn[sr][sc])


@functools.lru_cache(maxsize=None)
def dense_golden_routable(clearance_d2=151):
    """bool [48]: which worlds of dense_golden() still have a route at clearance_d2"""
    maps, origins, res, starts, goals = golden()
    out = dense_golden()[0]
    s, g = cells_of(starts, origins, res), cells_of(goals, origins, res)
    return np.array([routable(out[k], out[k].shape, clearance_d2, s[k], g[k]) for k in range(len(out))])

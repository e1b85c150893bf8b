"""numpy / heapq restatement of bcp_goal_field and bcp_goal_field_sample as include/bcplan.h specifies them: the blocked
mask from brute-force exact squared distances (inflate_ref), Dijkstra with the corner rule and the saturating addition, a
Jacobi relaxation that counts its passes and honours a cap, and the sampling rule with its carrot walk in float64."""
import functools
import heapq
import os

import numpy as np

import inflate_ref

ORTHO, DIAG, FAR, NONE = 12, 17, 65534, 65535
# neighbour k: E, NE, N, NW, W, SW, S, SE as (dcol, drow)
NBR = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
WEIGHT = tuple(DIAG if k & 1 else ORTHO for k in range(8))


def clamp_valid(shape, valid=None):
    rows, cols = shape
    if valid is None:
        return rows, cols
    return min(max(int(valid[0]), 0), rows), min(max(int(valid[1]), 0), cols)


def usable_seeds(seeds, shape, valid=None):
    vr, vc = clamp_valid(shape, valid)
    return [(int(r), int(c)) for r, c in np.asarray(seeds, dtype=np.int64).reshape(-1, 2) if 0 <= r < vr and 0 <= c < vc]


def free_mask(data, seeds, clearance_d2, valid=None):
    """bool [rows, cols]: the cells a route may use -- inside the valid shape and farther than clearance_d2 (squared, in
    cells) from every obstacle cell, plus every usable seed."""
    data = np.asarray(data, dtype=np.uint8)
    vr, vc = clamp_valid(data.shape, valid)
    free = np.zeros(data.shape, dtype=bool)
    free[:vr, :vc] = (inflate_ref.squared_distances(data, (vr, vc)) > clearance_d2)[:vr, :vc]
    for r, c in usable_seeds(seeds, data.shape, valid):
        free[r, c] = True
    return free


def dijkstra_on(free, seeds):
    """uint16 [rows, cols] on a free mask with seeds [(row, col)] inside it"""
    rows, cols = free.shape
    dist = np.full((rows, cols), NONE, dtype=np.int64)
    heap = []
    for r, c in seeds:
        dist[r, c] = 0
        heap.append((0, r, c))
    heapq.heapify(heap)
    fr = np.zeros((rows + 2, cols + 2), dtype=bool)   # (a border of walls: no bounds tests below)
    fr[1:-1, 1:-1] = free
    fr = fr.tolist()
    d = dist.tolist()
    while heap:
        v, r, c = heapq.heappop(heap)
        if v != d[r][c]:
            continue
        for k in range(8):
            dc, dr = NBR[k]
            rr, cc = r + dr, c + dc
            if not fr[rr + 1][cc + 1]:
                continue
            if k & 1 and not (fr[r + 1][cc + 1] and fr[rr + 1][c + 1]):   # both edge cells the move passes between
                continue
            nv = min(v + WEIGHT[k], FAR)
            if nv < d[rr][cc]:
                d[rr][cc] = nv
                heapq.heappush(heap, (nv, rr, cc))
    return np.array(d, dtype=np.int64).astype(np.uint16)


def dijkstra(data, seeds, clearance_d2, valid=None):
    data = np.asarray(data, dtype=np.uint8)
    return dijkstra_on(free_mask(data, seeds, clearance_d2, valid), usable_seeds(seeds, data.shape, valid))


def jacobi_on(free, seeds, max_passes=0):
    """-> (uint16 field, passes run, gave_up): every pass relaxes every cell from the values of the pass before"""
    rows, cols = free.shape
    cap = max_passes if max_passes > 0 else rows * cols
    big = np.int64(1) << 40
    pad = np.full((rows + 2, cols + 2), big, dtype=np.int64)
    fr = np.zeros((rows + 2, cols + 2), dtype=bool)
    fr[1:-1, 1:-1] = free
    for r, c in seeds:
        pad[r + 1, c + 1] = 0
    passes, gave_up = 0, 0
    while True:
        if passes == cap:
            gave_up = 1
            break
        passes += 1
        best = pad[1:-1, 1:-1].copy()
        for k in range(8):
            dc, dr = NBR[k]
            src = pad[1 + dr:rows + 1 + dr, 1 + dc:cols + 1 + dc]
            ok = fr[1 + dr:rows + 1 + dr, 1 + dc:cols + 1 + dc]
            if k & 1:
                ok = ok & fr[1:rows + 1, 1 + dc:cols + 1 + dc] & fr[1 + dr:rows + 1 + dr, 1:cols + 1]
            cand = np.where(ok & (src < big), np.minimum(src + WEIGHT[k], FAR), big)
            best = np.minimum(best, cand)
        best = np.where(free, best, big)
        if (best == pad[1:-1, 1:-1]).all():
            break
        pad[1:-1, 1:-1] = best
    out = pad[1:-1, 1:-1]
    return np.where(out >= big, NONE, out).astype(np.uint16), passes, gave_up


def jacobi(data, seeds, clearance_d2, valid=None, max_passes=0):
    data = np.asarray(data, dtype=np.uint8)
    return jacobi_on(free_mask(data, seeds, clearance_d2, valid), usable_seeds(seeds, data.shape, valid), max_passes)


def sample(fields, valids, origins, resolution, entry, poses, heading_cs, carrot_cells, max_dist):
    """bcp_goal_field_sample for rows with poses [n, 3] and (cos, sin) heading_cs [n, 2]; row i stands on map entry
    entry[i] (a negative entry: no result) with valid shape valids[entry] and origin origins[entry], and reads field
    entry[i] of fields uint16 [F, rows, cols], or field 0 when F == 1.
    -> out3 float32 [n, 3], cell_value int32 [n], carrot int32 [n, 2]"""
    fields = np.asarray(fields, dtype=np.uint16)
    n_f, rows, cols = fields.shape
    pad = np.full((n_f, rows + 2, cols + 2), NONE, dtype=np.int64)
    pad[:, 1:-1, 1:-1] = fields
    poses = np.asarray(poses, dtype=np.float64)
    cs = np.asarray(heading_cs, dtype=np.float64)
    entry = np.asarray(entry, dtype=np.int64)
    n = len(poses)
    res, inv_res = np.float64(resolution), np.float64(1.0) / np.float64(resolution)
    known = entry >= 0
    e = np.where(known, entry, 0)
    f = np.zeros(n, dtype=np.int64) if n_f == 1 else e
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 2)
    valids = np.array([clamp_valid((rows, cols), v) for v in valids], dtype=np.int64).reshape(-1, 2)
    ox, oy = origins[e, 0], origins[e, 1]
    vr, vc = valids[e, 0], valids[e, 1]

    def look(r, c):   # the field inside the row's valid shape, NONE outside it
        inside = (r >= 0) & (r < vr) & (c >= 0) & (c < vc)
        return np.where(inside, pad[f, np.clip(r, -1, rows) + 1, np.clip(c, -1, cols) + 1], NONE)

    x, y = poses[:, 0], poses[:, 1]
    with np.errstate(all="ignore"):
        fc, fr = np.rint((x - ox) * inv_res), np.rint((y - oy) * inv_res)
        ok = known & np.isfinite(poses).all(axis=1) & (fc >= 0) & (fc < vc) & (fr >= 0) & (fr < vr)
    r = np.where(ok, fr, 0).astype(np.int64)
    c = np.where(ok, fc, 0).astype(np.int64)
    v = look(r, c)
    ok &= v != NONE
    out3 = np.zeros((n, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        out3[:, 0] = np.where(ok, np.minimum((v.astype(np.float64) * res) / np.float64(12.0), np.float64(max_dist)),
                              np.float64(max_dist)).astype(np.float32)
    value = np.where(ok, v, NONE).astype(np.int32)
    r0, c0 = r.copy(), c.copy()
    cur = v.copy()
    active = ok.copy()
    weight = np.array(WEIGHT, dtype=np.int64)[:, None]
    dcols, drows = np.array([d[0] for d in NBR]), np.array([d[1] for d in NBR])
    big = np.int64(1) << 40
    for _step in range(int(carrot_cells)):
        active &= cur != 0
        if not active.any():
            break
        nb = np.stack([look(r + dr, c + dc) for dc, dr in NBR])
        adm = nb != NONE
        for k in (1, 3, 5, 7):
            adm[k] &= (nb[k - 1] != NONE) & (nb[(k + 1) & 7] != NONE)
        cost = np.where(adm, nb + weight, big)
        k = np.argmin(cost, axis=0)   # (the first minimum: the lowest k)
        active &= adm.any(axis=0)
        r = np.where(active, r + drows[k], r)
        c = np.where(active, c + dcols[k], c)
        cur = look(r, c)
    carrot = np.where(ok[:, None], np.stack([r, c], axis=1), -1).astype(np.int32)
    moved = ok & ((r != r0) | (c != c0))
    with np.errstate(all="ignore"):
        dx = (ox + c.astype(np.float64) * res) - x
        dy = (oy + r.astype(np.float64) * res) - y
        norm = np.sqrt(dx * dx + dy * dy)
        ux, uy = dx / norm, dy / norm
        bx = ux * cs[:, 0] + uy * cs[:, 1]
        by = uy * cs[:, 0] - ux * cs[:, 1]
    out3[:, 1] = np.where(moved, bx, 0.0).astype(np.float32)
    out3[:, 2] = np.where(moved, by, 0.0).astype(np.float32)
    return out3, value, carrot


def check_field_args(have_handle, n_maps, have_data, have_seeds, have_out, rows, cols, n_seeds, clearance_d2, max_passes,
                     have_valid_rows, have_valid_cols, shared):
    """goal_field_check_args: 0 = accepted, else the refusal's number"""
    if not have_handle:
        return 1
    if n_maps < 0:
        return 2
    if not (1 <= rows <= 2048 and 1 <= cols <= 2048):
        return 3
    if not 1 <= n_seeds <= 4096:
        return 4
    if not 0 <= clearance_d2 <= 16129:
        return 5
    if max_passes < 0:
        return 6
    if bool(have_valid_rows) != bool(have_valid_cols):
        return 7
    if shared and have_valid_rows:
        return 8
    if n_maps > 0 and not (have_data and have_seeds and have_out):
        return 9
    return 0


def check_sample_args(have_handle, have_field, have_out3, carrot_cells, max_dist, n, n_envs, have_poses, have_row_env,
                      final_form, rows, cols, map_rows, map_cols, n_fields, n_entries):
    if not (have_handle and have_field and have_out3):
        return 1
    if not 1 <= carrot_cells <= 256:
        return 2
    if not max_dist > 0:
        return 3
    if not final_form and (n <= 0 or (not have_poses and n != n_envs)):
        return 4
    if not have_poses and have_row_env:
        return 5
    if n_entries > 0 and (rows != map_rows or cols != map_cols):
        return 6
    if n_entries > 0 and n_fields != 1 and n_fields != n_entries:
        return 7
    return 0


# ---- the maps the tests share
def diagonal_wall(side=9):
    """an anti-diagonal 8-connected wall, cells touching at corners only"""
    data = np.zeros((side, side), dtype=np.uint8)
    data[np.arange(side), side - 1 - np.arange(side)] = 254
    return data


def serpentine(side):
    """walls on every second row with a one-cell gap at alternating ends: one long corridor from (0, 0)"""
    data = np.zeros((side, side), dtype=np.uint8)
    for k, r in enumerate(range(1, side, 2)):
        data[r, :] = 254
        data[r, side - 1 if k % 2 == 0 else 0] = 0
    return data


# ---- the reference worlds (tests/golden/g9_mini_geometry.npz), computed once per session and left unchanged
@functools.lru_cache(maxsize=None)
def mini_world(k):
    """-> (data uint8 [183, 183], origin [2], resolution, goal cell (row, col), start cell (row, col)) of reference world k"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_mini_geometry.npz"))
    cols = int(g["map_shape"][1])
    data = (np.unpackbits(g["maps"][k], axis=1)[:, :cols].astype(bool) * np.uint8(254)).astype(np.uint8)
    origin, res = g["origin"].astype(np.float64), float(g["resolution"])
    first = int(g["lens"][:k].sum())
    path = g["paths"][first:first + int(g["lens"][k])]

    def cell(p):
        return int(np.rint((p[1] - origin[1]) * (1.0 / res))), int(np.rint((p[0] - origin[0]) * (1.0 / res)))

    data.setflags(write=False)
    return data, origin, res, cell(path[-1]), cell(path[0])


@functools.lru_cache(maxsize=None)
def mini_field(k, clearance_d2):
    """Dijkstra's field of reference world k seeded at its goal"""
    data, _origin, _res, goal, _start = mini_world(k)
    field = dijkstra(data, [goal], clearance_d2)
    field.setflags(write=False)
    return field


def edge_poses(rng, n, field, origin, resolution, seed_cell):
    """float64 [n, 3] poses for a sampling test on `field`: most uniform over the map with a margin outside it, then rows on
    the seed cell, inside cells without a value (the blocked band), on half-cell boundaries (the rounding is half to even),
    and rows that are not finite or far outside."""
    rows, cols = field.shape
    ox, oy = origin
    poses = np.stack([rng.uniform(ox - 5 * resolution, ox + (cols + 5) * resolution, n),
                      rng.uniform(oy - 5 * resolution, oy + (rows + 5) * resolution, n),
                      rng.uniform(-4.0, 4.0, n)], axis=1)
    poses[0, :2] = [ox + seed_cell[1] * resolution, oy + seed_cell[0] * resolution]
    poses[1, :2] = poses[0, :2] + 0.3 * resolution
    none_r, none_c = np.nonzero(field == NONE)
    pick = rng.randint(0, len(none_r), 40)
    poses[2:42, 0] = ox + (none_c[pick] + rng.uniform(-0.4, 0.4, 40)) * resolution
    poses[2:42, 1] = oy + (none_r[pick] + rng.uniform(-0.4, 0.4, 40)) * resolution
    ks = rng.randint(0, min(rows, cols) - 1, size=(60, 2)).astype(np.float64)
    poses[42:102, 0] = ox + (ks[:, 0] + 0.5) * resolution     # col + 0.5, as near as the arithmetic lets it be
    poses[72:132, 1] = oy + (rng.randint(0, rows - 1, 60) + 0.5) * resolution
    poses[132, 0] = np.nan
    poses[133, 1] = np.inf
    poses[134, 2] = np.nan
    poses[135, 2] = -np.inf
    poses[136, :2] = [1e300, -1e300]
    poses[137, :2] = [ox - 0.5 * resolution, oy - 0.5 * resolution]     # rounds to cell (-0, -0): inside
    poses[138, :2] = [ox - 0.51 * resolution, oy]                        # rounds to col -1: outside
    poses[139, :2] = [ox + (cols - 0.5) * resolution, oy + (rows - 1) * resolution]
    return poses

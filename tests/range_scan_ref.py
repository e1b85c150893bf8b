"""The contract of bcp_range_scan (include/bcplan.h) restated in numpy: vectorised over rays, one Python loop over the
trips of the walk.  All arithmetic is float64, every product, quotient and sum rounded on its own, in the order the
header gives.  The reference takes (cos, sin) of every row's heading as an input: the library writes the ones it used to
heading_cs_out, numpy's may differ from them in the last place, and a walk is only bit for bit the same from the same
direction."""
import numpy as np

MAX_BEAMS = 1024
MAX_CELLS = 4096.0
LETHAL = 254


def trip_bound(cells):
    """2 * ceil(R) + 4: after that many trips the walk has certainly ended"""
    return 2 * int(np.ceil(cells)) + 4


def beam_table(angles):
    a = np.asarray(angles, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


def wrapper_angles(n_beams, fov):
    """BatchedRangeScan's beams: -fov/2 + fov * (k + 0.5) / n_beams"""
    return -fov / 2 + fov * (np.arange(n_beams) + 0.5) / n_beams


def pack_bits(lethal):
    """bool [rows, cols] -> uint32 [rows, wpr], bit (col & 31) of word col >> 5 (the library's row-major mask)"""
    rows, cols = lethal.shape
    wpr = (cols + 31) // 32
    padded = np.zeros((rows, wpr * 32), dtype=np.uint64)
    padded[:, :cols] = lethal
    return (padded.reshape(rows, wpr, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def range_scan(data, valid_rows, valid_cols, origins, resolution, entry, poses, heading_cs, beam_cs, max_range):
    """data uint8 [E, rows, cols] raw costmaps, valid_rows / valid_cols int [E], origins float64 [E, 2], resolution the
    float64 given to bcp_set_costmaps; entry int [n] (the map entry of every row), poses float64 [n, 3], heading_cs
    float64 [n, 2], beam_cs float64 [B, 2].  -> ranges float32 [n, B], hit int32 [n, B], trips int [n, B], bound."""
    data = np.asarray(data)
    entry = np.asarray(entry, dtype=np.int64)
    poses = np.asarray(poses, dtype=np.float64)
    heading_cs = np.asarray(heading_cs, dtype=np.float64)
    beam_cs = np.asarray(beam_cs, dtype=np.float64)
    n, n_beams = len(poses), len(beam_cs)
    cols_alloc = data.shape[2]
    resolution, max_range = np.float64(resolution), np.float64(max_range)
    with np.errstate(all="ignore"):
        inv_res = np.float64(1.0) / resolution
        x, y, th = poses[:, 0], poses[:, 1], poses[:, 2]
        u = (x - np.asarray(origins)[entry, 0]) * inv_res + 0.5
        v = (y - np.asarray(origins)[entry, 1]) * inv_res + 0.5
        cells = max_range * inv_res
        bound = trip_bound(cells)
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(th) & (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        u = np.where(ok, u, 0.0)[:, None]
        v = np.where(ok, v, 0.0)[:, None]
        reach = np.broadcast_to(np.where(ok, cells, 0.0)[:, None], (n, n_beams))
        c, s = heading_cs[:, 0:1], heading_cs[:, 1:2]
        cb, sb = beam_cs[None, :, 0], beam_cs[None, :, 1]
        dx = c * cb - s * sb
        dy = s * cb + c * sb
        col = np.broadcast_to(np.floor(u), (n, n_beams)).copy()
        row = np.broadcast_to(np.floor(v), (n, n_beams)).copy()
        sx = np.where(dx > 0, 1.0, -1.0)
        sy = np.where(dy > 0, 1.0, -1.0)
        tdx = np.where(dx != 0, np.abs(1.0 / dx), np.inf)
        tdy = np.where(dy != 0, np.abs(1.0 / dy), np.inf)
        tmx = np.where(dx > 0, (col + 1 - u) / dx, np.where(dx < 0, (col - u) / dx, np.inf))
        tmy = np.where(dy > 0, (row + 1 - v) / dy, np.where(dy < 0, (row - v) / dy, np.inf))
        t = np.zeros((n, n_beams))
        e = np.broadcast_to(entry[:, None], (n, n_beams))
        vr = np.asarray(valid_rows, dtype=np.int64)[e]
        vc = np.asarray(valid_cols, dtype=np.int64)[e]
        ranges = np.full((n, n_beams), np.float32(max_range), dtype=np.float32)
        hit = np.full((n, n_beams), -1, dtype=np.int32)
        trips = np.zeros((n, n_beams), dtype=np.int64)
        walking = np.ones((n, n_beams), dtype=bool)
        for trip in range(bound):
            walking &= t < reach
            if not walking.any():
                break
            trips[walking] = trip + 1
            inside = walking & (row >= 0) & (row < vr) & (col >= 0) & (col < vc)
            ri = np.where(inside, row, 0).astype(np.int64)
            ci = np.where(inside, col, 0).astype(np.int64)
            found = inside & (data[e, ri, ci] == LETHAL)
            ranges[found] = (t[found] * resolution).astype(np.float32)
            hit[found] = (ri[found] * cols_alloc + ci[found]).astype(np.int32)
            walking &= ~found
            in_x = tmx < tmy
            mx, my = walking & in_x, walking & ~in_x
            t[mx] = tmx[mx]
            tmx[mx] += tdx[mx]
            col[mx] += sx[mx]
            t[my] = tmy[my]
            tmy[my] += tdy[my]
            row[my] += sy[my]
    return ranges, hit, trips, bound


def edge_rows(rng, data, valid, origin, res, n_inside=24):
    """poses [16 + n_inside, 3] with the edge cases the contract names, on any map: rows 0-3 in a lethal cell, 4-9 outside the
    map on every side (9: out of reach), 10-15 non-finite or beyond 2^30 cells, the rest anywhere inside"""
    rows, cols = valid
    w, h = cols * res, rows * res
    lr, lc = np.nonzero(data[:rows, :cols] == LETHAL)
    k = rng.randint(len(lr), size=4)
    in_lethal = np.stack([origin[0] + (lc[k] + rng.uniform(-0.4, 0.4, 4)) * res, origin[1] + (lr[k] + rng.uniform(-0.4, 0.4, 4)) * res,
                          rng.uniform(-np.pi, np.pi, 4)], axis=1)
    cx, cy = origin[0] + w / 2, origin[1] + h / 2
    outside = np.array([[origin[0] - 0.7, cy, 0.1], [origin[0] + w + 0.6, cy, np.pi - 0.2], [cx, origin[1] - 0.9, 1.4],
                        [cx, origin[1] + h + 0.8, -1.5], [origin[0] - 0.3, origin[1] - 0.3, 0.8], [origin[0] - 50.0, cy, 0.0]])
    odd = np.array([[np.nan, cy, 0.0], [cx, np.inf, 0.0], [cx, cy, np.nan], [cx, cy, -np.inf], [1e12, cy, 0.0], [cx, -3e11, 0.0]])
    inside = np.stack([origin[0] + rng.uniform(0, w, n_inside), origin[1] + rng.uniform(0, h, n_inside), rng.uniform(-7, 7, n_inside)], axis=1)
    return np.concatenate([in_lethal, outside, odd, inside])


def check_args(have_handle, have_beams, have_ranges, n_beams, n, n_envs, have_poses, final_form, max_range, inv_res):
    """scan_check_args (csrc/bcp_scan_march.h): 0 ok, 1 null argument, 2 n_beams, 3 n, 4 max_range"""
    if not (have_handle and have_beams and have_ranges):
        return 1
    if n_beams < 1 or n_beams > MAX_BEAMS:
        return 2
    if not final_form and (n <= 0 or (not have_poses and n != n_envs)):
        return 3
    with np.errstate(all="ignore"):
        if not (np.isfinite(max_range) and max_range > 0 and np.float64(max_range) * np.float64(inv_res) <= MAX_CELLS):
            return 4
    return 0

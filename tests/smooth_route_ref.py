"""numpy / Python restatement of bcp_smooth_route as include/bcplan.h specifies it: passable cells, clear(a, b), the pull,
the blend of a corner with its halvings, the stretches, the count, LONG, the zero tail, the headings, the status bits, the
provider's initial state and info -- and the argument checks in their order.  Written from the header's text, not from the
kernel.  Python floats are IEEE float64 and every operation rounds on its own, as the contract asks."""
import math

import numpy as np

import goal_field_ref as GR
import goal_route_ref as RR

LONG, TOO_CLOSE, NO_ROUTE, BLOCKED = 1, 2, 4, 16
MAX_LEN = 4096
TOO_MANY = MAX_LEN + 1
compare = RR.compare
away_from_knife_edges = RR.away_from_knife_edges


class Map(object):
    """one entry: its field, valid shape, origin and resolution"""

    def __init__(self, field, valid, origin, resolution):
        self.field = np.asarray(field)
        self.vr, self.vc = GR.clamp_valid(self.field.shape, valid)
        self.ox, self.oy = float(origin[0]), float(origin[1])
        self.inv_res = float(np.float64(1.0) / np.float64(resolution))

    def passable(self, r, c):
        return 0 <= r < self.vr and 0 <= c < self.vc and int(self.field[r, c]) != GR.NONE

    def cell_of(self, x, y):
        """(row, col), or None"""
        if not (math.isfinite(x) and math.isfinite(y)):
            return None
        fc, fr = float(np.rint((x - self.ox) * self.inv_res)), float(np.rint((y - self.oy) * self.inv_res))
        if not (0 <= fc < self.vc and 0 <= fr < self.vr):
            return None
        return int(fr), int(fc)


def clear(m, a, b, visited=None):
    """clear(a, b) between cells a, b = (row, col) or None; visited: a list that receives the cells stepped on"""
    if a is None or b is None:
        return False
    r, c = a
    if visited is not None:
        visited.append((r, c))
    if not m.passable(r, c):
        return False
    dc, dr = b[1] - a[1], b[0] - a[0]
    ax, ay, sx, sy = abs(dc), abs(dr), (1 if dc >= 0 else -1), (1 if dr >= 0 else -1)
    i = j = 0
    while i < ax or j < ay:
        if j == ay:
            side = -1
        elif i == ax:
            side = 1
        else:
            side = (2 * i + 1) * ay - (2 * j + 1) * ax
        if side == 0 and not (m.passable(r, c + sx) and m.passable(r + sy, c)):
            return False
        if side <= 0:
            c, i = c + sx, i + 1
        if side >= 0:
            r, j = r + sy, j + 1
        if visited is not None:
            visited.append((r, c))
        if not m.passable(r, c):
            return False
    return True


def pieces(length, step):
    q = length / step
    if not q >= 1.0:      # (a NaN too)
        return 1
    q = math.ceil(q) if math.isfinite(q) else q
    return TOO_MANY if q > MAX_LEN else int(q)


def legs(p, v, n):
    px, py, nx, ny = p[0] - v[0], p[1] - v[1], n[0] - v[0], n[1] - v[1]
    return math.sqrt(px * px + py * py), math.sqrt(nx * nx + ny * ny)


def corner(p, v, n, lp, ln, d, delta):
    fp, fn = d / lp, d / ln
    a = tuple(v[e] + (p[e] - v[e]) * fp for e in range(2))
    b = tuple(v[e] + (n[e] - v[e]) * fn for e in range(2))
    return a, b, pieces(2.0 * d, delta)


def blend_point(a, v, b, k, q):
    t = float(k) / float(q)
    u = 1.0 - t
    wa, wv, wb = u * u, (2.0 * t) * u, t * t
    return tuple(((a[e] * wa) + (v[e] * wv)) + (b[e] * wb) for e in range(2))


def blend(m, p, v, n, blend_len, delta, halvings):
    """-> (level or None for a sharp corner, A, B, q)"""
    lp, ln = legs(p, v, n)
    sharp = (None, tuple(v[:2]), tuple(v[:2]), 0)
    if not blend_len > 0.0 or lp == 0.0 or ln == 0.0:
        return sharp
    d = blend_len
    if lp / 3.0 < d:
        d = lp / 3.0
    if ln / 3.0 < d:
        d = ln / 3.0
    for level in range(halvings + 1):
        a, b, q = corner(p, v, n, lp, ln, d, delta)
        if q != TOO_MANY:
            cells = [m.cell_of(*blend_point(a, v, b, k, q)) for k in range(q + 1)]
            if all(clear(m, cells[k], cells[k + 1]) for k in range(q)):
                return level, a, b, q
        d = d / 2.0
    return sharp


def smooth_row(m, wp_in, length, look, blend_len, delta, halvings, max_len, reward_params=RR.REWARD_PARAMS, pure_pursuit=False,
               valid=True):
    """-> (way points float64 [max_len, 3], len, status, init [2], info [4])"""
    out = np.zeros((max_len, 3), dtype=np.float64)
    none = (out, 0, NO_ROUTE, np.zeros(2), np.zeros(4, dtype=np.int32))
    wp_in = np.asarray(wp_in, dtype=np.float64)
    n_in = min(int(length), wp_in.shape[0])
    if not valid or n_in < 2 or not np.isfinite(wp_in[:n_in]).all():
        return none
    pts = [tuple(float(x) for x in wp_in[k]) for k in range(n_in)]
    cells = [m.cell_of(p[0], p[1]) for p in pts]
    status, anchors, k = 0, [0], 0
    while k < n_in - 1:
        nxt = None
        for j in range(min(k + look, n_in - 1), k, -1):
            if clear(m, cells[k], cells[j]):
                nxt = j
                break
        if nxt is None:
            nxt, status = k + 1, status | BLOCKED
        anchors.append(nxt)
        k = nxt
    V = [pts[k] for k in anchors]
    M = len(V) - 1
    info = np.array([M + 1, 0, 0, 0], dtype=np.int32)
    corners = {}
    for t in range(1, M):
        level, a, b, q = blend(m, V[t - 1], V[t], V[t + 1], blend_len, delta, halvings)
        corners[t] = (a, b, q)
        info[3 if level is None else (1 if level == 0 else 2)] += 1
    written = [V[0][:2]]
    too_many = False
    for s in range(M):
        S = V[0][:2] if s == 0 else corners[s][1]
        E = V[M][:2] if s == M - 1 else corners[s + 1][0]
        dx, dy = E[0] - S[0], E[1] - S[1]
        q = pieces(math.sqrt(dx * dx + dy * dy), delta)
        if q == TOO_MANY:
            too_many = True
            break
        for i in range(1, q):
            t = float(i) / float(q)
            written.append((S[0] + (E[0] - S[0]) * t, S[1] + (E[1] - S[1]) * t))
        written.append((E[0], E[1]))
        if s < M - 1:
            a, b, q = corners[s + 1]
            for i in range(1, q + 1):
                written.append(blend_point(a, V[s + 1], b, i, q))
    if too_many or len(written) > max_len:
        return out, 0, status | LONG, np.zeros(2), info
    total = len(written)
    out[:total, :2] = np.array(written, dtype=np.float64)
    out[0, 2], out[total - 1, 2] = pts[0][2], pts[-1][2]
    for j in range(1, total - 1):
        dx, dy = out[j + 1, 0] - out[j, 0], out[j + 1, 1] - out[j, 1]
        out[j, 2] = pts[-1][2] if dx == 0.0 and dy == 0.0 else np.arctan2(dy, dx)
    min_dist, target, too_close = RR.provider_state(out[:total], reward_params, pure_pursuit)
    if too_close:
        status |= TOO_CLOSE
    return out, total, status, np.array([min_dist, float(target)]), info


def smooth(fields, valids, origins, resolution, entry, paths_in, lens_in, look, blend_len, delta, halvings, max_len,
           reward_params=RR.REWARD_PARAMS, pure_pursuit=False):
    """bcp_smooth_route for rows on map entries entry[i] (negative: NO_ROUTE), reading field entry[i] of fields uint16
    [F, rows, cols], or field 0 when F == 1.  -> paths [n, max_len, 3], lens, status, init [n, 2], info [n, 4]"""
    fields = np.asarray(fields)
    n = len(paths_in)
    paths = np.zeros((n, max_len, 3), dtype=np.float64)
    lens, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    init, info = np.zeros((n, 2), dtype=np.float64), np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        e = int(entry[i])
        if e < 0:
            status[i] = NO_ROUTE
            continue
        m = Map(fields[0 if fields.shape[0] == 1 else e], valids[e], origins[e], resolution)
        paths[i], lens[i], status[i], init[i], info[i] = smooth_row(m, paths_in[i], lens_in[i], look, blend_len, delta, halvings,
                                                                    max_len, reward_params, pure_pursuit)
    return paths, lens, status, init, info


def check_args(have_pointers, have_params, look, halvings, blend_len, delta, max_len_in, max_len, n, have_row_env,
               rows_are_entries, rows, cols, map_rows, map_cols, n_fields, n_entries, shared_map, overlap, bound_arrays):
    """smooth_check_args: 0 = accepted, else the refusal's number (1 .. 12 BCP_E_INVALID, 13 .. 16 BCP_E_STATE)"""
    if not (have_pointers and have_params):
        return 1
    if not 1 <= look <= 4096:
        return 2
    if not 0 <= halvings <= 8:
        return 3
    if not (blend_len >= 0.0 and math.isfinite(blend_len)):
        return 4
    if not (delta > 0.0 and math.isfinite(delta)):
        return 5
    if not 2 <= max_len_in <= 4096:
        return 6
    if not 2 <= max_len <= 4096:
        return 7
    if n <= 0:
        return 8
    if rows_are_entries and have_row_env:
        return 9
    if n_entries > 0 and (rows != map_rows or cols != map_cols):
        return 10
    if n_entries > 0 and n_fields != n_entries and (rows_are_entries or n_fields != 1):
        return 11
    if n_entries > 0 and rows_are_entries and n != n_entries:
        return 12
    if n_entries <= 0:
        return 13
    if rows_are_entries and shared_map:
        return 14
    if overlap:
        return 15
    if bound_arrays:
        return 16
    return 0


def squares_met(a, b):
    """the cells whose OPEN unit square meets the segment between the centres of cells a and b = (row, col), and the
    lattice corners the segment passes through, by exact rationals: the definition clear() is checked against"""
    from fractions import Fraction as F
    (r0, c0), (r1, c1) = a, b
    met, corners = set(), set()
    for r in range(min(r0, r1), max(r0, r1) + 1):
        for c in range(min(c0, c1), max(c0, c1) + 1):
            # the segment P(t) = a + t (b - a), t in [0, 1], against the open square (c - 1/2, c + 1/2) x (r - 1/2, r + 1/2)
            lo, hi, empty = F(0), F(1), False
            for p0, d, centre in ((c0, c1 - c0, c), (r0, r1 - r0, r)):
                low, high = F(centre) - F(1, 2), F(centre) + F(1, 2)
                if d == 0:
                    if not low < p0 < high:
                        empty = True
                    continue
                t0, t1 = (low - p0) / F(d), (high - p0) / F(d)
                if t0 > t1:
                    t0, t1 = t1, t0
                lo, hi = max(lo, t0), min(hi, t1)
            # open intervals in each axis: the intersection is open unless cut by [0, 1]; a point of it exists iff lo < hi,
            # or lo == hi lies strictly inside both (only where the segment is a point)
            if not empty and (lo < hi or (r0, c0) == (r1, c1)):
                met.add((r, c))
    dr, dc = r1 - r0, c1 - c0
    for r2 in range(2 * min(r0, r1) + 1, 2 * max(r0, r1), 2):        # corners at half-integers (r2 / 2, c2 / 2)
        if dr == 0:
            break
        t = F(r2 - 2 * r0, 2 * dr)
        x2 = 2 * c0 + t * 2 * dc
        if x2.denominator == 1 and int(x2) % 2 == 1:
            corners.add((r2, int(x2)))
    return met, corners


# ---- the hand-built worlds the host and the GPU tests share --------------------------------------------------------------
RES = 0.1
PAD = (24, 31)          # the padded shape of the hand-built maps; every world's own shape is smaller in a row or a column


def _world(shape, walls, start, goal, origin, d2=0):
    data = np.zeros(shape, dtype=np.uint8)
    for r0, r1, c0, c1 in walls:
        data[r0:r1, c0:c1] = 254
    return dict(data=data, origin=np.array(origin, dtype=np.float64), start_cell=start, goal_cell=goal, d2=d2)


def hand_worlds():
    """name -> dict(data uint8 [rows, cols] (its own, valid shape), origin, start_cell, goal_cell, d2)"""
    diag = _world((23, 30), [], (4, 6), (19, 21), (0.3, -0.2))
    for r in range(5, 19):
        diag["data"][r, 23 - r + 2] = 254          # an anti-diagonal wall whose cells touch at corners only
    return {
        "L": _world((22, 29), [(10, 11, 0, 21)], (3, 3), (18, 4), (-0.4, 0.2), d2=1),
        "U": _world((24, 29), [(8, 9, 0, 22), (15, 16, 6, 29)], (3, 3), (20, 25), (0.1, 0.1)),
        "corridor": _world((22, 31), [(9, 13, 0, 14), (9, 13, 15, 31)], (3, 5), (19, 24), (-1.0, -1.0)),
        "diagonal": diag,
    }


def pose_in(world, cell, theta, off=(0.013, -0.021)):
    r, c = cell
    return np.array([world["origin"][0] + c * RES + off[0], world["origin"][1] + r * RES + off[1], theta])


def world_field(world):
    return GR.dijkstra(world["data"], [world["goal_cell"]], world["d2"])


def padded(a, shape=PAD, fill=0):
    out = np.full(shape, fill, dtype=a.dtype)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def corner_rows(world_origin, v_off):
    """a 3-way-point row P, V, N around cell (10, 10) turning from +x to +y, V off its cell's centre by v_off"""
    ox, oy = world_origin
    cx, cy = ox + 10 * RES, oy + 10 * RES
    return np.array([[cx - 0.8, cy + v_off[1], 0.1], [cx + v_off[0], cy + v_off[1], 0.7], [cx + v_off[0], cy + 0.8, 1.5]])

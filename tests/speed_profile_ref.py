"""The contract of bcp_path_speed and of bcp_track_profile's cap (include/bcplan.h), restated from the header's text in
Python floats: IEEE doubles whose every product, quotient and sum is rounded on its own, math.sqrt correctly rounded.
Curvature and limit element by element, the two passes sequentially -- the recurrence that defines the value.  Also what
the tests of the feature share: rows built on the CPU (legs with quadratic blends, some corners sharp), the bound on the
device's other association of the sums, and the argument rules."""
import math

import numpy as np

NO_PATH = 4
MAX_LEN, MAX_SPAN = 4096, 64
NAMES = ("v_max", "v_min", "a_lat", "w_max", "a_dec", "a_acc", "v_start", "v_end")   # bcp_speed_params behind span
STOCK = dict(span=1, v_max=0.5, v_min=0.0, a_lat=0.4, w_max=1.0, a_dec=0.8, a_acc=0.6, v_start=0.5, v_end=0.5)


def bound(m):
    """relative: how far another association of the passes' sums may leave speed from the recurrence's value"""
    return 2.0 * (m + 1) * 2.0 ** -52


def _len(dx, dy):
    return math.sqrt(dx * dx + dy * dy)


def curvature(x, y, m, j, span):
    a, b = max(j - span, 0), min(j + span, m - 1)
    if a == j or b == j:
        return 0.0
    ax, ay = x[j] - x[a], y[j] - y[a]
    bx, by = x[b] - x[j], y[b] - y[j]
    cx, cy = x[b] - x[a], y[b] - y[a]
    la, lb, lc = _len(ax, ay), _len(bx, by), _len(cx, cy)
    den = (la * lb) * lc
    cr = abs(ax * by - ay * bx)
    return 0.0 if den < 1e-18 else (2.0 * cr) / den


def limit(kappa, j, m, p):
    u = p["v_max"] * p["v_max"]
    if kappa > 0.0:
        t = p["a_lat"] / kappa
        if t < u:
            u = t
        s = p["w_max"] / kappa
        s2 = s * s
        if s2 < u:
            u = s2
    f = p["v_min"] * p["v_min"]
    if u < f:
        u = f
    if j == 0:
        u = min(u, p["v_start"] * p["v_start"])
    if j == m - 1:
        u = min(u, p["v_end"] * p["v_end"])
    return u


def row(points, length, max_len, p):
    """-> speed, kappa, v_limit (float64 [max_len] each), status, and (cd, ca) of the row's m - 1 stretches"""
    speed, kappa, v_limit = np.zeros(max_len), np.zeros(max_len), np.zeros(max_len)
    m = max(min(int(length), max_len), 0)
    x, y = [float(v) for v in points[:m, 0]], [float(v) for v in points[:m, 1]]
    if length < 1 or not all(math.isfinite(v) for v in x + y):
        return speed, kappa, v_limit, NO_PATH, (np.zeros(0), np.zeros(0))
    u = []
    for j in range(m):
        k = curvature(x, y, m, j, p["span"])
        u.append(limit(k, j, m, p))
        kappa[j], v_limit[j] = k, math.sqrt(u[j])
    ds = [_len(x[j + 1] - x[j], y[j + 1] - y[j]) for j in range(m - 1)]
    cd = [(2.0 * p["a_dec"]) * d for d in ds]
    ca = [(2.0 * p["a_acc"]) * d for d in ds]
    for j in range(m - 2, -1, -1):
        u[j] = min(u[j], u[j + 1] + cd[j])
    for j in range(1, m):
        u[j] = min(u[j], u[j - 1] + ca[j - 1])
    for j in range(m):
        speed[j] = math.sqrt(u[j])
    return speed, kappa, v_limit, 0, (np.array(cd), np.array(ca))


def path_speed(paths, lens, p):
    """-> speed, kappa, v_limit [n, max_len], status [n]"""
    paths = np.asarray(paths, dtype=np.float64)
    n, max_len = paths.shape[:2]
    out = [row(paths[i], int(lens[i]), max_len, p) for i in range(n)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out], dtype=np.int32))


def assert_speed_close(got, want, lens, max_len):
    """got within bound(m) of the recurrence's value, relatively, and +0.0 behind m; -> the largest share of the bound used"""
    worst = 0.0
    for i in range(len(want)):
        m = max(min(int(lens[i]), max_len), 0)
        assert (got[i, m:].view(np.uint64) == 0).all(), i
        w, g = want[i, :m], got[i, :m]
        if not m:
            continue
        zero = w == 0.0
        assert (g[zero] == 0.0).all(), i
        rel = np.abs(g[~zero] - w[~zero]) / w[~zero]
        share = float(rel.max() / bound(m)) if rel.size else 0.0
        assert share <= 1.0, (i, m, share)
        worst = max(worst, share)
    return worst


# ---- rows
def blended_row(vertices, blend=0.3, delta=0.05, sharp=()):
    """A polyline through `vertices` [k, 2] whose corners are quadratic blends reaching `blend` along each leg (clipped to a
    third of the leg), corners named in `sharp` left as they are; a way point about every delta metres -> [m, 3] with the
    headings of the stretches."""
    v = np.asarray(vertices, dtype=np.float64)
    pts = [v[0]]

    def line_to(p):
        a = pts[-1]
        k = max(int(math.ceil(np.hypot(*(p - a)) / delta)), 1)
        for i in range(1, k + 1):
            pts.append(a + (p - a) * (i / k))

    for c in range(1, len(v) - 1):
        a, b = v[c] - v[c - 1], v[c + 1] - v[c]
        la, lb = np.hypot(*a), np.hypot(*b)
        d = min(blend, la / 3, lb / 3)
        if c in sharp or d <= 0:
            line_to(v[c])
            continue
        p0, p2 = v[c] - a / la * d, v[c] + b / lb * d
        line_to(p0)
        k = max(int(math.ceil(2 * d / delta)), 2)
        for i in range(1, k + 1):
            t = i / k
            pts.append((1 - t) ** 2 * p0 + 2 * t * (1 - t) * v[c] + t ** 2 * p2)
    line_to(v[-1])
    xy = np.array(pts)
    th = np.arctan2(np.diff(xy[:, 1]), np.diff(xy[:, 0]))
    return np.column_stack([xy, np.append(th, th[-1] if len(th) else 0.0)])


def random_vertices(rng, legs, leg=(0.4, 1.6), turn=(-2.0, 2.0)):
    heading, p, out = rng.uniform(-3, 3), rng.uniform(-1, 1, 2), []
    out.append(p)
    for _ in range(legs):
        p = p + rng.uniform(*leg) * np.array([math.cos(heading), math.sin(heading)])
        out.append(p)
        heading += rng.uniform(*turn)
    return np.array(out)


def row_of_length(rng, m, sharp=(), blend=0.3):
    """a blended row cut to exactly m way points (as many legs as it takes)"""
    legs = 2
    while True:
        r = blended_row(random_vertices(rng, legs), blend=blend, sharp=sharp)
        if len(r) >= m:
            return r[:m].copy()
        legs += 1


def stack(rows, max_len, fill=0.0):
    paths = np.full((len(rows), max_len, 3), fill, dtype=np.float64)
    lens = np.zeros(len(rows), dtype=np.int32)
    for i, r in enumerate(rows):
        k = min(len(r), max_len)
        paths[i, :k] = r[:k]
        lens[i] = len(r)
    return paths, lens


# ---- the tracker's cap (step 4 of bcp_track_profile's law)
def cap(speed_row, m, target_idx, carrot):
    a, b = float(speed_row[max(min(int(target_idx), m - 1), 0)]), float(speed_row[int(carrot)])
    if a != a:
        return a
    if b != b:
        return b
    return b if b < a else a


def capped(speed, c):
    return c if (c >= 0.0 and c < speed) else speed


# ---- the argument rules, in the order the call looks
def check_args(ptrs, prm, max_len, n, span, v_max, v_min, a_lat, w_max, a_dec, a_acc, v_start, v_end, overlap):
    """-> (verdict, which): 0 ok, 1 null, 2 max_len, 3 n, 4 span, 5 a value that must be > 0, 6 one that must be >= 0,
    7 v_min > v_max, 8 overlap"""
    if not ptrs or not prm:
        return 1, 0
    if not 1 <= max_len <= MAX_LEN:
        return 2, 0
    if not 1 <= n <= 2 ** 31 - 1:
        return 3, 0
    if not 1 <= span <= MAX_SPAN:
        return 4, 0
    for k, v in enumerate((v_max, a_lat, w_max, a_dec, a_acc)):
        if not (math.isfinite(v) and v > 0):
            return 5, k
    for k, v in enumerate((v_min, v_start, v_end)):
        if not (math.isfinite(v) and v >= 0):
            return 6, k
    if v_min > v_max:
        return 7, 0
    if overlap:
        return 8, 0
    return 0, 0

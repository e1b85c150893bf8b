"""CPU side of the footprint zoo (tests/footprints.py): the zoo is what its comments claim, the oracle's polygon fill --
the pixel set every GPU mask is compared with -- lies inside bounds derived from geometry alone in exact integer
arithmetic, and the two claims behind the distance-field pre-classification hold for every member."""
from fractions import Fraction

import numpy as np
import pytest

import footprints as F

N_RANDOM = 400


def test_zoo_members_are_what_they_are_there_for():
    Z = F.ZOO
    assert [len(Z[k]) for k in ("triangle", "kat_rect", "ngon15", "ngon16", "ngon17", "star32")] == [3, 4, 15, 16, 17, 32]
    assert all(3 <= len(v) <= F.MAX_VERTS and v.dtype == np.float64 and v.shape[1] == 2 for v in Z.values())
    for name in ("ngon15", "ngon16", "ngon17", "triangle", "kat_rect", "broad", "tricycle_x1.7"):
        assert len(F.convex_hull(Z[name])) == len(Z[name]), name                 # convex
    for name in ("L", "U", "star32", "repeated", "diffdrive_x3"):
        assert len(F.convex_hull(Z[name])) < len(set(map(tuple, Z[name]))), name  # not convex
    assert len(set(map(tuple, Z["repeated"]))) * 2 == len(Z["repeated"])
    assert len(set(map(tuple, Z["point3"]))) == 1
    c = Z["collinear"]
    assert (c[1, 0] - c[0, 0]) * (c[2, 1] - c[0, 1]) == (c[2, 0] - c[0, 0]) * (c[1, 1] - c[0, 1])
    for name, v in Z.items():
        origin_inside = F.point_in_polygon(0.0, 0.0, v)
        assert origin_inside == (name not in ("offcentre", "point3", "collinear", "bowtie", "U")), name
    assert np.abs(Z["offcentre"]).min() >= 1.0
    b = Z["broad"]
    assert np.ptp(b[:, 1]) > 4 * np.ptp(b[:, 0])
    for name in Z:
        for res in F.resolutions(name):
            g = F.cull_geometry(Z[name], res)
            assert g["degenerate"] == (name == "broad"), name                    # a0 > a1 (point3: a0 == a1, no extent)
            assert (g["n_out"] == 1) == (name in ("broad", "point3")), name
            if name in ("U",):
                assert g["skipped_outside"] >= 3 and len(g["inner"]) >= 1        # axis samples in the notch
            if name in ("sliver", "collinear", "point3"):
                assert len(g["inner"]) == 0, name                                # n_in == 0
            if name in ("tricycle_x1.7", "tricycle_x3", "sliver", "collinear"):
                assert g["clamped"] and g["n_out"] == F.MAX_SAMPLES, name         # n_out clamped to kMaxSamples
            if name == "offcentre":
                assert g["ay"] > 1.0 and g["a0"] > 1.9                           # an axis off y = 0, away from the origin
    # sub-pixel sliver at every resolution it is tested at
    assert all(0.008 < res for res in F.resolutions("sliver"))


def test_every_wide_case_is_wide_and_every_case_is_accepted():
    n_wide = 0
    for name, v in F.ZOO.items():
        rs = F.resolutions(name)
        assert len(rs) >= 2, name
        assert all(F.check_kernel_size(v, r) for r in rs), name
        w = F.wide_resolution(v)
        assert (w is not None) == F.has_wide_resolution(v), name
        if w is None:
            assert name in ("offcentre", "point3"), name
            continue
        assert rs[-1] == w and F.footprint_is_wide(v, w) and not F.footprint_is_wide(v, 0.05) or name == "tricycle_x3"
        assert F.diameter(v) / w + 3.0 > 96.0 and F.radius(v) / w + 2.0 <= 127.0
        n_wide += 1
    assert n_wide == len(F.ZOO) - 2
    tri = F.TRICYCLE
    assert F.footprint_is_wide(tri, 0.017) and F.check_kernel_size(tri, 0.017) and not F.footprint_is_wide(tri, 0.03)
    for v in (tri, F.ZOO["star32"], F.ZOO["U"]):
        assert F.check_kernel_size(v, F.limit_resolution(v, True)) and not F.check_kernel_size(v, F.limit_resolution(v, False))


def _general_count(ivs):
    cc = [F.chain_changes(iv) for iv in ivs]
    return sum(1 for c, n in cc if n >= 2 and c != 2), max(c for c, _ in cc)


@pytest.mark.parametrize("name", sorted(F.ZOO))
def test_oracle_fill_within_geometric_bounds(oracle, name):
    """must <= oracle mask <= may for every member x resolution x (400 random angles + k pi / 8 + awkward ones); no pixel
    is exempt.  The concave members must really reach the general even-odd path (chain changes != 2)."""
    verts = F.ZOO[name]
    for res in F.resolutions(name):
        angles = F.angle_set(N_RANDOM, seed=1234)
        ivs, shapes, masks = F.oracle_masks(oracle, verts, res, angles)
        must, may = F.fill_bounds_batch(ivs, shapes)
        miss, far = F.fill_violations(masks, must, may)
        bad = np.nonzero((miss > 0) | (far > 0))[0]
        assert len(bad) == 0, "%s at %g: %d masks violate the bounds, first angle %r: %d required pixels unset, %d set " \
            "pixels outside the band" % (name, res, len(bad), angles[bad[0]], miss[bad[0]], far[bad[0]])
        assert must.any(axis=(1, 2)).all()
        ay, ax = np.repeat(np.arange(len(ivs)), ivs.shape[1]), ivs.reshape(-1, 2)
        assert (masks[ay, ax[:, 1], ax[:, 0]] != 0).all(), "a vertex pixel is not drawn"
        if name in F.CONCAVE:
            n_general, most = _general_count(ivs[:N_RANDOM])
            assert n_general >= 50, (name, res, n_general)
            if name == "star32":
                assert most >= 20
        if name == "bowtie":   # the other case of its own: two monotone chains that cross, through the fast path
            assert sum(1 for iv in ivs[:N_RANDOM] if F.chain_changes(iv)[0] == 2) >= 200


def _rowwise_first_to_last(mask):
    out = np.zeros_like(mask)
    for r, row in enumerate(mask):
        nz = np.flatnonzero(row)
        if len(nz):
            out[r, nz[0]:nz[-1] + 1] = 255
    return out


@pytest.mark.parametrize("name", ["U", "star32", "L", "bowtie"])
def test_bounds_convict_a_wrong_fill(oracle, name):
    """The check has teeth: a fill that pairs the first with the last crossing of a row (a concave shape filled across
    its notch) leaves `may`, a fill without its outline or with one span pixel missing leaves `must`."""
    verts, res = F.ZOO[name], 0.03
    angles = F.angle_set(60, seed=3)
    ivs, shapes, masks = F.oracle_masks(oracle, verts, res, angles)
    must, may = F.fill_bounds_batch(ivs, shapes)
    wrong = np.stack([_rowwise_first_to_last(m) for m in masks])
    miss, far = F.fill_violations(wrong, must, may)
    n_general = _general_count(ivs)[0]   # (only a contour that is not two monotone chains can have a gap in a row)
    assert (miss == 0).all() and n_general >= 20 and (far > 0).sum() >= 0.6 * n_general, (name, n_general, (far > 0).sum())
    # one pixel of the strict interior cleared
    broken = masks.copy()
    for i in range(len(broken)):
        vv, uu = np.nonzero(must[i])
        k = len(vv) // 2
        broken[i, vv[k], uu[k]] = 0
    miss, far = F.fill_violations(broken, must, may)
    assert (miss == 1).all() and (far == 0).all()
    # an image shifted by two pixels
    shifted = np.roll(masks, 2, axis=2)
    miss, far = F.fill_violations(shifted, must, may)
    assert ((miss > 0) & (far > 0)).all()


def test_fill_bounds_against_the_definition():
    """The vectorised int64 implementation against the definition evaluated pixel by pixel with Fractions."""
    def slow(iv, shape):
        h, w = shape
        K = len(iv)
        iv = [(int(x), int(y)) for x, y in iv]
        must, may = np.zeros(shape, bool), np.zeros(shape, bool)
        for v in range(h):
            xs = []
            for k in range(K):
                (x0, y0), (x1, y1) = iv[k - 1], iv[k]
                if y0 != y1 and min(y0, y1) <= v < max(y0, y1):
                    xs.append(Fraction(x0) + Fraction((v - y0) * (x1 - x0), y1 - y0))
            for u in range(w):
                near = any(abs(x - u) <= Fraction(1, 64) for x in xs)
                must[v, u] = near or sum(1 for x in xs if x < u) % 2 == 1 or (u, v) in iv
                d2 = Fraction(10 ** 9)
                for k in range(K):
                    (ax, ay), (bx, by) = iv[k - 1], iv[k]
                    ex, ey = bx - ax, by - ay
                    ee = ex * ex + ey * ey
                    t = Fraction(0) if ee == 0 else max(Fraction(0), min(Fraction(1), Fraction((u - ax) * ex + (v - ay) * ey, ee)))
                    d2 = min(d2, (u - ax - t * ex) ** 2 + (v - ay - t * ey) ** 2)
                may[v, u] = must[v, u] or d2 <= 1
        return must, may
    rng = np.random.RandomState(2)
    for k in (3, 4, 7, 12):
        for _ in range(6):
            shape = (int(rng.randint(4, 22)), int(rng.randint(4, 22)))
            iv = np.stack([rng.randint(0, shape[1], k), rng.randint(0, shape[0], k)], axis=1)
            a, b = F.fill_bounds(iv, shape), slow(iv, shape)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), (iv.tolist(), shape)


def _inside_exact(px, py, v):
    """even-odd membership of float points in the polygon of float vertices: a float filter, and Fractions for every
    point whose side of some edge the filter cannot decide (so the verdicts are the exact ones)"""
    inside = np.zeros(len(px), dtype=bool)
    doubt = np.zeros(len(px), dtype=bool)
    K = len(v)
    for i in range(K):
        (xi, yi), (xj, yj) = v[i], v[i - 1]
        if yi == yj:
            continue
        straddles = (yi > py) != (yj > py)
        side = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)       # px < x_cross  <=>  side * sign(yj - yi) > 0
        doubt |= straddles & (np.abs(side) < 1e-12)
        inside ^= straddles & ((side > 0) == (yj > yi))
    for k in np.nonzero(doubt)[0]:
        fx, fy = Fraction(float(px[k])), Fraction(float(py[k]))
        ins = False
        for i in range(K):
            xi, yi, xj, yj = (Fraction(float(c)) for c in (v[i][0], v[i][1], v[i - 1][0], v[i - 1][1]))
            if (yi > fy) != (yj > fy) and fx < (xj - xi) * (fy - yi) / (yj - yi) + xi:
                ins = not ins
        inside[k] = ins
    return inside


@pytest.mark.parametrize("name", sorted(F.ZOO))
def test_classification_geometry_claims(name):
    """The two claims build_cull_geometry rests on, for the restated sample geometry: every vertex lies within rho of
    the axis segment (so the outer discs cover the polygon), and every accepted inner disc lies inside the polygon."""
    verts = F.ZOO[name]
    rng = np.random.RandomState(17)
    for res in F.resolutions(name):
        g = F.cull_geometry(verts, res)
        for x, y in verts:
            assert F._seg_dist(x, y, g["a0"], g["ay"], g["a1"], g["ay"]) <= g["rho"] * (1 + 1e-12) + 1e-15
        # the disc row: spacing h, radius sqrt(rho^2 + h^2 / 4) covers the capsule; in pixels t_out exceeds it
        assert g["t_out"] > np.sqrt(g["rho"] ** 2 + 0.25 * g["h"] ** 2) / res + F.SLACK_OUTER - 1e-9
        assert len(g["out_x"]) == g["n_out"] <= F.MAX_SAMPLES
        for bx, rin, t in g["inner"]:
            assert t + 1 <= rin / res - F.SLACK_INNER + 1e-9
            r = rin * np.sqrt(rng.uniform(0, 1, 10000))
            a = rng.uniform(-np.pi, np.pi, 10000)
            r[:2000] = rin * (1 - 1e-9)                               # a fifth of the points on the rim
            inside = _inside_exact(bx + r * np.cos(a), g["ay"] + r * np.sin(a), verts)
            assert inside.all(), (name, res, bx, rin, int((~inside).sum()))

"""numpy restatement of inflate_costmap (utilities/costmap_inflation.py:47-92) as bcp_inflate_costmaps specifies it
(include/bcplan.h): brute-force exact distances and explicit float32 / float64 casts, so that the result does not depend
on the promotion rules of the numpy at hand."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_inflation.npz")
NONE = np.iinfo(np.int32).max   # d2 of a map without obstacles (every real one is below 2^24)

RECT_FOOTPRINT = np.array([[-0.77, -0.385], [-0.77, 0.385], [0.67, 0.385], [0.67, -0.385]])   # the reference test's


def squared_distances(data, valid=None):
    """int32 [rows, cols]: exact squared Euclidean distance in cells to the nearest cell == 254 of the valid region
    (NONE if there is none), by the minimum over all obstacle cells."""
    data = np.asarray(data, dtype=np.uint8)
    rows, cols = data.shape
    vr, vc = (rows, cols) if valid is None else (min(max(int(valid[0]), 0), rows), min(max(int(valid[1]), 0), cols))
    obstacle = np.zeros(data.shape, dtype=bool)
    obstacle[:vr, :vc] = data[:vr, :vc] == 254
    orr, occ = np.nonzero(obstacle)
    d2 = np.full(rows * cols, NONE, dtype=np.int32)
    rr, cc = [a.ravel().astype(np.int32) for a in np.indices((rows, cols))]
    for k in range(0, len(orr), 64):
        dr = rr[None, :] - orr[k:k + 64, None].astype(np.int32)
        dc = cc[None, :] - occ[k:k + 64, None].astype(np.int32)
        d2 = np.minimum(d2, (dr * dr + dc * dc).min(axis=0))
    return d2.reshape(rows, cols)


def distances(d2):
    """float32: sqrt(d2) correctly rounded (d2 < 2^24, so the float64 root rounds to it), +inf where there is no obstacle."""
    none = d2 == NONE
    d = np.sqrt(np.where(none, 0, d2).astype(np.float64)).astype(np.float32)
    d[none] = np.float32(np.inf)
    return d


def _pre_truncation(d, resolution, inscribed_radius, cost_scaling_factor):
    pir = np.float64(inscribed_radius) / np.float64(resolution)
    psf = np.float64(cost_scaling_factor) * np.float64(resolution)
    with np.errstate(over="ignore"):
        return np.float64(252.0) * np.exp(-psf * (d.astype(np.float64) - pir)), pir


def inflate_and_margin(data, resolution, inscribed_radius, cost_scaling_factor, valid=None):
    """-> (cost uint8 [rows, cols], distance float32 [rows, cols], margin); outside `valid` = (rows, cols) cost and
    distance are 0.  margin: the smallest |v - rint(v)| over the distinct pre-truncation values v >= 0.5 of the case -- how
    far the exponential may move before a truncated cost changes (inf if no cell has such a value)."""
    data = np.asarray(data, dtype=np.uint8)
    d = distances(squared_distances(data, valid))
    v, pir = _pre_truncation(d, resolution, inscribed_radius, cost_scaling_factor)
    d64 = d.astype(np.float64)
    cost = np.zeros(data.shape, dtype=np.uint8)
    other = d64 > pir
    cost[other] = np.trunc(v[other]).astype(np.uint8)
    cost[d64 <= pir] = 253
    cost[d64 < pir / np.float64(1000.)] = 254
    inside = np.ones(data.shape, dtype=bool)
    if valid is not None:
        inside[:] = False
        inside[:max(int(valid[0]), 0), :max(int(valid[1]), 0)] = True
        cost[~inside] = 0
        d[~inside] = 0
    w = np.unique(v[other & inside & (v >= 0.5)])
    return cost, d, (float(np.abs(w - np.rint(w)).min()) if w.size else float("inf"))


def inflate(data, resolution, inscribed_radius, cost_scaling_factor, valid=None):
    return inflate_and_margin(data, resolution, inscribed_radius, cost_scaling_factor, valid)[:2]


def margin(data, resolution, inscribed_radius, cost_scaling_factor, valid=None):
    return inflate_and_margin(data, resolution, inscribed_radius, cost_scaling_factor, valid)[2]


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def case_names():
    return [str(n) for n in golden()["names"]]


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """-> dict(data, resolution, inscribed_radius, cost_scaling_factor, expected) of one fixture case."""
    g = golden()
    return dict(data=g[name + "/data"], resolution=float(g[name + "/resolution"]),
                inscribed_radius=float(g[name + "/inscribed_radius"]),
                cost_scaling_factor=float(g[name + "/cost_scaling_factor"]), expected=g[name + "/expected"])


@functools.lru_cache(maxsize=None)
def restated_case(name):
    """(cost, distance, margin) of the restatement for one fixture case, computed once per session."""
    c = golden_case(name)
    cost, d, m = inflate_and_margin(c["data"], c["resolution"], c["inscribed_radius"], c["cost_scaling_factor"])
    cost.setflags(write=False)
    d.setflags(write=False)
    return cost, d, m

"""Expectations for bcp_mppi_field, numpy only: the value, distance and score rule of include/bcplan.h restated on top of
goal_field_ref (the cell and the field read) and mppi_ref (candidates, weights, the update)."""
import numpy as np

import goal_field_ref as GR
import mppi_ref as MR

NONE, FAR, ORTHO = GR.NONE, GR.FAR, GR.ORTHO


def values(fields, valids, origins, resolution, entry, xy):
    """int32 [n]: the field value bcp_mppi_field reads for final poses xy [n, 2] of rows on map entry entry[i] -- the cell
    rule of bcp_goal_field_sample (goal_field_ref.sample: half to even, the entry's origin and valid shape, field entry[i]
    or field 0 when there is one), with only x and y asked to be finite.  NONE outside the valid shape."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    poses = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1)   # (a heading of 0: the value does not depend on it)
    cs = np.broadcast_to(np.array([1.0, 0.0]), (len(xy), 2))
    return GR.sample(fields, valids, origins, resolution, entry, poses, cs, 1, np.inf)[1]


def distance(value, resolution):
    """float64 metres to go: ((double)(v == NONE ? FAR : v) * resolution) / 12.0, product and quotient rounded on their own"""
    v = np.asarray(value, dtype=np.int64)
    return (np.where(v == NONE, FAR, v).astype(np.float64) * np.float64(resolution)) / np.float64(12.0)


def scores(ret, reason, collision_penalty, value, resolution, weight):
    """s = ret; collided: s = s - penalty; then s = s - weight * d -- every product and sum an IEEE float64 operation"""
    s = MR.scores(ret, reason, collision_penalty)
    return s - np.float64(weight) * distance(value, resolution)


update = MR.update_from_scores    # (the scores enter as given bits)


def best_candidates(score):
    return np.asarray(score).argmax(axis=1)


"""Expectations for the MPPI tests (bcp_mppi), numpy and the CPU oracle only: the semantics of include/bcplan.h restated
on lookahead_ref.oracle_lookahead -- candidates u = clip(mean + sigma * eps), roll-outs, scores, weights (in
np.longdouble), the weighted mean -- and the scenarios the host and GPU tests share."""
import os

import numpy as np

import lookahead_ref as LR
from util import traj_config

DONE_COLLIDED = LR.DONE_COLLIDED


def candidates(mean, sigma, eps, low, high):
    """u [N, K, H, 2] float64 = min(max(mean + sigma * (double)eps, low), high): one product, one sum, two comparisons,
    each an IEEE float64 operation (numpy rounds every ufunc on its own).  mean [N, H, 2], eps [N, K, H, 2] float32; sigma
    one pair (2,), or a width per env, step and component [N, H, 2] (bcp_mppi_adapt's, already clamped)."""
    low, high = (np.asarray(v, np.float64).reshape(2) for v in (low, high))
    sigma = np.asarray(sigma, np.float64)
    e = np.asarray(eps, np.float32).astype(np.float64)
    u = np.asarray(mean, np.float64)[:, None] + (sigma if sigma.ndim == 1 else sigma[:, None]) * e
    return np.minimum(np.maximum(u, low), high)


def scores(ret, reason, collision_penalty):
    ret = np.asarray(ret, np.float64)
    return np.where((np.asarray(reason) & DONE_COLLIDED) != 0, ret - collision_penalty, ret)


def weights(score, lam):
    """w [N, K] in np.longdouble: exp((s - max s) / lam) / sum"""
    s = np.asarray(score, np.float64).astype(np.longdouble)
    e = np.exp((s - s.max(axis=1, keepdims=True)) / np.longdouble(lam))
    return e / e.sum(axis=1, keepdims=True)


def update_from_scores(u, score, lam):
    """the new mean [N, H, 2] (longdouble sum, rounded once to float64) and the weights [N, K] (longdouble) from scores
    taken as given bits"""
    w = weights(score, lam)
    new = (w[:, :, None, None] * np.asarray(u, np.float64).astype(np.longdouble)).sum(axis=1)
    return new.astype(np.float64), w


def update(u, ret, reason, lam, collision_penalty):
    return update_from_scores(u, scores(ret, reason, collision_penalty), lam)


def effective_sample_size(w):
    return np.asarray(1.0 / (w * w).sum(axis=1), np.float64)


def as_lookahead_actions(u):
    """[N, K, H, 2] -> the [H, N, K, 2] lookahead takes"""
    return np.ascontiguousarray(np.transpose(u, (2, 0, 1, 3)))


def host_eps(seed, iterations, n, k, horizon):
    """[I, N, K, H, 2] float32 standard normals, candidate 0 all zero (the parity mode's input)"""
    eps = np.random.RandomState(seed).standard_normal((iterations, n, k, horizon, 2)).astype(np.float32)
    eps[:, :, 0] = 0.0
    return eps


def mppi_ref(oracle, params, world, start, mean, sigma, low, high, lam, collision_penalty, eps, threads=8):
    """I iterations on the oracle.  Returns dict(mean, action, iter_mean [I, N, H, 2], iter_ret, iter_reason [I, N, K],
    iter_w [I, N, K], iter_err [I, N, K], err [N] = the OR of the oracle's error word over iterations and candidates)"""
    mean = np.array(mean, np.float64)
    out = dict(iter_mean=[], iter_ret=[], iter_reason=[], iter_w=[], iter_err=[])
    err = np.zeros(start.n, np.int32)
    for j in range(eps.shape[0]):
        u = candidates(mean, sigma, eps[j], low, high)
        la = LR.oracle_lookahead(oracle, params, world, start, as_lookahead_actions(u), threads=threads)
        err |= np.bitwise_or.reduce(la["err"], axis=1)
        out["iter_err"].append(la["err"])
        out["iter_mean"].append(mean)
        out["iter_ret"].append(la["ret"])
        out["iter_reason"].append(la["reason"])
        mean, w = update(u, la["ret"], la["reason"], lam, collision_penalty)
        out["iter_w"].append(w)
    out = {k: np.stack(v) for k, v in out.items()}
    out["mean"], out["action"], out["err"] = mean, mean[:, 0].copy(), err
    return out


# ---- the scenarios of tests/test_mppi_host.py (shown there to be non-vacuous) and tests/test_gpu_mppi.py
# the action box of BatchedPlanEnv (envs/base/env.py:237-240): [max_front_wheel_speed / 10, / 2] x [-pi / 2, pi / 2] held in
# float32 (the space's dtype), widened to float64
MAX_FRONT_WHEEL_SPEED = 1.0471975511965976
ACTION_LOW = np.array([MAX_FRONT_WHEEL_SPEED / 10, -np.pi / 2]).astype(np.float32).astype(np.float64)
ACTION_HIGH = np.array([MAX_FRONT_WHEEL_SPEED / 2, np.pi / 2]).astype(np.float32).astype(np.float64)
AISLE = "g8_traj_aisle_default.npz"
# Returns are whole numbers here (one per way point passed), so lambda sits a little below one way point.
# kind: (N, K, H), command the initial mean holds over the horizon, sigma, lambda, collision penalty
SCENARIOS = {
    "scatter": ((32, 64, 48), (0.5, 0.0), (0.05, 2.0), 0.4, 2.0),
    "goal": ((64, 64, 16), (0.3, 0.0), (0.2, 0.6), 0.3, 2.0),
    "aisle": ((64, 64, 16), (0.4, 0.0), (0.2, 0.8), 0.3, 2.0),
}
EPS_SEED = 1


def initial_mean(kind, n, horizon):
    return np.ascontiguousarray(np.broadcast_to(np.array(SCENARIOS[kind][1], np.float64), (n, horizon, 2)))


def scenario_world(kind, n):
    """(fixture, fixture name for util.env_from_traj / traj_config, StartState): 'scatter' and 'goal' are
    lookahead_ref.scenario_start on g8_traj_mini_00; 'aisle' starts n envs from the recorded states before steps
    300 .. 440 of g8_traj_aisle_default, whose robot runs into the wall at step 444."""
    if kind == "aisle":
        g = np.load(os.path.join(LR.GOLDEN, AISLE))
        start, _, _ = LR.recorded_windows(g, [int(v) for v in np.linspace(300, 440, n)], 1, noisy=False)
        return g, AISLE, start
    g = LR.mini_fixture()
    return g, "g8_traj_mini_00.npz", LR.scenario_start(g, n, kind)


def scenario_oracle_params(oracle, name, **kw):
    """the noise-free forward model with the precisions the fixture was recorded with"""
    _, sp, ap = traj_config(name)
    return oracle.make_params("tricycle", noise=None, spatial_precision=sp, angular_precision=ap, **kw)

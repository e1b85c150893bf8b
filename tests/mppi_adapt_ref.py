"""Expectations for the tests of bcp_mppi_adapt, numpy and the CPU oracle only: tests/mppi_ref.py with a width per env, step
and component -- the clamp, the candidates, the weighted spread about the new mean (weights and sums in np.longdouble) and
the move of a width towards it, as include/bcplan.h states them."""
import numpy as np

import lookahead_ref as LR
import mppi_ref as MR


def clampd(s, lo, hi):
    """!(s >= lo) ? lo : (s > hi ? hi : s) per component (last axis of 2): a NaN goes to the minimum"""
    s = np.asarray(s, np.float64)
    lo, hi = (np.broadcast_to(np.asarray(v, np.float64).reshape(2), s.shape) for v in (lo, hi))
    with np.errstate(invalid="ignore"):
        return np.where(~(s >= lo), lo, np.where(s > hi, hi, s))


candidates = MR.candidates    # (with sigma [N, H, 2], already clamped)


def spread(u, w, new_mean):
    """sd [N, H, 2] float64 = sqrt(sum_k w_k (u_k - m')^2), the differences, products, sum and root in np.longdouble, rounded
    once.  w [N, K] (longdouble), new_mean [N, H, 2]"""
    d = np.asarray(u, np.float64).astype(np.longdouble) - np.asarray(new_mean, np.float64).astype(np.longdouble)[:, None]
    v = (np.asarray(w, np.longdouble)[:, :, None, None] * (d * d)).sum(axis=1)
    return np.sqrt(v).astype(np.float64)


def next_sigma(sigma, sd, rate, lo, hi):
    """clampd(sigma + rate * (sd - sigma)) in float64, every operation rounded on its own"""
    sigma, sd = np.asarray(sigma, np.float64), np.asarray(sd, np.float64)
    return clampd(sigma + np.float64(rate) * (sd - sigma), lo, hi)


def update(u, score, lam, sigma, rate, lo, hi, new_mean=None):
    """(new mean [N, H, 2], new sigma [N, H, 2], weights [N, K]) from the scores [N, K]; new_mean given: the spread is taken
    about that mean (the kernel's own), not about the restatement's"""
    mean, w = MR.update_from_scores(u, score, lam)
    about = mean if new_mean is None else np.asarray(new_mean, np.float64)
    return mean, next_sigma(sigma, spread(u, w, about), rate, lo, hi), w


def on_clamp(sigma, lo, hi):
    """(share of the values equal to sigma_min, share equal to sigma_max) per component: two arrays of 2"""
    s = np.asarray(sigma, np.float64).reshape(-1, 2)
    lo, hi = (np.asarray(v, np.float64).reshape(2) for v in (lo, hi))
    return (s == lo).mean(axis=0), (s == hi).mean(axis=0)


def mppi_adapt_ref(oracle, params, world, start, mean, sigma, rate, lo, hi, low, high, lam, collision_penalty, eps, threads=8):
    """I iterations on the oracle.  Returns dict(mean, sigma, iter_mean, iter_sigma [I, N, H, 2], iter_ret, iter_reason
    [I, N, K])"""
    mean, sigma = np.array(mean, np.float64), clampd(sigma, lo, hi)
    out = dict(iter_mean=[], iter_sigma=[], iter_ret=[], iter_reason=[])
    for j in range(eps.shape[0]):
        u = candidates(mean, sigma, eps[j], low, high)
        la = LR.oracle_lookahead(oracle, params, world, start, MR.as_lookahead_actions(u), threads=threads)
        out["iter_mean"].append(mean)
        out["iter_sigma"].append(sigma)
        out["iter_ret"].append(la["ret"])
        out["iter_reason"].append(la["reason"])
        mean, sigma, _ = update(u, MR.scores(la["ret"], la["reason"], collision_penalty), lam, sigma, rate, lo, hi)
    out = {k: np.stack(v) for k, v in out.items()}
    out["mean"], out["sigma"] = mean, sigma
    return out


def scenario_widths(kind, n, h):
    """(sigma [N, H, 2] = the scenario's s0 in every row, sigma_min = s0 / 8, sigma_max = 2 s0)"""
    s0 = np.asarray(MR.SCENARIOS[kind][2], np.float64)
    return np.ascontiguousarray(np.broadcast_to(s0, (n, h, 2))), s0 / 8, 2 * s0

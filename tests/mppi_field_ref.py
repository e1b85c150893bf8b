"""Expectations for bcp_mppi_field, numpy only: the value, distance and score rule of include/bcplan.h restated on top of
goal_field_ref (the cell and the field read) and mppi_ref (candidates, weights, the update), and the few set-up helpers
the host and GPU tests of the terminal cost share."""
import numpy as np

import goal_field_ref as GR
import lookahead_ref as LR
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


def update(u, score, lam):
    """the new mean [N, H, 2] (longdouble sum, rounded once) and the weights [N, K] from scores taken as given bits"""
    w = MR.weights(score, lam)
    new = (w[:, :, None, None] * np.asarray(u, np.float64).astype(np.longdouble)).sum(axis=1)
    return new.astype(np.float64), w


def best_candidates(score):
    return np.asarray(score).argmax(axis=1)


# ---- set-up helpers (as tests/test_gpu_mppi.py has them)
def set_start(torch, env, start):
    env.state.robot.copy_(torch.from_numpy(start.robot))
    env.state.min_spat_dist_so_far.copy_(torch.from_numpy(start.min_dist))
    env.state.target_idx.copy_(torch.from_numpy(start.target_idx))
    env.state.current_iter.copy_(torch.from_numpy(start.cur_iter))
    env.state.robot_collided.copy_(torch.from_numpy(start.collided))
    if start.geom is not None:
        env.geom_of_env.copy_(torch.from_numpy(start.geom))


def read_start(env):
    s = env.state
    return LR.StartState(s.robot.cpu().numpy(), s.min_spat_dist_so_far.cpu().numpy(), s.target_idx.cpu().numpy(),
                         s.current_iter.cpu().numpy(), s.robot_collided.cpu().numpy(),
                         None if env.geom_of_env is None else env.geom_of_env.cpu().numpy())


def box(env):
    return np.asarray(env.action_space.low, np.float64), np.asarray(env.action_space.high, np.float64)


def tolerance(env, k):
    """4 (K + 16) 2^-53 max(|low|, |high|): tests/test_gpu_mppi.py derives it; the scores enter it as given bits"""
    low, high = box(env)
    return 4.0 * (k + 16) * 2.0 ** -53 * max(np.abs(low).max(), np.abs(high).max())


def random_mean(env, rng, n, h):
    low, high = box(env)
    return np.ascontiguousarray(rng.uniform(low, high, (n, h, 2)))


def drive(env, rng, steps, gain):
    for _ in range(steps):
        a = env.action_space.sample_batch(env.n_envs, rng)
        a[:, 0] *= gain
        env.step(a)

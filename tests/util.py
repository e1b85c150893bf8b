"""Shared helpers for the parity tests."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAJ = sorted(glob.glob(os.path.join(GOLDEN, "g8_traj_*.npz")))

# tolerance of the north star: done/collision bit-exact, pose/reward within 1e-5.  The HIP path differs from the
# oracle only through the last-ulp behaviour of device sin/cos/hypot, so the tests hold it to a far tighter bound.
ATOL = 1e-9


def traj_config(name):
    """(noise_parameters, spatial_precision, angular_precision) used when a g8 trajectory was recorded."""
    mini = "mini" in name
    noise = None if "nonoise" in name else 'planenv'
    sp, ap = (0.2, np.pi / 8) if mini else (1.0, np.pi / 2)
    return noise, sp, ap


def env_from_traj(g, name, n_envs=1, **kw):
    """BatchedPlanEnv replicating the recorded env n_envs times (shared costmap / path)."""
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    noise, sp, ap = traj_config(name)
    params = EnvParams(goal_spat_dist=sp, goal_ang_dist=ap, resolution=float(g["resolution"]), refine_path=False)
    costmap = CostMap2D(g["costmap"], float(g["resolution"]), g["origin"])
    return BatchedPlanEnv(costmap, g["path"], params, n_envs=n_envs, noise_parameters=noise, **kw)


def oracle_params_for(oracle, name, **kw):
    noise, sp, ap = traj_config(name)
    return oracle.make_params("tricycle", noise=oracle.PLANENV_NOISE if noise else None, spatial_precision=sp,
                              angular_precision=ap, **kw)


def z_in(z):
    """NaN (= slot not drawn in the reference) -> a poison value that must never be consumed."""
    return np.where(np.isnan(z), 1e300, z)


def random_batch(oracle, rng, n, g, name, timeout=1200, xy_sigma=0.15, th_sigma=0.3):
    """n envs on the recorded map/path, started from random poses near the path (many collide or progress), at a random
    iteration below `timeout` (the first eight one step before it).  -> state [7, n], min_dist, target_idx, current_iter"""
    path = g["path"]
    idx = rng.randint(0, len(path), n)
    st = np.zeros((7, n))
    st[0] = path[idx, 0] + rng.normal(0, xy_sigma, n)
    st[1] = path[idx, 1] + rng.normal(0, xy_sigma, n)
    st[2] = path[idx, 2] + rng.normal(0, th_sigma, n)
    st[3] = rng.uniform(0, 0.5, n)
    st[4] = rng.uniform(-0.5, 0.5, n)
    st[6] = rng.uniform(-1.0, 1.0, n)
    # a third of the robots start next to a lethal cell, so that collisions (and rollbacks) really happen
    ly, lx = np.nonzero(g["costmap"] == 254)
    near = rng.rand(n) < 0.33
    pick = rng.randint(0, len(ly), n)
    res = float(g["resolution"])
    ang = rng.uniform(-np.pi, np.pi, n)
    rad = rng.uniform(0.3, 1.0, n)
    st[0] = np.where(near, g["origin"][0] + lx[pick] * res + rad * np.cos(ang), st[0])
    st[1] = np.where(near, g["origin"][1] + ly[pick] * res + rad * np.sin(ang), st[1])
    tgt = np.clip(idx + rng.randint(-3, 4, n), 1, len(path) - 1).astype(np.int32)
    md = np.hypot(path[tgt, 0] - st[0], path[tgt, 1] - st[1]) + rng.uniform(-0.01, 0.05, n)
    it = rng.randint(0, timeout, n).astype(np.int32)
    it[:8] = timeout - 1  # timeout on this very step
    return st, md, tgt, it

"""Times bcp_range_scan beside the two image observations, in one run, and prints one JSON line:

  mini pool   65 536 BatchedRandomMiniEnv envs (n_chains = 1024, episodes = 4, 183 x 183 entries at 3 cm), after a few
              hundred auto-reset steps: 32, 64 and 256 beams over 2 pi at 3 m (100 cells)
  c4          bench.py's C4 leg: 65 536 private maps stored 256 x 256 (valid 256 x 141), 64 beams at 3 m
  images      on the same mini envs: the full egocentric window (133 x 117) and its block maxima at pool = 8

Each figure is the launch of the observation alone (no goal vector), HIP events around a region of at least 50 ms after a
warm-up; the ratios are taken within this run.

    python tools/bench_range_scan.py > profiles/range_scan_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bc_gym_planning_env_amd import EnvParams, mini_env  # noqa: E402
from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap  # noqa: E402
from bc_gym_planning_env_amd.range_scan import BatchedRangeScan  # noqa: E402

MAX_RANGE = 3.0


def timed_ms(fn, min_ms=50.0):
    """average milliseconds of fn() over a region of at least min_ms, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    reps = 1
    while True:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        total = start.elapsed_time(stop)
        if total >= min_ms:
            return total / reps, reps
        reps = max(reps * 2, int(reps * min_ms / max(total, 1e-3)) + 1)


def scan_leg(env, n_beams):
    wrap = BatchedRangeScan(env, n_beams=n_beams, max_range=MAX_RANGE)
    angles = wrap.beam_angles
    ms, reps = timed_ms(lambda: env.range_scan(angles, MAX_RANGE))
    again, _ = timed_ms(lambda: env.range_scan(angles, MAX_RANGE))    # (the same region once more: the run's own spread)
    ranges, hit = env.range_scan(angles, MAX_RANGE, want=("hit",))
    rays = env.n_envs * n_beams
    return {"n_beams": n_beams, "max_range_m": MAX_RANGE, "cells_of_range": round(MAX_RANGE / env.resolution, 1), "ms": round(ms, 4),
            "ms_again": round(again, 4), "reps": reps, "rays": rays, "rays_per_s": round(rays / (ms * 1e-3)), "bytes_per_env": 4 * n_beams,
            "hit_fraction": round(float((hit >= 0).float().mean()), 4), "mean_range_m": round(float(ranges.mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300, help="auto-reset steps before the measurement (spreads the robots)")
    args = ap.parse_args()
    n = args.envs
    out = {"tool": "tools/bench_range_scan.py", "device": torch.cuda.get_device_name(0), "n_envs": n, "legs": {}}

    params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2))
    env = mini_env.BatchedRandomMiniEnv(n, params, n_chains=1024, episodes=4, auto_reset=True, seed=1)
    rng = np.random.RandomState(0)
    for _ in range(args.steps):
        env.step(env.action_space.sample_batch(n, rng))
    torch.cuda.synchronize()
    for b in (32, 64, 256):
        out["legs"]["mini_pool_%d_beams" % b] = scan_leg(env, b)
    full, pooled = BatchedEgocentricCostmap(env), BatchedEgocentricCostmap(env, pool=8)
    for name, wrap in (("ego_full", full), ("ego_pool8", pooled)):
        ms, reps = timed_ms(wrap._refresh_images)
        out["legs"][name] = {"image_shape": list(wrap.image_shape), "bytes_per_env": int(np.prod(wrap.image_shape)), "ms": round(ms, 4),
                             "reps": reps, "kernel": wrap.route()["kernel"]}
    for b in (32, 64, 256):
        leg = out["legs"]["mini_pool_%d_beams" % b]
        leg["over_ego_full"] = round(leg["ms"] / out["legs"]["ego_full"]["ms"], 3)
        leg["over_ego_pool8"] = round(leg["ms"] / out["legs"]["ego_pool8"]["ms"], 3)
    env.close()
    del env, full, pooled
    torch.cuda.empty_cache()

    from bench import make_c4_env
    env = make_c4_env(n, 0)
    for _ in range(args.steps):
        env.step(env.action_space.sample_batch(n, rng))
    torch.cuda.synchronize()
    out["legs"]["c4_private_maps_64_beams"] = scan_leg(env, 64)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

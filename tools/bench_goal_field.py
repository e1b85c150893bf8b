"""Times bcp_goal_field and bcp_goal_field_sample, each beside a call of comparable shape in the same run, and prints one
JSON line:

  mini_pool   field build for 4 096 x 183 x 183 RandomMiniEnv entries (sampled on the device), seeded at each entry's goal,
              at clearance_d2 0 and 151 (the tricycle's inscribed radius at 3 cm); beside it bcp_inflate_costmaps on the
              same tensor
  c4_maps     field build for the 65 536 private maps of bench.py's C4 leg, stored 256 x 256 (valid 256 x 141)
  sample      bcp_goal_field_sample at 65 536 BatchedRandomMiniEnv envs (4 096 entries) after a few hundred auto-reset steps,
              carrot_cells 1 / 8 / 64; beside it bcp_goal_n_state

The passes a map needs depend on its data (a CPU prototype saw up to 199 under pure Jacobi for the reference worlds); the
figures are what was measured, whatever they are: there is no threshold.  HIP events around a region of at least 50 ms after
a warm-up (timed_ms, as in the other tools of this directory; tools/bench_lib.py is the A/B script of bench.py's metric leg
and offers nothing to import).

    python tools/bench_goal_field.py [--legs mini_pool,c4_maps,sample] > profiles/goal_field_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bc_gym_planning_env_amd import EnvParams, _lib, goal_field, mini_env, robots  # noqa: E402
from bc_gym_planning_env_amd.api import INDUSTRIAL_TRICYCLE_V1  # noqa: E402

RADIUS = robots.inscribed_radius(robots.get_footprint(INDUSTRIAL_TRICYCLE_V1))


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


def field_figures(env, clearance):
    """the build of env.goal_field(clearance), timed as the library call alone on the env's own tensors"""
    fields = env.goal_field(clearance)
    seeds, data, vr, vc = fields._keep
    f, info = fields.field, fields.info
    n, rows, cols = f.shape
    stream = env._stream()

    def build():
        _lib.check(env._lib.bcp_goal_field(env._h, data.data_ptr(), n, rows, cols, 0, vr.data_ptr() if vr is not None else None,
                                           vc.data_ptr() if vc is not None else None, seeds.data_ptr(), int(seeds.shape[1]),
                                           fields.clearance_d2, 0, f.data_ptr(), info.data_ptr(), stream))

    ms, reps = timed_ms(build)
    again, _ = timed_ms(build)     # (the same region once more: the run's own spread)
    host = info.cpu().numpy()
    values = f.to(torch.int32)
    reached = values != _lib.GOAL_NONE
    return fields, {"shape": [n, rows, cols], "clearance_d2": fields.clearance_d2, "ms": round(ms, 4), "ms_again": round(again, 4),
                    "reps": reps, "us_per_map": round(1e3 * ms / n, 3), "gave_up": int(host[:, 1].sum()),
                    "mean_cells_with_a_value": round(float(host[:, 0].mean()), 1),
                    "largest_value": int(torch.where(reached, values, torch.zeros_like(values)).max()),
                    "field_bytes": f.numel() * 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="mini_pool,c4_maps,sample")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300, help="auto-reset steps before the sample leg (spreads the robots)")
    args = ap.parse_args()
    legs = args.legs.split(",")
    n = args.envs
    out = {"tool": "tools/bench_goal_field.py", "device": torch.cuda.get_device_name(0), "inscribed_radius": RADIUS, "legs": {}}
    rng = np.random.RandomState(0)

    if "mini_pool" in legs or "sample" in legs:
        params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2))
        env = mini_env.BatchedRandomMiniEnv(n, params, n_chains=1024, episodes=4, auto_reset=True, seed=1)
        fields = None
        if "mini_pool" in legs:
            for clearance in (0.0, RADIUS):
                fields, leg = field_figures(env, clearance)
                out["legs"]["mini_pool_clearance_d2_%d" % leg["clearance_d2"]] = leg
            maps = env.costmap_tensor
            spare = torch.empty_like(maps)
            stream = env._stream()
            inflate_ms, reps = timed_ms(lambda: _lib.check(env._lib.bcp_inflate_costmaps(
                env._h, maps.data_ptr(), maps.shape[0], maps.shape[1], maps.shape[2], None, None, float(env.resolution), RADIUS, 3.0,
                spare.data_ptr(), None, stream)))
            out["legs"]["mini_pool_inflate_costmaps"] = {"shape": list(maps.shape), "ms": round(inflate_ms, 4), "reps": reps}
            for name, leg in out["legs"].items():
                if name.startswith("mini_pool_clearance"):
                    leg["over_inflate_costmaps"] = round(leg["ms"] / inflate_ms, 3)
            del spare
        if "sample" in legs:
            fields = fields if fields is not None else env.goal_field()
            for _ in range(args.steps):
                env.step(env.action_space.sample_batch(n, rng))
            torch.cuda.synchronize()
            world = np.array([10.0, 10.0])
            vec = torch.zeros((n, 9), dtype=torch.float32, device=env.device)
            vec_ms, reps = timed_ms(lambda: _lib.check(env._lib.bcp_goal_n_state(env._h, world.ctypes.data_as(_lib._f64p), vec.data_ptr(),
                                                                               env._stream())))
            out["legs"]["goal_n_state"] = {"n_envs": n, "ms": round(vec_ms, 4), "reps": reps}
            for carrot in (1, 8, 64):
                ms, reps = timed_ms(lambda: fields.sample(carrot_cells=carrot, max_dist=10.0))
                again, _ = timed_ms(lambda: fields.sample(carrot_cells=carrot, max_dist=10.0))
                out3, value = fields.sample(carrot_cells=carrot, max_dist=10.0, want=("cell_value",))
                out["legs"]["sample_carrot_%d" % carrot] = {
                    "n_envs": n, "carrot_cells": carrot, "ms": round(ms, 4), "ms_again": round(again, 4), "reps": reps,
                    "over_goal_n_state": round(ms / vec_ms, 3), "rows_with_a_result": int((value != _lib.GOAL_NONE).sum()),
                    "mean_distance_m": round(float(out3[:, 0].mean()), 4)}
        env.close()
        del env, fields
        torch.cuda.empty_cache()

    if "c4_maps" in legs:
        from bench import make_c4_env
        env = make_c4_env(n, 0)
        _fields, leg = field_figures(env, RADIUS)
        out["legs"]["c4_maps"] = leg
        env.close()
    assert goal_field.clearance_cells_squared(RADIUS, 0.03) == 151
    print(json.dumps(out))


if __name__ == "__main__":
    main()

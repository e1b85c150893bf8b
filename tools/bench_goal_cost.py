"""Times bcp_goal_field_cost beside bcp_goal_field on the same tensor in the same run, counts what the weighted fields do to
the routes, and repeats the closed-loop table of DESIGN 7.17 with weighted routes.  Writes profiles/goal_cost_bench.json:

  build     4 096 RandomMiniEnv entries of 183 x 183 (sampled on the device), inflated at cost_scaling_factor 3.0, seeded at
            each entry's goal, clearance_d2 151: bcp_goal_field, then bcp_goal_field_cost at cost weights 0, 2 and 8
            (goal_field.cost_table), each as the library call alone on the env's own tensors; per weight the ratio to the
            plain call, the largest value, the count of gave_up, the passes are the kernel's own business; and for
            bcp_goal_route_bound at stride 2 / max_len 160 -- the call route_paths() makes -- the count of entries whose
            status is not 0
  episodes  256 envs x 200 ticks under MPPIPlanner on scattered worlds, the seeds and settings of tools/bench_scatter_boxes.py:
            straight and routed paths as there, and routed with cost_weight 2 and 8 (scatter, inflate, weighted field,
            route), each without and with the goal field as terminal cost; how the episodes ended (EpisodeEnds.reason)

HIP events around regions of at least 50 ms after a warm-up, the median of 5 regions with their minimum and maximum, and the
first measurement once more at the end of the leg (the run's own spread).  There is no threshold: the figures are what was
measured.

    python tools/bench_goal_cost.py [--legs build,episodes] [--out profiles/goal_cost_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bc_gym_planning_env_amd import MPPIPlanner, _lib, goal_field  # noqa: E402
from bc_gym_planning_env_amd.mini_env import BatchedRandomMiniEnv  # noqa: E402

DENSE = dict(half_size=(0.2, 0.5), along=(0.2, 0.8), lateral=2.0, n_yaws=16, seed=7, max_attempts=32)   # bench_scatter_boxes.py's
COST_SCALING = 3.0
WEIGHTS = (0, 2, 8)


def timed(fn, min_ms=50.0, regions=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        if a.elapsed_time(b) >= min_ms or reps >= 1 << 16:
            break
        reps *= 2
    out = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return {"ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "calls_per_region": reps}


def leg_build():
    env = BatchedRandomMiniEnv(4096, n_chains=1024, episodes=4, auto_reset=True, sampler="device_resident")
    env.inflate_costmaps(COST_SCALING)
    fields = env.goal_field()
    seeds, data, vr, vc = fields._keep
    f, info = fields.field, fields.info
    n, rows, cols = (int(v) for v in f.shape)
    stream = env._stream()
    head = (env._h, data.data_ptr(), n, rows, cols, 0, vr.data_ptr() if vr is not None else None,
            vc.data_ptr() if vc is not None else None, seeds.data_ptr(), int(seeds.shape[1]), fields.clearance_d2, 0)
    tail = (f.data_ptr(), info.data_ptr(), stream)

    def plain():
        _lib.check(env._lib.bcp_goal_field(*(head + tail)))

    def figures(gf):
        values = gf.field.to(torch.int32)
        reached = values != _lib.GOAL_NONE
        _p, lens, status = gf.route_bound(stride=2, max_len=160)
        ok = status == 0
        return {"gave_up": int(gf.info[:, 1].sum()), "largest_value": int(torch.where(reached, values, torch.zeros_like(values)).max()),
                "mean_cells_with_a_value": float(gf.info[:, 0].double().mean()), "routes_with_status_not_0": int((~ok).sum()),
                "mean_route_len": float(lens[ok].double().mean())}

    res = {"shape": [n, rows, cols], "clearance_d2": fields.clearance_d2, "cost_scaling_factor": COST_SCALING,
           "distinct_costs": int(torch.unique(data).numel())}
    res["goal_field"] = timed(plain)
    res["goal_field"].update(figures(fields), us_per_map=1e3 * res["goal_field"]["ms"] / n)
    for w in WEIGHTS:
        table = goal_field.cost_table(w)

        def cost():
            _lib.check(env._lib.bcp_goal_field_cost(*(head + (table.ctypes.data,) + tail)))

        t = timed(cost)
        t.update(figures(env.goal_field(cost_weight=w)), us_per_map=1e3 * t["ms"] / n, over_goal_field=t["ms"] / res["goal_field"]["ms"])
        res["goal_field_cost_weight_%d" % w] = t
    res["goal_field_again"] = timed(plain)
    return res


def leg_episodes(ticks=200, n=256, n_boxes=4):
    out = {"n_boxes": n_boxes, "ticks": ticks, "n_envs": n}
    rows = [("straight", None), ("routed", None), ("routed, cost_weight 2", 2), ("routed, cost_weight 8", 8)]
    for paths, weight in rows:
        for terminal in (False, True):
            env = BatchedRandomMiniEnv(n, n_chains=n, episodes=4, auto_reset=True, seed=0)
            status, _c, _b = env.scatter_obstacles(n_boxes, **DENSE)
            name = paths + ("+field" if terminal else "")
            out.setdefault("reverted_entries", int(((status & _lib.SCATTER_REVERTED) != 0).sum()))
            if weight is not None:
                env.inflate_costmaps(COST_SCALING)
            fields = env.goal_field(cost_weight=weight)
            tally = {"goal": 0, "timeout": 0, "collided": 0, "episodes": 0}
            if paths != "straight":
                routed = env.route_paths(fields, stride=2, max_len=160)
                tally["routed_entries"] = int((routed == 0).sum())
            ends = env.enable_episode_record()
            kw = dict(goal_field=fields, terminal_weight=1.0) if terminal else {}
            planner = MPPIPlanner(env, horizon=16, n_candidates=64, iterations=2, sigma=(0.2, 0.6), lam=0.3, collision_penalty=2.0,
                                  **kw)
            for _ in range(ticks):
                _o, _r, done, _info = env.step(planner.act())
                planner.reset_plans(done)
                reason = ends.reason.cpu().numpy()
                reason = reason[reason != 0]
                if len(reason):
                    tally["episodes"] += len(reason)
                    tally["collided"] += int(((reason & _lib.DONE_COLLIDED) != 0).sum())
                    tally["goal"] += int((((reason & _lib.DONE_GOAL) != 0) & ((reason & _lib.DONE_COLLIDED) == 0)).sum())
                    tally["timeout"] += int((reason == _lib.DONE_TIMEOUT).sum())
            out[name] = tally
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="build,episodes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goal_cost_bench.json"))
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    doc = {"tool": "tools/bench_goal_cost.py", "device": torch.cuda.get_device_name(0)}
    if "build" in legs:
        doc["build"] = leg_build()
    if "episodes" in legs:
        doc["episodes"] = leg_episodes()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

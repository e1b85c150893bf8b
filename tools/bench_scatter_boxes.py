"""Measurements of bcp_scatter_boxes and of what scattered worlds do to episodes, as one JSON document on
stdout and in profiles/scatter_boxes_bench.json:
  call      bcp_scatter_boxes for 4 096 mini entries of 183 x 183 with 4 and with 12 boxes (the dense configuration: half
            sizes 0.2 - 0.5 m, along (0.2, 0.8), 2 m to either side, the default keep-out, 16 yaws, 32 attempts), each call
            on maps restored by a device copy whose own time is measured and given beside it; reference points of the same
            run: the pool build, and bcp_goal_field on the same entries
  shares    the shares of SHORT and REVERTED entries of scatter_obstacles on those 4 096 sampled worlds
  episodes  256 envs x 200 ticks under MPPIPlanner (the settings of DESIGN 7.16, the same seeds) on scattered worlds:
            straight against routed paths, without against with goal_field=; how the episodes ended (EpisodeEnds.reason)
Times: HIP events around back-to-back calls, regions of at least 50 ms after a warm-up, the median of 5 regions."""
import argparse
import json
import os
import time

import numpy as np
import torch

from bc_gym_planning_env_amd import MPPIPlanner, _lib, boxes
from bc_gym_planning_env_amd.mini_env import BatchedRandomMiniEnv

DENSE = dict(half_size=(0.2, 0.5), along=(0.2, 0.8), lateral=2.0, n_yaws=16, seed=7, max_attempts=32)


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


def leg_call():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env = BatchedRandomMiniEnv(4096, n_chains=1024, episodes=4, auto_reset=True, sampler="device_resident")
    torch.cuda.synchronize()
    res = {"entries": int(env.costmap_tensor.shape[0]), "pool_build_wall_ms": (time.perf_counter() - t0) * 1e3}
    data, origins = env._keep["map"], env._keep["origins"]
    pts, lens = env._keep["path"], env._keep["lens"]
    n = int(data.shape[0])
    starts = pts[:, 0, :].cpu().numpy()
    goals = pts[torch.arange(n, device=data.device), lens.long() - 1].cpu().numpy()
    org = origins.cpu().numpy()
    radius = float(np.linalg.norm(env.footprint(), axis=1).max())
    d2 = (int(np.ceil(radius / env.resolution)) + 1) ** 2
    keep = torch.from_numpy(boxes.keep_outs([boxes.cells_of(starts, org, env.resolution), boxes.cells_of(goals, org, env.resolution)],
                                            d2)).cuda()
    frame = torch.from_numpy(boxes.path_frames(starts, goals, DENSE["lateral"])).cuda()
    yaw = torch.from_numpy(boxes.yaw_table(DENSE["n_yaws"])).cuda()
    bare, work = data.clone(), data.clone()
    res["restore_copy"] = timed(lambda: work.copy_(bare))
    for n_boxes in (4, 12):
        def call():
            work.copy_(bare)
            return boxes.scatter_boxes(env, work, origins, env.resolution, frame, yaw, n_boxes, DENSE["half_size"], DENSE["along"],
                                       keep, None, DENSE["seed"], DENSE["max_attempts"])
        t = timed(call)
        _b, counts = call()
        t.update(ms_less_copy=t["ms"] - res["restore_copy"]["ms"], mean_boxes=float(counts.double().mean()),
                 cells_written=int((work != bare).sum()))
        res["boxes_%d" % n_boxes] = t
    res["goal_field_same_entries"] = timed(lambda: env.goal_field())
    return res


def leg_shares():
    out = {}
    for n_boxes in (4, 12):
        env = BatchedRandomMiniEnv(4096, n_chains=1024, episodes=4, auto_reset=True, sampler="device_resident")
        status, counts, _b = env.scatter_obstacles(n_boxes, **DENSE)
        out["boxes_%d" % n_boxes] = {"entries": int(status.numel()),
                                     "short": float(((status & _lib.SCATTER_SHORT) != 0).double().mean()),
                                     "reverted": float(((status & _lib.SCATTER_REVERTED) != 0).double().mean()),
                                     "mean_boxes": float(counts.double().mean())}
    return out


def leg_episodes(ticks=200, n=256, n_boxes=4):
    out = {"n_boxes": n_boxes}
    for paths in ("straight", "routed"):
        for terminal in (False, True):
            env = BatchedRandomMiniEnv(n, n_chains=n, episodes=4, auto_reset=True, seed=0)
            status, _c, _b = env.scatter_obstacles(n_boxes, **DENSE)
            name = paths + ("+field" if terminal else "")
            out.setdefault("reverted_entries", int(((status & _lib.SCATTER_REVERTED) != 0).sum()))
            fields = env.goal_field()
            if paths == "routed":
                routed = env.route_paths(fields, stride=2, max_len=160)
                out["routed_entries"] = int((routed == 0).sum())
            ends = env.enable_episode_record()
            kw = dict(goal_field=fields, terminal_weight=1.0) if terminal else {}
            planner = MPPIPlanner(env, horizon=16, n_candidates=64, iterations=2, sigma=(0.2, 0.6), lam=0.3, collision_penalty=2.0,
                                  **kw)
            tally = {"goal": 0, "timeout": 0, "collided": 0, "episodes": 0}
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
    ap.add_argument("--legs", default="call,shares,episodes")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "scatter_boxes_bench.json"))
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    doc = {}
    if "call" in legs:
        doc["call"] = leg_call()
    if "shares" in legs:
        doc["shares"] = leg_shares()
    if "episodes" in legs:
        doc["episodes"] = leg_episodes()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

"""bcp_smooth_route (stride-1 routes pulled taut and blended, one wave per row) measured: writes
profiles/smooth_route_bench.json.

    python tools/bench_smooth_route.py [--legs call,paths,episodes] [--out FILE]

call      bcp_smooth_route at 4 096 entries of 183 x 183 (rows_are_entries, on stride-1 routes of 1 024 slots) and at 65 536
          rows (the same routes, 16 rows per entry through row_env), beside bcp_goal_route_bound at strides 1 and 2 in the same
          process.  HIP events around back-to-back calls, regions of at least 50 ms after a warm-up, median of 5.
paths     what smoothing does to the routes of the 4 096-world pool with 4 boxes per world (tools/bench_scatter_boxes.py's
          dense set-up): vertices kept, corners blended at full size / at a reduced size / left sharp, the change of length,
          the largest heading change between successive way points before and after, LONG / TOO_CLOSE / BLOCKED rows.
episodes  tools/bench_track.py's closed loop (256 envs x 200 ticks, one chain per env, seed 0, 4 boxes): its nine rows on
          straight, routed and weighted-routed paths again, and smoothed and smoothed-weighted routes under TrackingPlanner
          and MPPIPlanner(nominal=tracker)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bc_gym_planning_env_amd import MPPIPlanner, TrackingPlanner, _lib, pursuit_gain_library  # noqa: E402
from bc_gym_planning_env_amd.mini_env import BatchedRandomMiniEnv  # noqa: E402
from bench_track import COST_SCALING, DENSE, REACHES, timed  # noqa: E402

SMOOTH = dict(look=64, blend=0.3, delta=0.05, halvings=2)
ROUTE_LEN, MAX_LEN = 1024, 400


def leg_call():
    env = BatchedRandomMiniEnv(4096, n_chains=1024, episodes=4, auto_reset=True, sampler="device_resident")
    fields = env.goal_field()
    n = int(fields.field.shape[0])
    res = {"entries": n, "route_len": ROUTE_LEN, "max_len": MAX_LEN, "params": SMOOTH}
    for stride, slots in ((1, ROUTE_LEN), (2, 160)):
        res["route_bound_stride_%d" % stride] = timed(lambda: fields.route_bound(stride=stride, max_len=slots, want=("init",)))
    cells, cell_lens, status = fields.route_bound(stride=1, max_len=ROUTE_LEN)
    cells, cell_lens = cells.clone(), cell_lens.clone()
    res["route_mean_len"] = float(cell_lens.double().mean())
    res["route_status_nonzero"] = int((status != 0).sum())
    res["smooth_entries"] = timed(lambda: fields.smooth(cells, cell_lens, entries=True, max_len=MAX_LEN, want=("init", "info"), **SMOOTH))
    _p, lens, st, _i, info = fields.smooth(cells, cell_lens, entries=True, max_len=MAX_LEN, want=("init", "info"), **SMOOTH)
    res["smooth_entries"].update(mean_len=float(lens.double().mean()), status_nonzero=int((st != 0).sum()),
                                 mean_vertices=float(info[:, 0].double().mean()))
    res["route_bound_stride_1_again"] = timed(lambda: fields.route_bound(stride=1, max_len=ROUTE_LEN, want=("init",)))
    # 65 536 rows: every entry's route 16 times, through row_env (env i stands on entry geom_of_env[i])
    geom = env.geom_of_env.to(torch.int64)
    row_env = torch.arange(65536, device="cuda", dtype=torch.int32) % env.n_envs
    by_row = geom[row_env.to(torch.int64)]
    short = int(cell_lens.max())
    rows, row_lens = cells[by_row, :short].contiguous(), cell_lens[by_row].contiguous()
    res["rows"] = {"rows": 65536, "max_len_in": short}
    res["rows"]["smooth"] = timed(lambda: fields.smooth(rows, row_lens, row_env=row_env, max_len=MAX_LEN, want=("init", "info"), **SMOOTH))
    wide = torch.zeros((8192, ROUTE_LEN, 3), dtype=torch.float64, device="cuda")
    wide[:, :short] = rows[:8192]
    res["rows"]["smooth_8192_rows_of_1024_slots"] = timed(
        lambda: fields.smooth(wide, row_lens[:8192], row_env=row_env[:8192], max_len=MAX_LEN, want=("init", "info"), **SMOOTH))
    print(json.dumps(res), flush=True)
    return res


def heading_jumps(paths, lens):
    """the largest |heading change| between successive interior way points of every row, float64 [n] (0 for short rows)"""
    th = paths[..., 2]
    d = torch.remainder(th[:, 2:] - th[:, 1:-1] + np.pi, 2 * np.pi) - np.pi
    k = torch.arange(d.shape[1], device=paths.device)[None, :]
    live = k + 3 < lens[:, None]          # both way points interior: indices k + 1 and k + 2 below lens - 1
    return torch.where(live, d.abs(), torch.zeros_like(d)).max(dim=1).values


def lengths(paths, lens):
    seg = torch.hypot(paths[:, 1:, 0] - paths[:, :-1, 0], paths[:, 1:, 1] - paths[:, :-1, 1])
    k = torch.arange(seg.shape[1], device=paths.device)[None, :]
    return torch.where(k + 1 < lens[:, None], seg, torch.zeros_like(seg)).sum(1)


def leg_paths():
    out = {}
    for weight in (None, 2):
        env = BatchedRandomMiniEnv(4096, n_chains=1024, episodes=4, auto_reset=True, sampler="device_resident")
        status, _c, _b = env.scatter_obstacles(4, **DENSE)
        if weight is not None:
            env.inflate_costmaps(COST_SCALING)
        fields = env.goal_field(cost_weight=weight)
        cells, cell_lens, rst = fields.route_bound(stride=1, max_len=ROUTE_LEN)
        paths, lens, st, _i, info = fields.smooth(cells, cell_lens, entries=True, max_len=MAX_LEN, want=("init", "info"), **SMOOTH)
        ok = (rst == 0) & ((st & ~_lib.SMOOTH_BLOCKED) == 0)
        before, after = heading_jumps(cells, cell_lens)[ok], heading_jumps(paths, lens)[ok]
        l0, l1 = lengths(cells, cell_lens)[ok], lengths(paths, lens)[ok]
        corners = info[ok][:, 1:].double().sum(0)
        q = lambda t, p: float(torch.quantile(t.double(), p))   # noqa: E731
        res = {
            "worlds": int(len(ok)), "route_status_nonzero": int((rst != 0).sum()), "smoothed": int(ok.sum()),
            "long": int(((st & _lib.ROUTE_LONG) != 0).sum()), "too_close": int(((st & _lib.ROUTE_TOO_CLOSE) != 0).sum()),
            "blocked": int(((st & _lib.SMOOTH_BLOCKED) != 0).sum()), "no_route": int(((st & _lib.ROUTE_NO_ROUTE) != 0).sum()),
            "reverted_entries": int(((status & _lib.SCATTER_REVERTED) != 0).sum()),
            "route_cells": {"min": int(cell_lens[ok].min()), "median": q(cell_lens[ok], 0.5), "max": int(cell_lens[ok].max())},
            "vertices": {"min": int(info[ok][:, 0].min()), "median": q(info[ok][:, 0], 0.5), "p90": q(info[ok][:, 0], 0.9),
                         "max": int(info[ok][:, 0].max())},
            "way_points": {"median": q(lens[ok], 0.5), "max": int(lens[ok].max())},
            "corners": int(corners.sum()),
            "share_full": float(corners[0] / corners.sum()), "share_reduced": float(corners[1] / corners.sum()),
            "share_sharp": float(corners[2] / corners.sum()),
            "length_change": {"min": float((l1 / l0 - 1).min()), "median": q(l1 / l0 - 1, 0.5), "max": float((l1 / l0 - 1).max())},
            "heading_jump_before": {"min": float(before.min()), "median": q(before, 0.5), "max": float(before.max())},
            "heading_jump_after": {"min": float(after.min()), "median": q(after, 0.5), "p90": q(after, 0.9), "max": float(after.max()),
                                   "share_at_most_0.26": float((after <= 0.26).double().mean())},
        }
        name = "cost_weight %d" % (weight or 0)
        print(name, json.dumps(res), flush=True)
        out[name] = res
    return out


def leg_episodes(ticks=200, n=256, n_boxes=4, horizon=16):
    out = {"n_boxes": n_boxes, "ticks": ticks, "n_envs": n, "gains": "3 speeds x reaches %s" % (REACHES,), "smooth": SMOOTH}
    plan = [("straight", None, w) for w in ("tracker", "mppi", "mppi+nominal")]
    plan += [("routed", wt, w) for wt in (None, 2) for w in ("tracker", "mppi", "mppi+nominal")]
    plan += [("smoothed", wt, w) for wt in (None, 2) for w in ("tracker", "mppi+nominal")]
    for paths, weight, who in plan:
        env = BatchedRandomMiniEnv(n, n_chains=n, episodes=4, auto_reset=True, seed=0)
        env.scatter_obstacles(n_boxes, **DENSE)
        if weight is not None:
            env.inflate_costmaps(COST_SCALING)
        tally = {"goal": 0, "timeout": 0, "collided": 0, "episodes": 0}
        if paths == "routed":
            routed = env.route_paths(env.goal_field(cost_weight=weight), stride=2, max_len=160)
            tally["routed_entries"] = int((routed == 0).sum())
        elif paths == "smoothed":
            routed = env.route_paths(env.goal_field(cost_weight=weight), max_len=MAX_LEN, smooth=dict(SMOOTH, route_len=ROUTE_LEN))
            tally["routed_entries"] = int(((routed & ~_lib.SMOOTH_BLOCKED) == 0).sum())
        ends = env.enable_episode_record()
        tracker = TrackingPlanner(env, pursuit_gain_library(env.action_space, 3, REACHES), horizon)
        planner = tracker if who == "tracker" else MPPIPlanner(
            env, horizon=horizon, n_candidates=64, iterations=2, sigma=(0.2, 0.6), lam=0.3, collision_penalty=2.0,
            nominal=tracker if who == "mppi+nominal" else None)
        total = torch.zeros(n, dtype=torch.float64, device="cuda")
        for _ in range(ticks):
            _o, rew, done, _info = env.step(planner.act())
            if who != "tracker":
                planner.reset_plans(done)
            total += rew
            reason = ends.reason.cpu().numpy()
            reason = reason[reason != 0]
            if len(reason):
                tally["episodes"] += len(reason)
                tally["collided"] += int(((reason & _lib.DONE_COLLIDED) != 0).sum())
                tally["goal"] += int((((reason & _lib.DONE_GOAL) != 0) & ((reason & _lib.DONE_COLLIDED) == 0)).sum())
                tally["timeout"] += int((reason == _lib.DONE_TIMEOUT).sum())
        tally["mean_return"] = float(total.mean())
        name = "%s, cost_weight %d: %s" % (paths, weight or 0, who)
        print(name, json.dumps(tally), flush=True)
        out[name] = tally
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="call,paths,episodes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_route_bench.json"))
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    doc = {"tool": "tools/bench_smooth_route.py", "device": torch.cuda.get_device_name(0)}
    if os.path.exists(args.out):          # legs run one at a time add to the document
        with open(args.out) as f:
            doc.update(json.load(f))
    for leg, fn in (("call", leg_call), ("paths", leg_paths), ("episodes", leg_episodes)):
        if leg in legs:
            doc[leg] = fn()
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()

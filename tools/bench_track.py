"""bcp_track (K gain settings of the pure-pursuit tracker per env, rolled out over H steps) measured: writes
profiles/track_bench.json.

    python tools/bench_track.py [--legs timing,episodes] [--out FILE]

timing    bcp_track on BatchedRandomMiniEnv at N = 65 536 and 4 096, K = 8 and 64, H = 16, with and without `trace`, against
          bcp_lookahead at the same N, K, H with per-env float64 actions in the same run (the same trips; it reads the
          16 N K H bytes of actions that the tracker writes).  HIP events around back-to-back calls, regions of at least 50 ms
          after a warm-up, median of 5; the legs alternate.  And what MPPIPlanner(nominal=) costs per tick at 4 096 envs.
episodes  closed loop with the set-up of tools/bench_goal_cost.py's table (256 envs x 200 ticks, one chain per env, seed 0, 4
          boxes): episodes ended by reason under TrackingPlanner alone (3 speeds x 3 reaches, H = 16) and under MPPIPlanner
          without and with nominal=, on straight and on routed paths, each with cost_weight 0 and 2."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bc_gym_planning_env_amd import MPPIPlanner, TrackingPlanner, _lib, pursuit_gain_library  # noqa: E402
from bc_gym_planning_env_amd.mini_env import BatchedRandomMiniEnv  # noqa: E402

DENSE = dict(half_size=(0.2, 0.5), along=(0.2, 0.8), lateral=2.0, n_yaws=16, seed=7, max_attempts=32)   # bench_scatter_boxes.py's
COST_SCALING = 3.0
REACHES = (0.4, 0.8, 1.6)


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


def leg_timing(horizon=16):
    rows = []
    for n in (65536, 4096):
        env = BatchedRandomMiniEnv(n, n_chains=1024, episodes=4, auto_reset=True, seed=3, sampler="device_resident")
        rng = np.random.RandomState(0)
        for _ in range(30):   # the envs spread over their episodes
            env.step(env.action_space.sample_batch(n, rng))
        for k in (8, 64):
            speeds = max(k // 4, 1)
            gains = torch.from_numpy(pursuit_gain_library(env.action_space, speeds, np.linspace(0.3, 2.0, k // speeds))).cuda()
            tr = env.track(gains, horizon, want=("best", "best_plan"))
            forced = tr.actions.permute(2, 0, 1, 3).contiguous()   # per-env float64 actions for the yardstick
            legs = {"track": lambda: env.track(gains, horizon), "track_trace": lambda: env.track(gains, horizon, want=("trace",)),
                    "track_best_plan": lambda: env.track(gains, horizon, want=("best", "best_plan")),
                    "lookahead": lambda: env.lookahead(forced, want=())}
            res = {"n_envs": n, "n_candidates": k, "horizon": horizon, "mean_steps": float(tr.steps.double().mean())}
            for name in ("lookahead", "track", "track_trace", "track_best_plan", "lookahead_again", "track_again"):
                res[name] = timed(legs[name.replace("_again", "")])
            yard = 0.5 * (res["lookahead"]["ms"] + res["lookahead_again"]["ms"])
            res["track_over_lookahead"] = 0.5 * (res["track"]["ms"] + res["track_again"]["ms"]) / yard
            res["track_trace_over_lookahead"] = res["track_trace"]["ms"] / yard
            res["ns_per_lane_step"] = 1e6 * res["track"]["ms"] / (n * k * horizon)
            print(json.dumps(res), flush=True)
            rows.append(res)
            del tr, forced
        env.check_errors()
        del env
        torch.cuda.empty_cache()
    return rows


def leg_tick(n=4096, horizon=16):
    """What nominal= costs per tick when no episode ends: MPPIPlanner.act() + reset_plans(zeros) with and without it -- with it
    every reset_plans() launches bcp_track, whose masked-out lanes take no trip."""
    env = BatchedRandomMiniEnv(n, n_chains=1024, episodes=4, auto_reset=True, seed=3, sampler="device_resident")
    tracker = TrackingPlanner(env, pursuit_gain_library(env.action_space, 3, REACHES), horizon)
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    res = {"n_envs": n, "horizon": horizon, "mppi": "K = 64, I = 2", "tracker": "K = 9"}
    for name, nominal in (("mppi_tick", None), ("mppi_nominal_tick", tracker), ("mppi_tick_again", None)):
        planner = MPPIPlanner(env, horizon=horizon, n_candidates=64, iterations=2, sigma=(0.2, 0.6), lam=0.3, collision_penalty=2.0,
                              nominal=nominal)

        def tick():
            planner.act()
            planner.reset_plans(done)

        res[name] = timed(tick)
    res["tracker_act"] = timed(tracker.act)
    print(json.dumps(res), flush=True)
    return res


def leg_episodes(ticks=200, n=256, n_boxes=4, horizon=16):
    out = {"n_boxes": n_boxes, "ticks": ticks, "n_envs": n, "gains": "3 speeds x reaches %s" % (REACHES,)}
    for paths in ("straight", "routed"):
        for weight in (None, 2):
            for who in ("tracker", "mppi", "mppi+nominal"):
                env = BatchedRandomMiniEnv(n, n_chains=n, episodes=4, auto_reset=True, seed=0)
                status, _c, _b = env.scatter_obstacles(n_boxes, **DENSE)
                out.setdefault("reverted_entries", int(((status & _lib.SCATTER_REVERTED) != 0).sum()))
                if weight is not None:
                    env.inflate_costmaps(COST_SCALING)
                tally = {"goal": 0, "timeout": 0, "collided": 0, "episodes": 0}
                if paths != "straight":
                    routed = env.route_paths(env.goal_field(cost_weight=weight), stride=2, max_len=160)
                    tally["routed_entries"] = int((routed == 0).sum())
                ends = env.enable_episode_record()
                tracker = TrackingPlanner(env, pursuit_gain_library(env.action_space, 3, REACHES), horizon)
                if who == "tracker":
                    planner = tracker
                else:
                    planner = MPPIPlanner(env, horizon=horizon, n_candidates=64, iterations=2, sigma=(0.2, 0.6), lam=0.3,
                                          collision_penalty=2.0, nominal=tracker if who == "mppi+nominal" else None)
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
    ap.add_argument("--legs", default="timing,episodes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    doc = {"tool": "tools/bench_track.py", "device": torch.cuda.get_device_name(0)}
    if "timing" in legs:
        doc["timing"] = leg_timing()
    if "timing" in legs:
        doc["tick"] = leg_tick()
    if "episodes" in legs:
        doc["episodes"] = leg_episodes()
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()

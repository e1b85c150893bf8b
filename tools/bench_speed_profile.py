"""bcp_path_speed (a curvature speed profile per path, one wave per row) and bcp_track_profile (the tracker that follows it)
measured: writes profiles/speed_profile_bench.json.

    python tools/bench_speed_profile.py [--legs call,track,episodes] [--out FILE]

call      bcp_path_speed on the 4 096 smoothed entries of tools/bench_smooth_route.py's pool (400 slots), beside
          bcp_smooth_route on the same rows in the same process, and on 65 536 rows (every entry's path 16 times).  HIP events
          around back-to-back calls, regions of at least 50 ms after a warm-up, median of 5 (bench_track.timed).
track     bcp_track_profile beside bcp_track at 4 096 and 65 536 envs (K = 9, H = 16), the legs alternating.
episodes  tools/bench_smooth_route.py's closed loop (256 envs x 200 ticks, one chain per env, seed 0, 4 boxes, the same gains and
          smoothing): its 13 rows again -- compared with profiles/smooth_route_bench.json to the episode --, and TrackingPlanner
          and MPPIPlanner(nominal=tracker) on smoothed and smoothed-weighted paths with a speed profile: the ONE setting chosen
          beforehand from the robot (SETTING), then the further settings tried (FURTHER), every one reported."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bc_gym_planning_env_amd import MPPIPlanner, TrackingPlanner, _lib, pursuit_gain_library, robots  # noqa: E402
from bc_gym_planning_env_amd.mini_env import BatchedRandomMiniEnv  # noqa: E402
from bench_smooth_route import MAX_LEN, ROUTE_LEN, SMOOTH  # noqa: E402
from bench_track import COST_SCALING, DENSE, REACHES, timed  # noqa: E402

TOP, LOWEST = robots.MAX_FRONT_WHEEL_SPEED / 2, robots.MAX_FRONT_WHEEL_SPEED / 10    # action_space.high[0], low[0]
# The setting, fixed before any episode was run.  v_max: the top of the action box.  w_max: the yaw rate the tricycle reaches
# with its wheel at the stop and at top speed, high[0] * sin(max_front_wheel_angle) / front_wheel_from_axis.  a_dec, a_acc: the
# robot's linear acceleration limit.  a_lat: the same figure sideways.  v_min: the bottom of the action box -- the wheel
# command is clipped there, so a lower cap would ask for what the robot cannot do.  v_start, v_end: v_max (the env's default).
SETTING = dict(v_max=TOP, w_max=TOP * np.sin(robots.MAX_FRONT_WHEEL_ANGLE) / robots.FRONT_WHEEL_FROM_AXIS,
               a_dec=robots.MAX_LINEAR_ACCELERATION, a_acc=robots.MAX_LINEAR_ACCELERATION, a_lat=robots.MAX_LINEAR_ACCELERATION,
               v_min=LOWEST, span=1)
FURTHER = {"a_lat halved": dict(SETTING, a_lat=SETTING["a_lat"] / 2), "v_min 0": dict(SETTING, v_min=0.0)}


def leg_call():
    env = BatchedRandomMiniEnv(4096, n_chains=1024, episodes=4, auto_reset=True, sampler="device_resident")
    fields = env.goal_field()
    cells, cell_lens, _st = fields.route_bound(stride=1, max_len=ROUTE_LEN)
    cells, cell_lens = cells.clone(), cell_lens.clone()
    smooth = lambda: fields.smooth(cells, cell_lens, entries=True, max_len=MAX_LEN, want=("init", "info"), **SMOOTH)   # noqa: E731
    paths, lens, _s, _i, _info = smooth()
    paths, lens = paths.clone(), lens.clone()
    n = int(paths.shape[0])
    res = {"entries": n, "max_len": MAX_LEN, "params": SETTING, "mean_len": float(lens.double().mean())}
    speed = lambda p, ln, want=(): env.path_speed(p, ln, want=want, **SETTING)   # noqa: E731
    res["smooth_entries"] = timed(smooth)
    res["path_speed_entries"] = timed(lambda: speed(paths, lens))
    res["path_speed_entries_all_outputs"] = timed(lambda: speed(paths, lens, ("kappa", "v_limit")))
    res["smooth_entries_again"] = timed(smooth)
    res["path_speed_entries_again"] = timed(lambda: speed(paths, lens))
    yard = 0.5 * (res["smooth_entries"]["ms"] + res["smooth_entries_again"]["ms"])
    res["path_speed_over_smooth"] = 0.5 * (res["path_speed_entries"]["ms"] + res["path_speed_entries_again"]["ms"]) / yard
    prof = speed(paths, lens, ("kappa",))
    live = torch.arange(MAX_LEN, device="cuda")[None] < lens[:, None]
    res["status_nonzero"] = int((prof.status != 0).sum())
    res["share_of_way_points_below_0.9_v_max"] = float(((prof.speed < 0.9 * TOP) & live).sum() / live.sum())
    res["share_of_way_points_at_v_min"] = float(((prof.speed <= LOWEST) & live).sum() / live.sum())
    rows, row_lens = paths.repeat(16, 1, 1), lens.repeat(16)
    res["rows"] = {"rows": int(rows.shape[0]), "path_speed": timed(lambda: speed(rows, row_lens))}
    res["rows"]["path_speed_over_entries"] = res["rows"]["path_speed"]["ms"] / res["path_speed_entries"]["ms"]
    print(json.dumps(res), flush=True)
    return res


def leg_track(horizon=16):
    out = []
    for n in (4096, 65536):
        env = BatchedRandomMiniEnv(n, n_chains=1024, episodes=4, auto_reset=True, seed=3, sampler="device_resident")
        rng = np.random.RandomState(0)
        for _ in range(30):   # the envs spread over their episodes
            env.step(env.action_space.sample_batch(n, rng))
        gains = torch.from_numpy(pursuit_gain_library(env.action_space, 3, REACHES)).cuda()
        prof = env.speed_profile(**{k: v for k, v in SETTING.items() if k != "v_max"})
        legs = {"track": lambda: env.track(gains, horizon), "track_profile": lambda: env.track(gains, horizon, speed_profile=prof)}
        res = {"n_envs": n, "n_candidates": int(gains.shape[0]), "horizon": horizon}
        for name in ("track", "track_profile", "track_again", "track_profile_again"):
            res[name] = timed(legs[name.replace("_again", "")])
        res["track_profile_over_track"] = (res["track_profile"]["ms"] + res["track_profile_again"]["ms"]) / (
            res["track"]["ms"] + res["track_again"]["ms"])
        print(json.dumps(res), flush=True)
        out.append(res)
        del env
        torch.cuda.empty_cache()
    return out


def episodes_row(paths, weight, who, setting, ticks=200, n=256, n_boxes=4, horizon=16):
    """bench_smooth_route.leg_episodes' row; setting: None, or the parameters of env.speed_profile()"""
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
    profile = None if setting is None else env.speed_profile(**{k: v for k, v in setting.items() if k != "v_max"})
    ends = env.enable_episode_record()
    tracker = TrackingPlanner(env, pursuit_gain_library(env.action_space, 3, REACHES), horizon, speed_profile=profile)
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
    return tally


def leg_episodes():
    out = {"n_boxes": 4, "ticks": 200, "n_envs": 256, "gains": "3 speeds x reaches %s" % (REACHES,), "smooth": SMOOTH,
           "setting": SETTING, "further_settings": FURTHER}
    plan = [("straight", None, w) for w in ("tracker", "mppi", "mppi+nominal")]
    plan += [("routed", wt, w) for wt in (None, 2) for w in ("tracker", "mppi", "mppi+nominal")]
    plan += [("smoothed", wt, w) for wt in (None, 2) for w in ("tracker", "mppi+nominal")]
    before = {}
    known = os.path.join(ROOT, "profiles", "smooth_route_bench.json")
    if os.path.exists(known):
        with open(known) as f:
            before = json.load(f).get("episodes", {})
    differ = []
    for paths, weight, who in plan:
        name = "%s, cost_weight %d: %s" % (paths, weight or 0, who)
        out[name] = episodes_row(paths, weight, who, None)
        print(name, json.dumps(out[name]), flush=True)
        if name in before and any(before[name][k] != out[name][k] for k in ("goal", "timeout", "collided", "episodes")):
            differ.append(name)
    out["existing_rows_compared"] = sum(1 for p, wt, w in plan if "%s, cost_weight %d: %s" % (p, wt or 0, w) in before)
    out["existing_rows_that_differ"] = differ
    for label, setting in [("profile", SETTING)] + [("profile (%s)" % k, v) for k, v in FURTHER.items()]:
        for weight in (None, 2):
            for who in ("tracker", "mppi+nominal"):
                name = "smoothed, cost_weight %d: %s + %s" % (weight or 0, who, label)
                out[name] = episodes_row("smoothed", weight, who, setting)
                print(name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="call,track,episodes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speed_profile_bench.json"))
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    doc = {"tool": "tools/bench_speed_profile.py", "device": torch.cuda.get_device_name(0)}
    if os.path.exists(args.out):          # legs run one at a time add to the document
        with open(args.out) as f:
            doc.update(json.load(f))
    for leg, fn in (("call", leg_call), ("track", leg_track), ("episodes", leg_episodes)):
        if leg in legs:
            doc[leg] = fn()
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()

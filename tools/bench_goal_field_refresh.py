"""Goal fields that follow an endless pool (goal_field(follow_refresh=True)): what the bound build costs beside the existing
one, and what a following field adds to endless stepping and to a planner loop.  Prints one JSON line:

  build     bcp_goal_field_bound over all entries of a 4 096 x 4 endless pool against bcp_goal_field with
            goal_field.path_seeds on the same tensors (the seeds in torch, then the launch), clearance_d2 151
  stepping  endless stepping at 4 096 and 16 384 envs x 4 entries, refresh(overlap=True) every 128 steps, with no field and
            with one following field: ms per step over a region of at least 50 ms, the region once more, and the longest
            single step launch (an event pair per step, in a pass of its own)
  priority  (not in the default set) the stepping leg once more with the steps on a high-priority stream
  planner   MPPIPlanner at 4 096 endless envs, (K, H, I) = (64, 16, 2), a tick = act + step + reset_plans, refresh(overlap=True)
            every 128 ticks: ms per tick with goal_field = a following field, and with no field at all (plain bcp_mppi)

HIP events on the steps' stream; every region follows a warm-up and is run twice (tools/bench_goal_field.py's habits).
Nothing here is a threshold: the figures are what was measured.  65 536 envs x 4 entries would be 17.6 GB of fields and is
left out.

    python tools/bench_goal_field_refresh.py [--legs build,stepping,planner] > profiles/goal_field_refresh_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bc_gym_planning_env_amd import EnvParams, MPPIPlanner, _lib, goal_field, mini_env  # noqa: E402

EVERY = 128


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


def endless(n):
    params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2))
    return mini_env.BatchedRandomMiniEnv(n, params, episodes=4, endless=True, auto_reset=True, seed=1)


def actions(n):
    g = torch.Generator(device="cuda").manual_seed(0)
    scale = torch.tensor([1.0, 1.0], device="cuda", dtype=torch.float64)
    shift = torch.tensor([0.0, 0.5], device="cuda", dtype=torch.float64)
    return [torch.rand(n, 2, device="cuda", generator=g, dtype=torch.float64) * scale - shift for _ in range(16)]


def build_leg(n):
    env = endless(n)
    data = env.costmap_tensor
    entries, rows, cols = (int(v) for v in data.shape)
    field = torch.empty((entries, rows, cols), dtype=torch.uint16, device=env.device)
    other = torch.empty_like(field)
    info = torch.zeros((entries, 2), dtype=torch.int32, device=env.device)
    stream = env._stream()
    seeds = goal_field.path_seeds(env, "goal")

    def bound():
        _lib.check(env._lib.bcp_goal_field_bound(env._h, None, None, entries, 151, 0, field.data_ptr(), info.data_ptr(), stream))

    def launch(s):
        _lib.check(env._lib.bcp_goal_field(env._h, data.data_ptr(), entries, rows, cols, 0, None, None, s.data_ptr(), 1, 151, 0,
                                           other.data_ptr(), info.data_ptr(), stream))

    def existing():
        launch(goal_field.path_seeds(env, "goal"))

    out = {"entries": entries, "shape": [rows, cols], "clearance_d2": 151}
    for name, fn in (("bound", bound), ("goal_field_with_path_seeds", existing), ("goal_field_launch_alone", lambda: launch(seeds))):
        ms, reps = timed_ms(fn)
        again, _ = timed_ms(fn)
        out[name] = {"ms": round(ms, 4), "ms_again": round(again, 4), "reps": reps, "us_per_entry": round(1e3 * ms / entries, 3)}
    torch.cuda.synchronize()
    out["same_bytes"] = bool(torch.equal(field.view(torch.int16), other.view(torch.int16)))
    out["gave_up"] = int(info[:, 1].sum())
    env.close()
    return out


def stepping_region(env, acts, steps):
    """ms per step of `steps` steps with an overlapped refresh every EVERY steps, and the worlds the refreshes re-sampled"""
    infos = []
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(steps):
        env.step(acts[k % 16])
        if k % EVERY == EVERY - 1:
            done = env.refresh(overlap=True)
            if done is not None:
                infos.append(done.clone())
    stop.record()
    stop.synchronize()
    worlds = int(torch.stack(infos)[:, 0].sum()) if infos else 0
    return start.elapsed_time(stop) / steps, worlds, len(infos)


def longest_step(env, acts, steps):
    pairs = []
    for k in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        env.step(acts[k % 16])
        b.record()
        pairs.append((a, b))
        if k % EVERY == EVERY - 1:
            env.refresh(overlap=True)
    torch.cuda.synchronize()
    times = np.array([a.elapsed_time(b) for a, b in pairs])
    return float(times.max()), float(np.median(times)), int(times.argmax() % EVERY)


def stepping_leg(n):
    out = {"n_envs": n, "entries": 4 * n, "refresh_every": EVERY}
    acts = actions(n)
    for name, follow in (("no_field", False), ("one_following_field", True)):
        env = endless(n)
        fields = env.goal_field(follow_refresh=True) if follow else None
        for k in range(16 * EVERY):    # warm-up: until episodes end at a steady rate; creates the side stream
            env.step(acts[k % 16])
            if k % EVERY == EVERY - 1:
                env.refresh(overlap=True)
        torch.cuda.synchronize()
        steps = 32 * EVERY             # the same region in both legs: 60 ms of bare steps
        ms, worlds, refreshes = stepping_region(env, acts, steps)
        assert ms * steps >= 50.0, "region shorter than 50 ms"
        again, worlds_again, _ = stepping_region(env, acts, steps)
        worst, median, at = longest_step(env, acts, 4 * EVERY)
        env.finish_refresh()
        torch.cuda.synchronize()
        out[name] = {"ms_per_step": round(ms, 5), "ms_per_step_again": round(again, 5), "steps": steps, "refreshes": refreshes,
                     "worlds_resampled": worlds, "worlds_resampled_again": worlds_again,
                     "longest_step_ms": round(worst, 4), "median_step_ms": round(median, 5), "longest_step_is_step_after_refresh": at,
                     "field_bytes": 0 if fields is None else fields.field.numel() * 2,
                     "gave_up": 0 if fields is None else int(fields.info[:, 1].sum())}
        env.close()
        del env, fields
        torch.cuda.empty_cache()
    a, b = out["no_field"], out["one_following_field"]
    for tag in ("", "_again"):
        added = b["ms_per_step" + tag] - a["ms_per_step" + tag]
        out["field_adds_ms_per_step" + tag] = round(added, 5)
        if b["worlds_resampled" + tag]:
            out["field_adds_us_per_resampled_world" + tag] = round(1e3 * added * b["steps"] / b["worlds_resampled" + tag], 3)
    return out


def stepping_leg_high_priority(n):
    """the stepping leg with everything but the refresh on a high-priority stream, as refresh()'s docstring advises"""
    hi = torch.cuda.Stream(priority=-1)
    hi.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(hi):
        out = stepping_leg(n)
    torch.cuda.current_stream().wait_stream(hi)
    out["steps_on"] = "torch.cuda.Stream(priority=-1)"
    return out


def planner_leg(n):
    out = {"n_envs": n, "K_H_I": [64, 16, 2], "refresh_every": EVERY}
    for name, follow in (("no_field", False), ("one_following_field", True)):
        env = endless(n)
        fields = env.goal_field(follow_refresh=True) if follow else None
        kw = dict(goal_field=fields, terminal_weight=4.0) if follow else {}
        planner = MPPIPlanner(env, horizon=16, n_candidates=64, iterations=2, sigma=(0.2, 0.6), lam=0.3, collision_penalty=2.0,
                              seed=0, **kw)
        tick = [0]

        def one():
            _o, _r, done, _i = env.step(planner.act())
            planner.reset_plans(done)
            tick[0] += 1
            if tick[0] % EVERY == 0:
                env.refresh(overlap=True)

        for _ in range(EVERY):
            one()
        ms, reps = timed_ms(lambda: [one() for _ in range(EVERY)])
        again, _ = timed_ms(lambda: [one() for _ in range(EVERY)])
        env.finish_refresh()
        torch.cuda.synchronize()
        out[name] = {"ms_per_tick": round(ms / EVERY, 5), "ms_per_tick_again": round(again / EVERY, 5), "ticks": reps * EVERY}
        env.close()
        del env, fields, planner
        torch.cuda.empty_cache()
    out["field_adds_ms_per_tick"] = round(out["one_following_field"]["ms_per_tick"] - out["no_field"]["ms_per_tick"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="build,stepping,planner")
    ap.add_argument("--envs", default="4096,16384", help="env counts of the stepping leg")
    args = ap.parse_args()
    legs = args.legs.split(",")
    out = {"tool": "tools/bench_goal_field_refresh.py", "device": torch.cuda.get_device_name(0), "legs": {}}
    if "build" in legs:
        out["legs"]["build_4096x4"] = build_leg(4096)
    if "stepping" in legs:
        for n in (int(v) for v in args.envs.split(",")):
            out["legs"]["stepping_%dx4" % n] = stepping_leg(n)
    if "priority" in legs:
        for n in (int(v) for v in args.envs.split(",")):
            out["legs"]["stepping_%dx4_high_priority_steps" % n] = stepping_leg_high_priority(n)
    if "planner" in legs:
        out["legs"]["planner_4096x4"] = planner_leg(4096)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

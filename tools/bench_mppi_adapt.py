"""bcp_mppi_adapt (sampling widths that follow the weights, rate 0.5) against bcp_mppi of the same build: what the second
walk over a row's candidates costs; and MPPIPlanner with a fixed sigma against adapt_rate 0.25 / 0.5 x sigma_recover 0 / 0.1,
with and without the goal field, in closed loop.  Metric configuration of tools/bench_mppi.py (RandomMiniEnv seed-0 geometry,
shared map and path) at steady state.  HIP events around every repetition, after warm-up; median (min - max).

    python tools/bench_mppi_adapt.py [reps] [--label NAME] [--json FILE] [--quality]

--label NAME  goes into every printed line and record
--json FILE   append one JSON record per shape (and per --quality run) to FILE
--quality     instead of the timings: the planners on BatchedRandomMiniEnv, 256 envs, 200 ticks, H = 16, K = 64, I = 2, the
              same seeds -- mean return per env, the share of ended episodes that reached the goal, and where the widths
              ended (median sigma / sigma0 per component, share on a clamp)

(bcp_mppi of this build against a parent commit's: tools/bench_mppi.py --lib, alternated, every run a process of its own.)"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
import bench

ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=7)
ap.add_argument("--label", default="")
ap.add_argument("--json")
ap.add_argument("--quality", action="store_true")
args = ap.parse_args()
reps = args.reps
SIGMA, LAM, PENALTY = (0.2, 0.6), 0.3, 2.0
RATE = 0.5
TERMINAL_WEIGHT = 4.0   # as tools/bench_mppi.py --quality


def record(rec):
    rec = dict(rec, label=args.label)
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


def timed(fn, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return "%.3f ms (%.3f - %.3f)" % (float(np.median(ms)), float(np.min(ms)), float(np.max(ms))), float(np.median(ms)), ms


def quality():
    from bc_gym_planning_env_amd import MPPIPlanner, mini_env
    n, ticks = 256, 200
    runs = [(None, 0.0)] + [(rate, recover) for rate in (0.25, 0.5) for recover in (0.0, 0.1)]
    for field in (False, True):
        for rate, recover in runs:
            env = mini_env.BatchedRandomMiniEnv(n, n_chains=64, episodes=4, auto_reset=True, seed=3)
            ends = env.enable_episode_record()
            kw = dict(goal_field=env.goal_field(), terminal_weight=TERMINAL_WEIGHT) if field else {}
            planner = MPPIPlanner(env, horizon=16, n_candidates=64, iterations=2, sigma=SIGMA, lam=LAM, collision_penalty=PENALTY,
                                  seed=0, adapt_rate=rate, sigma_recover=recover, **kw)
            total = torch.zeros(n, dtype=torch.float64, device="cuda")
            ended = torch.zeros(3, dtype=torch.int64, device="cuda")   # episodes ended, at the goal, collided
            for _ in range(ticks):
                _, rew, done, _ = env.step(planner.act())
                planner.reset_plans(done)
                total += rew
                r = ends.reason
                ended += torch.stack([(r != 0).sum(), ((r & ends.GOAL) != 0).sum(), ((r & ends.COLLIDED) != 0).sum()])
            env.check_errors()
            e = [int(v) for v in ended.cpu()]
            rec = dict(leg="quality", goal_field=field, adapt_rate=rate, sigma_recover=recover, n_envs=n, ticks=ticks,
                       mean_return=float(total.mean()), episodes_ended=e[0], reached_goal=e[1], collided=e[2],
                       goal_rate=e[1] / max(e[0], 1))
            widths = ""
            if rate is not None:
                s = planner.sigma.cpu().numpy().reshape(-1, 2)
                lo, hi = np.asarray(planner.sigma_min), np.asarray(planner.sigma_max)
                rec.update(median_sigma_ratio=[float(v) for v in np.median(s / np.asarray(SIGMA), axis=0)],
                           on_sigma_min=[float(v) for v in (s == lo).mean(axis=0)], on_sigma_max=[float(v) for v in (s == hi).mean(axis=0)])
                widths = ", median sigma / sigma0 (v, w) %.2f, %.2f, on sigma_min %.1f %% / %.1f %%, on sigma_max %.1f %% / %.1f %%" % (
                    tuple(rec["median_sigma_ratio"]) + tuple(100 * v for v in rec["on_sigma_min"] + rec["on_sigma_max"]))
            print("%s MPPIPlanner %s the goal field, %s: mean return %.4f, %d episodes ended, %d at the goal (%.3f), %d collided%s"
                  % (args.label, "with" if field else "without",
                     "fixed sigma" if rate is None else "adapt_rate %.2f, sigma_recover %.1f" % (rate, recover),
                     rec["mean_return"], e[0], e[1], rec["goal_rate"], e[2], widths), flush=True)
            record(rec)


if args.quality:
    quality()
    sys.exit(0)

for n, k, h, it in ((4096, 64, 16, 4), (65536, 16, 8, 2)):
    env, g = bench.make_env(n, 0, 0, 2024)
    rng = np.random.RandomState(1234)
    pool = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(16)])).cuda()
    bench.steady_state(env, pool, rng)
    low = torch.from_numpy(np.asarray(env.action_space.low, np.float64)).cuda()
    high = torch.from_numpy(np.asarray(env.action_space.high, np.float64)).cuda()
    mean0 = (0.5 * (low + high)).expand(n, h, 2).contiguous()
    sigma0 = torch.tensor(SIGMA, dtype=torch.float64, device="cuda").expand(n, h, 2).contiguous()
    mean, widths = mean0.clone(), sigma0.clone()
    adapt = dict(sigma=widths, rate=RATE, sigma_min=tuple(s / 8 for s in SIGMA), sigma_max=tuple(2 * s for s in SIGMA))
    out = {}

    def plain():
        mean.copy_(mean0)
        widths.copy_(sigma0)    # (the same two copies in both legs: only the launch differs)
        out["plain"] = env.mppi(mean, SIGMA, it, k, LAM, PENALTY, seed=1, draw_index=0)

    def adaptive():
        mean.copy_(mean0)
        widths.copy_(sigma0)
        out["adapt"] = env.mppi(mean, SIGMA, it, k, LAM, PENALTY, seed=1, draw_index=0, adapt=adapt)

    # adapt, plain, adapt, plain: the two kernels in turn, so that a drift of the clocks shows in both
    a1, a1_med, a1_all = timed(adaptive)
    p1, p1_med, p1_all = timed(plain)
    a2, a2_med, a2_all = timed(adaptive)
    ratio = (widths / sigma0).reshape(-1, 2).median(dim=0).values.cpu().numpy()   # (before the plain leg puts them back)
    p2, p2_med, p2_all = timed(plain)
    plain_med, adapt_med = 0.5 * (p1_med + p2_med), 0.5 * (a1_med + a2_med)
    print("%sN = %d, K = %d, H = %d, I = %d (%d candidate steps): bcp_mppi_adapt (rate %.1f) %s, %s | bcp_mppi %s, %s | the widths: "
          "%+.3f ms per call (%+.2f %%), %.3f ns per candidate, step and iteration; median sigma / sigma0 after the call %.2f, %.2f"
          % (args.label + "  " if args.label else "", n, k, h, it, n * k * h * it, RATE, a1, a2, p1, p2, adapt_med - plain_med,
             100 * (adapt_med / plain_med - 1), 1e6 * (adapt_med - plain_med) / (n * k * h * it), ratio[0], ratio[1]), flush=True)
    record(dict(leg="timing", shape=[n, k, h, it], reps=reps, rate=RATE, mppi_ms=[round(p1_med, 4), round(p2_med, 4)],
                mppi_adapt_ms=[round(a1_med, 4), round(a2_med, 4)], mppi_min_ms=round(min(p1_all + p2_all), 4),
                mppi_max_ms=round(max(p1_all + p2_all), 4), mppi_adapt_min_ms=round(min(a1_all + a2_all), 4),
                mppi_adapt_max_ms=round(max(a1_all + a2_all), 4), widths_ms=round(adapt_med - plain_med, 4),
                widths_percent=round(100 * (adapt_med / plain_med - 1), 3)))
    env.check_errors()
    del env, out, mean, mean0, widths, sigma0
    torch.cuda.empty_cache()

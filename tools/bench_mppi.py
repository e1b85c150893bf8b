"""bcp_mppi against the composition the package allowed before it -- per iteration torch.randn of [H, N, K, 2], add / clip,
a per-env env.lookahead, and torch reductions for the weights and the new mean -- and against I plain look-aheads, the floor
(the roll-outs alone, their actions already in memory); and bcp_mppi_field (the goal field's distance to go in the score, read
inside the launch) against bcp_mppi in the same build: what the terminal read costs.  Metric configuration (RandomMiniEnv
seed-0 geometry, shared map and path) at steady state.  HIP events around every repetition, after warm-up; median (min - max).

    python tools/bench_mppi.py [reps] [--lib PATH] [--label NAME] [--json FILE] [--quality]

--lib PATH    time another build of libbcplan.so (a parent commit's, for a comparison across commits: alternate the two
              libraries, every run a process of its own); a library without bcp_mppi_field skips that leg
--label NAME  goes into every printed line and record
--json FILE   append one JSON record per shape (and per --quality run) to FILE
--quality     instead of the timings: MPPIPlanner with and without the terminal cost on BatchedRandomMiniEnv, 256 envs, 200
              ticks, the same seeds -- mean return per env and the share of ended episodes that reached the goal"""
import argparse
import ctypes
import json
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
import bench

ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=7)
ap.add_argument("--lib")
ap.add_argument("--label", default="")
ap.add_argument("--json")
ap.add_argument("--quality", action="store_true")
args = ap.parse_args()
reps = args.reps
SIGMA, LAM, PENALTY = (0.2, 0.6), 0.3, 2.0
TERMINAL_WEIGHT = 4.0   # reward per metre of distance to go (the weight tests/test_mppi_field_host.py settles on)

from bc_gym_planning_env_amd import _lib
if args.lib:
    _lib.LIB_PATH = args.lib
have_field = hasattr(ctypes.CDLL(_lib.LIB_PATH), "bcp_mppi_field")
for younger in ("bcp_mppi_field", "bcp_mppi_adapt"):
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), younger):
        _lib.SYMBOLS.pop(younger)   # an older build: everything else binds as it is


def record(rec):
    rec = dict(rec, label=args.label, lib=args.lib or "this build")
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
    for which in ("without", "with"):
        env = mini_env.BatchedRandomMiniEnv(n, n_chains=64, episodes=4, auto_reset=True, seed=3)
        ends = env.enable_episode_record()
        kw = dict(goal_field=env.goal_field(), terminal_weight=TERMINAL_WEIGHT) if which == "with" else {}
        planner = MPPIPlanner(env, horizon=16, n_candidates=64, iterations=2, sigma=(0.2, 0.6), lam=0.3, collision_penalty=2.0,
                              seed=0, **kw)
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
        rec = dict(leg="quality", terminal_cost=which, terminal_weight=TERMINAL_WEIGHT if which == "with" else 0.0, n_envs=n,
                   ticks=ticks, mean_return=float(total.mean()), episodes_ended=e[0], reached_goal=e[1], collided=e[2],
                   goal_rate=e[1] / max(e[0], 1))
        print("%s MPPIPlanner %s the terminal cost, %d envs, %d ticks: mean return %.4f, %d episodes ended, %d at the goal (%.3f), "
              "%d collided" % (args.label, which, n, ticks, rec["mean_return"], e[0], e[1], rec["goal_rate"], e[2]), flush=True)
        record(rec)


if args.quality:
    if not have_field:
        sys.exit("--quality needs a library with bcp_mppi_field")
    quality()
    sys.exit(0)

for n, k, h, it in ((4096, 64, 16, 4), (65536, 16, 8, 2)):
    env, g = bench.make_env(n, 0, 0, 2024)
    rng = np.random.RandomState(1234)
    pool = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(16)])).cuda()
    bench.steady_state(env, pool, rng)
    low = torch.from_numpy(np.asarray(env.action_space.low, np.float64)).cuda()
    high = torch.from_numpy(np.asarray(env.action_space.high, np.float64)).cuda()
    sigma = torch.tensor(SIGMA, dtype=torch.float64, device="cuda")
    mean0 = (0.5 * (low + high)).expand(n, h, 2).contiguous()
    mean = mean0.clone()
    out = {}

    def fused():
        mean.copy_(mean0)
        out["fused"] = env.mppi(mean, SIGMA, it, k, LAM, PENALTY, seed=1, draw_index=0)

    def composed():
        m = mean0.clone()                                                  # [N, H, 2]
        for _ in range(it):
            eps = torch.randn(h, n, k, 2, dtype=torch.float32, device="cuda")
            eps[:, :, 0] = 0.0
            u = torch.minimum(torch.maximum(m.transpose(0, 1)[:, :, None] + sigma * eps.double(), low), high).contiguous()
            la = env.lookahead(u, want=())
            score = torch.where((la.reason & 4) != 0, la.ret - PENALTY, la.ret)
            w = torch.softmax(score / LAM, dim=1)                          # [N, K]
            m = (w[None, :, :, None] * u).sum(dim=2).transpose(0, 1).contiguous()
        out["composed"] = m

    u_fixed = torch.minimum(torch.maximum(mean0.transpose(0, 1)[:, :, None] + sigma *
                                          torch.randn(h, n, k, 2, dtype=torch.float64, device="cuda"), low), high).contiguous()

    def floor():
        for _ in range(it):
            out["la"] = env.lookahead(u_fixed, want=())

    f_txt, f_med, f_all = timed(fused)
    c_txt, c_med, _ = timed(composed)
    l_txt, l_med, _ = timed(floor)
    print("%sN = %d, K = %d, H = %d, I = %d (%d candidate steps): bcp_mppi %s | randn + clip + lookahead + softmax update, I "
          "times %s | I x lookahead alone %s | composition / fused %.2f, fused / floor %.2f | bytes of the composition's "
          "buffers per iteration: %.1f MB, of the fused call: %.3f MB"
          % (args.label + "  " if args.label else "", n, k, h, it, n * k * h * it, f_txt, c_txt, l_txt, c_med / f_med,
             f_med / l_med, (4 + 8) * 2 * h * n * k / 1e6, 16 * h * n / 1e6), flush=True)
    rec = dict(leg="timing", shape=[n, k, h, it], reps=reps, mppi_ms=round(f_med, 4), mppi_min_ms=round(min(f_all), 4),
               mppi_max_ms=round(max(f_all), 4), composed_ms=round(c_med, 4), floor_ms=round(l_med, 4))
    if have_field:
        fields = env.goal_field()

        def fused_field():
            mean.copy_(mean0)
            out["field"] = env.mppi(mean, SIGMA, it, k, LAM, PENALTY, seed=1, draw_index=0, goal_field=fields,
                                    terminal_weight=TERMINAL_WEIGHT)

        # field, plain, field, plain: the two kernels in turn, so that a drift of the clocks shows in both
        t1, t1_med, t1_all = timed(fused_field)
        p2, p2_med, p2_all = timed(fused)
        t2, t2_med, t2_all = timed(fused_field)
        plain_med, field_med = 0.5 * (f_med + p2_med), 0.5 * (t1_med + t2_med)
        res = env.mppi(mean0.clone(), SIGMA, it, k, LAM, PENALTY, seed=1, draw_index=0, goal_field=fields,
                       terminal_weight=TERMINAL_WEIGHT, want=("iter_value",))
        none = float((res.iter_value == _lib.GOAL_NONE).double().mean())
        print("%s    bcp_mppi_field %s, %s | bcp_mppi again %s | terminal read: %+.3f ms per call (%+.2f %%), %.3f ns per candidate "
              "and iteration; %.1f %% of the final poses without a route"
              % (args.label + "  " if args.label else "", t1, t2, p2, field_med - plain_med, 100 * (field_med / plain_med - 1),
                 1e6 * (field_med - plain_med) / (n * k * it), 100 * none), flush=True)
        rec.update(mppi_again_ms=round(p2_med, 4), mppi_field_ms=[round(t1_med, 4), round(t2_med, 4)],
                   mppi_field_min_ms=round(min(t1_all + t2_all), 4), mppi_field_max_ms=round(max(t1_all + t2_all), 4),
                   terminal_read_ms=round(field_med - plain_med, 4), terminal_read_percent=round(100 * (field_med / plain_med - 1), 3),
                   terminal_weight=TERMINAL_WEIGHT, final_poses_without_a_route=round(none, 4))
    record(rec)
    env.check_errors()
    del env, out, u_fixed, mean, mean0
    torch.cuda.empty_cache()

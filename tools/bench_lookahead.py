"""bcp_lookahead against the composition the package allowed before it: a second handle of N * K envs, set_state from
repeat_interleave'd tensors, rollout(H) with the expanded actions, torch reductions for ret and best.  Metric
configuration (RandomMiniEnv seed-0 geometry, shared map and path), shared candidate library, noise-free model,
best_action requested.  HIP events around every repetition, after warm-up; median and min.

    python tools/bench_lookahead.py [reps]"""
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
import bench
from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, constant_command_library

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STATE = ("robot", "min_spat_dist_so_far", "target_idx", "current_iter", "robot_collided")


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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


for n, k, h in ((4096, 64, 16), (65536, 16, 8)):
    env, g = bench.make_env(n, 0, 0, 2024)
    rng = np.random.RandomState(1234)
    pool = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(16)])).cuda()
    bench.steady_state(env, pool, rng)
    n_v = 4
    lib = torch.from_numpy(constant_command_library(env.action_space, n_v, k // n_v, h)).cuda()
    assert lib.shape == (h, k, 2)
    res = float(g["resolution"])                               # the composition's second handle: noise-free, no auto-reset
    twin = BatchedPlanEnv(CostMap2D(g["costmap"], res, g["origin"]), g["path"], env.params, n_envs=n * k, noise_parameters=None)
    expanded = lib[:, None].expand(h, n, k, 2).reshape(h, n * k, 2).contiguous()
    coll = torch.zeros(h, n * k, dtype=torch.uint8, device="cuda")
    out = {}

    def fused():
        out["la"] = env.lookahead(lib, want=("best", "best_action"))

    def composed():
        snap = env.get_state()
        for name in STATE:
            setattr(snap, name, getattr(snap, name).repeat_interleave(k, dim=-1))
        twin.set_state(snap)
        rew, done = twin.rollout(expanded, collided_out=coll)
        ended_before = (torch.cumsum(done, 0, dtype=torch.int32) - done) > 0     # a done step earlier in the sequence
        ret = torch.where(ended_before, torch.zeros_like(rew), rew).cumsum(0)[-1].reshape(n, k)
        hit = (torch.where(ended_before, torch.zeros_like(coll), coll).sum(0) > 0).reshape(n, k) | \
            snap.robot_collided.reshape(n, k).bool()
        best = torch.argmax(torch.where(hit, ret - 1e12, ret), dim=1)
        out["ret"], out["best"], out["action"] = ret, best, lib[0][best]

    f_med, f_min, f_max = timed(fused)
    c_med, c_min, c_max = timed(composed)
    la = out["la"]
    same_ret = bool(torch.equal(la.ret, out["ret"]))
    same_best = float((la.best.long() == out["best"]).float().mean())
    print("N = %d, K = %d, H = %d (%d candidate steps): bcp_lookahead median %.3f ms (min %.3f, max %.3f) | second handle + "
          "set_state + rollout + torch median %.3f ms (min %.3f, max %.3f) | ratio of medians %.2f | ret equal: %s, best equal "
          "for %.4f of the envs" % (n, k, h, n * k * h, f_med, f_min, f_max, c_med, c_min, c_max, c_med / f_med, same_ret,
                                    same_best), flush=True)
    env.check_errors()
    twin.check_errors()
    del env, twin, expanded, coll, out
    torch.cuda.empty_cache()

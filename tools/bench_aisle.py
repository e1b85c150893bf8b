"""Informational timing of BatchedRandomAisleTurnEnv: pool build (host numpy vs device sampler) and env-steps/s at
65 536 envs with auto-reset onto new turns, the step alone and step + ColoredEgoCostmap observation.
Usage: python tools/bench_aisle.py [n_envs] [chains] [episodes] [steps]   (prints one JSON line at the end)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bc_gym_planning_env_amd import EnvParams, aisle_env  # noqa: E402
from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
chains = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
episodes = int(sys.argv[3]) if len(sys.argv) > 3 else 4
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 200
ep = EnvParams()
out = {"n_envs": n, "chains": chains, "episodes": episodes, "steps": steps}

for worlds in (4096, 16384):
    seeds = list(range(worlds // 4))
    t0 = time.perf_counter()
    host = aisle_env.sample_aisle_pool(ep, seeds, 4)
    out["host_pool_s_%d" % worlds] = time.perf_counter() - t0
    del host
    for resident in (False, True):
        aisle_env.sample_aisle_pool_device(ep, seeds[:64], 4, keep_on_device=resident)   # warm-up (module load)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dp = aisle_env.sample_aisle_pool_device(ep, seeds, 4, keep_on_device=resident)
        torch.cuda.synchronize()
        out["device%s_pool_s_%d" % ("_resident" if resident else "", worlds)] = time.perf_counter() - t0
        del dp
    print(json.dumps({k: v for k, v in out.items() if "pool" in k}), flush=True)

env = aisle_env.BatchedRandomAisleTurnEnv(n, ep, n_chains=chains, episodes=episodes, sampler="device_resident",
                                          auto_reset=True, seed=3)
out["pool_maps_shape"] = list(env.pool.maps.shape)
out["pool_device_mb"] = env.pool.nbytes() / 1e6
wrap = BatchedColoredEgoCostmap(env)
rng = np.random.RandomState(0)
acts = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(8)])).cuda()
acts[:, :, 0] *= 3.0
for name, fn in (("step", env.step), ("step_colored_ego", wrap.step)):
    for k in range(20):
        fn(acts[k % 8])
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(steps):
        fn(acts[k % 8])
    end.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(end) / steps
    out[name + "_ms"] = ms
    out[name + "_env_steps_per_s"] = n / (ms * 1e-3)
env.check_errors()
resets = 0
for k in range(100):
    env.step(acts[k % 8])
    resets += int(env.done.sum())
out["resets_per_step"] = resets / 100.
print(json.dumps(out), flush=True)

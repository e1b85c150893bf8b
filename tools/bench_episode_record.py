"""Cost of the episode record (bcp_bind_episode_record, BatchedPlanEnv.enable_episode_record) on an MI355X.

  1. RandomMiniEnv pool, 65 536 envs, auto-reset (bench.py's workload): the step without a record, with a record
     (reason, return, final states), and the host workaround a caller needs without it (no auto-reset; torch gathers of
     the done envs' state; reset(mask)).
  2. RandomAisleTurnEnv, 65 536 envs, BatchedColoredEgoCostmap: the tick without and with final observations, and the
     host workaround (no auto-reset, gathers, the observation drawn a second time after reset(mask)).
Every figure is the mean of `steps` back-to-back ticks between two HIP events, after `warmup` ticks; the with / without
pairs are measured in alternating blocks, five each, and their medians reported.
Usage: python tools/bench_episode_record.py [steps] [warmup] [n_envs]     (prints one JSON line)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bc_gym_planning_env_amd import EnvParams, aisle_env, mini_env  # noqa: E402
from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
out = {"n_envs": n, "steps": steps, "warmup": warmup}


def timed(fn, acts):
    for k in range(warmup):
        fn(acts[k % len(acts)])
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(steps):
        fn(acts[k % len(acts)])
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def actions(env, scale):
    rng = np.random.RandomState(0)
    a = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(8)])).cuda()
    a[:, :, 0] *= scale
    return a


def workaround(env, obs=None):
    """no auto-reset: what a caller gathers from the done envs before it resets them (and re-draws the observation)"""
    def tick(a):
        o, _r, d, _i = env.step(a)
        mask = d.bool()
        s = env.state
        keep = (s.robot[:, mask], s.min_spat_dist_so_far[mask], s.target_idx[mask], s.current_iter[mask],
                s.robot_collided[mask])
        if obs is not None:
            first = obs.observation()
            keep = keep + tuple(v[mask] for v in first.values())
        env.reset(mask=d)
        if obs is not None:
            obs.observation()
        return keep
    return tick


# 1. mini pool (bench.py's RandomMiniEnv workload): unbound and bound blocks alternate, medians of `rounds`
rounds = 5
params = mini_env.default_random_mini_env_params()
pool = mini_env.sample_pool_device(params, list(range(1024)), 8, 0)
env = mini_env.BatchedRandomMiniEnv(n, params, pool=pool, auto_reset=True, seed=3)
acts = actions(env, 1.0)
unbound, bound = [], []
for _ in range(rounds):
    unbound.append(timed(env.step, acts))
    env.enable_episode_record()
    bound.append(timed(env.step, acts))
    out["mini_ends_last_step"] = int(env.episode_ends.count[0])
    env.check_errors()
    env.disable_episode_record()
out["mini_step_ms"], out["mini_step_record_ms"] = float(np.median(unbound)), float(np.median(bound))
out["mini_step_ms_all"], out["mini_step_record_ms_all"] = unbound, bound
del env
env = mini_env.BatchedRandomMiniEnv(n, params, pool=pool, auto_reset=False, seed=3)
out["mini_workaround_ms"] = timed(workaround(env), acts)
del env, pool

# 2. aisle turns + coloured egocentric observation, without and with final observations, alternating
ep = EnvParams()
apool = aisle_env.sample_aisle_pool_device(ep, list(range(1024)), 4, keep_on_device=True)
env = aisle_env.BatchedRandomAisleTurnEnv(n, ep, pool=apool, episodes=4, auto_reset=True, seed=3)
acts = actions(env, 3.0)
wrap = BatchedColoredEgoCostmap(env)
wrap_f = BatchedColoredEgoCostmap(env, final_observation=True)
env.disable_episode_record()
plain, final = [], []
for _ in range(rounds):
    plain.append(timed(wrap.step, acts))
    env.enable_episode_record()
    final.append(timed(wrap_f.step, acts))
    out["aisle_ends_last_step"] = int(env.episode_ends.count[0])
    env.check_errors()
    env.disable_episode_record()
out["aisle_tick_ms"], out["aisle_tick_final_obs_ms"] = float(np.median(plain)), float(np.median(final))
out["aisle_tick_ms_all"], out["aisle_tick_final_obs_ms_all"] = plain, final
del env, wrap, wrap_f
env = aisle_env.BatchedRandomAisleTurnEnv(n, ep, pool=apool, episodes=4, auto_reset=False, seed=3)
out["aisle_workaround_ms"] = timed(workaround(env, BatchedColoredEgoCostmap(env)), acts)
out["mini_record_ratio"] = out["mini_step_record_ms"] / out["mini_step_ms"]
out["aisle_final_obs_ratio"] = out["aisle_tick_final_obs_ms"] / out["aisle_tick_ms"]
print(json.dumps(out), flush=True)

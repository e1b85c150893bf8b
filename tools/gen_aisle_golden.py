#!/usr/bin/env python
"""Generate tests/golden/g14_aisle_worlds.npz from the GENUINE reference (RandomAisleTurnEnv,
envs/synth_turn_env.py:219-332), imported through oracle/ref_harness.py.  Run from the repo root where the reference
is available:  python tools/gen_aisle_golden.py

Contents (data only):
  seeds [S]; per seed s and world k (world 0 = drawn by the constructor, world k = by the k-th reset()):
    turn_params [S, K, 8]  main/turn corridor length, angle, main/turn width, flip_oy, flip_ox, rot_theta
    origin [S, K, 2], shape [S, K, 2] (rows, cols), coarse_path [S, K, 4, 3]
    lethal: np.packbits(costmap == 254, axis=1) of every map, flattened and concatenated; lethal_offset [S*K + 1]
    path: refined paths concatenated, path_offset [S*K + 1]; init [S, K, 2] = (min_spat_dist_so_far, target_idx)
  ColoredEgoCostmapRandomAisleTurnEnv trajectories t = 0 .. T-1: seed(s), reset(), sampled actions (x 2.5 speed) and
  the noise slots; every done is followed by reset() (onto the chain's next world) and recorded as reset_* rows.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_harness as H  # noqa: E402

SEEDS = list(range(12)) + [1000, 65535, 2 ** 31 - 1]
WORLDS = 4
TRAJ = [(3, 78, 6, 400), (7, 79, 7, 400), (11, 80, 8, 400)]   # (seed, action seed, noise seed, max steps)


def _turn_vec(tp):
    return np.array([tp.main_corridor_length, tp.turn_corridor_length, tp.turn_corridor_angle, tp.main_corridor_width,
                     tp.turn_corridor_width, float(tp.flip_arnd_oy), float(tp.flip_arnd_ox), tp.rot_theta],
                    dtype=np.float64)


def gen_worlds():
    from bc_gym_planning_env.envs.synth_turn_env import RandomAisleTurnEnv, path_and_costmap_from_config
    turn, origin, shape, coarse, init = [], [], [], [], []
    lethal, paths = [], []
    for s in SEEDS:
        env = RandomAisleTurnEnv(seed=s)
        row = [[], [], [], [], []]
        for k in range(WORLDS):
            if k:
                env.reset()
            plan = env._env
            st = plan.get_state()
            cm = st.costmap
            row[0].append(_turn_vec(plan._config.turn_params))
            row[1].append(np.array(cm.get_origin(), dtype=np.float64))
            row[2].append(np.array(cm.get_data().shape, dtype=np.int32))
            row[3].append(np.array(path_and_costmap_from_config(plan._config)[0], dtype=np.float64))
            rps = st.reward_provider_state
            row[4].append(np.array([rps.min_spat_dist_so_far, rps.target_idx], dtype=np.float64))
            lethal.append(np.packbits(cm.get_data() == 254, axis=1).ravel())
            paths.append(np.array(rps.path, dtype=np.float64))
        for lst, r in zip((turn, origin, shape, coarse, init), row):
            lst.append(np.stack(r))
    loff = np.concatenate([[0], np.cumsum([len(x) for x in lethal])]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return dict(seeds=np.array(SEEDS, dtype=np.int64), turn_params=np.stack(turn), origin=np.stack(origin),
                shape=np.stack(shape), coarse_path=np.stack(coarse), init=np.stack(init),
                lethal=np.concatenate(lethal), lethal_offset=loff, path=np.concatenate(paths), path_offset=poff,
                resolution=np.float64(0.03))


def gen_trajectories():
    from bc_gym_planning_env.envs.synth_turn_env import ColoredEgoCostmapRandomAisleTurnEnv
    from bc_gym_planning_env.envs.base import spaces
    from bc_gym_planning_env.robot_models import differential_drive as dd
    out = {}
    for j, (seed, aseed, nseed, steps) in enumerate(TRAJ):
        env = ColoredEgoCostmapRandomAisleTurnEnv()
        env.seed(seed)
        env.reset()
        spaces.SPACE_LOCAL_RANDOM_STATE.seed(aseed)
        rec = {k: [] for k in ("actions", "z", "states", "reward", "done", "collided", "images", "goal", "world",
                               "reset_images", "reset_goal", "reset_states")}
        world, ends = 0, 0
        with GG.SlotTap(dd, nseed) as tap:
            for t in range(steps):
                a = env.action_space.sample()
                a = type(a)(command=np.array([a.command[0] * 2.5, a.command[1]]))
                obs, r, done, _ = env.step(a)
                plan = env._env
                rec["actions"].append(np.asarray(a.command, dtype=np.float64))
                rec["z"].append(tap.take())
                rec["states"].append(GG.tri_state_vec(plan._state.robot_state))
                rec["reward"].append(r)
                rec["done"].append(int(done))
                rec["collided"].append(int(plan._state.robot_collided))
                rec["world"].append(world)
                img = obs['environment'][:, :, 0]
                rec["images"].append(np.packbits(img == 254, axis=1))
                rec["goal"].append(obs['goal'][:, 0].copy())
                if done:
                    obs = env.reset()
                    world += 1
                    ends += 1
                    rec["reset_images"].append(np.packbits(obs['environment'][:, :, 0] == 254, axis=1))
                    rec["reset_goal"].append(obs['goal'][:, 0].copy())
                    rec["reset_states"].append(GG.tri_state_vec(env._env._state.robot_state))
                    if ends == 2:
                        break
        assert ends >= 1, "trajectory %d never ended an episode" % j
        print("trajectory %d: seed %d, %d steps, %d episode ends" % (j, seed, len(rec["done"]), ends))
        for k, v in rec.items():
            out["t%d_%s" % (j, k)] = np.array(v)
        out["t%d_seed" % j] = np.int64(seed)
        out["t%d_image_cols" % j] = np.int64(img.shape[1])
    out["n_traj"] = np.int64(len(TRAJ))
    return out


def main():
    GG.O.build()
    H.load()
    data = gen_worlds()
    data.update(gen_trajectories())
    GG.save("g14_aisle_worlds.npz", **data)


if __name__ == "__main__":
    main()

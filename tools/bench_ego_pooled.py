"""The pooled egocentric observation (bcp_egocentric_costmaps_pooled) beside the full-resolution call of the same process:
    config 1  BatchedRandomMiniEnv, 65 536 envs, 133 x 117 window (the metric config's observation)
    config 2  the 133 x 133 coloured window on the 350 x 512 AisleTurn map of the g12 fixture, 65 536 replicas
Per config: the full call and pool = 2, 4, 8, each timed with HIP events over a region of at least 50 ms, three rounds that
alternate the four variants (the spread between rounds is reported beside the median).  Only the image call is timed
(wrap._refresh_images), not the goal vector.  One JSON document: times, routes taken, bytes written.

    python tools/bench_ego_pooled.py [--envs 65536] [--out profiles/ego_pooled_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench   # noqa: E402  (steady_state: random episode phases + one time-out of pre-roll, as bench.py's legs)
from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams, mini_env   # noqa: E402
from bc_gym_planning_env_amd.egocentric import BatchedColoredEgoCostmap, BatchedEgocentricCostmap   # noqa: E402

POOLS = (2, 4, 8)
MIN_REGION_MS = 50.0
ROUNDS = 3


def timed(wrap, stream):
    """ms per image call over a region of at least MIN_REGION_MS (sized from a short probe of the same call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def region(reps):
        e0.record(stream)
        for _ in range(reps):
            wrap._refresh_images()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    probe = region(20) / 20
    reps = max(20, int(np.ceil(1.2 * MIN_REGION_MS / max(probe, 1e-4))))
    total = region(reps)
    assert total >= MIN_REGION_MS, (total, reps)
    return total / reps, reps, total


def measure(env, wrapper, what):
    stream = torch.cuda.current_stream(env.device)
    wraps = [("full", wrapper(env))] + [("pool%d" % p, wrapper(env, pool=p)) for p in POOLS]
    routes = {}
    for name, w in wraps:        # warm-up: code objects, the counting pass and the lists of the sparse route
        for _ in range(3):
            w._refresh_images()
        routes[name] = w.route()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in wraps}
    regions = {}
    for _ in range(ROUNDS):
        for name, w in wraps:
            t, reps, total = timed(w, stream)
            ms[name].append(t)
            regions[name] = {"calls": reps, "ms": total}
    # the pooled images of the timed state agree with the block maxima of the full image of the same state (a sanity
    # check of the run, not the parity test: tests/test_gpu_ego_pooled.py checks against the reference)
    full = wraps[0][1].images[..., 0]
    h, w_ = full.shape[1:]
    agree = {}
    for (name, w), p in zip(wraps[1:], POOLS):
        pad = torch.zeros((full.shape[0], -(-h // p) * p, -(-w_ // p) * p), dtype=torch.uint8, device=full.device)
        pad[:, :h, :w_] = full
        want = pad.view(full.shape[0], pad.shape[1] // p, p, pad.shape[2] // p, p).amax(dim=(2, 4))
        agree[name] = bool((want == w.images[..., 0]).all())
    out = {"what": what, "envs": env.n_envs, "full_image_shape": list(wraps[0][1].image_shape), "variants": {}}
    full_ms = float(np.median(ms["full"]))
    for name, w in wraps:
        med = float(np.median(ms[name]))
        out["variants"][name] = {
            "pool": w.pool, "image_shape": list(w.image_shape), "kernel": routes[name]["kernel"],
            "non_zero_cells_of_the_map": routes[name]["max_cells"], "sparse_limit": routes[name]["limit"],
            "ms_per_call_median": med, "ms_per_call_rounds": [float(v) for v in ms[name]], "timed_region": regions[name],
            "bytes_written_per_call": int(w.images.numel()), "full_over_this": full_ms / med}
        if name in agree:
            out["variants"][name]["equals_block_max_of_full_image"] = agree[name]
    out["lit_pixel_fraction_of_full_image"] = float((full != 0).float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ego_pooled_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ego_pooled.py needs a GPU: nothing is measured without one")
    n = args.envs
    doc = {"device": torch.cuda.get_device_name(0), "min_timed_region_ms": MIN_REGION_MS, "rounds": ROUNDS, "configs": {}}
    rng = np.random.RandomState(0)

    worlds = mini_env.sample_pool_device(None, list(range(4096)), 4)
    env = mini_env.BatchedRandomMiniEnv(n, pool=worlds, auto_reset=True, seed=3)
    acts = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(8)])).to(env.device)
    bench.steady_state(env, acts, rng)
    doc["configs"]["random_mini_env_133x117"] = measure(
        env, BatchedEgocentricCostmap, "EgocentricCostmap(RandomMiniEnv) images, %d envs over %d pre-sampled worlds" % (n, len(worlds)))
    env.close()
    del env
    torch.cuda.empty_cache()

    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_colored_ego.npz"))
    res = float(g["resolution"])
    env = BatchedPlanEnv(CostMap2D(g["costmap"], res, g["origin"]), g["path"], EnvParams(resolution=res, refine_path=False),
                         n_envs=n, auto_reset=True, seed=17)
    acts = torch.from_numpy(np.stack([env.action_space.sample_batch(n, rng) for _ in range(8)])).to(env.device)
    bench.steady_state(env, acts, rng)
    doc["configs"]["colored_ego_aisle_350x512_133x133"] = measure(
        env, BatchedColoredEgoCostmap, "ColoredEgoCostmapRandomAisleTurnEnv images, %d replicas of the 350 x 512 map" % n)
    env.close()

    c1 = doc["configs"]["random_mini_env_133x117"]["variants"]
    doc["pool8_not_slower_than_full_on_config_1"] = c1["pool8"]["ms_per_call_median"] <= c1["full"]["ms_per_call_median"]
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

"""Times bcp_inflate_costmaps on the three pool shapes the library is built for and prints one JSON line:

  mini_pool    4 096 x 183 x 183      a RandomMiniEnv pool sampled on the device
  aisle_pool   16 384 aisle entries   at their padded shape, with valid shapes
  c4_maps      65 536 x 256 x 256     in place, the four C4 aisle maps (valid 256 x 141) of bench.py's C4 leg

Beside each leg: bcp_set_costmaps for the same tensor (the clamped transform of the private-map bind: comparable passes
over the same maps; that entry point is untouched by the inflation work, so this build's figure is the parent's) and a plain
device copy of the same bytes (the memory floor).  HIP events around a region of at least 50 ms after a warm-up.

    python tools/bench_inflate.py [--legs mini_pool,aisle_pool,c4_maps] > profiles/inflate_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bc_gym_planning_env_amd import EnvParams, _lib, aisle_env, mini_env, robots  # noqa: E402
from bc_gym_planning_env_amd.api import INDUSTRIAL_TRICYCLE_V1  # noqa: E402

FACTOR = 3.0
RADIUS = robots.inscribed_radius(robots.get_footprint(INDUSTRIAL_TRICYCLE_V1))


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


def leg(L, name, maps, resolution, vr, vc, in_place):
    n, rows, cols = maps.shape
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = robots.make_bcp_params(EnvParams(resolution=resolution), INDUSTRIAL_TRICYCLE_V1, None)
    h = C.c_void_p()
    _lib.check(L.bcp_create(C.byref(p), n, 0, 0, C.byref(h)))
    out = maps if in_place else torch.empty_like(maps)
    origins = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    vrp, vcp = (vr.data_ptr(), vc.data_ptr()) if vr is not None else (None, None)

    def inflate():
        _lib.check(L.bcp_inflate_costmaps(h, maps.data_ptr(), n, rows, cols, vrp, vcp, resolution, RADIUS, FACTOR, out.data_ptr(),
                                          None, stream))

    def bind():
        _lib.check(L.bcp_set_costmaps(h, maps.data_ptr(), rows, cols, 0, vrp, vcp, origins.data_ptr(), 1, resolution, stream))

    # (the bind is timed first: in place, the maps it sees later would be inflated ones -- the same lethal cells, though)
    bind_ms, bind_reps = timed_ms(bind)
    inflate_ms, reps = timed_ms(inflate)
    spare = torch.empty_like(maps)
    copy_ms, _ = timed_ms(lambda: spare.copy_(maps))
    del spare
    lethal = int((out == 254).sum())
    inscribed = int((out == 253).sum())
    L.bcp_destroy(h)
    gb = maps.numel() / 1e9
    return {"shape": [n, rows, cols], "bytes": maps.numel(), "in_place": in_place, "valid_shapes": vr is not None,
            "inflate_ms": round(inflate_ms, 4), "reps": reps, "set_costmaps_ms": round(bind_ms, 4), "set_costmaps_reps": bind_reps,
            "copy_ms": round(copy_ms, 4), "inflate_over_set_costmaps": round(inflate_ms / bind_ms, 3),
            "inflate_over_copy": round(inflate_ms / copy_ms, 3), "read_plus_write_gbs": round(2 * gb / (inflate_ms * 1e-3), 1),
            "lethal_cells": lethal, "inscribed_cells": inscribed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="mini_pool,aisle_pool,c4_maps")
    args = ap.parse_args()
    L = _lib.load()
    out = {"tool": "tools/bench_inflate.py", "device": torch.cuda.get_device_name(0), "cost_scaling_factor": FACTOR,
           "inscribed_radius": RADIUS, "legs": {}}
    for name in args.legs.split(","):
        if name == "mini_pool":
            params = mini_env.default_random_mini_env_params()
            pool = mini_env.sample_pool_device(params, list(range(1024)), 4, 0, keep_on_device=True)
            out["legs"][name] = leg(L, name, pool.maps.contiguous(), pool.resolution, None, None, False)
        elif name == "aisle_pool":
            pool = aisle_env.sample_aisle_pool_device(EnvParams(), list(range(4096)), 4, 0, keep_on_device=True)
            out["legs"][name] = leg(L, name, pool.maps.contiguous(), pool.resolution, pool.valid_rows, pool.valid_cols, False)
        elif name == "c4_maps":
            names = ["g8_traj_aisle_c4_00.npz", "g8_traj_aisle_c4_10.npz", "g8_traj_aisle_c4_01.npz", "g8_traj_aisle_c4_11.npz"]
            g = [np.load(os.path.join(ROOT, "tests", "golden", f)) for f in names]
            four = np.zeros((4, 256, 256), dtype=np.uint8)
            for k, t in enumerate(g):
                four[k, :t["costmap"].shape[0], :t["costmap"].shape[1]] = t["costmap"]
            n = 65536
            maps = torch.from_numpy(four).cuda()[torch.arange(n, device="cuda") % 4].contiguous()
            vr = torch.full((n,), g[0]["costmap"].shape[0], dtype=torch.int32, device="cuda")
            vc = torch.full((n,), g[0]["costmap"].shape[1], dtype=torch.int32, device="cuda")
            out["legs"][name] = leg(L, name, maps, float(g[0]["resolution"]), vr, vc, True)
        else:
            raise SystemExit("unknown leg %r" % name)
        pool = None
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""One process of a parent / new alternation of bcp_goal_field (the rule of profiles/r08_plan_core.txt): the mini_pool leg of
tools/bench_goal_field.py (4 096 entries of 183 x 183) on the source tree given as argv[1] -- a checkout with its library
built, whose package and tool are the ones imported -- 15 regions of at least 50 ms each per clearance, median (min - max)
as one JSON line.

    python tools/bench_goal_field_ab.py <tree> <label>        # e.g. ../parent parent1, then . new1, ../parent parent2, . new2
"""
import importlib.util
import json
import os
import sys

import numpy as np

root = os.path.abspath(sys.argv[1])
label = sys.argv[2]
os.chdir(root)
sys.path.insert(0, root)
spec = importlib.util.spec_from_file_location("bench_goal_field", os.path.join(root, "tools", "bench_goal_field.py"))
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

import torch  # noqa: E402
from bc_gym_planning_env_amd import EnvParams, _lib, mini_env  # noqa: E402

assert os.path.dirname(os.path.abspath(_lib.LIB_PATH)).startswith(root), _lib.LIB_PATH
params = mini_env.RandomMiniEnvParams(env_params=EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2))
env = mini_env.BatchedRandomMiniEnv(4096, params, n_chains=1024, episodes=4, auto_reset=True, seed=1)
out = {"label": label, "lib": _lib.LIB_PATH}
for clearance in (0.0, tool.RADIUS):
    fields = env.goal_field(clearance)
    seeds, data, vr, vc = fields._keep
    f, info = fields.field, fields.info
    n, rows, cols = f.shape
    stream = env._stream()

    def build():
        _lib.check(env._lib.bcp_goal_field(env._h, data.data_ptr(), n, rows, cols, 0, None, None, seeds.data_ptr(), int(seeds.shape[1]),
                                           fields.clearance_d2, 0, f.data_ptr(), info.data_ptr(), stream))

    samples = [tool.timed_ms(build)[0] for _ in range(15)]
    out["d2_%d" % fields.clearance_d2] = {"entries": int(n), "median_ms": round(float(np.median(samples)), 4),
                                          "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}
    torch.cuda.synchronize()
print(json.dumps(out))

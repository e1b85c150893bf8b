"""bench.py's plain run: --steps is the number of timed steps, the line carries the headline figure and nothing measured
beside it, and --dump-outputs writes the last timed step's outputs -- the same files, bit for bit, run after run."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


def _run(launcher, out_dir):
    r = launcher.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                      "--envs-per-gpu", str(N), "--dump-outputs", out_dir], timeout=600, cwd=ROOT)
    assert r["rc"] == 0, r["err"][-3000:]
    lines = [x for x in r["out"].splitlines() if x.startswith("{")]
    assert len(lines) == 1, r["out"][-2000:]
    return json.loads(lines[0])


def test_plain_run_times_steps_and_dumps_the_same_outputs(launcher, tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    lines = [_run(launcher, d) for d in dirs]
    for line in lines:
        tr = line["timed_region"]
        assert line["steps"] == 7 and line["reps"] == 1 and tr["steps_timed"] == 7 and not line["full"]
        assert line["ms_per_step"] == pytest.approx(tr["wall_ms"] / 7, rel=1e-9)
        assert line["value"] == pytest.approx(N * 7 / (tr["wall_ms"] * 1e-3), rel=1e-9)
        assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert not set(line) & {"cpu_baseline", "aux", "parked_pose_fraction", "gather_every_8"}
    shapes = {"pose": (3, N), "robot_state": (4, N), "target_idx": (N,), "current_iter": (N,), "reward": (N,), "done": (N,)}
    for name, shape in shapes.items():
        a, b = [np.load(os.path.join(d, name + ".npy")) for d in dirs]
        assert a.shape == shape and a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all() and np.array_equal(a, b), name
    done = np.load(os.path.join(dirs[0], "done.npy"))
    assert set(np.unique(done)) <= {0.0, 1.0}
    assert sorted(os.listdir(dirs[0])) == sorted(k + ".npy" for k in shapes)

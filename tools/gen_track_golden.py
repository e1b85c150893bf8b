"""Makes tests/golden/g13_dd2tri.npz: inputs and outputs of the reference's own diff_drive_control_to_tricycle
(robot_models/tricycle_model.py:191-231), the function bcp_track's law restates (csrc/bcp_track_law.h).  Runs only where the
reference is present (oracle/ref_harness.py); no test imports it.  From the repository root:  python tools/gen_track_golden.py

The file holds data only:
  known_in [6, 5], known_out [6, 2], known_expected [6, 2]: the six calls of robot_models/test_tricycle_model.py
      (v, w, wheel_angle, max_front_wheel_angle, front_wheel_from_axis), what the function returns for them and the answers
      that test states to seven decimals;
  v, w, wheel_angle [n]; out [n, 2]: random calls with the stock tricycle constants `max_front_wheel_angle` and
      `front_wheel_from_axis` (scalars), among them v = 0, |v| on both sides of 1e-6, w = 0 and wheel angles at the clip.
Inputs within 1e-9 of a branch boundary (|v| = 1e-6; |diff_angles| = pi/8 where that rule is looked at) are left out; the
count is printed and may not pass 1 % of the 2 048 drawn."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402

N_DRAWN, SEED, MARGIN = 2048, 13, 1e-9


def main():
    H.load()
    from bc_gym_planning_env.robot_models.tricycle_model import diff_drive_control_to_tricycle
    from bc_gym_planning_env.robot_models.robot_dimensions_examples import get_dimensions_example
    from bc_gym_planning_env.robot_models.standard_robot_names_examples import StandardRobotExamples
    from bc_gym_planning_env.utilities.coordinate_transformations import diff_angles
    dims = get_dimensions_example(StandardRobotExamples.INDUSTRIAL_TRICYCLE_V1)
    max_wa, dist = float(dims.max_front_wheel_angle()), float(dims.front_wheel_from_axis())

    h = np.pi / 2
    known_in = np.array([[1.0, 0.0, 0.0, h, 1.0], [1.0, 0.0, h, h, 1.0], [1.0, 0.0, -np.pi / 4, h, 1.0],
                         [0.0, 1.0, -np.pi / 4, h, 1.0], [0.0, 1.0, h - 0.1, h, 1.0], [1.0, 1.0, h - 0.1, h, 1.0]])
    known_expected = np.array([[1.0, 0.0], [0.0, 0.0], [0.7071068, 0.0], [0.0, h], [0.9950042, h], [1.0948376, np.pi / 4]])
    known_out = np.array([diff_drive_control_to_tricycle(*row) for row in known_in], dtype=np.float64)
    np.testing.assert_almost_equal(known_out, known_expected)

    rng = np.random.RandomState(SEED)
    v = rng.uniform(0.0, 1.2, N_DRAWN)
    w = rng.uniform(-2.0, 2.0, N_DRAWN)
    wa = rng.uniform(-max_wa, max_wa, N_DRAWN)
    v[:64] = 0.0
    v[64:128] = 1e-6 * (1.0 + rng.choice([-1.0, 1.0], 64) * rng.uniform(0.01, 0.5, 64)) * rng.choice([-1.0, 1.0], 64)
    v[128:192] = -rng.uniform(0.0, 0.5, 64)
    w[32:96] = 0.0
    w[192:256] = 0.0
    wa[16:48] = max_wa
    wa[96:112] = -max_wa
    wa[256:288] = rng.choice([-max_wa, max_wa], 32)
    keep = np.abs(np.abs(v) - 1e-6) >= MARGIN
    out = np.zeros((N_DRAWN, 2))
    for j in range(N_DRAWN):
        out[j] = diff_drive_control_to_tricycle(v[j], w[j], wa[j], max_wa, dist)
        if abs(v[j]) < 1e-6 and abs(abs(float(diff_angles(wa[j], out[j, 1]))) - np.pi / 8) < MARGIN:
            keep[j] = False
    left_out = int((~keep).sum())
    print("%d of %d inputs left out (within %g of a branch boundary)" % (left_out, N_DRAWN, MARGIN))
    assert left_out <= N_DRAWN // 100
    path = os.path.join(ROOT, "tests", "golden", "g13_dd2tri.npz")
    np.savez_compressed(path, known_in=known_in, known_out=known_out, known_expected=known_expected, v=v[keep], w=w[keep],
                        wheel_angle=wa[keep], out=out[keep], max_front_wheel_angle=max_wa, front_wheel_from_axis=dist)
    print("wrote %s: %d rows, %d bytes" % (path, int(keep.sum()), os.path.getsize(path)))


if __name__ == "__main__":
    main()

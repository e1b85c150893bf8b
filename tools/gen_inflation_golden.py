"""Writes tests/golden/g18_inflation.npz: inputs and expected outputs of the GENUINE reference inflate_costmap
(utilities/costmap_inflation.py:73-92) and inscribed_radius (utilities/path_tools.py:519-528).

Runs only where the reference is present (oracle.ref_harness).  The harness's cv2 stand-in has no distanceTransform, so this
tool gives it one: the exact transform by brute force, sqrt of the integer minimum over the zero pixels, as float32 -- what
cv2.distanceTransform(DIST_L2, DIST_MASK_PRECISE) returns.  Everything else that runs is the reference's own code.

    python tools/gen_inflation_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def distance_transform(img, *_a, **_k):
    """float32 [rows, cols]: distance of every pixel to the nearest zero pixel of img."""
    img = np.asarray(img)
    zr, zc = np.nonzero(img == 0)
    rows, cols = img.shape
    if len(zr) == 0:
        return np.full(img.shape, np.inf, dtype=np.float32)
    rr, cc = [a.ravel().astype(np.int64) for a in np.indices((rows, cols))]
    d2 = np.full(rows * cols, np.iinfo(np.int64).max, dtype=np.int64)
    for k in range(0, len(zr), 64):
        dr = rr[None, :] - zr[k:k + 64, None]
        dc = cc[None, :] - zc[k:k + 64, None]
        d2 = np.minimum(d2, (dr * dr + dc * dc).min(axis=0))
    return np.sqrt(d2.astype(np.float64)).astype(np.float32).reshape(rows, cols)


def main():
    from oracle import ref_harness
    ref_harness.load()
    sys.modules["cv2"].distanceTransform = distance_transform
    from bc_gym_planning_env.robot_models.robot_dimensions_examples import get_dimensions_example
    from bc_gym_planning_env.utilities.costmap_2d import CostMap2D
    from bc_gym_planning_env.utilities.costmap_inflation import inflate_costmap
    from bc_gym_planning_env.utilities.map_drawing_utils import add_wall_to_static_map
    from bc_gym_planning_env.utilities.path_tools import inscribed_radius

    rect = np.array([[-0.77, -0.385], [-0.77, 0.385], [0.67, 0.385], [0.67, -0.385]])
    footprints = {"rect": rect,
                  "tricycle": get_dimensions_example('industrial_tricycle_v1').footprint(),
                  "diffdrive": get_dimensions_example('industrial_diffdrive_v1').footprint()}
    out, names = {}, []

    def case(name, data, resolution, footprint, factor):
        costmap = CostMap2D(np.array(data, dtype=np.uint8), float(resolution), np.zeros(2))
        expected = inflate_costmap(costmap, factor, footprints[footprint]).get_data()
        assert expected.dtype == np.uint8
        names.append(name)
        out[name + "/data"] = np.array(data, dtype=np.uint8)
        out[name + "/resolution"] = np.float64(resolution)
        out[name + "/inscribed_radius"] = np.float64(inscribed_radius(footprints[footprint]))
        out[name + "/cost_scaling_factor"] = np.float64(factor)
        out[name + "/expected"] = expected

    known = CostMap2D.create_empty((1, 1), 0.1, (0, 0))
    add_wall_to_static_map(known, (0, 0), (1, 1))
    case("known_answer", known.get_data(), 0.1, "rect", 1.)
    assert int((out["known_answer/expected"] == 253).sum()) == 70

    def fixture(name):
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        return g["costmap"], float(g["resolution"])

    for m in ("g8_traj_mini_00", "g8_traj_mini_05"):
        data, res = fixture(m)
        for fp in ("tricycle", "diffdrive"):
            for factor in (1., 3.):
                case("%s_%s_f%d" % (m[8:], fp, factor), data, res, fp, factor)
    data, res = fixture("g8dd_traj_mini64_00")
    case("mini64_00_diffdrive_f3", data, res, "diffdrive", 3.)
    data, res = fixture("g8_traj_aisle_c4_01")
    case("aisle_c4_01_tricycle_f3", data, res, "tricycle", 3.)
    data, res = fixture("g12_colored_ego")
    case("colored_350x512_tricycle_f3", data, res, "tricycle", 3.)
    data, res = fixture("g8_traj_mini_00")
    odd = data.copy()
    free = np.argwhere(odd == 0)
    for value, k in ((255, len(free) // 4), (253, len(free) // 2), (1, 3 * len(free) // 4)):
        odd[tuple(free[k])] = value
    case("mini_00_odd_values_tricycle_f3", odd, res, "tricycle", 3.)

    for fp in footprints:
        out["inscribed_radius/" + fp] = np.float64(inscribed_radius(footprints[fp]))
    out["names"] = np.array(names)
    path = os.path.join(GOLDEN, "g18_inflation.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes (numpy %s)" % (path, len(names), os.path.getsize(path), np.__version__))


if __name__ == "__main__":
    main()

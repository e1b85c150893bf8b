"""Host side of the geometry binding (bc_gym_planning_env_amd/geometry.py): costmaps padded to one shape, paths refined
and padded to one length, the chain layout of the pool envs; and what the package promises about its imports (no GPU
needed)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from bc_gym_planning_env_amd import CostMap2D, geometry, host_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps():
    rng = np.random.RandomState(0)
    a = CostMap2D(rng.randint(1, 255, (3, 5)).astype(np.uint8), 0.05, np.array([-1.0, 2.0]))
    b = CostMap2D(rng.randint(1, 255, (4, 2)).astype(np.uint8), 0.05, np.array([0.5, -0.25]))
    return a, b


def test_stack_costmaps_pads_to_the_largest_shape():
    a, b = _maps()
    data, shapes, origins, res = geometry.stack_costmaps([a, b])
    assert data.shape == (2, 4, 5) and data.dtype == np.uint8
    assert shapes.dtype == np.int32 and shapes.tolist() == [[3, 5], [4, 2]]
    assert origins.dtype == np.float64 and origins.tolist() == [[-1.0, 2.0], [0.5, -0.25]]
    assert res == 0.05
    for k, c in enumerate((a, b)):
        r, w = c.get_data().shape
        np.testing.assert_array_equal(data[k, :r, :w], c.get_data())
        outside = data[k].copy()
        outside[:r, :w] = 0
        assert not outside.any()   # (the maps themselves hold no zero: every zero is padding)
        assert c.get_data().all()


def test_stack_costmaps_min_shape():
    a, b = _maps()
    data, shapes, _, _ = geometry.stack_costmaps([a, b], min_shape=(8, 4))
    assert data.shape == (2, 8, 5) and shapes.tolist() == [[3, 5], [4, 2]]
    np.testing.assert_array_equal(data[:, :4], geometry.stack_costmaps([a, b])[0])
    assert not data[:, 4:].any()


def test_stack_costmaps_refuses_mixed_resolutions():
    a, _ = _maps()
    other = CostMap2D(np.zeros((3, 5), dtype=np.uint8), 0.1, np.zeros(2))
    with pytest.raises(ValueError, match="all costmaps must share one resolution"):
        geometry.stack_costmaps([a, other])


def _paths():
    short = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    long = np.array([[0.0, 0.0, 0.5], [0.3, 0.1, 0.5], [0.9, 0.2, 0.4], [1.0, 0.7, 0.3], [1.6, 1.0, 0.2]])
    return short, long


def test_stack_paths_identity():
    short, long = _paths()
    points, lens, paths = geometry.stack_paths([short, long], lambda p: p)
    assert points.shape == (2, 5, 3) and points.dtype == np.float64
    assert lens.dtype == np.int32 and lens.tolist() == [2, 5]
    np.testing.assert_array_equal(points[0, :2], short)
    assert not points[0, 2:].any()
    np.testing.assert_array_equal(points[1], long)
    np.testing.assert_array_equal(paths[0], short)
    np.testing.assert_array_equal(paths[1], long)


def test_stack_paths_refines_every_path():
    delta = 0.05
    points, lens, paths = geometry.stack_paths(_paths(), functools.partial(host_init.refine_path, delta=delta))
    for k, p in enumerate(_paths()):
        want = host_init.refine_path(p, delta)
        np.testing.assert_array_equal(paths[k], want)
        assert lens[k] == len(want) > len(p)
        np.testing.assert_array_equal(points[k, :lens[k]], want)
        assert not points[k, lens[k]:].any()
    assert points.shape[1] == lens.max()


def test_chain_layout():
    assert geometry.chain_layout(7, 3, 2).tolist() == [0, 2, 4, 1, 3, 5, 0]


def test_unknown_sampler_is_a_value_error():
    with pytest.raises(ValueError, match="sampler must be"):
        geometry.pool_or_sample(None, {"device": None, "device_resident": None, "host": None}, "gpu", None, None, 4)
    pool = object()
    assert geometry.pool_or_sample(pool, {}, "anything", None, None, 4) is pool
    seen = []
    geometry.pool_or_sample(None, {"host": seen.append}, "host", None, 3, 100)
    geometry.pool_or_sample(None, {"host": seen.append}, "host", None, None, 5000)
    geometry.pool_or_sample(None, {"host": seen.append}, "host", (7, 9), 3, 100)
    assert seen[0] == [0, 1, 2] and seen[1] == list(range(1024)) and seen[2] == [7, 9]


def test_importing_the_package_does_not_import_torch():
    code = "import sys; import bc_gym_planning_env_amd; assert 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_batched_env_still_exports_every_name():
    pytest.importorskip("torch")
    from bc_gym_planning_env_amd import batched_env
    for name in ("DeviceGeometryPool", "BatchedState", "BatchedObservation", "EnvView", "EpisodeEnds", "Lookahead", "Mppi",
                 "beam_table_cached", "SCAN_CACHE_ENTRIES", "BatchedPlanEnv"):
        assert hasattr(batched_env, name), name

"""Host side of the geometry binding (bc_gym_planning_env_amd/geometry.py): costmaps padded to one shape, paths refined
and padded to one length, the host copies of what is bound (HostEntries), the chain layout of the pool envs; and what the
package promises about its imports (no GPU needed)."""
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


class _LazySequence(object):
    """what a DeviceGeometryPool hands out: nothing but __len__ and __getitem__"""

    def __init__(self, items):
        self._held = items

    def __len__(self):
        return len(self._held)

    def __getitem__(self, k):
        return self._held[k]


def _items(n):
    return [object() for _ in range(n)]


def _host_entries_modes():
    """(name, HostEntries, its items, the item index of every env, the item index of every bound entry, the entry of every
    env to hand to of_env) for 3 envs"""
    one, three, two, pool, lazy = _items(1), _items(3), _items(2), _items(3), _items(3)
    return [("shared", geometry.HostEntries.shared(one[0]), one, [0, 0, 0], [0], [None] * 3),
            ("per env", geometry.HostEntries.per_env(three), three, [0, 1, 2], [0, 1, 2], [None] * 3),
            ("templates", geometry.HostEntries.templates(two, np.array([1, 0, 1])), two, [1, 0, 1], [1, 0, 1], [None] * 3),
            ("pool", geometry.HostEntries.pool_entries(pool), pool, [2, 0, 2], [0, 1, 2], [2, 0, 2]),
            ("lazy pool", geometry.HostEntries.pool_entries(_LazySequence(lazy)), lazy, [2, 0, 2], [0, 1, 2], [2, 0, 2])]


@pytest.mark.parametrize("mode", range(5))
def test_host_entries_of_every_mode(mode):
    name, host, items, of_env, of_entry, entries = _host_entries_modes()[mode]
    assert host.n_entries == len(of_entry), name
    for i in range(3):
        assert host.of_env(i, entries[i]) is items[of_env[i]], (name, i)
    for k, item in enumerate(of_entry):
        assert host.of_entry(k) is items[item], (name, k)
    index = host.index()
    assert isinstance(index, np.ndarray) and index.dtype == np.int64 and index.tolist() == of_entry, name
    assert len(host.items) == len(items) and all(host.items[k] is items[k] for k in range(len(items)))


def test_host_entries_replace_gives_every_env_of_a_template_its_own_item():
    two = _items(2)
    host = geometry.HostEntries.templates(two, np.array([1, 0, 1]))
    assert host.of_env(0) is host.of_env(2) is two[1]
    for _ in range(2):   # (a second replace behaves like the first)
        new = _items(3)
        host.replace(new)
        assert host.items is new and host.n_entries == 3 and host.index().tolist() == [0, 1, 2]
        for i in range(3):
            assert host.of_env(i) is new[i] and host.of_entry(i) is new[i]
        assert host.of_env(0) is not host.of_env(2)
        with pytest.raises(ValueError):
            host.replace(_items(2))
        assert host.items is new   # (a refused replace leaves everything as it was)


def test_host_entries_replace_keeps_a_shared_item_shared():
    host = geometry.HostEntries.shared(object())
    new = _items(1)
    host.replace(new)
    assert host.n_entries == 1 and all(host.of_env(i) is new[0] for i in range(3)) and host.of_entry(0) is new[0]
    with pytest.raises(ValueError):
        host.replace(_items(3))


def test_host_entries_replace_stored_keeps_the_rule():
    """an edit that treats equal entries equally (inflation): one new item per stored item, templates stay templates"""
    host = geometry.HostEntries.templates(_items(2), np.array([1, 0, 1]))
    new = _items(2)
    host.replace_stored(new)
    assert [host.of_env(i) for i in range(3)] == [new[1], new[0], new[1]] and host.index().tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        host.replace_stored(_items(3))


def test_importing_the_package_does_not_import_torch():
    code = "import sys; import bc_gym_planning_env_amd; assert 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_batched_env_still_exports_every_name():
    pytest.importorskip("torch")
    from bc_gym_planning_env_amd import batched_env
    for name in ("DeviceGeometryPool", "BatchedState", "BatchedObservation", "EnvView", "EpisodeEnds", "Lookahead", "Mppi",
                 "beam_table_cached", "SCAN_CACHE_ENTRIES", "BatchedPlanEnv"):
        assert hasattr(batched_env, name), name

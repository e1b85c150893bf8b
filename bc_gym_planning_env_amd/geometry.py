"""Host side of the geometry BatchedPlanEnv binds: costmaps padded to one shape, paths refined and padded to one
length, the host copies of what is bound (HostEntries), the env -> pool-entry layout of the pool envs, and the pool that
already lives on the GPU.  numpy only; torch is imported where a device tensor is made."""
import numpy as np

from .api import CostMap2D


def stack_costmaps(costmaps, min_shape=(0, 0)):
    """T CostMap2D -> (data uint8 [T, rows, cols], shapes int32 [T, 2], origins float64 [T, 2], resolution): rows x cols
    is the largest shape among them, at least min_shape; every map sits in the top left corner of its zero-padded slice."""
    costmaps = list(costmaps)
    res = float(costmaps[0].get_resolution())
    if any(float(c.get_resolution()) != res for c in costmaps):
        raise ValueError("all costmaps must share one resolution")
    shapes = np.array([c.get_data().shape for c in costmaps], dtype=np.int32).reshape(len(costmaps), 2)
    rows, cols = max(int(min_shape[0]), int(shapes[:, 0].max())), max(int(min_shape[1]), int(shapes[:, 1].max()))
    data = np.zeros((len(costmaps), rows, cols), dtype=np.uint8)
    origins = np.zeros((len(costmaps), 2), dtype=np.float64)
    for t, c in enumerate(costmaps):
        data[t, :shapes[t, 0], :shapes[t, 1]] = c.get_data()
        origins[t] = c.get_origin()
    return data, shapes, origins, res


def stack_paths(paths, refine):
    """T paths [m_t, 3] -> (points float64 [T, max_len, 3], lens int32 [T], the refined paths): every path goes through
    `refine` (host_init.refine_path bound to a path_delta, or the identity) and is followed by zero rows."""
    refined = [np.ascontiguousarray(refine(np.asarray(p)), dtype=np.float64) for p in paths]
    assert all(p.ndim == 2 and p.shape[1] == 3 for p in refined)
    lens = np.array([len(p) for p in refined], dtype=np.int32)
    points = np.zeros((len(refined), int(lens.max()), 3), dtype=np.float64)
    for t, p in enumerate(refined):
        points[t, :len(p)] = p
    return points, lens, refined


def chain_layout(n_envs, chains, per):
    """geom_of_env of the pool envs: env i follows chain i % chains (`per` entries each), starting (i // chains) % per
    entries into it, so replicas of a chain are out of phase."""
    i = np.arange(int(n_envs))
    return (i % chains) * per + (i // chains) % per


def pool_or_sample(pool, samplers, sampler, seeds, n_chains, n_envs):
    """The pool a pool env runs on: `pool` itself, or samplers[sampler](seeds) -- by default one chain per env, at most
    1024."""
    if pool is not None:
        return pool
    if sampler not in samplers:
        raise ValueError("sampler must be 'device', 'device_resident' or 'host', not %r" % (sampler,))
    if seeds is None:
        seeds = range(int(n_chains) if n_chains else min(int(n_envs), 1024))
    return samplers[sampler](list(seeds))


class HostEntries(object):
    """The host copies behind one binding of BatchedPlanEnv -- its costmaps, or its paths -- with the rule from an env, or
    from a bound entry, to its item.  `items` is a list, or the lazy sequence a DeviceGeometryPool hands out; the bound
    entries are 1 for a shared item, the pool's entries for a pool, else one per env."""

    def __init__(self, items, n_entries, item_of_entry=None, pool=False):
        self.items, self.n_entries, self.pool = items, int(n_entries), pool
        self._item_of_entry = item_of_entry   # int array [n_entries], None = entry k holds items[k]

    @classmethod
    def shared(cls, item):
        return cls([item], 1)

    @classmethod
    def per_env(cls, items):
        return cls(items, len(items))

    @classmethod
    def templates(cls, items, template_of_env):
        """env i holds a private copy of items[template_of_env[i]] (until a replace() gives every env its own item)"""
        return cls(items, len(template_of_env), np.asarray(template_of_env, dtype=np.int64))

    @classmethod
    def pool_entries(cls, items):
        """env i holds items[geom_of_env[i]]; the entry an env is on lives on the device, so of_env() is told"""
        return cls(items, len(items), pool=True)

    def index(self):
        """int64 [n_entries]: the item of every bound entry"""
        return np.arange(self.n_entries) if self._item_of_entry is None else self._item_of_entry

    def of_entry(self, k):
        return self.items[int(k) if self._item_of_entry is None else int(self._item_of_entry[k])]

    def of_env(self, i, entry=None):
        """The item of env i; a pool needs `entry`, the pool entry the env is on."""
        if self.pool:
            return self.of_entry(entry)
        return self.of_entry(0 if self.n_entries == 1 else i)

    def replace(self, items):
        """After an edit of the bound entries: `items`, one per bound entry, are the host copies from now on."""
        if len(items) != self.n_entries:
            raise ValueError("need one item per bound entry (%d), got %d" % (self.n_entries, len(items)))
        self.items, self._item_of_entry = items, None

    def replace_stored(self, items):
        """After an edit that treats equal entries equally: one new item per stored item, the rule stays."""
        if len(items) != len(self.items):
            raise ValueError("need one item per stored item (%d), got %d" % (len(self.items), len(items)))
        self.items = items


class DeviceGeometryPool(object):
    """G geometries that already live on the GPU (e.g. from mini_env.sample_device_pool): what BatchedPlanEnv's
    geometry-pool mode needs, as device tensors.  `costmaps` / `paths` hand out host copies on demand, for the per-env
    views (envs[i].get_state())."""

    def __init__(self, maps, origin, resolution, paths, lens, init, origins=None, valid_rows=None, valid_cols=None):
        self.maps = maps                  # uint8 [G, rows, cols]
        self.origin = np.asarray(origin, dtype=np.float64) if origin is not None else None   # one origin for all entries
        self.resolution = float(resolution)
        self.path_points = paths          # float64 [G, max_len, 3], already refined
        self.lens = lens                  # int32 [G]
        self.init = init                  # float64 [G, 2] = (min_spat_dist_so_far, target_idx)
        # optional, for entries of different sizes: float64 [G, 2] origin of every entry, int32 [G] true shape of every
        # entry (the rest of its [rows, cols] is padding); None = one origin, every entry uses all of [rows, cols]
        self.origins, self.valid_rows, self.valid_cols = origins, valid_rows, valid_cols

    def __len__(self):
        return int(self.maps.shape[0])

    class _Lazy(object):
        def __init__(self, n, fetch):
            self._n, self._fetch = n, fetch

        def __len__(self):
            return self._n

        def __getitem__(self, k):
            if not -self._n <= k < self._n:
                raise IndexError(k)
            return self._fetch(int(k) % self._n)

    @property
    def costmaps(self):
        if self.origins is None:
            return self._Lazy(len(self), lambda k: CostMap2D(self.maps[k].cpu().numpy(), self.resolution, self.origin))

        def fetch(k):   # the entry cropped to its true shape, with its own origin
            vr = int(self.valid_rows[k]) if self.valid_rows is not None else self.maps.shape[1]
            vc = int(self.valid_cols[k]) if self.valid_cols is not None else self.maps.shape[2]
            return CostMap2D(self.maps[k, :vr, :vc].cpu().numpy(), self.resolution, self.origins[k].cpu().numpy())
        return self._Lazy(len(self), fetch)

    def entry_origins(self, device):
        """float64 [G, 2] device tensor: the origin of every entry."""
        import torch
        if self.origins is not None:
            return self.origins.to(device).contiguous()
        return torch.from_numpy(np.tile(self.origin, (len(self), 1))).to(device)

    @property
    def paths(self):
        return self._Lazy(len(self), lambda k: self.path_points[k, :int(self.lens[k])].cpu().numpy())

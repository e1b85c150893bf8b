"""RandomAisleTurnEnv geometry: the reset-time side of a batched aisle-turn env.

The reference's RandomAisleTurnEnv (envs/synth_turn_env.py:219-332) draws a new random aisle turn on every reset():
eight numbers from its RandomState (_draw_random_turn_params, :317-332), then path_and_costmap_from_config (:110-192)
builds the turn's map -- five 1-px walls on an empty map just large enough for the turn -- and its 4-point coarse path.
There is no rejection loop, so a world is a pure function of its eight numbers.

As for RandomMiniEnv (mini_env.py), a reset at 65 536 envs cannot be a host round trip: the worlds are drawn ahead of
time into a POOL and the step / reset kernels walk each env along its chain of pool entries.  Chain c of a pool is the
sequence of worlds `RandomAisleTurnEnv(seed=seeds[c])` goes through: world 0 is drawn by the constructor, world k by
the k-th reset().

  * sample_aisle_pool          host numpy, bit-identical to the reference
  * sample_aisle_pool_device   the same pool drawn and rendered on the GPU (csrc/bcp_aisle.h)
  * BatchedRandomAisleTurnEnv  N RandomAisleTurnEnv on one GPU (geometry-pool mode of BatchedPlanEnv)
"""
import ctypes as C

import attr
import numpy as np
import torch

from . import _lib, robots
from .api import CostMap2D, EnvParams
from .batched_env import BatchedPlanEnv
from .geometry import DeviceGeometryPool, pool_or_sample
from .mini_env import add_wall, map_shape

# one world record of the device sampler (bcp_sample_aisle_worlds, include/bcplan.h)
RECORD = 44
_R_ORIGIN, _R_WAY, _R_LEN = 8, 30, 42   # world origin, way points B K L F, refined path length


@attr.s
class TurnParams(object):
    """Parametrization of one turn (envs/synth_turn_env.py:21-32, same fields and defaults)."""
    main_corridor_length = attr.ib(default=8, type=float)
    turn_corridor_length = attr.ib(default=5, type=float)
    turn_corridor_angle = attr.ib(default=2 * np.pi / 8, type=float)
    main_corridor_width = attr.ib(default=1.0, type=float)
    turn_corridor_width = attr.ib(default=1.0, type=float)
    margin = attr.ib(default=1.0, type=float)
    flip_arnd_oy = attr.ib(default=False, type=bool)
    flip_arnd_ox = attr.ib(default=False, type=bool)
    rot_theta = attr.ib(default=0, type=float)


@attr.s
class AisleTurnEnvParams(object):
    """Parametrization of an aisle-turn env (envs/synth_turn_env.py:35-39)."""
    env_params = attr.ib(factory=EnvParams)
    turn_params = attr.ib(factory=TurnParams)


@attr.s
class TurnRanges(object):
    """The ranges RandomAisleTurnEnv._draw_random_turn_params draws from (envs/synth_turn_env.py:317-332)."""
    main_corridor_length = attr.ib(default=(10., 16.))
    turn_corridor_length = attr.ib(default=(4., 12.))
    turn_corridor_angle = attr.ib(default=(-3. / 8. * np.pi, 3. / 8. * np.pi))
    main_corridor_width = attr.ib(default=(0.5, 1.5))
    turn_corridor_width = attr.ib(default=(0.5, 1.5))
    margin = attr.ib(default=1.0)   # TurnParams' default: the random env never sets it


def draw_random_turn_params(rng, ranges=None):
    """RandomAisleTurnEnv._draw_random_turn_params (envs/synth_turn_env.py:317-332): five uniform draws, two
    rand() < 0.5 and uniform(0, 2 pi), in this order -- 8 doubles of the stream."""
    r = TurnRanges() if ranges is None else ranges
    return TurnParams(
        main_corridor_length=rng.uniform(*r.main_corridor_length),
        turn_corridor_length=rng.uniform(*r.turn_corridor_length),
        turn_corridor_angle=rng.uniform(*r.turn_corridor_angle),
        main_corridor_width=rng.uniform(*r.main_corridor_width),
        turn_corridor_width=rng.uniform(*r.turn_corridor_width),
        margin=r.margin,
        flip_arnd_oy=bool(rng.rand() < 0.5),
        flip_arnd_ox=bool(rng.rand() < 0.5),
        rot_theta=rng.uniform(0, 2 * np.pi))


def _pts_in_standard_coords(d, h, alpha, z, w):
    # _draw_pts_in_standard_coords (:42-79): the corners A .. J of the unrotated, unflipped turn
    far_x = w
    return (np.array([-d, -h]), np.array([0, -h]), np.array([d, -h]),
            np.array([d, d * np.tan(alpha) - z / np.cos(alpha)]),
            np.array([far_x, far_x * np.tan(alpha) - z / np.cos(alpha)]),
            np.array([far_x, far_x * np.tan(alpha)]),
            np.array([d, d * np.tan(alpha) + z / np.cos(alpha)]),
            np.array([far_x, far_x * np.tan(alpha) + z / np.cos(alpha)]),
            np.array([-d, h]), np.array([d, h]))


def _path_in_standard_coords(d, h, alpha, z, w):
    # _generate_path_in_standard_coords (:82-97): the oriented way points B, K, L, F
    return (np.array([0, -h, np.pi / 2]),
            np.array([0, d * np.tan(alpha) - z / np.cos(alpha), np.pi / 2]),
            np.array([d, d * np.tan(alpha), alpha]),
            np.array([w * np.cos(alpha), w * np.cos(alpha) * np.tan(alpha), alpha]))


def turn_geometry(tp):
    """-> (corners [10, 2], coarse path [4, 3], world_size (x, y), world_origin (x, y)) of a turn: the geometric
    half of path_and_costmap_from_config (:110-172), with the reference's numpy operations (np.dot included)."""
    hh = tp.main_corridor_length / 2
    w = tp.turn_corridor_length / 2
    alpha = tp.turn_corridor_angle
    dd = tp.main_corridor_width
    z = tp.turn_corridor_width
    margin = tp.margin
    pts = _pts_in_standard_coords(dd, hh, alpha, z, w)
    way = _path_in_standard_coords(dd, hh, alpha, z, w)
    c, s = np.cos(tp.rot_theta), np.sin(tp.rot_theta)
    rot = np.array(((c, -s), (s, c)))
    flip = np.array([[-1. if tp.flip_arnd_oy else 1., 0.], [0., -1. if tp.flip_arnd_ox else 1.]])
    transform = np.dot(rot, flip)
    new_pts = [np.dot(transform, pt) for pt in pts]
    new_way = []
    for x, y, t in way:
        nx, ny = np.dot(transform, np.array([x, y]))
        angle = t
        if tp.flip_arnd_ox:
            angle = -angle
        if tp.flip_arnd_oy:
            angle = np.pi - angle
        angle = np.mod(angle + tp.rot_theta, 2 * np.pi)
        new_way.append(np.array([nx, ny, angle]))
    all_pts = np.array(list(new_pts))
    min_x, max_x = all_pts[:, 0].min(), all_pts[:, 0].max()
    min_y, max_y = all_pts[:, 1].min(), all_pts[:, 1].max()
    world_size = abs(max_x - min_x) + 2 * margin, abs(max_y - min_y) + 2 * margin
    world_origin = min_x - margin, min_y - margin
    return all_pts, np.array(new_way), world_size, np.asarray(world_origin, dtype=np.float64)


# the five walls A-I, C-D, D-E, J-G, G-H as corner indices (:174-180)
WALLS = ((0, 8), (2, 3), (3, 4), (9, 6), (6, 7))


def path_and_costmap_from_config(config):
    """path_and_costmap_from_config (envs/synth_turn_env.py:110-192) -> (coarse path [4, 3], CostMap2D).
    config: AisleTurnEnvParams."""
    corners, path, world_size, origin = turn_geometry(config.turn_params)
    res = config.env_params.resolution
    data = np.zeros(map_shape(world_size[0], world_size[1], res), dtype=np.uint8)
    costmap = CostMap2D(data, res, origin)
    for i, j in WALLS:
        add_wall(costmap, corners[i], corners[j])
    return path, costmap


class AislePool(object):
    """n_chains x episodes pre-drawn turns.  Entry c * episodes + k is the k-th world of chain c; `next_geom` walks a
    chain and wraps around at its end.  costmaps have each their own shape and origin."""

    def __init__(self, env_params, seeds, episodes, worlds, built=None):
        self.env_params, self.seeds, self.episodes = env_params, list(seeds), int(episodes)
        self.worlds = worlds                                        # TurnParams, chain-major
        if built is None:
            built = [path_and_costmap_from_config(AisleTurnEnvParams(env_params, w)) for w in worlds]
        self.paths = [b[0] for b in built]
        self.costmaps = [b[1] for b in built]
        g = np.arange(len(worlds), dtype=np.int32)
        self.next_geom = ((g // self.episodes) * self.episodes + (g % self.episodes + 1) % self.episodes).astype(np.int32)

    def __len__(self):
        return len(self.worlds)


def sample_aisle_pool(params=None, seeds=(0,), episodes=1, ranges=None):
    """Host sampler: chain c is the worlds RandomAisleTurnEnv(params, seed=seeds[c]) goes through, world 0 drawn at
    construction, world k at the k-th reset() (envs/synth_turn_env.py:226-252, 269-281).  Bit-identical to the
    reference."""
    params = EnvParams() if params is None else params
    worlds = []
    for s in seeds:
        rng = np.random.RandomState()   # RandomAisleTurnEnv.__init__: an unseeded RandomState, then seed(seed)
        if s is not None:
            rng.seed(s)
        worlds.extend(draw_random_turn_params(rng, ranges) for _ in range(int(episodes)))
    return AislePool(params, seeds, episodes, worlds)


class DeviceAislePool(DeviceGeometryPool):
    """An aisle pool that never leaves the GPU (sample_aisle_pool_device(..., keep_on_device=True)): world records,
    padded maps with per-entry origins and shapes, refined paths and initial reward states as device tensors."""

    def __init__(self, env_params, seeds, episodes, worlds, shapes, maps, paths, lens, init):
        super(DeviceAislePool, self).__init__(maps, None, env_params.resolution, paths, lens, init,
                                              origins=worlds[:, _R_ORIGIN:_R_ORIGIN + 2].contiguous(),
                                              valid_rows=shapes[:, 0].contiguous(), valid_cols=shapes[:, 1].contiguous())
        self.env_params, self.seeds, self.episodes = env_params, list(seeds), int(episodes)
        self.world_params = worlds        # float64 [G, RECORD]
        self.shapes = shapes              # int32 [G, 2]
        g = np.arange(len(self), dtype=np.int32)
        self.next_geom = ((g // self.episodes) * self.episodes + (g % self.episodes + 1) % self.episodes).astype(np.int32)

    @property
    def worlds(self):
        return self._Lazy(len(self), lambda k: _turn_of_record(self.world_params[k].cpu().numpy()))

    def nbytes(self):
        """Device memory of the pool's tensors."""
        return sum(int(t.numel() * t.element_size()) for t in (self.maps, self.path_points, self.lens, self.init,
                                                               self.world_params, self.shapes))


def _turn_of_record(v):
    return TurnParams(main_corridor_length=float(v[0]), turn_corridor_length=float(v[1]), turn_corridor_angle=float(v[2]),
                      main_corridor_width=float(v[3]), turn_corridor_width=float(v[4]), flip_arnd_oy=bool(v[5]),
                      flip_arnd_ox=bool(v[6]), rot_theta=float(v[7]))


def aisle_world_params(env_params, ranges=None):
    """The bcp_aisle_world_params of an EnvParams and a TurnRanges."""
    r = TurnRanges() if ranges is None else ranges
    p = _lib.BcpAisleWorldParams()
    for name in ("main_corridor_length", "turn_corridor_length", "turn_corridor_angle", "main_corridor_width",
                 "turn_corridor_width"):
        lo, hi = getattr(r, name)
        getattr(p, name)[0], getattr(p, name)[1] = float(lo), float(hi)
    p.margin, p.resolution, p.path_delta = float(r.margin), float(env_params.resolution), float(env_params.path_delta)
    return p


def sample_aisle_pool_device(params=None, seeds=(0,), episodes=1, device=0, keep_on_device=False, ranges=None):
    """The pool of sample_aisle_pool(), made on the GPU (csrc/bcp_aisle.h): bcp_sample_aisle_worlds draws every chain's
    turns (one wavefront per seed), the host reads the largest map shape and path length back (the one synchronisation),
    sizes the pool [G, max_rows, max_cols rounded up to 64] and bcp_render_aisle_worlds draws the walls.  A coordinate
    can differ from numpy's in its last bit: the transcendentals are the device's.
    keep_on_device=True returns a DeviceAislePool: refined paths and initial reward states are made on the GPU as well
    (bcp_aisle_world_paths) and nothing is downloaded; otherwise an AislePool of host arrays."""
    params = EnvParams() if params is None else params
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("sampling aisle-turn worlds needs a GPU (libbcplan has no CPU path)")
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    h = C.c_void_p()
    bp = robots.make_bcp_params(params, params.robot_name, None)
    _lib.check(lib.bcp_create(C.byref(bp), 1, dev.index or 0, 0, C.byref(h)))
    try:
        seeds = [int(s) for s in seeds]
        n, episodes = len(seeds), int(episodes)
        g_n = n * episodes
        ap = aisle_world_params(params, ranges)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        seed_t = torch.tensor(seeds, dtype=torch.int64, device=dev)
        mt = torch.empty((n, 625), dtype=torch.int32, device=dev)
        worlds = torch.empty((g_n, RECORD), dtype=torch.float64, device=dev)
        shapes = torch.empty((g_n, 2), dtype=torch.int32, device=dev)
        _lib.check(lib.bcp_mini_world_seed(h, seed_t.data_ptr(), n, mt.data_ptr(), stream))
        _lib.check(lib.bcp_sample_aisle_worlds(h, C.byref(ap), mt.data_ptr(), n, episodes, worlds.data_ptr(),
                                               shapes.data_ptr(), stream))
        top = torch.cat([shapes.max(0).values, worlds[:, _R_LEN].max().to(torch.int32).reshape(1)]).cpu().numpy()
        rows, cols, max_len = int(top[0]), int(top[1]), int(top[2])
        pitch = (cols + 63) // 64 * 64
        maps = torch.empty((g_n, rows, pitch), dtype=torch.uint8, device=dev)
        _lib.check(lib.bcp_render_aisle_worlds(h, worlds.data_ptr(), shapes.data_ptr(), g_n, float(params.resolution),
                                               rows, pitch, maps.data_ptr(), stream))
        if keep_on_device:
            if not params.refine_path:
                raise NotImplementedError("device pools always carry refined paths")
            paths = torch.zeros((g_n, max_len, 3), dtype=torch.float64, device=dev)
            lens = torch.zeros(g_n, dtype=torch.int32, device=dev)
            init = torch.zeros((g_n, 2), dtype=torch.float64, device=dev)
            pstat = torch.zeros(g_n, dtype=torch.int32, device=dev)
            _lib.check(lib.bcp_aisle_world_paths(h, worlds.data_ptr(), g_n, float(params.path_delta), max_len,
                                                 paths.data_ptr(), lens.data_ptr(), init.data_ptr(), pstat.data_ptr(),
                                                 stream))
            worst = int(pstat.max())
            if worst == 2:
                raise ValueError("Goal pose too close to initial pose")
            assert worst == 0, "refined path longer than expected"
            return DeviceAislePool(params, seeds, episodes, worlds, shapes, maps, paths, lens, init)
        # download the true rows x cols of every entry only (one after the other, row-major: the padding stays behind),
        # in groups of entries small enough for torch's boolean indexing (< 2^31 elements)
        r = torch.arange(rows, device=dev, dtype=torch.int32)[None, :, None]
        c = torch.arange(pitch, device=dev, dtype=torch.int32)[None, None, :]
        group = max(1, (1 << 30) // (rows * pitch))
        parts = []
        for g0 in range(0, g_n, group):
            sh = shapes[g0:g0 + group]
            parts.append(maps[g0:g0 + group][(r < sh[:, 0, None, None]) & (c < sh[:, 1, None, None])].cpu().numpy())
        cells = np.concatenate(parts)
        w_host, s_host = worlds.cpu().numpy(), shapes.cpu().numpy()
    finally:
        lib.bcp_destroy(h)
    world_list, built = [], []
    offsets = np.concatenate([[0], np.cumsum(s_host[:, 0].astype(np.int64) * s_host[:, 1])])
    for g in range(g_n):
        v = w_host[g]
        world_list.append(_turn_of_record(v))
        data = cells[offsets[g]:offsets[g + 1]].reshape(int(s_host[g, 0]), int(s_host[g, 1]))
        built.append((v[_R_WAY:_R_WAY + 12].reshape(4, 3).copy(),
                      CostMap2D(data, params.resolution, v[_R_ORIGIN:_R_ORIGIN + 2].copy())))
    return AislePool(params, seeds, episodes, world_list, built=built)


class BatchedRandomAisleTurnEnv(BatchedPlanEnv):
    """N RandomAisleTurnEnv instances (envs/synth_turn_env.py:219-332) on one GPU: a BatchedPlanEnv in geometry-pool
    mode, each env with its own turn, map and path, and auto-reset / reset() moving it to its chain's next turn.

    Env i follows chain i % n_chains of the pool, starting (i // n_chains) % episodes entries into it (as
    BatchedRandomMiniEnv).  With one chain per env and seeds[i] = s_i, env i sees the turns RandomAisleTurnEnv(seed=s_i)
    sees for its first `episodes` worlds (then the chain wraps around).  As in the reference, construction leaves the
    env on world 0 of its chain and the first reset() moves it to world 1 -- BatchedPlanEnv's constructor already ends
    with that reset().

    :param params EnvParams: the PlanEnv parameters (RandomAisleTurnEnv's `params`), EnvParams() by default
    :param pool: AislePool / DeviceAislePool, or None to draw `n_chains` x `episodes` turns here
    :param sampler: "device" (sample_aisle_pool_device: drawn and rendered on the GPU, coordinates within 1e-12 of the
        reference's), "device_resident" (the same, and the pool never leaves the GPU: for 10^4 .. 10^5 worlds) or
        "host" (sample_aisle_pool: numpy, bit-identical to the reference)
    :param draw_new_turn_on_reset bool: False keeps every env on its first world (RandomAisleTurnEnv's flag)
    Remaining keyword arguments go to BatchedPlanEnv (auto_reset, seed, noise_parameters, env_id_base, ...).
    """

    def __init__(self, n_envs, params=None, pool=None, seeds=None, n_chains=None, episodes=4, device=0,
                 draw_new_turn_on_reset=True, sampler="device", ranges=None, **kw):
        params = EnvParams() if params is None else params
        pool = pool_or_sample(pool, {
            "device": lambda s: sample_aisle_pool_device(params, s, episodes, device, ranges=ranges),
            "device_resident": lambda s: sample_aisle_pool_device(params, s, episodes, device, keep_on_device=True, ranges=ranges),
            "host": lambda s: sample_aisle_pool(params, s, episodes, ranges)}, sampler, seeds, n_chains, n_envs)
        self._init_from_pool(pool, params, n_envs, pool.next_geom if draw_new_turn_on_reset else None, device=device, **kw)

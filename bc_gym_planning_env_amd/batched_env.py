"""BatchedPlanEnv: N PlanEnv instances advanced by one fused HIP kernel per step.

Mirrors the reference's object API (envs/base/env.py:217-439): reset() / step() / get_state() / set_state() /
seed() / action_space, batched over N envs, plus `envs[i]` views that hand back reference-shaped
Observation / State objects for one env.  Device tensors are torch tensors only because they cross the C ABI as
raw pointers (tensor.data_ptr()); all arithmetic happens in libbcplan.so.
"""
import ctypes as C
import functools
import weakref
from collections import OrderedDict

import attr

import numpy as np
import torch

from . import _lib, boxes, host_init, robots
from .api import Action, Box, CONTINUOUS_REWARD_PURE_PURSUIT, CostMap2D, EnvParams, INDUSTRIAL_TRICYCLE_V1, State
from .episode_record import EpisodeEnds
from .geometry import DeviceGeometryPool, HostEntries, chain_layout, stack_costmaps, stack_paths
from .handle import Handle, SCAN_CACHE_ENTRIES, beam_table_cached, cached
from .planning import Lookahead, Mppi, Track
from .state import BatchedObservation, BatchedState, EnvView, _EnvViews

# (everything that was ever importable from here still is)
__all__ = ["BatchedPlanEnv", "DeviceGeometryPool", "BatchedState", "BatchedObservation", "EnvView", "EpisodeEnds",
           "Lookahead", "Mppi", "Track", "beam_table_cached", "SCAN_CACHE_ENTRIES"]


def _as_device_actions(actions, n, device):
    """list[Action] | ndarray | tensor -> contiguous [n,2] float32/float64 tensor on the device."""
    if isinstance(actions, torch.Tensor):
        t = actions
    else:
        if isinstance(actions, Action):
            actions = [actions]
        if isinstance(actions, (list, tuple)) and len(actions) and isinstance(actions[0], Action):
            actions = np.stack([np.asarray(a.command) for a in actions])
        t = torch.from_numpy(np.ascontiguousarray(actions))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    t = t.to(device).contiguous()
    if tuple(t.shape) != (n, 2):
        raise ValueError("actions must have shape (%d, 2), got %s" % (n, tuple(t.shape)))
    return t


class BatchedPlanEnv(Handle):
    """N planning envs on one MI355X.

    :param costmap: CostMap2D shared by all envs, or a list of N CostMap2D of equal resolution (private maps)
    :param path: array(M, 3) shared oriented path, or a list of N such arrays (private paths)
    :param params EnvParams: as the reference (delays must be 0; continuous reward provider)
    :param n_envs int: number of envs on this device
    :param device: torch device / index of the GPU
    :param robot_name: robot model + footprint; default params.robot_name (PlanEnv itself always drives a tricycle)
    :param noise_parameters: 'planenv' = the odometry noise PlanEnv hard-codes on its tricycle (env.py:226-232; for a
        diff-drive robot, which PlanEnv never builds, that default means None), None = off, or a dict alpha1..alpha6.
        A diff-drive robot WITH noise raises IndexError like the reference (differential_drive.py:73) unless
        unpinned_diffdrive_noise=True opts in to the library's unpinned analogue
    :param auto_reset bool: restore an env's initial state right after the step that finished it
    :param env_id_base int: global index of env 0 (rank * n_envs when sharded over GPUs); keys the noise stream
    :param template_of_env: optional int array [n_envs]; `costmap` and `path` are then lists of T templates and env i
        gets a PRIVATE copy of costmap[template_of_env[i]] / path[template_of_env[i]] (built on the device)
    :param geom_of_env: optional int array [n_envs] -> GEOMETRY POOL mode: `costmap` and `path` are lists of G pool
        entries, env i runs on entry geom_of_env[i], and every reset (reset(), auto-reset) moves an env to
        next_geom[entry] (RandomMiniEnv.reset with draw_new_turn_on_reset, envs/mini_env.py:469-481).  Note that the
        constructor ends with reset(), like the reference's usage `env = RandomMiniEnv(); env.reset()`.
    :param next_geom: optional int array [G], successor of every pool entry; None = stay on the same entry
    :param map_storage: optional (rows, cols): private costmaps are stored with at least this (padded) shape, e.g.
        (256, 256) for BASELINE's "per-env 256x256 costmap"; the true shapes still bound the collision test
    :param robot_constants: optional dict replacing any of robots.ROBOT_CONSTANTS (wheel base, steering and
        acceleration limits, front-column P gain) for a robot of other dimensions than the stock ones
    """

    _path_epoch = 0   # path bindings so far (_bind_paths)

    def __init__(self, costmap, path, params=None, n_envs=1, device=0, robot_name=None, noise_parameters='planenv',
                 auto_reset=False, env_id_base=0, seed=0, footprint_scale=1.0, dynamic_model=True,
                 model_front_column_pid=True, template_of_env=None, geom_of_env=None, next_geom=None, map_storage=None,
                 unpinned_diffdrive_noise=False, robot_constants=None):
        params = EnvParams() if params is None else params
        self.params = params
        self._pure_pursuit = params.reward_provider_name == CONTINUOUS_REWARD_PURE_PURSUIT
        self.n_envs = int(n_envs)
        self.robot_name = params.robot_name if robot_name is None else robot_name
        self.is_tricycle = self.robot_name == INDUSTRIAL_TRICYCLE_V1
        if noise_parameters == 'planenv':
            noise_parameters = dict(robots.PLANENV_NOISE) if self.is_tricycle else None
        self.noise_parameters = noise_parameters
        self.auto_reset = bool(auto_reset)
        super(BatchedPlanEnv, self).__init__(
            robots.make_bcp_params(params, self.robot_name, noise_parameters, footprint_scale, dynamic_model,
                                   model_front_column_pid, unpinned_diffdrive_noise, robot_constants),
            self.n_envs, device, env_id_base, needs_gpu="BatchedPlanEnv")
        self.action_space = Box(low=np.array([robots.MAX_FRONT_WHEEL_SPEED / 10, -np.pi / 2]),
                                high=np.array([robots.MAX_FRONT_WHEEL_SPEED / 2, np.pi / 2]), dtype=np.float32)
        self.reward_range = (0.0, 1.0)
        self.time_table = host_init.time_table(params.dt, params.iteration_timeout + 1)
        self._time_table_dev = torch.from_numpy(self.time_table).to(self.device)

        n, dev = self.n_envs, self.device
        def f64(*shape):
            return torch.zeros(*shape, dtype=torch.float64, device=dev)

        cd, pd, sd = int(params.control_delay), int(params.pose_delay), int(params.state_delay)
        self.state = BatchedState(f64(7, n), f64(n), torch.zeros(n, dtype=torch.int32, device=dev),
                                  torch.zeros(n, dtype=torch.int32, device=dev),
                                  torch.zeros(n, dtype=torch.uint8, device=dev),
                                  pose_seen=f64(3, n) if pd else None, robot_state_seen=f64(7, n) if sd else None,
                                  control_queue=f64(cd, 2, n) if cd else None, poses_queue=f64(pd, 3, n) if pd else None,
                                  robot_state_queue=f64(sd, 7, n) if sd else None)
        self.reward = torch.zeros(n, dtype=torch.float64, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.collided_now = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.err = torch.zeros(n, dtype=torch.int32, device=dev)
        self.envs = _EnvViews(self)
        # what only some modes or subclasses change, at its neutral value
        self.endless = False       # BatchedRandomMiniEnv(endless=True)
        self._inflated = False     # inflate_costmaps()
        self._goal_followers = []  # weak references to the GoalFields a refresh() keeps current (goal_field(follow_refresh=True))
        self._rollout_buffers, self._lookahead_buffers, self._mppi_buffers = OrderedDict(), OrderedDict(), OrderedDict()
        self._range_scan_buffers, self._track_buffers = OrderedDict(), OrderedDict()

        # the geometry, in one of five modes (a shared costmap may go with private paths and the other way round); the host
        # copies of either half and which of them is env i's: self._map_host, self._path_host (geometry.HostEntries)
        self._map_storage = (0, 0) if map_storage is None else (int(map_storage[0]), int(map_storage[1]))
        self._template_of_env = None if template_of_env is None else np.asarray(template_of_env, dtype=np.int64)
        self._device_pool = None
        self.geom_of_env = None
        if geom_of_env is not None:
            assert template_of_env is None
            if isinstance(costmap, DeviceGeometryPool):   # DEVICE POOL: everything is on the device already
                self._device_pool = costmap
                self._set_geometry_pool(len(costmap), geom_of_env, next_geom)
                self._set_from_device_pool(costmap)
            else:                                         # HOST POOL: the library indexes the entries itself
                costmap, path = list(costmap), list(path)
                assert len(costmap) == len(path)
                self._set_geometry_pool(len(costmap), geom_of_env, next_geom)
                self._set_from_templates(costmap, path, None)
        elif self._template_of_env is not None:           # TEMPLATES: expanded to private copies on the device
            self._set_from_templates(list(costmap), list(path), self._template_of_env)
        else:                                             # SHARED (one object) or ONE PER ENV (a list), each of the two
            self._set_costmaps(costmap)
            self._set_paths(path)
        self._bind(self.state, self._lib.bcp_bind_state)
        self._initial_state = self._make_initial_state()
        self._bind_initial_state()
        # per-step call state, built once (the step path itself should cost microseconds of host time)
        self._io = _lib.BcpStepIO()
        self._io.reward = self.reward.data_ptr()
        self._io.done = self.done.data_ptr()
        self._io.collided_now = self.collided_now.data_ptr()
        self._io.err = self.err.data_ptr()
        self._io_ref = C.byref(self._io)
        self._bcp_step = self._lib.bcp_step
        self._flags_f64 = _lib.STEP_AUTO_RESET if self.auto_reset else 0
        self._flags_f32 = self._flags_f64 | _lib.STEP_ACTIONS_F32
        self._obs = BatchedObservation(self)
        self._info = {}
        self.episode_ends = None   # enable_episode_record()
        self.seed(seed)
        self.reset()

    def _init_from_pool(self, pool, params, n_envs, next_geom, **kw):
        """The constructor of the pool envs (BatchedRandomMiniEnv, BatchedRandomAisleTurnEnv): geometry-pool mode with env i
        on chain i % chains of `pool` (geometry.chain_layout); a pool on the device is bound as it is, a host pool through
        its costmaps and paths."""
        self.pool = pool
        on_device = isinstance(pool, DeviceGeometryPool)
        BatchedPlanEnv.__init__(self, pool if on_device else pool.costmaps, None if on_device else pool.paths, params,
                                n_envs=n_envs, geom_of_env=chain_layout(n_envs, len(pool.seeds), pool.episodes),
                                next_geom=next_geom, **kw)

    # ------------------------------------------------------------------ construction helpers
    def _bind(self, s, fn):
        _lib.check(fn(self._h, C.byref(s.fill_pointers(_lib.BcpState()))))

    def _bind_initial_state(self):
        """Binds self._initial_state and, where one shared path gives every env the same initial state (no pool, no expanded
        templates), declares it uniform (declare_uniform_initial_state): the library checks the arrays and refuses otherwise."""
        self._bind(self._initial_state, self._lib.bcp_bind_initial_state)
        if self._shared_path and self.geom_of_env is None and self._template_of_env is None:
            self.declare_uniform_initial_state(True)

    def declare_uniform_initial_state(self, on=True):
        """bcp_declare_uniform_initial_state: on=True checks (on the host, synchronising) that every env's bound initial state
        equals env 0's bit for bit and keeps that entry as a snapshot; auto-reset steps of the shared-geometry kernel then
        reset from it without loading the arrays.  Raises _lib.BcpError where the arrays differ or the env has a geometry
        pool.  The snapshot is a value: after writing the initial tensors in place, declare again.  on=False drops it."""
        _lib.check(self._lib.bcp_declare_uniform_initial_state(self._h, 1 if on else 0, self._stream()))

    def step_uniform_reset(self):
        """True when the last step() took its resets from the declared uniform initial state (bcp_step_uniform_reset)."""
        rc = self._lib.bcp_step_uniform_reset(self._h)
        if rc < 0:
            _lib.check(rc)
        return rc == 1

    def _refine(self):
        """What every path given to the constructor goes through: refine_path at params.path_delta, or nothing."""
        if self.params.refine_path:
            return functools.partial(host_init.refine_path, delta=self.params.path_delta)
        return lambda p: p

    def _set_geometry_pool(self, n_entries, geom_of_env, next_geom):
        g0 = np.asarray(geom_of_env, dtype=np.int32)
        assert g0.shape == (self.n_envs,) and 0 <= g0.min() and g0.max() < n_entries
        self.geom_of_env = torch.from_numpy(g0.copy()).to(self.device)
        nxt = None
        if next_geom is not None:
            nx = np.asarray(next_geom, dtype=np.int32)
            assert nx.shape == (n_entries,) and 0 <= nx.min() and nx.max() < n_entries
            nxt = torch.from_numpy(nx.copy()).to(self.device)
        self._keep.update(next_geom=nxt)
        _lib.check(self._lib.bcp_set_geometry_pool(self._h, n_entries, self.geom_of_env.data_ptr(),
                                                   nxt.data_ptr() if nxt is not None else None))

    def _set_costmaps(self, costmap):
        if isinstance(costmap, CostMap2D) or hasattr(costmap, "get_data") and not isinstance(costmap, (list, tuple)):
            self._map_host, self._shared_map = HostEntries.shared(costmap), True
            data = np.ascontiguousarray(costmap.get_data(), dtype=np.uint8)
            self._origin_host = np.ascontiguousarray(costmap.get_origin(), dtype=np.float64)
            self.resolution = float(costmap.get_resolution())
            self._keep["map"] = torch.from_numpy(data).to(self.device)
            self._rebind_costmaps()
        else:
            costmaps = list(costmap)
            if len(costmaps) != self.n_envs:
                raise ValueError("need one costmap per env (%d), got %d" % (self.n_envs, len(costmaps)))
            data, shapes, origins, res = stack_costmaps(costmaps, self._map_storage)
            self._map_host = HostEntries.per_env(costmaps)
            self.set_costmap_tensors(self._device_tensor(data, torch.uint8), self._device_tensor(origins), res,
                                     self._device_tensor(shapes[:, 0], torch.int32),
                                     self._device_tensor(shapes[:, 1], torch.int32))

    def _set_from_device_pool(self, dp):
        """A pool whose maps, refined paths and initial states are on the device already: bound where they are."""
        # (the lazy sequences read the pool's tensors at every fetch: they follow edits of the pool, also of its attributes)
        self._map_host, self._path_host = HostEntries.pool_entries(dp.costmaps), HostEntries.pool_entries(dp.paths)
        self._shared_path = False
        self.set_costmap_tensors(dp.maps, dp.entry_origins(self.device), dp.resolution, dp.valid_rows, dp.valid_cols)
        self._bind_paths(dp.path_points, dp.lens)

    def _set_from_templates(self, costmaps, paths, template_of_env):
        """Private costmaps / paths from a few templates: one copy per env, expanded on the device, or -- template_of_env
        None -- the templates themselves, as the entries of a geometry pool."""
        dev = self.device
        pick, entries = (lambda t: t), HostEntries.pool_entries   # noqa: E731
        if template_of_env is not None:
            entries = functools.partial(HostEntries.templates, template_of_env=template_of_env)
            idx = torch.from_numpy(template_of_env).to(dev)
            assert idx.numel() == self.n_envs and int(idx.max()) < len(costmaps) == len(paths)
            pick = lambda t: t[idx]   # noqa: E731
        data, shapes, origins, res = stack_costmaps(costmaps, self._map_storage)
        shape = pick(torch.from_numpy(shapes).to(dev))
        self._map_host = entries(costmaps)
        self.set_costmap_tensors(pick(torch.from_numpy(data).to(dev)).contiguous(),
                                 pick(torch.from_numpy(origins).to(dev)).contiguous(), res,
                                 shape[:, 0].contiguous(), shape[:, 1].contiguous())
        points, lens, refined = stack_paths(paths, self._refine())
        self._path_host, self._shared_path = entries(refined), False
        self._bind_paths(pick(torch.from_numpy(points).to(dev)).contiguous(), pick(torch.from_numpy(lens).to(dev)).contiguous())

    def _bind_paths(self, points, lens):
        """Device paths [., max_len, 3] of lens [.] points each; lens None: ONE path [len, 3] shared by all envs.  Every
        binding counts (self._path_epoch): what was derived from an earlier one -- a SpeedProfile -- is stale."""
        self._keep.update(path=points, lens=lens)
        self._path_epoch += 1
        _lib.check(self._lib.bcp_set_paths(self._h, points.data_ptr(), lens.data_ptr() if lens is not None else None,
                                           int(points.shape[-2]), int(lens is None), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # a staging tensor may now be released

    def set_costmap_tensors(self, data, origins, resolution, valid_rows=None, valid_cols=None):
        """Private costmaps straight from device tensors: data uint8 [N, rows, cols], origins float64 [N, 2]
        (N = pool entries in geometry-pool mode)."""
        n = self.n_envs if self.geom_of_env is None else data.shape[0]
        assert data.dtype == torch.uint8 and data.dim() == 3 and data.shape[0] == n and data.is_contiguous()
        assert origins.dtype == torch.float64 and tuple(origins.shape) == (n, 2) and origins.is_contiguous()
        self._keep.update(map=data, origins=origins, vr=valid_rows, vc=valid_cols)
        self._shared_map = False
        self.resolution = float(resolution)
        _lib.check(self._lib.bcp_set_costmaps(
            self._h, data.data_ptr(), data.shape[1], data.shape[2], 0,
            valid_rows.data_ptr() if valid_rows is not None else None,
            valid_cols.data_ptr() if valid_cols is not None else None, origins.data_ptr(), 1, float(resolution),
            self._stream()))

    def _rebind_costmaps(self):
        """Binds the maps of self._keep["map"] again, with the arguments of the original binding: after an edit of the maps
        on the device, so that everything the library derives from them is rebuilt."""
        data = self._keep["map"]
        if self._shared_map:
            _lib.check(self._lib.bcp_set_costmaps(self._h, data.data_ptr(), data.shape[0], data.shape[1], 1, None, None,
                                                  self._origin_host.ctypes.data, 0, float(self.resolution), self._stream()))
        else:
            self.set_costmap_tensors(data, self._keep["origins"], self.resolution, self._keep.get("vr"), self._keep.get("vc"))

    def _bound_maps(self):
        """(maps uint8 [entries, rows, cols], valid_rows, valid_cols, shared): the bound maps as entries, a shared map as one."""
        if self._shared_map:
            return self._keep["map"][None], None, None, True
        return self._keep["map"], self._keep.get("vr"), self._keep.get("vc"), False

    def _bound_origins(self):
        """float64 device tensor [entries, 2], [1, 2] for a shared map: the origins of the bound maps."""
        if self._shared_map:
            return torch.tensor(self._origin_host, device=self.device)[None]
        return self._keep["origins"]

    _costmaps = property(lambda self: self._map_host.items, doc="the host costmaps as stored (HostEntries.items)")
    _paths = property(lambda self: self._path_host.items, doc="the host paths, refined, as stored (HostEntries.items)")

    @property
    def costmap_tensor(self):
        """The device costmap(s) the library reads: uint8 [rows, cols] (shared) or [entries, rows, cols] (private maps,
        pool entries), padded to one shape where the entries differ."""
        return self._keep["map"]

    def _inflate(self, maps, vr, vc, radius, cost_scaling_factor, out):
        _lib.check(self._lib.bcp_inflate_costmaps(
            self._h, maps.data_ptr(), maps.shape[0], maps.shape[1], maps.shape[2],
            vr.data_ptr() if vr is not None else None, vc.data_ptr() if vc is not None else None, float(self.resolution),
            float(radius), float(cost_scaling_factor), out.data_ptr(), None, self._stream()))

    def inflate_costmaps(self, cost_scaling_factor, footprint=None):
        """inflate_costmap (utilities/costmap_inflation.py:73-92) applied, in place and on the device, to every costmap
        this env has bound -- the shared map, the private maps, or the entries of a geometry pool within their valid
        shapes -- followed by a re-bind with the arguments of the original one, so that everything derived from the maps
        (the egocentric cell lists among it) is rebuilt.  Exactly the lethal cells stay 254, so the env steps bit for bit
        as before; the egocentric observations and every per-env Observation.costmap show the inflated costs.
        `footprint` [k, 2] gives the inscribed radius (robots.inscribed_radius); None = the env's own footprint.
        A pool that lives on the device (sampler="device_resident") is inflated where it is: whoever else holds that pool
        sees the inflated entries.  Refused on endless=True pools (refresh() would write raw worlds into the inflated
        pool; inflating re-sampled worlds is not implemented), and when called a second time."""
        if self.endless:
            raise RuntimeError("inflate_costmaps: not supported on endless=True pools -- refresh() re-samples raw worlds "
                               "into the pool, and inflating re-sampled worlds is out of scope")
        if self._inflated:
            raise RuntimeError("inflate_costmaps: the costmaps of this env are inflated already")
        radius = robots.inscribed_radius(self.footprint() if footprint is None else footprint)
        maps, vr, vc, _shared = self._bound_maps()
        self._inflate(maps, vr, vc, radius, cost_scaling_factor, maps)
        self._rebind_costmaps()
        # the host copies behind envs[i].get_state().costmap (a device pool hands out copies of its tensors on demand):
        # inflated as they are stored, templates once each
        if self._device_pool is None:
            host = list(self._costmaps)
            stack, shapes, _, _ = stack_costmaps(host)
            dev_stack = torch.from_numpy(stack).to(self.device)
            self._inflate(dev_stack, self._device_tensor(shapes[:, 0], torch.int32),
                          self._device_tensor(shapes[:, 1], torch.int32), radius, cost_scaling_factor, dev_stack)
            inflated = dev_stack.cpu().numpy()
            self._map_host.replace_stored([CostMap2D(inflated[k, :s[0], :s[1]].copy(), c.get_resolution(), c.get_origin())
                                           for k, (c, s) in enumerate(zip(host, shapes))])
        torch.cuda.current_stream(self.device).synchronize()
        self._inflated = True

    def _set_paths(self, path):
        self._shared_path = isinstance(path, np.ndarray) and path.ndim == 2
        points, lens, refined = stack_paths([path] if self._shared_path else path, self._refine())
        self._path_host = HostEntries.shared(refined[0]) if self._shared_path else HostEntries.per_env(refined)
        if self._shared_path:
            self._bind_paths(torch.from_numpy(points[0]).to(self.device), None)
        else:
            if len(refined) != self.n_envs:
                raise ValueError("need one path per env (%d), got %d" % (self.n_envs, len(refined)))
            self._bind_paths(torch.from_numpy(points).to(self.device), torch.from_numpy(lens).to(self.device))

    def _make_initial_state(self):
        """make_initial_state (env.py:179-214): pose = path[0], v = w = 0, wheel at initial_wheel_angle... the
        reference's TricycleRobotState() default wheel angle is 0.0 and PlanEnv never applies
        params.initial_wheel_angle to it, so neither do we."""
        dev, dp = self.device, self._device_pool
        n = self.n_envs if self.geom_of_env is None else len(self._paths)
        if dp is not None:   # initial states computed on the device with the paths (bcp_mini_world_paths)
            robot_t = torch.zeros(7, n, dtype=torch.float64, device=dev)
            robot_t[0:3] = dp.path_points[:, 0, :].t()
            return BatchedState(robot_t, dp.init[:, 0].contiguous(), dp.init[:, 1].to(torch.int32).contiguous(),
                                torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
        # one initial state per stored path, then per env (per entry with a geometry pool) the one of its path
        per = [self._first_reward_state(p, self.params.reward_provider_params) for p in self._paths]
        of = np.zeros(n, dtype=np.int64) if self._shared_path else self._path_host.index()
        robot = np.zeros((7, n), dtype=np.float64)
        robot[0:3] = np.stack([p[0] for p in self._paths])[of].T
        md = np.array([m for m, _ in per], dtype=np.float64)[of]
        ti = np.array([t for _, t in per], dtype=np.int32)[of]
        return BatchedState(torch.from_numpy(robot).to(dev), torch.from_numpy(md).to(dev), torch.from_numpy(ti).to(dev),
                            torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))

    def _first_reward_state(self, path, reward_params):
        if self._pure_pursuit:
            return host_init.initial_pure_pursuit_state(path)
        return host_init.initial_reward_state(path, reward_params)

    @classmethod
    def deserialize(cls, records, **kw):
        """PlanEnv.deserialize (env.py:263-276), batched: one env per record of `EnvView.serialize()` (or of the
        reference's `PlanEnv.serialize()`), each with its own costmap and path; the parametrisation is the first
        record's (they must agree).  Extra keyword arguments go to the constructor (device, seed, auto_reset, ...)."""
        records = [dict(r) for r in records]
        for r in records:
            assert r.pop('version') == EnvView.VERSION
        params = EnvParams.deserialize(records[0]['params'])
        if any(EnvParams.deserialize(r['params']) != params for r in records[1:]):
            raise ValueError("all envs of a batch share one EnvParams")
        costmaps = [CostMap2D.from_state(r['costmap']) for r in records]
        paths = [np.asarray(r['path'], dtype=np.float64) for r in records]
        # `path` is State.original_path, i.e. already refined: it is taken as it is.  (The reference's deserialize goes
        # through the constructor's refine_path once more -- a no-op except for segments within rounding of path_delta --
        # but then set_state puts the recorded path back anyway.)
        env = cls(costmaps, paths, attr.evolve(params, refine_path=False), n_envs=len(records), **kw)
        env.params = params
        for i, r in enumerate(records):
            env.envs[i].set_state(State.deserialize(r['state']))
        return env

    def distance_field(self, first=0, count=1):
        """The distance fields libbcplan pre-classifies poses with (bcp_get_distance_field), for `count` map entries
        from `first`: (uint8 device tensor [count, rows + 2 pad, cols + 2 pad], pad, clamp)."""
        shape = (C.c_int32 * 4)()
        _lib.check(self._lib.bcp_get_distance_field(self._h, 0, 0, None, shape, None))
        out = torch.empty((int(count), shape[0], shape[1]), dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.bcp_get_distance_field(self._h, int(first), int(count), out.data_ptr(), shape, self._stream()))
        return out, int(shape[2]), int(shape[3])

    def near_field(self, first=0, count=1, raw=False):
        """The 1-bit form of the distance fields the step's outer test reads (bcp_get_near_field), unpacked:
        (bool device tensor [count, rows + 2 pad, cols + 2 pad] -- True where the field is < t_out --, t_out);
        raw: the tile words themselves, int32 [count, tile rows, tile columns, 32]."""
        shape = (C.c_int32 * 3)()
        _lib.check(self._lib.bcp_get_near_field(self._h, 0, 0, None, shape, None))
        ty, tx, t_out = int(shape[0]), int(shape[1]), int(shape[2])
        words = torch.empty((int(count), ty, tx, 32), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.bcp_get_near_field(self._h, int(first), int(count), words.data_ptr(), shape, self._stream()))
        dshape = (C.c_int32 * 4)()
        _lib.check(self._lib.bcp_get_distance_field(self._h, 0, 0, None, dshape, None))
        bits = (words.unsqueeze(-1) >> torch.arange(32, device=self.device, dtype=torch.int32)) & 1   # [count, ty, tx, 32 rows, 32 bits]
        cells = bits.permute(0, 1, 3, 2, 4).reshape(int(count), ty * 32, tx * 32)
        if raw:
            return words, t_out
        return cells[:, :dshape[0], :dshape[1]].bool(), t_out

    # ------------------------------------------------------------------ per-env lookups
    def _entry_of(self, i):
        return None if self.geom_of_env is None else int(self.geom_of_env[i])

    def path_of(self, i):
        return self._path_host.of_env(i, self._entry_of(i))

    def costmap_of(self, i):
        return self._map_host.of_env(i, self._entry_of(i))

    def time_of(self, current_iter):
        """Observation.time for iteration counters (device tensor): dt accumulated current_iter times."""
        idx = current_iter.to(torch.int64)
        top = int(idx.max()) if idx.numel() else 0
        if top >= len(self.time_table):  # envs stepped past the timeout without a reset: grow the table
            self.time_table = host_init.time_table(self.params.dt, 2 * top)
            self._time_table_dev = torch.from_numpy(self.time_table).to(self.device)
        return self._time_table_dev[idx]

    # ------------------------------------------------------------------ reference API
    def reset(self, mask=None):
        """PlanEnv.reset for all envs, or for those with mask[i] != 0 (uint8/bool device tensor)."""
        ptr = None
        if mask is not None:
            mask = mask.to(self.device).to(torch.uint8).contiguous()
            ptr = mask.data_ptr()
        _lib.check(self._lib.bcp_reset_masked(self._h, ptr, self._stream()))
        return self._obs

    def get_state(self):
        """Snapshot of every env's state (device tensors); with a geometry pool the entries the envs are on ride
        along as `.geom_of_env`."""
        snap = self.state.copy()
        snap.geom_of_env = self.geom_of_env.clone() if self.geom_of_env is not None else None
        return snap

    def set_state(self, state):
        s = self.state
        s.robot.copy_(state.robot)
        s.min_spat_dist_so_far.copy_(state.min_spat_dist_so_far)
        s.target_idx.copy_(state.target_idx)
        s.current_iter.copy_(state.current_iter)
        s.robot_collided.copy_(state.robot_collided)
        for name in BatchedState.DELAY_FIELDS:
            if getattr(s, name) is not None:
                getattr(s, name).copy_(getattr(state, name))
        if self.geom_of_env is not None and getattr(state, "geom_of_env", None) is not None:
            self.geom_of_env.copy_(state.geom_of_env)

    def fan_out(self, src, mask=None):
        """Monte-Carlo fan-out (reference README, 'Statefullness of the env'): every env (or those with mask[i] != 0)
        takes over env `src`'s complete state -- the batched `s = env.get_state(); others.set_state(s)`."""
        ptr = None
        if mask is not None:
            mask = mask.to(self.device).to(torch.uint8).contiguous()
            ptr = mask.data_ptr()
        _lib.check(self._lib.bcp_broadcast_state(self._h, int(src), ptr, self._stream()))
        self._alive["fan_out"] = (mask,)   # keep the mask alive until the stream has consumed it

    def step(self, actions, noise_z=None, noise_z_out=None, done_out=None):
        """One tick for every env.  actions: [N,2] (float32 or float64) tensor / array, or a list of Action.
        noise_z: optional [N,3] float64 standard normals (slot order) replacing the on-device RNG.
        done_out: optional uint8 [N] device tensor that receives the done mask instead of `self.done` (e.g. a row of
        a ring buffer that is all-gathered every few steps).
        Returns (BatchedObservation, reward float64[N], done uint8[N], info) -- device tensors, no sync; info is {} or,
        with enable_episode_record(), {"episode_ends": EpisodeEnds}."""
        # fast path: a device tensor of the right shape and dtype goes straight to the library
        if not (isinstance(actions, torch.Tensor) and actions.device == self.device and actions.is_contiguous()
                and actions.dtype in (torch.float32, torch.float64) and tuple(actions.shape) == (self.n_envs, 2)):
            actions = _as_device_actions(actions, self.n_envs, self.device)
        io = self._io
        io.actions = actions.data_ptr()
        flags = self._flags_f32 if actions.dtype == torch.float32 else self._flags_f64
        z = None
        if noise_z is not None:
            z = noise_z if isinstance(noise_z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(noise_z))
            z = z.to(self.device, torch.float64).contiguous()
            assert tuple(z.shape) == (self.n_envs, 3)
            io.noise_z = z.data_ptr()
        else:
            io.noise_z = None
        if noise_z_out is not None:
            assert noise_z_out.dtype == torch.float64 and tuple(noise_z_out.shape) == (self.n_envs, 3)
            io.noise_z_out = noise_z_out.data_ptr()
        else:
            io.noise_z_out = None
        done = self.done
        if done_out is not None:
            assert done_out.dtype == torch.uint8 and done_out.numel() == self.n_envs and done_out.is_contiguous()
            done = done_out
        io.done = done.data_ptr()
        rc = self._bcp_step(self._h, self._io_ref, flags, torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            _lib.check(rc)
        self._alive["step"] = (actions, z, done)  # keep inputs alive until the stream has consumed them
        return self._obs, self.reward, done, self._info

    def _cached_outputs(self, cache, key, shapes, names, limit=None):
        """{name: zero-initialised device buffer of shapes[name] = (shape, dtype)}, made on first use and kept in
        cache[key] -- a planner that calls every tick allocates nothing."""
        buf = cached(cache, key, dict, limit)
        out = {}
        for name in names:
            shape, dtype = shapes[name]
            if (name, dtype) not in buf:
                buf[(name, dtype)] = torch.zeros(shape, dtype=dtype, device=self.device)
            out[name] = buf[(name, dtype)]
        return out

    def rollout(self, actions, noise_z=None, noise_z_out=None, collided_out=None, err_out=None):
        """K ticks for every env in one library call (bcp_rollout): actions [K, N, 2] float32 / float64 on the device (or
        anything torch can put there).  Returns (reward float64 [K, N], done uint8 [K, N]) device tensors, no sync; the
        state ends where K calls of step() with actions[k] would leave it, bit for bit (auto-reset and the on-device
        noise stream included).  noise_z / noise_z_out: optional [K, N, 3]; collided_out uint8 / err_out int32: optional
        [K, N] (without them the rows go to cached internal buffers).  Afterwards the per-step views show the last row --
        reward, done, collided_now -- except err, which is the OR over all K rows: check_errors() after a rollout raises
        for an env that any of the K steps flagged.  With the single-launch step form the K steps are ONE kernel launch --
        open-loop Monte-Carlo rollouts from one state (the reference's README) pay launch, argument fetch and staging once,
        and no workgroup waits for the chip's slowest one between steps."""
        actions = self._device_tensor(actions)
        k, n = int(actions.shape[0]), self.n_envs
        assert tuple(actions.shape) == (k, n, 2) and k >= 1
        io = _lib.BcpStepIO()
        io.actions = actions.data_ptr()
        flags = self._flags_f32 if actions.dtype == torch.float32 else self._flags_f64
        keep = [actions]
        if noise_z is not None:
            z = self._device_tensor(noise_z, torch.float64, (k, n, 3))
            io.noise_z = z.data_ptr()
            keep.append(z)
        if noise_z_out is not None:
            assert noise_z_out.dtype == torch.float64 and tuple(noise_z_out.shape) == (k, n, 3) and noise_z_out.is_contiguous()
            io.noise_z_out = noise_z_out.data_ptr()
        reward = torch.empty((k, n), dtype=torch.float64, device=self.device)
        done = torch.empty((k, n), dtype=torch.uint8, device=self.device)
        io.reward, io.done = reward.data_ptr(), done.data_ptr()
        if collided_out is not None:
            assert collided_out.dtype == torch.uint8 and tuple(collided_out.shape) == (k, n) and collided_out.is_contiguous()
        if err_out is not None:
            assert err_out.dtype == torch.int32 and tuple(err_out.shape) == (k, n) and err_out.is_contiguous()
        rows = self._cached_outputs(self._rollout_buffers, k, {"collided": ((k, n), torch.uint8), "err": ((k, n), torch.int32)},
                                    [name for name, given in (("collided", collided_out), ("err", err_out)) if given is None])
        collided_out = rows["collided"] if collided_out is None else collided_out
        err_out = rows["err"] if err_out is None else err_out
        io.collided_now, io.err = collided_out.data_ptr(), err_out.data_ptr()
        _lib.check(self._lib.bcp_rollout(self._h, C.byref(io), k, flags, self._stream()))
        # the per-step views of step() show the last row; err holds every bit that any of the K rows holds
        self.reward.copy_(reward[-1])
        self.done.copy_(done[-1])
        self.collided_now.copy_(collided_out[-1])
        self.err.zero_()
        for bit in (_lib.ERR_ANGLE_JUMP, _lib.ERR_TIME_ORDER, _lib.ERR_INTERNAL):
            self.err |= (err_out & bit).amax(dim=0)
        self._alive["rollout"] = tuple(keep)
        return reward, done

    def lookahead(self, actions, noise_z=None, mask=None, want=("final_pose", "best")):
        """Score K candidate action sequences for every env over the next H steps WITHOUT stepping it (bcp_lookahead):
        nothing of the env changes -- state, pool entries, noise stream, episode record.  actions: [H, K, 2] = one
        candidate library shared by all envs, or [H, N, K, 2] = candidates per env; float32 or float64.  noise_z: None =
        the noise-free forward model (whatever the env's noise setting), or [H, N, K, 3] standard normals.  mask:
        optional [N]; rows of envs with mask 0 keep what the cached buffers held.  want: optional outputs to compute, from
        "final_pose", "final_target_idx", "err", "best", "best_action" ("best_action" implies "best").  Each candidate
        stops after its first done step (no auto-reset).  Returns a Lookahead of device tensors, no sync; the buffers are
        cached per (H, K), so a planner that calls this every tick allocates nothing.  Delays > 0 are refused."""
        actions = self._device_tensor(actions)
        n = self.n_envs
        if actions.dim() == 3 and actions.shape[2] == 2:
            flags = 0
        elif actions.dim() == 4 and actions.shape[1] == n and actions.shape[3] == 2:
            flags = _lib.LOOKAHEAD_PER_ENV
        else:
            raise ValueError("actions must have shape (H, K, 2) or (H, %d, K, 2), got %s" % (n, tuple(actions.shape)))
        h, k = int(actions.shape[0]), int(actions.shape[-2])
        if actions.dtype == torch.float32:
            flags |= _lib.STEP_ACTIONS_F32
        want = set(want)
        unknown = want - set(Lookahead.FIELDS[3:])
        if unknown:
            raise ValueError("lookahead: unknown outputs %s" % sorted(unknown))
        if "best_action" in want:
            want.add("best")
        shapes = {"ret": ((n, k), torch.float64), "steps": ((n, k), torch.int32), "reason": ((n, k), torch.uint8),
                  "final_pose": ((n, k, 3), torch.float64), "final_target_idx": ((n, k), torch.int32),
                  "err": ((n, k), torch.int32), "best": ((n,), torch.int32), "best_action": ((n, 2), actions.dtype)}
        io = _lib.BcpLookaheadIO()
        io.actions, io.horizon, io.n_candidates = actions.data_ptr(), h, k
        keep = [actions]
        if noise_z is not None:
            z = self._device_tensor(noise_z, torch.float64, (h, n, k, 3))
            io.noise_z = z.data_ptr()
            keep.append(z)
        if mask is not None:
            mask = self._device_tensor(mask, torch.uint8, (n,))
            io.mask = mask.data_ptr()
            keep.append(mask)
        out = self._cached_outputs(self._lookahead_buffers, (h, k), shapes,
                                   [name for name in Lookahead.FIELDS if name in want or name in Lookahead.FIELDS[:3]])
        for name, t in out.items():
            setattr(io, name, t.data_ptr())
        _lib.check(self._lib.bcp_lookahead(self._h, C.byref(io), flags, self._stream()))
        self._alive["lookahead"] = tuple(keep)   # alive until the stream has consumed them
        return Lookahead(h, k, **out)

    def mppi(self, mean, sigma, iterations, n_candidates, lam, collision_penalty, seed=0, draw_index=0, mask=None, eps=None,
             want=(), action_dtype=None, goal_field=None, terminal_weight=0.0, adapt=None):
        """Refine one plan per env by sampling around it (bcp_mppi, one kernel launch, nothing of the env changes): for each
        of `iterations` rounds, n_candidates plans u = clip(mean + sigma * eps, action box) -- candidate 0 is the mean itself
        -- are rolled out with the noise-free forward model as lookahead() rolls them out, scored ret - collision_penalty *
        collided, and the mean becomes their average under the weights softmax(score / lam).
        mean: [N, H, 2]; a contiguous float64 tensor on the env's device is refined IN PLACE (and returned), anything else
        is copied first.  sigma: two standard deviations (v, w).  n_candidates: a power of two in [8, 1024].  seed,
        draw_index: the perturbation stream (the env's own noise stream is not involved); draw_index may be a one-element
        int64 / uint64 tensor on the device, read by the kernel -- a captured call then draws afresh on every replay once the
        word was changed.  eps: optional [I, N, K, H, 2] float32 perturbations to use instead (replay).  mask: optional [N];
        rows of envs with mask 0 are left untouched.  want: from "eps", "iter_mean", "iter_ret", "iter_reason", "err".
        action_dtype: torch.float64 (default) or torch.float32.  goal_field: a goal_field.GoalField of this env
        (self.goal_field()): the score of a candidate then also loses terminal_weight (reward per metre, finite, >= 0) times
        the distance to go from its final pose through free space, read from the field inside the same launch
        (bcp_mppi_field); a pose without a route counts as GOAL_FAR cells.  want then also takes "iter_value" (int32
        [I, N, K], the field value read, GOAL_NONE = none) and "iter_score" (float64 [I, N, K], the scores as weighted).
        Without a field the call is bcp_mppi as ever.
        adapt: None, or a dict(sigma=, rate=, sigma_min=, sigma_max=) -- the sampling widths then follow the weights
        (bcp_mppi_adapt, the same launch).  sigma: [N, H, 2], a width per env, step and component in place of the two of
        `sigma` (which is still checked); a contiguous float64 tensor on the env's device is refined IN PLACE, as `mean` is.
        Every iteration moves a width by `rate` (in [0, 1]) of the way to the weighted standard deviation of its commands
        about the new mean, inside [sigma_min, sigma_max] (two values each).  want then also takes "iter_sigma" (float64
        [I, N, H, 2], the widths going into each iteration), and the result carries `sigma`.
        Returns an Mppi; buffers are cached per (H, K, I).  Delays > 0 are refused."""
        n = self.n_envs
        mean = self._device_tensor(mean, torch.float64)   # (a contiguous float64 tensor on the device: itself)
        if mean.dim() != 3 or mean.shape[0] != n or mean.shape[2] != 2:
            raise ValueError("mean must have shape (%d, H, 2), got %s" % (n, tuple(mean.shape)))
        h, k, it = int(mean.shape[1]), int(n_candidates), int(iterations)
        want = set(want)
        unknown = want - set(Mppi.FIELDS)
        if unknown:
            raise ValueError("mppi: unknown outputs %s" % sorted(unknown))
        if goal_field is None and (want & set(Mppi.TERMINAL_FIELDS) or terminal_weight != 0.0):
            raise ValueError("mppi: iter_value / iter_score / terminal_weight need a goal_field")
        if goal_field is not None and goal_field.owner is not self:
            raise ValueError("mppi: goal_field belongs to another env")
        if adapt is None and "iter_sigma" in want:
            raise ValueError("mppi: iter_sigma needs adapt")
        widths = None
        if adapt is not None:
            if set(adapt) != {"sigma", "rate", "sigma_min", "sigma_max"}:
                raise ValueError("mppi: adapt takes exactly sigma, rate, sigma_min and sigma_max, got %s" % sorted(adapt))
            widths = self._device_tensor(adapt["sigma"], torch.float64)   # (as for mean: itself where it can be)
            if tuple(widths.shape) != tuple(mean.shape):
                raise ValueError("adapt['sigma'] must have shape %s, got %s" % (tuple(mean.shape), tuple(widths.shape)))
        action_dtype = torch.float64 if action_dtype is None else action_dtype
        if action_dtype not in (torch.float32, torch.float64):
            raise ValueError("action_dtype must be torch.float32 or torch.float64")
        p = _lib.BcpMppiParams()
        p.horizon, p.n_candidates, p.iterations = h, k, it
        sigma = np.asarray(sigma, dtype=np.float64).reshape(2)
        low, high = (np.asarray(b, dtype=np.float64).reshape(2) for b in (self.action_space.low, self.action_space.high))
        for d in range(2):
            p.sigma[d], p.low[d], p.high[d] = sigma[d], low[d], high[d]
        p.lambda_, p.collision_penalty, p.seed = float(lam), float(collision_penalty), int(seed) & (2 ** 64 - 1)
        io = _lib.BcpMppiIO()
        io.mean = mean.data_ptr()
        keep = [mean]
        if isinstance(draw_index, torch.Tensor):
            assert draw_index.numel() == 1 and draw_index.dtype in (torch.int64, torch.uint64) and draw_index.is_cuda
            io.draw_index = draw_index.data_ptr()
            keep.append(draw_index)
        else:
            p.draw_index = int(draw_index) & (2 ** 64 - 1)
        if mask is not None:
            mask = self._device_tensor(mask, torch.uint8, (n,))
            io.mask = mask.data_ptr()
            keep.append(mask)
        if eps is not None:
            eps = self._device_tensor(eps, torch.float32)
            if tuple(eps.shape) != (it, n, k, h, 2):
                raise ValueError("eps must have shape %s, got %s" % ((it, n, k, h, 2), tuple(eps.shape)))
            io.eps_in = eps.data_ptr()
            keep.append(eps)
        shapes = {"action": ((n, 2), action_dtype), "eps": ((it, n, k, h, 2), torch.float32),
                  "iter_mean": ((it, n, h, 2), torch.float64), "iter_ret": ((it, n, k), torch.float64),
                  "iter_reason": ((it, n, k), torch.uint8), "err": ((n,), torch.int32),
                  "iter_value": ((it, n, k), torch.int32), "iter_score": ((it, n, k), torch.float64),
                  "iter_sigma": ((it, n, h, 2), torch.float64)}
        out = self._cached_outputs(self._mppi_buffers, (h, k, it), shapes,
                                   ["action"] + [name for name in Mppi.FIELDS if name in want])
        term, ad = _lib.BcpMppiTerminal(), _lib.BcpMppiWidths()
        for name, t in out.items():
            owner = term if name in Mppi.TERMINAL_FIELDS else ad if name == "iter_sigma" else io
            setattr(owner, "eps_out" if name == "eps" else name, t.data_ptr())
        flags = _lib.STEP_ACTIONS_F32 if action_dtype == torch.float32 else 0
        if goal_field is not None:
            f = goal_field.field
            term.field, term.n_fields, term.rows, term.cols = f.data_ptr(), int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
            term.weight = float(terminal_weight)
            keep.append(f)
        if adapt is not None:
            ad.sigma, ad.rate = widths.data_ptr(), float(adapt["rate"])
            lo, hi = (np.asarray(adapt[name], dtype=np.float64).reshape(2) for name in ("sigma_min", "sigma_max"))
            for d in range(2):
                ad.sigma_min[d], ad.sigma_max[d] = lo[d], hi[d]
            keep.append(widths)
            _lib.check(self._lib.bcp_mppi_adapt(self._h, C.byref(p), C.byref(io), C.byref(ad),
                                                None if goal_field is None else C.byref(term), flags, self._stream()))
        elif goal_field is None:
            _lib.check(self._lib.bcp_mppi(self._h, C.byref(p), C.byref(io), flags, self._stream()))
        else:
            _lib.check(self._lib.bcp_mppi_field(self._h, C.byref(p), C.byref(io), C.byref(term), flags, self._stream()))
        self._alive["mppi"] = tuple(keep)   # alive until the stream has consumed them
        return Mppi(h, k, it, mean, sigma=widths, **out)

    def default_max_curvature(self):
        """The curvature clamp track() uses when none is given: what the robot can turn -- tan(max_front_wheel_angle) /
        front_wheel_from_axis for the tricycle, high[1] / max(low[0], 1e-3) of the action box for the diff-drive."""
        if self.is_tricycle:
            p = self._bcp_params
            return float(np.tan(p.max_front_wheel_angle) / p.front_wheel_from_axis)
        low, high = np.asarray(self.action_space.low, np.float64), np.asarray(self.action_space.high, np.float64)
        return float(high[1] / max(low[0], 1e-3))

    def speed_profile(self, v_max=None, a_lat=1.0, w_max=1.0, a_dec=1.0, a_acc=1.0, v_start=None, v_end=None, v_min=0.0, span=1,
                      want=()):
        """The speed profile of the env's own bound paths (bcp_path_speed on the device copy the env keeps, one launch):
        Handle.path_speed's parameters, with v_max, v_start and v_end defaulting to action_space.high[0].  Returns a
        SpeedProfile with speed [entries, max_len] ([max_len] for a shared path) for track(speed_profile=...) and
        TrackingPlanner(speed_profile=...); it belongs to this binding of the paths -- after route_paths() make a new one.
        Refused on endless=True pools (refresh() re-samples paths into the pool, which would leave a stale profile), and by
        the library for paths of more than 4096 slots."""
        if self.endless:
            raise RuntimeError("speed_profile: not supported on endless=True pools -- refresh() re-samples paths into the "
                               "pool, which would leave a stale profile")
        from . import speed_profile
        top = float(np.asarray(self.action_space.high, np.float64)[0])
        v_max = top if v_max is None else v_max
        prm = speed_profile.speed_params(v_max, a_lat, w_max, a_dec, a_acc, top if v_start is None else v_start,
                                         top if v_end is None else v_end, v_min, span)
        paths, lens = self._keep["path"], self._keep["lens"]
        if lens is None:   # the shared path: one row
            paths = paths[None]
            lens = torch.full((1,), int(paths.shape[1]), dtype=torch.int32, device=self.device)
        out = speed_profile.path_speed(self, paths, lens, prm, want, owner=self, epoch=self._path_epoch)
        if self._keep["lens"] is None:
            out.speed, out.kappa, out.v_limit = (None if t is None else t[0] for t in (out.speed, out.kappa, out.v_limit))
        return out

    def _checked_profile(self, profile):
        """The speeds of a SpeedProfile track() may read: made for the paths bound now, one row per bound path."""
        if profile.owner is not None and (profile.owner is not self or profile.epoch != self._path_epoch):
            raise ValueError("track: the speed profile was made for another env or an earlier binding of the paths (binding "
                             "%s, now %d) -- make a new one with speed_profile()" % (profile.epoch, self._path_epoch))
        bound = self._keep["path"]
        shape = (int(bound.shape[-2]),) if self._keep["lens"] is None else (int(bound.shape[0]), int(bound.shape[1]))
        if profile.max_len != shape[-1]:
            raise ValueError("track: the speed profile has max_len %d, the bound paths %d" % (profile.max_len, shape[-1]))
        speed = profile.speed
        if tuple(speed.shape) != shape or speed.dtype != torch.float64 or speed.device != self.device or not speed.is_contiguous():
            raise ValueError("track: the speed profile must be a contiguous float64 tensor %s on %s, got %s"
                             % (shape, self.device, tuple(speed.shape)))
        return speed

    def track(self, gains, horizon, max_curvature=None, mask=None, want=(), action_dtype=None, speed_profile=None):
        """Roll a pure-pursuit path tracker out for every env under K gain settings over the next `horizon` steps WITHOUT
        stepping it (bcp_track, nothing of the env changes): every trip's command steers for the first way point at least
        `reach` ahead at `speed`, through the reference's diff_drive_control_to_tricycle for the tricycle, clipped to the
        action box; the trips are lookahead()'s (noise-free forward model, stop after the first done step).
        gains: [K, 2] (speed, reach) shared by all envs, or [N, K, 2] per env; a setting that is not finite, with
        speed < 0 or reach <= 0 takes no trip (steps 0, zeros) and comes last in `best`.  max_curvature: the clamp of the
        arc's curvature in 1/m, None: default_max_curvature().  mask: optional [N]; rows of envs with mask 0 keep what the
        cached buffers held.  want: optional outputs from "final_pose", "final_target_idx", "err", "trace", "best",
        "best_plan", "best_action" (the last two imply "best").  action_dtype: of best_action, torch.float64 (default) or
        torch.float32.  speed_profile: None, or a SpeedProfile of the paths bound now (speed_profile()): every command's
        speed is then the gain's capped by the profile at the way point the robot heads for and at the carrot
        (bcp_track_profile); one made for an earlier binding of the paths or with another max_len is a ValueError.  A
        SpeedProfile built by hand or by path_speed() (owner None) is checked for its shape alone: it is the caller's to
        renew after route_paths().
        Returns a Track of device tensors, no sync; buffers are cached per (H, K).  Delays > 0 and the pure-pursuit reward
        provider are refused."""
        gains = self._device_tensor(gains, torch.float64)
        n, h = self.n_envs, int(horizon)
        if gains.dim() == 2 and gains.shape[1] == 2:
            flags = 0
        elif gains.dim() == 3 and gains.shape[0] == n and gains.shape[2] == 2:
            flags = _lib.LOOKAHEAD_PER_ENV
        else:
            raise ValueError("gains must have shape (K, 2) or (%d, K, 2), got %s" % (n, tuple(gains.shape)))
        k = int(gains.shape[-2])
        want = set(want)
        unknown = want - set(Track.FIELDS[4:])
        if unknown:
            raise ValueError("track: unknown outputs %s" % sorted(unknown))
        if want & {"best_plan", "best_action"}:
            want.add("best")
        action_dtype = torch.float64 if action_dtype is None else action_dtype
        if action_dtype not in (torch.float32, torch.float64):
            raise ValueError("action_dtype must be torch.float32 or torch.float64")
        if action_dtype == torch.float32:
            flags |= _lib.STEP_ACTIONS_F32
        p = _lib.BcpTrackParams()
        p.horizon, p.n_candidates = h, k
        low, high = (np.asarray(b, dtype=np.float64).reshape(2) for b in (self.action_space.low, self.action_space.high))
        for d in range(2):
            p.low[d], p.high[d] = low[d], high[d]
        p.max_curvature = self.default_max_curvature() if max_curvature is None else float(max_curvature)
        shapes = {"actions": ((n, k, max(h, 0), 2), torch.float64), "ret": ((n, k), torch.float64),
                  "steps": ((n, k), torch.int32), "reason": ((n, k), torch.uint8), "final_pose": ((n, k, 3), torch.float64),
                  "final_target_idx": ((n, k), torch.int32), "err": ((n, k), torch.int32),
                  "trace": ((n, k, max(h, 0), 6), torch.float64), "best": ((n,), torch.int32),
                  "best_plan": ((n, max(h, 0), 2), torch.float64), "best_action": ((n, 2), action_dtype)}
        io = _lib.BcpTrackIO()
        io.gains = gains.data_ptr()
        keep = [gains]
        if mask is not None:
            mask = self._device_tensor(mask, torch.uint8, (n,))
            io.mask = mask.data_ptr()
            keep.append(mask)
        out = self._cached_outputs(self._track_buffers, (h, k), shapes,
                                   [name for name in Track.FIELDS if name in want or name in Track.REQUIRED])
        for name, t in out.items():
            setattr(io, name, t.data_ptr())
        if speed_profile is None:
            _lib.check(self._lib.bcp_track(self._h, C.byref(p), C.byref(io), flags, self._stream()))
        else:
            prof = _lib.BcpTrackProfileIO()
            speed = self._checked_profile(speed_profile)
            prof.speed, prof.max_len = speed.data_ptr(), int(speed.shape[-1])
            keep.append(speed)
            _lib.check(self._lib.bcp_track_profile(self._h, C.byref(p), C.byref(io), C.byref(prof), flags, self._stream()))
        self._alive["track"] = tuple(keep)   # alive until the stream has consumed them
        return Track(h, k, **out)

    def _beam_table(self, beam_angles):
        """The device table [B, 2] of (cos, sin) of the beam angles (beam_table_cached)."""
        return beam_table_cached(self._beam_tables, beam_angles, self.device)

    def range_scan(self, beam_angles, max_range, poses=None, want=()):
        """A planar range scan per env (bcp_range_scan, one kernel launch, nothing of the env changes): the distance in
        metres from the robot to the nearest lethal cell along each beam, beam_angles [B] being the beams' angles from the
        robot's heading, counter-clockwise; max_range where nothing lethal lies within max_range.  Only cells that are 254
        inside a map's valid shape stop a ray -- the set pose_collides tests -- so inflated maps scan like raw ones.
        poses: None = every env's current pose (the delayed one under pose_delay), or [n, 3] (row i on the map of env
        i % n_envs).  want: optional outputs from "hit" (int32 [n, B]: row * cols + col of the cell that stopped the ray,
        -1 for none) and "heading_cs" (float64 [n, 2]: the cos / sin of the heading the walk used).  Returns ranges float32
        [n, B], or (ranges, *wanted in the order given), device tensors, no sync.  The (cos, sin) table of an angle set is
        uploaded once; the outputs are cached per (n, B), so a caller that scans every tick allocates nothing (both caches keep
        the SCAN_CACHE_ENTRIES most recently used entries)."""
        if poses is not None:
            poses = self._device_tensor(poses, torch.float64)
            assert poses.dim() == 2 and poses.shape[1] == 3
        return self._range_scan(poses, self.n_envs if poses is None else int(poses.shape[0]), beam_angles, max_range, want,
                                lambda n, b, shapes, names: self._cached_outputs(self._range_scan_buffers, (n, b), shapes,
                                                                                 names, SCAN_CACHE_ENTRIES))

    def _follow_goal_fields(self, fields):
        """Keep `fields` (a goal_field.GoalField built with follow_refresh=True) current across refresh(): by weak
        reference, so a field nobody holds any more costs nothing."""
        self._goal_followers.append(weakref.ref(fields))

    def goal_field(self, clearance=None, seeds="goal", max_passes=0, follow_refresh=False, cost_weight=None,
                   extra_of_cost=None):
        """The geodesic cost-to-go of every bound map to its path's goal (bcp_goal_field, one launch): for each free cell
        the length of the cheapest route through free space to the nearest seed, as a goal_field.GoalField whose sample()
        gives distance to go and route direction at any pose.  clearance: how far in metres a route keeps from every
        lethal cell; None = robots.inscribed_radius of the env's footprint (clearance_d2 = floor((clearance /
        resolution)^2): 151 for the tricycle at 0.03).  seeds: "goal" = the last way point of each entry's path, "path" =
        every way point (the field is then the distance to the path).  max_passes: 0 = as many as it takes.
        Fields: one for a shared map with a shared path, one per pool entry, one per env for private maps -- and one per env
        for a shared map with private paths, the one map read n_envs times: n_envs * rows * cols * 2 bytes of fields.
        Only cells == 254 are obstacles, so inflated maps give the same fields -- unless the costs are asked for:
        cost_weight=w (finite, >= 0) weighs the field by the inflation layer's costs (bcp_goal_field_cost with
        goal_field.cost_table(w): entering a cell of cost c costs the step plus rint(w * 12 * c / 252), so a cell of cost
        252 counts as 1 + w cells of travel).  Routes then run down the middle of free space where there is room and still
        squeeze through where there is not; `clearance` stays the hard limit.  Needs inflate_costmaps() first
        (RuntimeError otherwise).  extra_of_cost: the table itself, 256 integers in [0, _lib.GOAL_MAX_EXTRA] indexed by the
        map's byte, taken on any map.  Both together: ValueError; either with follow_refresh=True: ValueError.  The
        GoalField carries the table (extra_of_cost); its values are costs to go in metre-equivalents, and sample(),
        route(), route_paths(), mppi(goal_field=...) and the planners take it as they take a plain one.
        follow_refresh=True: the fields are built from the handle's own binding with the seeds derived on the device
        (bcp_goal_field_bound: private maps with private paths, seeds="goal" only -- ValueError otherwise; the same
        bytes).  On an endless=True pool the call first completes a refresh in flight (finish_refresh()), and from then
        on every refresh() rebuilds, behind the re-sampled worlds and in the same stream order, the fields of exactly the
        entries it re-sampled (bcp_refresh_goal_fields): the GoalField stays current for as long as it is alive.  With
        follow_refresh=False an endless=True pool is refused (RuntimeError): a refresh() would leave stale fields."""
        from . import goal_field
        return goal_field.build(self, clearance, seeds, max_passes, follow_refresh, cost_weight, extra_of_cost)

    def route_paths(self, fields=None, stride=2, max_len=None, clearance=None, cost_weight=None, smooth=None):
        """Replace every entry's path by the route traced down its goal field (bcp_goal_route_bound, one launch): from the
        entry's own start pose, through the centre of every stride-th cell of the cheapest route that keeps `clearance`
        from the walls, to its own goal pose -- a path a robot can follow, where the straight path of a pool world may
        cross a wall.  fields: a goal_field.GoalField of this env with one field per entry, None = built here
        (self.goal_field(clearance, cost_weight=cost_weight); clearance None = the footprint's inscribed radius;
        cost_weight as in goal_field(): the route of a weighted field keeps to the middle of free space, and needs
        inflate_costmaps() first -- scatter_obstacles(), then inflate_costmaps(), then route_paths(cost_weight=w)).
        max_len: the slots a route may take, None = the binding's; a route that needs more is ROUTE_LONG.
        Entries whose status is 0 get the routed path, its length and the reward provider's initial state on it; every
        other entry keeps what it had (merged on the device).  The paths and the initial state are bound again, path_of(i),
        the per-env views and a device pool's path_points / lens / init follow, and the call ends with reset().  While
        max_len does not exceed the binding's, the path and length tensors -- a device-resident pool's own -- are written
        in place; a larger max_len replaces them (the pool's attributes then name the new tensors).  Either way another
        env that holds the same device pool keeps stepping on what it bound (its derived path data and its initial
        states are its own) until it binds the pool again, while the pool's `paths` already show the routes.
        Starts and goals do not change: GoalFields of this env built before the call stay valid, and calling again
        changes nothing.  clearance and cost_weight only apply when the fields are built here: with `fields` either is a
        ValueError.
        smooth: None, or a dict of GoalField.smooth's parameters (look, blend, delta, halvings) and route_len (default
        1024): the route is then traced at stride 1 into a scratch buffer of route_len slots and smoothed
        (bcp_smooth_route: pulled taut, corners blended, a way point every delta metres) into max_len <= 4096 slots, and
        `stride` is not used.  An entry keeps its old path unless its route status and its smooth status are both 0,
        SMOOTH_BLOCKED aside; the returned status is the two OR-ed.
        Returns the int32 status [entries] (device tensor; _lib.ROUTE_* bits).
        Refused on endless=True pools (refresh() would write straight paths back), on a shared map or path, and on fields
        whose owner or shape is not this env's."""
        from . import goal_field
        return goal_field.route_paths(self, fields, stride, max_len, clearance, cost_weight, smooth)

    def scatter_obstacles(self, n_boxes, half_size, along=(0.2, 0.8), lateral=1.0, keep_clear=None, n_yaws=16, seed=0,
                          max_attempts=32, ensure_route=True, clearance=None):
        """Stamp up to n_boxes box obstacles into every entry's map, on the device and reproducibly (bcp_scatter_boxes, one
        launch): boxes with half sizes uniform in half_size = (lo, hi) metres and one of n_yaws yaws (multiples of
        2 pi / n_yaws), centred at start + t * (goal - start) + l * lateral * normal of the entry's bound path -- t uniform
        in `along`, l in (-1, 1), `lateral` in metres.  Entry m tries attempts 0 .. max_attempts - 1, drawn from
        (seed, m, attempt), and keeps the first n_boxes that stay inside its valid shape and clear of its start and goal
        cells by keep_clear metres (None = the footprint's circumscribed radius R; d2 = (ceil(R / resolution) + 1)^2 cells),
        so the start and goal poses of every entry stay collision-free.  Boxes may overlap walls and each other.
        ensure_route: a goal field is then built on the new maps at `clearance` (None = the footprint's inscribed radius, as
        in goal_field()); an entry whose start cell has no value -- its boxes cut the goal off -- gets its original map
        back, on the device, and SCATTER_REVERTED in its status.  SCATTER_SHORT marks counts < n_boxes.
        The maps are bound again with the arguments of the original binding, so that everything derived from them is
        rebuilt; the host copies behind envs[i].get_state().costmap follow, a pool that lives on the device is changed
        where it is (whoever else holds it sees the boxes), and the call ends with reset().  GoalFields of this env built
        before the call are stale: build them again.  Scatter first, then inflate_costmaps().
        Returns (status int32 [entries], counts int32 [entries], boxes int32 [entries, n_boxes, 9] = (attempt, four (x, y)
        corners in cells), zeros behind counts) -- device tensors; counts and boxes of a reverted entry say what had been
        placed.
        Refused on endless=True pools (refresh() would write bare worlds back), on a shared map or path, and on maps that
        are inflated already."""
        return boxes.scatter_obstacles(self, n_boxes, half_size, along, lateral, keep_clear, n_yaws, seed, max_attempts,
                                       ensure_route, clearance)

    def enable_episode_record(self, capacity=None):
        """Keep what every episode end leaves behind (bcp_bind_episode_record): from now on step() returns
        info = {"episode_ends": EpisodeEnds} -- why each env's episode ended, its final state before the auto-reset, its
        return and length, as device tensors the step kernel fills (no sync, no extra launch).  capacity: slots for envs
        that end in one step (default n_envs: never overflows).  Binding synchronises the device.  The running returns
        start at 0 here: bound in the middle of episodes, the first return of each env covers only the steps since.
        Returns the EpisodeEnds."""
        ends = EpisodeEnds(self, self.n_envs if capacity is None else capacity)
        rec = ends._c_struct()
        _lib.check(self._lib.bcp_bind_episode_record(self._h, C.byref(rec)))
        self.episode_ends = ends
        self._info = {"episode_ends": ends}
        return ends

    def disable_episode_record(self):
        """Unbind the episode record: step() returns info = {} again."""
        _lib.check(self._lib.bcp_bind_episode_record(self._h, None))
        self.episode_ends = None
        self._info = {}

    def check_errors(self):
        """Raise what the reference would have raised during the last step (synchronises); and a RuntimeError if a
        wait inside the step kernel ever gave up (bcp_expired_waits: a defect of the library, not of the data), or if the
        episode record had more episode ends in one step than slots since the last call."""
        if self.episode_ends is not None:
            steps = C.c_int64()
            _lib.check(self._lib.bcp_episode_record_overflows(self._h, C.byref(steps), self._stream()))
            if steps.value:
                raise RuntimeError("episode record: %d step(s) ended more episodes than its %d slots hold"
                                   % (steps.value, self.episode_ends.capacity))
        gave_up = C.c_int64()
        _lib.check(self._lib.bcp_expired_waits(self._h, C.byref(gave_up), self._stream()))
        if gave_up.value:
            raise RuntimeError("libbcplan: %d bounded wait(s) of the step kernel ran into their limit" % gave_up.value)
        bad = torch.nonzero(self.err & _lib.ERR_ANGLE_JUMP).flatten()
        if len(bad):
            raise Exception("Path has missing/corrupted angle data at env indices: %s" % bad.cpu().numpy())

    def geometry_digest(self):
        """Digest of the geometry this rank's envs share (distributed.geometry_digest): the costmap(s) and path(s) as they
        were given -- for distributed.check_same_geometry at set-up of a sharded job."""
        from . import distributed
        parts = []
        dp = self._device_pool
        if dp is not None:   # a pool that lives on the GPU: its first entries stand for it
            return distributed.geometry_digest(dp.maps[:16].cpu().numpy(), dp.origin, np.float64(dp.resolution),
                                               dp.path_points[:16].cpu().numpy(), dp.lens[:16].cpu().numpy())
        for cm in self._costmaps[:16]:
            parts += [cm.get_data(), np.asarray(cm.get_origin(), dtype=np.float64), np.float64(cm.get_resolution())]
        parts += [np.asarray(p, dtype=np.float64) for p in self._paths[:16]]
        return distributed.geometry_digest(*parts)

    def parked_poses(self):
        """Poses the single-launch step handed to the exact footprint test since the env was created (bcp_parked_poses;
        synchronises).  Measurement only."""
        count = C.c_int64()
        _lib.check(self._lib.bcp_parked_poses(self._h, C.byref(count), self._stream()))
        return int(count.value)

    def _timing_io(self, actions, noise_z):
        a = _as_device_actions(actions, self.n_envs, self.device)
        io = _lib.BcpStepIO()
        io.actions = a.data_ptr()
        flags = (_lib.STEP_ACTIONS_F32 if a.dtype == torch.float32 else 0) | (_lib.STEP_AUTO_RESET if self.auto_reset else 0)
        if noise_z is not None:
            io.noise_z = noise_z.data_ptr()
        io.reward, io.done = self.reward.data_ptr(), self.done.data_ptr()
        io.collided_now, io.err = self.collided_now.data_ptr(), self.err.data_ptr()
        return a, io, flags

    STEP_FORMS = {0: "step_kernel", 1: "step_fast_pair_kernel",
                  2: "step_fast_pair_kernel + step_pending_kernel (one step = these two launches)",
                  3: "step_local_kernel"}

    def step_kernels(self):
        """The kernels one step() launches as the handle is configured now (bcp_step_form)."""
        form = self._lib.bcp_step_form(self._h)
        if form < 0:
            _lib.check(form)
        return self.STEP_FORMS[form]

    def step_shared_variant(self):
        """True when the last step() ran step_local_kernel's shared-geometry variant (bcp_step_shared_variant)."""
        rc = self._lib.bcp_step_shared_variant(self._h)
        if rc < 0:
            _lib.check(rc)
        return rc == 1

    def time_steps(self, actions, steps, noise_z=None):
        """Average device time (ms) of one step over `steps` back-to-back steps, measured with HIP events on the
        launch stream."""
        a, io, flags = self._timing_io(actions, noise_z)
        ms = C.c_float()
        _lib.check(self._lib.bcp_time_steps(self._h, C.byref(io), flags, int(steps), self._stream(), C.byref(ms)))
        return ms.value

    def time_step_kernels(self, actions, steps, noise_z=None):
        """(step_kernel ms, step_pending_kernel ms): average launch durations, HIP events around each launch."""
        a, io, flags = self._timing_io(actions, noise_z)
        ms = (C.c_float * 2)()
        _lib.check(self._lib.bcp_time_step_kernels(self._h, C.byref(io), flags, int(steps), self._stream(), ms))
        return ms[0], ms[1]

    def render(self, mode='human'):
        raise NotImplementedError("rendering is out of scope of the batched step path")

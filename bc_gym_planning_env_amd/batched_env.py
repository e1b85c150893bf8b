"""BatchedPlanEnv: N PlanEnv instances advanced by one fused HIP kernel per step.

Mirrors the reference's object API (envs/base/env.py:217-439): reset() / step() / get_state() / set_state() /
seed() / action_space, batched over N envs, plus `envs[i]` views that hand back reference-shaped
Observation / State objects for one env.  Device tensors are torch tensors only because they cross the C ABI as
raw pointers (tensor.data_ptr()); all arithmetic happens in libbcplan.so.
"""
import ctypes as C
from collections import OrderedDict

import attr

import numpy as np
import torch

from . import _lib, host_init, robots
from .api import (Action, Box, CONTINUOUS_REWARD_PURE_PURSUIT, ContinuousRewardProviderState,
                  ContinuousRewardPurePursuitProviderState, CostMap2D, DiffdriveRobotState, EnvParams,
                  INDUSTRIAL_TRICYCLE_V1, Observation, State, TricycleRobotState)

_STATE_FIELDS = ("x", "y", "angle", "v", "w", "steering_motor_command", "wheel_angle")


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
        if self.origins is not None:
            return self.origins.to(device).contiguous()
        return torch.from_numpy(np.tile(self.origin, (len(self), 1))).to(device)

    @property
    def paths(self):
        return self._Lazy(len(self), lambda k: self.path_points[k, :int(self.lens[k])].cpu().numpy())


class BatchedState(object):
    """Snapshot of every env's mutable state (what PlanEnv.get_state() deep-copies, env.py:287-291)."""

    # with delays > 0 (EnvParams.pose_delay / state_delay / control_delay, env.py:27-49, 363-398): what State exposes
    # and the FIFO contents; `robot` is always the robot's TRUE state.  Element k pushed since the last reset lives
    # in slot (k - 1) % delay.
    DELAY_FIELDS = ("pose_seen", "robot_state_seen", "control_queue", "poses_queue", "robot_state_queue")

    def __init__(self, robot, min_spat_dist_so_far, target_idx, current_iter, robot_collided, pose_seen=None,
                 robot_state_seen=None, control_queue=None, poses_queue=None, robot_state_queue=None):
        self.robot = robot                      # float64 [7, N]: x, y, angle, v, w, steering_motor_command, wheel_angle
        self.min_spat_dist_so_far = min_spat_dist_so_far
        self.target_idx = target_idx
        self.current_iter = current_iter
        self.robot_collided = robot_collided
        self.pose_seen = pose_seen                      # [3, N] State.pose when pose_delay > 0
        self.robot_state_seen = robot_state_seen        # [7, N] State.robot_state when state_delay > 0
        self.control_queue = control_queue              # [control_delay, 2, N]
        self.poses_queue = poses_queue                  # [pose_delay, 3, N]
        self.robot_state_queue = robot_state_queue      # [state_delay, 7, N]

    FIELDS = ("robot", "min_spat_dist_so_far", "target_idx", "current_iter", "robot_collided") + DELAY_FIELDS
    VERSION = 1

    def copy(self):
        extra = {k: (getattr(self, k).clone() if getattr(self, k) is not None else None) for k in self.DELAY_FIELDS}
        return BatchedState(self.robot.clone(), self.min_spat_dist_so_far.clone(), self.target_idx.clone(),
                            self.current_iter.clone(), self.robot_collided.clone(), **extra)

    def serialize(self):
        """Basic python types only (dict of numpy arrays + version), as the reference's Serializable objects
        (utilities/serialize.py): picklable, device independent."""
        out = {k: (getattr(self, k).cpu().numpy() if getattr(self, k) is not None else None) for k in self.FIELDS}
        out['version'] = self.VERSION
        return out

    @classmethod
    def deserialize(cls, state, device="cpu"):
        state = dict(state)
        assert state.pop('version') == cls.VERSION
        return cls(**{k: (torch.from_numpy(np.ascontiguousarray(v)).to(device) if v is not None else None)
                      for k, v in state.items()})


class BatchedObservation(object):
    """Observation of all envs after a step: references to the live device tensors (as the reference's Observation
    holds references, obs.py:14-23).  `obs[i]` builds the reference-shaped Observation of env i."""

    def __init__(self, env):
        self._env = env
        st = env.state
        # (with delays the observation shows the delayed pose / robot state, env.py:377-394)
        self.pose = st.pose_seen if st.pose_seen is not None else st.robot[0:3]          # [3, N]
        seen = st.robot_state_seen if st.robot_state_seen is not None else st.robot
        self.robot_state = seen[3:7]              # [4, N] view: v, w, steering_motor_command, wheel_angle
        self.target_idx = env.state.target_idx
        self.current_iter = env.state.current_iter
        self.dt = env.params.dt

    @property
    def time(self):
        return self._env.time_of(self.current_iter)

    def __len__(self):
        return self._env.n_envs

    def __getitem__(self, i):
        return self._env.envs[i].observation()


class EnvView(object):
    """One env of the batch behind the reference's per-env API (copies a few scalars from the device on demand)."""

    def __init__(self, env, i):
        self._env, self._i = env, i

    def _robot_state(self, col):
        if self._env.is_tricycle:
            return TricycleRobotState(*[float(v) for v in col])
        return DiffdriveRobotState(*[float(v) for v in col[:5]])

    def get_state(self):
        e, i = self._env, self._i
        s = e.state
        col = s.robot[:, i].cpu().numpy()
        path = e.path_of(i)
        tidx = int(s.target_idx[i])
        it = int(s.current_iter[i])
        cls = (ContinuousRewardPurePursuitProviderState if e.params.reward_provider_name == CONTINUOUS_REWARD_PURE_PURSUIT
               else ContinuousRewardProviderState)
        rps = cls(min_spat_dist_so_far=float(s.min_spat_dist_so_far[i]), path=path, target_idx=tidx)
        pose = s.pose_seen[:, i].cpu().numpy() if s.pose_seen is not None else col[:3].copy()
        seen = s.robot_state_seen[:, i].cpu().numpy() if s.robot_state_seen is not None else col

        def fifo(q):   # the queue as the reference's list: oldest element first
            if q is None:
                return []
            d = q.shape[0]
            rows = q[:, :, i].cpu().numpy()
            return [rows[(k - 1) % d].copy() for k in range(max(1, it - d + 1), it + 1)]

        return State(reward_provider_state=rps, path=rps.current_path(), original_path=np.copy(path),
                     costmap=e.costmap_of(i), iter_timeout=e.params.iteration_timeout,
                     current_time=float(e.time_of(s.current_iter[i:i + 1])[0]), current_iter=it,
                     robot_collided=bool(s.robot_collided[i]), poses_queue=fifo(s.poses_queue),
                     robot_state_queue=[self._robot_state(v) for v in fifo(s.robot_state_queue)],
                     control_queue=[Action(command=v) for v in fifo(s.control_queue)], pose=pose,
                     robot_state=self._robot_state(seen))

    VERSION = 1

    def serialize(self):
        """PlanEnv.serialize (env.py:251-261): this env, its parametrisation included, as basic python types;
        BatchedPlanEnv.deserialize builds a batch from such records."""
        st = self.get_state()
        return {'version': self.VERSION, 'state': st.serialize(), 'params': self._env.params.serialize(),
                'path': st.original_path, 'costmap': st.costmap.get_state()}

    def set_state(self, state):
        """PlanEnv.set_state (env.py:278-285) for this env: like the reference, the robot takes over
        `state.robot_state` (with a state delay that is the delayed state -- the reference does the same)."""
        e, i = self._env, self._i
        s = e.state

        def vec(rs):
            return [rs.x, rs.y, rs.angle, rs.v, rs.w, getattr(rs, "steering_motor_command", 0.0),
                    getattr(rs, "wheel_angle", 0.0)]

        s.robot[:, i] = torch.tensor(vec(state.robot_state), dtype=torch.float64)
        s.min_spat_dist_so_far[i] = state.reward_provider_state.min_spat_dist_so_far
        s.target_idx[i] = state.reward_provider_state.target_idx
        s.current_iter[i] = state.current_iter
        s.robot_collided[i] = int(state.robot_collided)
        if s.pose_seen is not None:
            s.pose_seen[:, i] = torch.tensor(np.asarray(state.pose, dtype=np.float64))
        if s.robot_state_seen is not None:
            s.robot_state_seen[:, i] = torch.tensor(vec(state.robot_state), dtype=torch.float64)
        it = int(state.current_iter)
        for q, items in ((s.poses_queue, [np.asarray(p, dtype=np.float64) for p in state.poses_queue]),
                         (s.robot_state_queue, [np.array(vec(r)) for r in state.robot_state_queue]),
                         (s.control_queue, [np.asarray(a.command, dtype=np.float64) for a in state.control_queue])):
            if q is None:
                continue
            d = q.shape[0]
            # the list holds pushes it - len + 1 .. it (oldest first); push k lives in slot (k - 1) % d
            for k, item in zip(range(it - len(items) + 1, it + 1), items):
                q[(k - 1) % d, :, i] = torch.tensor(item)

    def observation(self):
        s = self.get_state()
        return Observation(pose=s.pose, path=s.path, costmap=s.costmap, robot_state=s.robot_state,
                           time=s.current_time, dt=self._env.params.dt)


class _EnvViews(object):
    def __init__(self, env):
        self._env = env

    def __len__(self):
        return self._env.n_envs

    def __getitem__(self, i):
        if not -self._env.n_envs <= i < self._env.n_envs:
            raise IndexError(i)
        return EnvView(self._env, i % self._env.n_envs)


class EpisodeEnds(object):
    """The episodes that ended in the last step (libbcplan's episode record, bcp_bind_episode_record): what a caller of the
    reference's PlanEnv sees from step() before it calls reset() (envs/base/env.py:334-361, 293-303), kept although the
    step has already auto-reset the env.  Device tensors, filled by the step kernel itself (no sync, no extra launch):

      reason        uint8 [N]          BCP_DONE_* bits of every env (GOAL | TIMEOUT | COLLIDED, env.py:400-419), 0 = not done
      count         int32 [1]          envs that ended in the last step (may exceed `capacity`: overflow)
      env_ids       int32 [capacity]   slot j < count: which env ended (order unspecified)
      geom          int32 [capacity]   the geometry-pool entry the episode ran on (-1 without a pool)
      final_state   BatchedState over the slots: the state the env held after its last step, before the reset
                    (robot, reward-provider state, current_iter = episode length, robot_collided; the seen pose / robot
                    state with delays; no queues)
      final_return  float64 [capacity] the episode's return, the float64 sum of its rewards in step order
      ret           float64 [N]        every env's running return (zeroed by every reset; set_state / fan_out leave it)

    The running returns start at 0 when the record is bound: bound in the middle of episodes, each env's first
    final_return covers only the steps since then (bind right after a reset() for whole-episode returns).
    """

    GOAL, TIMEOUT, COLLIDED = _lib.DONE_GOAL, _lib.DONE_TIMEOUT, _lib.DONE_COLLIDED

    def __init__(self, env, capacity):
        n, dev, cap = env.n_envs, env.device, int(capacity)
        if cap < 1:
            raise ValueError("capacity must be positive")
        self._env, self.capacity = env, cap

        def zeros(*shape, dtype=torch.float64):
            return torch.zeros(*shape, dtype=dtype, device=dev)

        self.reason = zeros(n, dtype=torch.uint8)
        self.ret = zeros(n)
        self.count = zeros(1, dtype=torch.int32)
        self.env_ids = zeros(cap, dtype=torch.int32)
        self.geom = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        self.final_return = zeros(cap)
        pd, sd = int(env.params.pose_delay), int(env.params.state_delay)
        self.final_state = BatchedState(zeros(7, cap), zeros(cap), zeros(cap, dtype=torch.int32),
                                        zeros(cap, dtype=torch.int32), zeros(cap, dtype=torch.uint8),
                                        pose_seen=zeros(3, cap) if pd else None,
                                        robot_state_seen=zeros(7, cap) if sd else None)

    def _c_struct(self):
        rec = _lib.BcpEpisodeRecord()
        rec.capacity = self.capacity
        rec.reason, rec.ret, rec.count = self.reason.data_ptr(), self.ret.data_ptr(), self.count.data_ptr()
        rec.env_id, rec.geom, rec.final_ret = self.env_ids.data_ptr(), self.geom.data_ptr(), self.final_return.data_ptr()
        f = self.final_state
        for k, name in enumerate(_STATE_FIELDS):
            setattr(rec.final, name, f.robot[k].data_ptr())
        rec.final.min_spat_dist_so_far = f.min_spat_dist_so_far.data_ptr()
        rec.final.target_idx = f.target_idx.data_ptr()
        rec.final.current_iter = f.current_iter.data_ptr()
        rec.final.robot_collided = f.robot_collided.data_ptr()
        rec.final.pose_seen = f.pose_seen.data_ptr() if f.pose_seen is not None else None
        rec.final.robot_state_seen = f.robot_state_seen.data_ptr() if f.robot_state_seen is not None else None
        return rec

    @property
    def length(self):
        """int32 [capacity]: the episodes' lengths in steps (final_state.current_iter)."""
        return self.final_state.current_iter

    def terminated(self):
        """bool [N]: the episode ended in a terminal state -- goal reached or collided (a time-out together with one
        of them counts as terminal)."""
        return (self.reason & (self.GOAL | self.COLLIDED)) != 0

    def truncated(self):
        """bool [N]: the episode was cut by the time limit alone (gymnasium's `truncated`, SB3's TimeLimit.truncated):
        bootstrap V(final observation) there."""
        return self.reason == self.TIMEOUT

    def overflowed(self):
        """True if more envs ended in the last step than there are slots (synchronises)."""
        return int(self.count[0]) > self.capacity

    def slots(self):
        """Number of filled slots of the last step, min(count, capacity) (synchronises)."""
        return min(int(self.count[0]), self.capacity)

    def to_host(self):
        """The last step's episode ends as a list of (env id, reference State, reason bits, return, length); the States
        hold no delay queues.  Synchronises -- for debugging and tests."""
        e = self._env
        m = self.slots()
        ids = self.env_ids[:m].cpu().numpy()
        geom = self.geom[:m].cpu().numpy()
        reason = self.reason.cpu().numpy()
        ret = self.final_return[:m].cpu().numpy()
        f = self.final_state
        robot = f.robot[:, :m].cpu().numpy()
        md = f.min_spat_dist_so_far[:m].cpu().numpy()
        ti = f.target_idx[:m].cpu().numpy()
        it = f.current_iter[:m].cpu().numpy()
        col = f.robot_collided[:m].cpu().numpy()
        ps = f.pose_seen[:, :m].cpu().numpy() if f.pose_seen is not None else None
        rs = f.robot_state_seen[:, :m].cpu().numpy() if f.robot_state_seen is not None else None
        view = EnvView(e, 0)
        cls = (ContinuousRewardPurePursuitProviderState if e.params.reward_provider_name == CONTINUOUS_REWARD_PURE_PURSUIT
               else ContinuousRewardProviderState)
        out = []
        for j in range(m):
            i, g = int(ids[j]), int(geom[j])
            path = e._paths[g] if g >= 0 else e.path_of(i)
            costmap = e._costmaps[g] if g >= 0 else e.costmap_of(i)
            rps = cls(min_spat_dist_so_far=float(md[j]), path=path, target_idx=int(ti[j]))
            n_it = int(it[j])
            st = State(reward_provider_state=rps, path=rps.current_path(), original_path=np.copy(path), costmap=costmap,
                       iter_timeout=e.params.iteration_timeout,
                       current_time=float(e.time_of(f.current_iter[j:j + 1])[0]), current_iter=n_it,
                       robot_collided=bool(col[j]), poses_queue=[], robot_state_queue=[], control_queue=[],
                       pose=ps[:, j].copy() if ps is not None else robot[:3, j].copy(),
                       robot_state=view._robot_state(rs[:, j] if rs is not None else robot[:, j]))
            out.append((i, st, int(reason[i]), float(ret[j]), n_it))
        return out


class Lookahead(object):
    """What BatchedPlanEnv.lookahead() returns: device tensors over [N, K] candidates (no sync).  `ret` float64 return of
    the steps taken, `steps` int32, `reason` uint8 DONE_* bits (0: not done within the horizon); optional, None unless
    asked for: `final_pose` [N, K, 3], `final_target_idx`, `err`, `best` int32 [N], `best_action` [N, 2].  The tensors
    are the env's cached buffers for this (H, K): the next lookahead() with the same shape overwrites them."""

    FIELDS = ("ret", "steps", "reason", "final_pose", "final_target_idx", "err", "best", "best_action")

    def __init__(self, horizon, n_candidates, **tensors):
        self.horizon, self.n_candidates = horizon, n_candidates
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))

    def collided(self):
        """bool [N, K]: the candidate ends in a collision"""
        return (self.reason & _lib.DONE_COLLIDED) != 0

    def timed_out(self):
        return (self.reason & _lib.DONE_TIMEOUT) != 0

    def reached_goal(self):
        return (self.reason & _lib.DONE_GOAL) != 0


class Mppi(object):
    """What BatchedPlanEnv.mppi() returns (device tensors, no sync): `mean` [N, H, 2] float64, the refined plan; `action`
    [N, 2] = mean[:, 0], ready for step(); optional, None unless asked for: `eps` [I, N, K, H, 2] float32 (the
    perturbations used), `iter_mean` [I, N, H, 2] (the mean going into each iteration), `iter_ret` / `iter_reason`
    [I, N, K], `err` int32 [N].  Everything but `mean` is a cached buffer of the env for this (H, K, I)."""

    FIELDS = ("eps", "iter_mean", "iter_ret", "iter_reason", "err")

    def __init__(self, horizon, n_candidates, iterations, mean, action, **tensors):
        self.horizon, self.n_candidates, self.iterations = horizon, n_candidates, iterations
        self.mean, self.action = mean, action
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))


SCAN_CACHE_ENTRIES = 8   # beam tables / output buffer sets of range_scan kept per env (least recently used go first)


def beam_table_cached(tables, beam_angles, device):
    """The device table [B, 2] of (cos, sin) of beam_angles for bcp_range_scan, from `tables` (an OrderedDict keyed by the
    angles' bytes, least recently used first) or uploaded and added to it; at most SCAN_CACHE_ENTRIES tables are kept."""
    angles = np.ascontiguousarray(beam_angles.detach().cpu().numpy() if isinstance(beam_angles, torch.Tensor) else beam_angles,
                                  dtype=np.float64).reshape(-1)
    key = angles.tobytes()
    if key in tables:
        tables.move_to_end(key)
    else:
        tables[key] = torch.from_numpy(np.stack([np.cos(angles), np.sin(angles)], axis=1)).to(device).contiguous()
        while len(tables) > SCAN_CACHE_ENTRIES:
            tables.popitem(last=False)
    return tables[key]


class BatchedPlanEnv(object):
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

    def __init__(self, costmap, path, params=None, n_envs=1, device=0, robot_name=None, noise_parameters='planenv',
                 auto_reset=False, env_id_base=0, seed=0, footprint_scale=1.0, dynamic_model=True,
                 model_front_column_pid=True, template_of_env=None, geom_of_env=None, next_geom=None, map_storage=None,
                 unpinned_diffdrive_noise=False, robot_constants=None):
        params = EnvParams() if params is None else params
        self.params = params
        self._pure_pursuit = params.reward_provider_name == CONTINUOUS_REWARD_PURE_PURSUIT
        self.n_envs = int(n_envs)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.robot_name = params.robot_name if robot_name is None else robot_name
        self.is_tricycle = self.robot_name == INDUSTRIAL_TRICYCLE_V1
        if noise_parameters == 'planenv':
            noise_parameters = dict(robots.PLANENV_NOISE) if self.is_tricycle else None
        self.noise_parameters = noise_parameters
        self.auto_reset = bool(auto_reset)
        self._lib = _lib.load()  # raises when libbcplan.so is missing: no fallback
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedPlanEnv needs a GPU (libbcplan has no CPU path)")
        self._bcp_params = robots.make_bcp_params(params, self.robot_name, noise_parameters, footprint_scale,
                                                  dynamic_model, model_front_column_pid, unpinned_diffdrive_noise,
                                                  robot_constants)
        self._h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self._lib.bcp_create(C.byref(self._bcp_params), self.n_envs, dev_index, int(env_id_base),
                                        C.byref(self._h)))
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
        self._keep = {}  # device buffers the library holds pointers to

        self._map_storage = (0, 0) if map_storage is None else (int(map_storage[0]), int(map_storage[1]))
        self._template_of_env = None if template_of_env is None else np.asarray(template_of_env, dtype=np.int64)
        self.geom_of_env = None
        if geom_of_env is not None:
            assert template_of_env is None
            self._device_pool = costmap if isinstance(costmap, DeviceGeometryPool) else None
            if self._device_pool is not None:
                costmap, path = self._device_pool.costmaps, self._device_pool.paths
            else:
                costmap, path = list(costmap), list(path)
            g0 = np.asarray(geom_of_env, dtype=np.int32)
            assert g0.shape == (n,) and len(costmap) == len(path) and 0 <= g0.min() and g0.max() < len(costmap)
            self.geom_of_env = torch.from_numpy(g0.copy()).to(dev)
            nxt = None
            if next_geom is not None:
                nx = np.asarray(next_geom, dtype=np.int32)
                assert nx.shape == (len(costmap),) and 0 <= nx.min() and nx.max() < len(costmap)
                nxt = torch.from_numpy(nx.copy()).to(dev)
            self._keep.update(next_geom=nxt)
            _lib.check(self._lib.bcp_set_geometry_pool(self._h, len(costmap), self.geom_of_env.data_ptr(),
                                                       nxt.data_ptr() if nxt is not None else None))
            self._set_from_templates(costmap, path)
        elif self._template_of_env is not None:
            self._set_from_templates(list(costmap), list(path))
        else:
            self._set_costmaps(costmap)
            self._set_paths(path)
        self._bind(self.state, self._lib.bcp_bind_state)
        self._initial_state = self._make_initial_state()
        self._bind(self._initial_state, self._lib.bcp_bind_initial_state)
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

    # ------------------------------------------------------------------ construction helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _bind(self, s, fn):
        st = _lib.BcpState()
        for k, name in enumerate(_STATE_FIELDS):
            setattr(st, name, s.robot[k].data_ptr())
        st.min_spat_dist_so_far = s.min_spat_dist_so_far.data_ptr()
        st.target_idx = s.target_idx.data_ptr()
        st.current_iter = s.current_iter.data_ptr()
        st.robot_collided = s.robot_collided.data_ptr()
        for name in BatchedState.DELAY_FIELDS:
            t = getattr(s, name)
            setattr(st, name, t.data_ptr() if t is not None else None)
        _lib.check(fn(self._h, C.byref(st)))

    def _set_costmaps(self, costmap):
        n = self.n_envs
        if isinstance(costmap, CostMap2D) or hasattr(costmap, "get_data") and not isinstance(costmap, (list, tuple)):
            self._costmaps, self._shared_map = [costmap], True
            data = np.ascontiguousarray(costmap.get_data(), dtype=np.uint8)
            rows, cols = data.shape
            origins = np.ascontiguousarray(costmap.get_origin(), dtype=np.float64)
            res = float(costmap.get_resolution())
            data_dev = torch.from_numpy(data).to(self.device)
            self._keep["map"] = data_dev
            self._origin_host = origins
            _lib.check(self._lib.bcp_set_costmaps(self._h, data_dev.data_ptr(), rows, cols, 1, None, None,
                                                  origins.ctypes.data, 0, res, self._stream()))
        else:
            costmaps = list(costmap)
            if len(costmaps) != n:
                raise ValueError("need one costmap per env (%d), got %d" % (n, len(costmaps)))
            res = float(costmaps[0].get_resolution())
            if any(float(c.get_resolution()) != res for c in costmaps):
                raise ValueError("all costmaps must share one resolution")
            self._costmaps, self._shared_map = costmaps, False
            rows = max(self._map_storage[0], max(c.get_data().shape[0] for c in costmaps))
            cols = max(self._map_storage[1], max(c.get_data().shape[1] for c in costmaps))
            data = np.zeros((n, rows, cols), dtype=np.uint8)
            vr = np.zeros(n, dtype=np.int32)
            vc = np.zeros(n, dtype=np.int32)
            origins = np.zeros((n, 2), dtype=np.float64)
            for i, c in enumerate(costmaps):
                d = c.get_data()
                data[i, :d.shape[0], :d.shape[1]] = d
                vr[i], vc[i] = d.shape
                origins[i] = c.get_origin()
            self.set_costmap_tensors(torch.from_numpy(data).to(self.device), torch.from_numpy(origins).to(self.device),
                                     res, torch.from_numpy(vr).to(self.device), torch.from_numpy(vc).to(self.device))
        self.resolution = res

    def _set_from_templates(self, costmaps, paths):
        """Private per-env costmaps / paths expanded on the device from a few templates."""
        n, dev = self.n_envs, self.device
        dp = getattr(self, "_device_pool", None)
        if dp is not None:   # everything is on the device already (refined paths included)
            self._costmaps, self._paths, self._shared_path = costmaps, paths, False
            self.set_costmap_tensors(dp.maps, dp.entry_origins(dev), dp.resolution, dp.valid_rows, dp.valid_cols)
            self._keep.update(path=dp.path_points, lens=dp.lens)
            _lib.check(self._lib.bcp_set_paths(self._h, dp.path_points.data_ptr(), dp.lens.data_ptr(),
                                               int(dp.path_points.shape[1]), 0, self._stream()))
            torch.cuda.current_stream(dev).synchronize()
            return
        if self.geom_of_env is not None:   # geometry pool: the library indexes the entries itself
            idx = torch.arange(len(costmaps), device=dev)
        else:
            idx = torch.from_numpy(self._template_of_env).to(dev)
            assert idx.numel() == n and int(idx.max()) < len(costmaps) == len(paths)
        res = float(costmaps[0].get_resolution())
        rows = max(self._map_storage[0], max(c.get_data().shape[0] for c in costmaps))
        cols = max(self._map_storage[1], max(c.get_data().shape[1] for c in costmaps))
        t_data = np.zeros((len(costmaps), rows, cols), dtype=np.uint8)
        t_shape = np.zeros((len(costmaps), 2), dtype=np.int32)
        t_org = np.zeros((len(costmaps), 2), dtype=np.float64)
        for t, c in enumerate(costmaps):
            d = c.get_data()
            t_data[t, :d.shape[0], :d.shape[1]] = d
            t_shape[t] = d.shape
            t_org[t] = c.get_origin()
        data = torch.from_numpy(t_data).to(dev)[idx].contiguous()
        shape = torch.from_numpy(t_shape).to(dev)[idx]
        self._costmaps, self._shared_map = costmaps, False
        self.set_costmap_tensors(data, torch.from_numpy(t_org).to(dev)[idx].contiguous(), res,
                                 shape[:, 0].contiguous(), shape[:, 1].contiguous())
        refine = (lambda p: host_init.refine_path(p, self.params.path_delta)) if self.params.refine_path else (lambda p: p)
        tp = [np.ascontiguousarray(refine(np.asarray(p)), dtype=np.float64) for p in paths]
        max_len = max(len(p) for p in tp)
        buf = np.zeros((len(tp), max_len, 3), dtype=np.float64)
        for t, p in enumerate(tp):
            buf[t, :len(p)] = p
        self._paths, self._shared_path = tp, False
        pdev = torch.from_numpy(buf).to(dev)[idx].contiguous()
        lens = torch.from_numpy(np.array([len(p) for p in tp], dtype=np.int32)).to(dev)[idx].contiguous()
        self._keep.update(path=pdev, lens=lens)
        _lib.check(self._lib.bcp_set_paths(self._h, pdev.data_ptr(), lens.data_ptr(), max_len, 0, self._stream()))
        torch.cuda.current_stream(dev).synchronize()

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

    @property
    def costmap_tensor(self):
        """The device costmap(s) the library reads: uint8 [rows, cols] (shared) or [entries, rows, cols] (private maps,
        pool entries), padded to one shape where the entries differ."""
        return self._keep["map"]

    def footprint(self):
        """The footprint [n_verts, 2] in metres the handle was created with (footprint_scale applied)."""
        p = self._bcp_params
        return np.array([[p.verts[k][0], p.verts[k][1]] for k in range(p.n_verts)], dtype=np.float64)

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
        if getattr(self, "endless", False):
            raise RuntimeError("inflate_costmaps: not supported on endless=True pools -- refresh() re-samples raw worlds "
                               "into the pool, and inflating re-sampled worlds is out of scope")
        if getattr(self, "_inflated", False):
            raise RuntimeError("inflate_costmaps: the costmaps of this env are inflated already")
        radius = robots.inscribed_radius(self.footprint() if footprint is None else footprint)
        data = self._keep["map"]
        maps = data[None] if data.dim() == 2 else data
        vr, vc = (None, None) if self._shared_map else (self._keep.get("vr"), self._keep.get("vc"))
        self._inflate(maps, vr, vc, radius, cost_scaling_factor, maps)
        if self._shared_map:
            _lib.check(self._lib.bcp_set_costmaps(self._h, data.data_ptr(), data.shape[0], data.shape[1], 1, None, None,
                                                  self._origin_host.ctypes.data, 0, float(self.resolution), self._stream()))
        else:
            self.set_costmap_tensors(data, self._keep["origins"], self.resolution, vr, vc)
        # the host copies behind envs[i].get_state().costmap (a device pool hands out copies of its tensors on demand)
        if getattr(self, "_device_pool", None) is None:
            host = list(self._costmaps)
            rows, cols = max(c.get_data().shape[0] for c in host), max(c.get_data().shape[1] for c in host)
            stack = np.zeros((len(host), rows, cols), dtype=np.uint8)
            for k, c in enumerate(host):
                d = c.get_data()
                stack[k, :d.shape[0], :d.shape[1]] = d
            shapes = np.array([c.get_data().shape for c in host], dtype=np.int32)
            dev_stack = torch.from_numpy(stack).to(self.device)
            self._inflate(dev_stack, torch.from_numpy(shapes[:, 0].copy()).to(self.device),
                          torch.from_numpy(shapes[:, 1].copy()).to(self.device), radius, cost_scaling_factor, dev_stack)
            inflated = dev_stack.cpu().numpy()
            self._costmaps = [CostMap2D(inflated[k, :s[0], :s[1]].copy(), c.get_resolution(), c.get_origin())
                              for k, (c, s) in enumerate(zip(host, shapes))]
        torch.cuda.current_stream(self.device).synchronize()
        self._inflated = True

    def _set_paths(self, path):
        refine = (lambda p: host_init.refine_path(p, self.params.path_delta)) if self.params.refine_path else (lambda p: p)
        if isinstance(path, np.ndarray) and path.ndim == 2:
            p = np.ascontiguousarray(refine(path), dtype=np.float64)
            assert p.shape[1] == 3
            self._paths, self._shared_path = [p], True
            dev = torch.from_numpy(p).to(self.device)
            self._keep["path"] = dev
            _lib.check(self._lib.bcp_set_paths(self._h, dev.data_ptr(), None, p.shape[0], 1, self._stream()))
        else:
            paths = [np.ascontiguousarray(refine(np.asarray(p)), dtype=np.float64) for p in path]
            if len(paths) != self.n_envs:
                raise ValueError("need one path per env (%d), got %d" % (self.n_envs, len(paths)))
            self._paths, self._shared_path = paths, False
            max_len = max(len(p) for p in paths)
            buf = np.zeros((self.n_envs, max_len, 3), dtype=np.float64)
            lens = np.zeros(self.n_envs, dtype=np.int32)
            for i, p in enumerate(paths):
                buf[i, :len(p)] = p
                lens[i] = len(p)
            dev, lens_dev = torch.from_numpy(buf).to(self.device), torch.from_numpy(lens).to(self.device)
            self._keep.update(path=dev, lens=lens_dev)
            _lib.check(self._lib.bcp_set_paths(self._h, dev.data_ptr(), lens_dev.data_ptr(), max_len, 0,
                                               self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # the [.,3] staging tensor may now be released

    def _make_initial_state(self):
        """make_initial_state (env.py:179-214): pose = path[0], v = w = 0, wheel at initial_wheel_angle... the
        reference's TricycleRobotState() default wheel angle is 0.0 and PlanEnv never applies
        params.initial_wheel_angle to it, so neither do we."""
        n = self.n_envs if self.geom_of_env is None else len(self._paths)
        dp = getattr(self, "_device_pool", None)
        if dp is not None:   # initial states computed on the device with the paths (bcp_mini_world_paths)
            dev = self.device
            robot_t = torch.zeros(7, n, dtype=torch.float64, device=dev)
            robot_t[0:3] = dp.path_points[:, 0, :].t()
            return BatchedState(robot_t, dp.init[:, 0].contiguous(), dp.init[:, 1].to(torch.int32).contiguous(),
                                torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
        robot = np.zeros((7, n), dtype=np.float64)
        md = np.zeros(n, dtype=np.float64)
        ti = np.zeros(n, dtype=np.int32)
        rp = self.params.reward_provider_params
        if self.geom_of_env is not None:   # one initial state per pool entry
            for g, p in enumerate(self._paths):
                md[g], ti[g] = self._first_reward_state(p, rp)
                robot[0:3, g] = p[0]
        elif self._shared_path:
            p = self._paths[0]
            m0, t0 = self._first_reward_state(p, rp)
            robot[0:3, :] = p[0][:, None]
            md[:], ti[:] = m0, t0
        elif self._template_of_env is not None:
            per = [self._first_reward_state(p, rp) for p in self._paths]
            tix = self._template_of_env
            md[:] = np.array([m for m, _ in per])[tix]
            ti[:] = np.array([t for _, t in per])[tix]
            robot[0:3, :] = np.stack([p[0] for p in self._paths])[tix].T
        else:
            for i, p in enumerate(self._paths):
                md[i], ti[i] = self._first_reward_state(p, rp)
                robot[0:3, i] = p[0]
        dev = self.device
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

    def set_tuning(self, exact_mode=None, dense_threshold=None, cull=None, defer=None, edt_lds=None, fused=None,
                   ego_sparse=None, near_dilate=None, local_pairs=None, ego_list_stride=None, near_shift=None):
        """Execution knobs of libbcplan (bcp_set_tuning); results never depend on them.
        (near_shift takes effect when the costmaps are bound the next time.)"""
        for key, val in ((_lib.TUNE_EXACT_MODE, exact_mode), (_lib.TUNE_DENSE_THRESHOLD, dense_threshold),
                         (_lib.TUNE_CULL, cull), (_lib.TUNE_DEFER, defer), (_lib.TUNE_EDT_LDS, edt_lds),
                         (_lib.TUNE_FUSED, fused), (_lib.TUNE_EGO_SPARSE, ego_sparse), (_lib.TUNE_LOCAL_PAIRS, local_pairs), (_lib.TUNE_EGO_LIST_STRIDE, ego_list_stride),
                         (_lib.TUNE_NEAR_DILATE, near_dilate), (_lib.TUNE_NEAR_SHIFT, near_shift)):
            if val is not None:
                _lib.check(self._lib.bcp_set_tuning(self._h, key, int(val)))

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
    def path_of(self, i):
        if self.geom_of_env is not None:
            return self._paths[int(self.geom_of_env[i])]
        if self._template_of_env is not None:
            return self._paths[self._template_of_env[i]]
        return self._paths[0] if self._shared_path else self._paths[i]

    def costmap_of(self, i):
        if self.geom_of_env is not None:
            return self._costmaps[int(self.geom_of_env[i])]
        if self._template_of_env is not None:
            return self._costmaps[self._template_of_env[i]]
        if self._shared_map or len(self._costmaps) == 1:
            return self._costmaps[0]
        return self._costmaps[i]

    def time_of(self, current_iter):
        """Observation.time for iteration counters (device tensor): dt accumulated current_iter times."""
        idx = current_iter.to(torch.int64)
        top = int(idx.max()) if idx.numel() else 0
        if top >= len(self.time_table):  # envs stepped past the timeout without a reset: grow the table
            self.time_table = host_init.time_table(self.params.dt, 2 * top)
            self._time_table_dev = torch.from_numpy(self.time_table).to(self.device)
        return self._time_table_dev[idx]

    # ------------------------------------------------------------------ reference API
    def seed(self, seed=None):
        """Seeds the on-device odometry-noise stream (the reference draws from numpy's global RNG)."""
        if seed is not None:
            _lib.check(self._lib.bcp_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))

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
        self._last_inputs = (mask,)   # keep the mask alive until the stream has consumed it

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
        self._last_inputs = (actions, z, done)  # keep inputs alive until the stream has consumed them
        return self._obs, self.reward, done, self._info

    def _device_tensor(self, x, dtype=None, shape=None):
        """A tensor, or anything numpy can wrap, on the env's device and contiguous.  dtype None keeps float32 / float64
        and widens everything else to float64; a shape, if given, is asserted."""
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if dtype is None:
            dtype = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float64
        x = x.to(self.device).to(dtype).contiguous()
        assert shape is None or tuple(x.shape) == shape
        return x

    def _cached_outputs(self, cache_name, key, shapes, names):
        """{name: zero-initialised device buffer of shapes[name] = (shape, dtype)}, made on first use and cached in
        self.<cache_name>[key] -- a planner that calls every tick allocates nothing."""
        buf = self.__dict__.setdefault(cache_name, {}).setdefault(key, {})
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
        rows = self._cached_outputs("_rollout_buffers", k, {"collided": ((k, n), torch.uint8), "err": ((k, n), torch.int32)},
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
        self._last_inputs = tuple(keep)
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
        out = self._cached_outputs("_lookahead_buffers", (h, k), shapes,
                                   [name for name in Lookahead.FIELDS if name in want or name in Lookahead.FIELDS[:3]])
        for name, t in out.items():
            setattr(io, name, t.data_ptr())
        _lib.check(self._lib.bcp_lookahead(self._h, C.byref(io), flags, self._stream()))
        self._last_lookahead_inputs = tuple(keep)   # alive until the stream has consumed them
        return Lookahead(h, k, **out)

    def mppi(self, mean, sigma, iterations, n_candidates, lam, collision_penalty, seed=0, draw_index=0, mask=None, eps=None,
             want=(), action_dtype=None):
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
        action_dtype: torch.float64 (default) or torch.float32.  Returns an Mppi; buffers are cached per (H, K, I).  Delays
        > 0 are refused."""
        n = self.n_envs
        mean = self._device_tensor(mean, torch.float64)   # (a contiguous float64 tensor on the device: itself)
        if mean.dim() != 3 or mean.shape[0] != n or mean.shape[2] != 2:
            raise ValueError("mean must have shape (%d, H, 2), got %s" % (n, tuple(mean.shape)))
        h, k, it = int(mean.shape[1]), int(n_candidates), int(iterations)
        want = set(want)
        unknown = want - set(Mppi.FIELDS)
        if unknown:
            raise ValueError("mppi: unknown outputs %s" % sorted(unknown))
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
                  "iter_reason": ((it, n, k), torch.uint8), "err": ((n,), torch.int32)}
        out = self._cached_outputs("_mppi_buffers", (h, k, it), shapes,
                                   ["action"] + [name for name in Mppi.FIELDS if name in want])
        for name, t in out.items():
            setattr(io, "eps_out" if name == "eps" else name, t.data_ptr())
        flags = _lib.STEP_ACTIONS_F32 if action_dtype == torch.float32 else 0
        _lib.check(self._lib.bcp_mppi(self._h, C.byref(p), C.byref(io), flags, self._stream()))
        self._last_mppi_inputs = tuple(keep)   # alive until the stream has consumed them
        return Mppi(h, k, it, mean, **out)

    def _beam_table(self, beam_angles):
        """The device table [B, 2] of (cos, sin) of the beam angles (beam_table_cached)."""
        return beam_table_cached(self.__dict__.setdefault("_beam_tables", OrderedDict()), beam_angles, self.device)

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
        table = self._beam_table(beam_angles)
        b = int(table.shape[0])
        unknown = set(want) - {"hit", "heading_cs"}
        if unknown:
            raise ValueError("range_scan: unknown outputs %s" % sorted(unknown))
        keep = [table]
        if poses is not None:
            poses = self._device_tensor(poses, torch.float64)
            assert poses.dim() == 2 and poses.shape[1] == 3
            keep.append(poses)
        n = self.n_envs if poses is None else int(poses.shape[0])
        shapes = {"ranges": ((n, b), torch.float32), "hit": ((n, b), torch.int32), "heading_cs": ((n, 2), torch.float64)}
        buffers = self.__dict__.setdefault("_range_scan_buffers", OrderedDict())
        out = self._cached_outputs("_range_scan_buffers", (n, b), shapes, ["ranges"] + [w for w in want])
        buffers.move_to_end((n, b))
        while len(buffers) > SCAN_CACHE_ENTRIES:   # (a caller that sweeps shapes does not pile up device memory)
            buffers.popitem(last=False)
        _lib.check(self._lib.bcp_range_scan(
            self._h, poses.data_ptr() if poses is not None else None, n, table.data_ptr(), b, float(max_range),
            out["ranges"].data_ptr(), out["hit"].data_ptr() if "hit" in out else None,
            out["heading_cs"].data_ptr() if "heading_cs" in out else None, self._stream()))
        self._last_scan_inputs = tuple(keep)   # alive until the stream has consumed them
        return out["ranges"] if not want else (out["ranges"],) + tuple(out[w] for w in want)

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
        import numpy as np
        from . import distributed
        parts = []
        dp = getattr(self, "_device_pool", None)
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

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.bcp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

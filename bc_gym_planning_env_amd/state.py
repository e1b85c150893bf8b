"""The batch's state and observation as device tensors (BatchedState, BatchedObservation), and one env of the batch
behind the reference's per-env API (EnvView): reference-shaped State / Observation objects built from a few scalars."""
import numpy as np
import torch

from .api import (Action, CONTINUOUS_REWARD_PURE_PURSUIT, ContinuousRewardProviderState,
                  ContinuousRewardPurePursuitProviderState, DiffdriveRobotState, Observation, State, TricycleRobotState)

_STATE_FIELDS = ("x", "y", "angle", "v", "w", "steering_motor_command", "wheel_angle")


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

    def fill_pointers(self, st):
        """The pointer fields of `st`, a BcpState-shaped ctypes struct (_lib.BcpState, BcpEpisodeRecord.final), from these
        tensors; NULL for what is None."""
        for k, name in enumerate(_STATE_FIELDS):
            setattr(st, name, self.robot[k].data_ptr())
        for name in self.FIELDS[1:]:
            t = getattr(self, name)
            setattr(st, name, t.data_ptr() if t is not None else None)
        return st

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


def reference_state(env, path, costmap, min_spat_dist_so_far, target_idx, current_iter, current_time, robot_collided, pose,
                    robot_state, queues=((), (), ())):
    """The reference's State of one env of `env` from host scalars and arrays: robot_state [7] (or [5] for a diff-drive
    robot), queues = (poses, robot states, commands) as lists of such arrays, oldest first."""
    def robot(col):
        return TricycleRobotState(*[float(v) for v in col]) if env.is_tricycle else DiffdriveRobotState(*[float(v) for v in col[:5]])

    cls = (ContinuousRewardPurePursuitProviderState if env.params.reward_provider_name == CONTINUOUS_REWARD_PURE_PURSUIT
           else ContinuousRewardProviderState)
    rps = cls(min_spat_dist_so_far=float(min_spat_dist_so_far), path=path, target_idx=int(target_idx))
    return State(reward_provider_state=rps, path=rps.current_path(), original_path=np.copy(path), costmap=costmap,
                 iter_timeout=env.params.iteration_timeout, current_time=float(current_time),
                 current_iter=int(current_iter), robot_collided=bool(robot_collided), poses_queue=list(queues[0]),
                 robot_state_queue=[robot(v) for v in queues[1]], control_queue=[Action(command=v) for v in queues[2]],
                 pose=pose, robot_state=robot(robot_state))


class EnvView(object):
    """One env of the batch behind the reference's per-env API (copies a few scalars from the device on demand)."""

    def __init__(self, env, i):
        self._env, self._i = env, i

    def get_state(self):
        e, i = self._env, self._i
        s = e.state
        col = s.robot[:, i].cpu().numpy()
        it = int(s.current_iter[i])

        def fifo(q):   # the queue as the reference's list: oldest element first
            if q is None:
                return []
            d = q.shape[0]
            rows = q[:, :, i].cpu().numpy()
            return [rows[(k - 1) % d].copy() for k in range(max(1, it - d + 1), it + 1)]

        return reference_state(
            e, e.path_of(i), e.costmap_of(i), s.min_spat_dist_so_far[i], s.target_idx[i], it,
            e.time_of(s.current_iter[i:i + 1])[0], s.robot_collided[i],
            s.pose_seen[:, i].cpu().numpy() if s.pose_seen is not None else col[:3].copy(),
            s.robot_state_seen[:, i].cpu().numpy() if s.robot_state_seen is not None else col,
            (fifo(s.poses_queue), fifo(s.robot_state_queue), fifo(s.control_queue)))

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

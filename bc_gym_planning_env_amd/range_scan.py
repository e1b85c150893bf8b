"""Range-scan observations for the whole batch: what a navigation learner is usually fed instead of an image -- the
distances to the nearest obstacle along beams fixed to the robot, and the goal_n_state vector -- as two launches over all
envs (bcp_range_scan, bcp_goal_n_state; include/bcplan.h).  The reference has no such wrapper; the shape follows
BatchedEgocentricCostmap (egocentric.py)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib


class BatchedRangeScan(object):
    """Observation wrapper around a BatchedPlanEnv (or BatchedRandomMiniEnv): step() / reset() return
    OrderedDict(scan=float32 [N, B, 1] in metres, goal_n_state=float32 [N, 9, 1]) device tensors (8 rows for a diff-drive
    robot).  Beam k looks along -fov/2 + fov * (k + 0.5) / n_beams from the robot's heading, counter-clockwise; a beam that
    meets no lethal cell within max_range reads max_range.  goal_n_state is the egocentric wrapper's vector with world size
    (max_range, max_range).
    final_observation=True: the env's episode record is enabled (env.enable_episode_record) and step() adds
    info["final_observation"], the observation of every episode that ended in the step, scanned from its final state on
    the map it ran on, before the auto-reset: the same keys with leading dimension `capacity`, row j belongs to env
    info["episode_ends"].env_ids[j] for j < count."""

    def __init__(self, env, n_beams=64, fov=2 * np.pi, max_range=3.0, final_observation=False):
        self.env = env
        self.action_space = env.action_space
        self.n_beams, self.fov, self.max_range = int(n_beams), float(fov), float(max_range)
        self.beam_angles = -self.fov / 2 + self.fov * (np.arange(self.n_beams) + 0.5) / self.n_beams
        self._lib = env._lib
        self._table = env._beam_table(self.beam_angles)
        self._world = np.array([self.max_range, self.max_range], dtype=np.float64)
        n, dev = env.n_envs, env.device
        self.n_state = 6 if env.is_tricycle else 5
        self.scan = torch.zeros((n, self.n_beams, 1), dtype=torch.float32, device=dev)
        self.goal_n_state = torch.zeros((n, 3 + self.n_state, 1), dtype=torch.float32, device=dev)
        self._obs = OrderedDict((('scan', self.scan), ('goal_n_state', self.goal_n_state)))
        self._final = None
        if final_observation:
            ends = env.episode_ends if env.episode_ends is not None else env.enable_episode_record()
            self._alloc_final(ends.capacity)

    def unwrapped(self):
        return self.env

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.env.device).cuda_stream)

    def observation(self, _observation=None):
        """Refresh and return the observation of the envs' current state (device tensors, no sync)."""
        e = self.env
        stream = self._stream()
        _lib.check(self._lib.bcp_range_scan(e._h, None, e.n_envs, self._table.data_ptr(), self.n_beams, self.max_range,
                                            self.scan.data_ptr(), None, None, stream))
        _lib.check(self._lib.bcp_goal_n_state(e._h, self._world.ctypes.data_as(_lib._f64p), self.goal_n_state.data_ptr(), stream))
        return self._obs

    def _alloc_final(self, cap):
        dev = self.env.device
        self.final_scan = torch.zeros((cap, self.n_beams, 1), dtype=torch.float32, device=dev)
        self.final_vector = torch.zeros((cap, 3 + self.n_state, 1), dtype=torch.float32, device=dev)
        self._final = OrderedDict((('scan', self.final_scan), ('goal_n_state', self.final_vector)))

    def _final_buffers(self):
        """The buffers follow the env's record: a record bound again with another capacity gets buffers of that size."""
        ends = self.env.episode_ends
        if ends is None:
            raise RuntimeError("final_observation=True needs the env's episode record (env.disable_episode_record() "
                               "was called)")
        if self.final_scan.shape[0] != ends.capacity:
            self._alloc_final(ends.capacity)
        return self._final

    def step(self, actions, **kw):
        _o, reward, done, info = self.env.step(actions, **kw)
        if self._final is not None:
            # scanned now, on the step's stream: a pool refresh after this step may release the worlds the envs just left
            final = self._final_buffers()
            e, stream = self.env, self._stream()
            _lib.check(self._lib.bcp_final_range_scan(e._h, self._table.data_ptr(), self.n_beams, self.max_range,
                                                      self.final_scan.data_ptr(), None, None, stream))
            _lib.check(self._lib.bcp_final_goal_n_state(e._h, self._world.ctypes.data_as(_lib._f64p),
                                                        self.final_vector.data_ptr(), stream))
            info = dict(info, final_observation=final)   # (a copy: the env's own info dict stays as the env keeps it)
        return self.observation(), reward, done, info

    def reset(self, mask=None):
        self.env.reset(mask)
        return self.observation()

    def seed(self, seed=None):
        self.env.seed(seed)

    def lookahead(self, actions, **kw):
        return self.env.lookahead(actions, **kw)

    def mppi(self, mean, *args, **kw):
        return self.env.mppi(mean, *args, **kw)

    def get_state(self):
        return self.env.get_state()

    def set_state(self, state):
        self.env.set_state(state)

    def render(self, mode='human'):
        return self.env.render(mode)

    def close(self):
        self.env.close()

"""Range-scan observations for the whole batch: what a navigation learner is usually fed instead of an image -- the
distances to the nearest obstacle along beams fixed to the robot, and the goal_n_state vector -- as two launches over all
envs (bcp_range_scan, bcp_goal_n_state; include/bcplan.h).  The reference has no such wrapper; the shape follows
BatchedEgocentricCostmap (egocentric.py)."""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .wrappers import BatchedObservationWrapper


class BatchedRangeScan(BatchedObservationWrapper):
    """Observation wrapper around a BatchedPlanEnv (or BatchedRandomMiniEnv): step() / reset() return
    OrderedDict(scan=float32 [N, B, 1] in metres, goal_n_state=float32 [N, 9, 1]) device tensors (8 rows for a diff-drive
    robot).  Beam k looks along -fov/2 + fov * (k + 0.5) / n_beams from the robot's heading, counter-clockwise; a beam that
    meets no lethal cell within max_range reads max_range.  goal_n_state is the egocentric wrapper's vector with world size
    (max_range, max_range).
    final_observation=True: step() adds info["final_observation"] (BatchedObservationWrapper), scanned from every ended
    episode's final state on the map it ran on."""

    def __init__(self, env, n_beams=64, fov=2 * np.pi, max_range=3.0, final_observation=False):
        super(BatchedRangeScan, self).__init__(env)
        self.n_beams, self.fov, self.max_range = int(n_beams), float(fov), float(max_range)
        self.beam_angles = -self.fov / 2 + self.fov * (np.arange(self.n_beams) + 0.5) / self.n_beams
        self._table = env._beam_table(self.beam_angles)
        self._world = np.array([self.max_range, self.max_range], dtype=np.float64)
        self.scan = self._scan(env.n_envs)
        self.goal_n_state = self._goal_vector(env.n_envs)
        self._obs = OrderedDict((('scan', self.scan), ('goal_n_state', self.goal_n_state)))
        self._init_final(final_observation)

    def _scan(self, rows):
        return torch.zeros((rows, self.n_beams, 1), dtype=torch.float32, device=self.env.device)

    def observation(self, _observation=None):
        """Refresh and return the observation of the envs' current state (device tensors, no sync)."""
        e, stream = self.env, self._stream()
        _lib.check(self._lib.bcp_range_scan(e._h, None, e.n_envs, self._table.data_ptr(), self.n_beams, self.max_range,
                                            self.scan.data_ptr(), None, None, stream))
        _lib.check(self._lib.bcp_goal_n_state(e._h, self._world.ctypes.data_as(_lib._f64p), self.goal_n_state.data_ptr(), stream))
        return self._obs

    def _alloc_final(self, cap):
        self.final_scan, self.final_vector = self._scan(cap), self._goal_vector(cap)
        return OrderedDict((('scan', self.final_scan), ('goal_n_state', self.final_vector)))

    def _draw_final(self, stream):
        e = self.env
        _lib.check(self._lib.bcp_final_range_scan(e._h, self._table.data_ptr(), self.n_beams, self.max_range,
                                                  self.final_scan.data_ptr(), None, None, stream))
        _lib.check(self._lib.bcp_final_goal_n_state(e._h, self._world.ctypes.data_as(_lib._f64p),
                                                    self.final_vector.data_ptr(), stream))

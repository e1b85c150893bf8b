"""Egocentric observations for the whole batch: what the reference's EgocentricCostmap wrapper
(envs/egocentric.py:102-160) computes per env on the host -- the costmap rotated and cut around the robot
(extract_egocentric_costmap, utilities/costmap_utils.py:25-75) and the goal_n_state vector -- as two launches over
all envs (bcp_egocentric_costmaps, bcp_goal_n_state; include/bcplan.h)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .wrappers import BatchedObservationWrapper


def _f64x2(v):
    a = np.ascontiguousarray(v, dtype=np.float64)
    assert a.shape == (2,)
    return a


class BatchedEgocentricCostmap(BatchedObservationWrapper):
    """Observation wrapper around a BatchedPlanEnv (or BatchedRandomMiniEnv): step() / reset() return
    OrderedDict(env=uint8 [N, H, W, 1], goal_n_state=float32 [N, 9, 1]) device tensors (8 rows for a diff-drive robot).
    The window defaults are the reference's: 0.5 m behind to 3 m ahead of the robot, 2 m to each side.
    final_observation=True: step() adds info["final_observation"] (BatchedObservationWrapper).
    pool=p > 1: the images are the maxima of the p x p blocks of the full image (bcp_egocentric_costmaps_pooled), made
    without the full image reaching memory: image_shape is the pooled shape, full_image_shape the window's (H, W); the
    goal vectors stay those of the full window."""

    def __init__(self, env, x_bounds=(-0.5, 3.), y_bounds=(-2., 2.), border_value=0, final_observation=False, pool=1):
        super(BatchedEgocentricCostmap, self).__init__(env)
        self.pool = int(pool)
        self._origin = _f64x2([x_bounds[0], y_bounds[0]])
        self._size = _f64x2([x_bounds[1] - x_bounds[0], y_bounds[1] - y_bounds[0]])
        self._border = int(border_value)
        shape = (C.c_int32 * 2)()
        _lib.check(self._lib.bcp_egocentric_shape(env._h, self._size.ctypes.data_as(_lib._f64p), shape))
        self.full_image_shape = (int(shape[0]), int(shape[1]))
        self.image_shape = self.full_image_shape
        if self.pool != 1:
            pooled = (C.c_int32 * 2)()
            _lib.check(self._lib.bcp_egocentric_pooled_shape(env._h, self._size.ctypes.data_as(_lib._f64p), self.pool, pooled))
            self.image_shape = (int(pooled[0]), int(pooled[1]))
        res = env.resolution
        # CostMap2D.world_size() of the extracted map (utilities/costmap_2d.py:107-121)
        self._world = _f64x2([(self._origin[0] + res * shape[1]) - self._origin[0],
                              (self._origin[1] + res * shape[0]) - self._origin[1]])
        self.images = torch.zeros((env.n_envs,) + self.image_shape + (1,), dtype=torch.uint8, device=env.device)
        self.goal_n_state = self._goal_vector(env.n_envs)
        self._obs = OrderedDict((('env', self.images), ('goal_n_state', self.goal_n_state)))
        self._init_final(final_observation)

    def observation(self, _observation=None):
        """Refresh and return the observation of the envs' current state (device tensors, no sync)."""
        stream = self._refresh_images()
        _lib.check(self._lib.bcp_goal_n_state(self.env._h, self._world.ctypes.data_as(_lib._f64p),
                                              self.goal_n_state.data_ptr(), stream))
        return self._obs

    def _refresh_images(self):
        e, stream = self.env, self._stream()
        if self.pool == 1:
            _lib.check(self._lib.bcp_egocentric_costmaps(
                e._h, None, e.n_envs, self._origin.ctypes.data_as(_lib._f64p), self._size.ctypes.data_as(_lib._f64p),
                self._border, self.images.data_ptr(), stream))
        else:
            _lib.check(self._lib.bcp_egocentric_costmaps_pooled(
                e._h, None, e.n_envs, self._origin.ctypes.data_as(_lib._f64p), self._size.ctypes.data_as(_lib._f64p),
                self._border, self.pool, self.images.data_ptr(), stream))
        return stream

    def route(self):
        """Which kernel drew the last observation (bcp_egocentric_route): dict(kernel=name, max_cells, list_stride, limit)."""
        info = (C.c_int32 * 4)()
        _lib.check(self._lib.bcp_egocentric_route(self.env._h, info))
        return {"kernel": _lib.EGO_KERNELS.get(int(info[0]), "?"), "max_cells": int(info[1]), "list_stride": int(info[2]),
                "limit": int(info[3])}

    # the final observation's keys and vector, [capacity] rows (BatchedColoredEgoCostmap has its own)
    _FINAL_KEYS = ('env', 'goal_n_state')

    def _final_vector(self, cap):
        return self._goal_vector(cap)

    def _alloc_final(self, cap):
        self.final_images = torch.zeros((cap,) + self.image_shape + (1,), dtype=torch.uint8, device=self.env.device)
        self.final_vector = self._final_vector(cap)
        return OrderedDict(zip(self._FINAL_KEYS, (self.final_images, self.final_vector)))

    def _final_images(self, stream):
        e = self.env
        if self.pool == 1:
            _lib.check(self._lib.bcp_final_egocentric_costmaps(
                e._h, self._origin.ctypes.data_as(_lib._f64p), self._size.ctypes.data_as(_lib._f64p), self._border,
                self.final_images.data_ptr(), stream))
        else:
            _lib.check(self._lib.bcp_final_egocentric_costmaps_pooled(
                e._h, self._origin.ctypes.data_as(_lib._f64p), self._size.ctypes.data_as(_lib._f64p), self._border,
                self.pool, self.final_images.data_ptr(), stream))

    def _draw_final(self, stream):
        """The final observations of the record's slots (bcp_final_egocentric_costmaps / bcp_final_goal_n_state)."""
        self._final_images(stream)
        _lib.check(self._lib.bcp_final_goal_n_state(self.env._h, self._world.ctypes.data_as(_lib._f64p),
                                                    self.final_vector.data_ptr(), stream))


class BatchedColoredEgoCostmap(BatchedEgocentricCostmap):
    """The observation of ColoredEgoCostmapRandomAisleTurnEnv (envs/synth_turn_env.py:376-451) for a whole batch:
    OrderedDict(environment=uint8 [N, 133, 133, 1], goal=float64 [N, 5, 1]) -- the egocentric costmap 0.5 m behind to
    3.5 m ahead of the robot, and (unit direction to the final way point, v, w, wheel_angle)."""

    def __init__(self, env, x_bounds=(-0.5, 3.5), y_bounds=(-2., 2.), border_value=0, final_observation=False, pool=1):
        super(BatchedColoredEgoCostmap, self).__init__(env, x_bounds, y_bounds, border_value, final_observation, pool)
        self.goal = torch.zeros((env.n_envs, 5, 1), dtype=torch.float64, device=env.device)
        self._obs = OrderedDict((('environment', self.images), ('goal', self.goal)))

    _FINAL_KEYS = ('environment', 'goal')

    def _final_vector(self, cap):
        return torch.zeros((cap, 5, 1), dtype=torch.float64, device=self.env.device)

    def _draw_final(self, stream):
        self._final_images(stream)
        _lib.check(self._lib.bcp_final_goal_direction_state(self.env._h, self._world.ctypes.data_as(_lib._f64p),
                                                            self.final_vector.data_ptr(), stream))

    def observation(self, _observation=None):
        stream = self._refresh_images()
        _lib.check(self._lib.bcp_goal_direction_state(self.env._h, self._world.ctypes.data_as(_lib._f64p),
                                                      self.goal.data_ptr(), stream))
        return self._obs

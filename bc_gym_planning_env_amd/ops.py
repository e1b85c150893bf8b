"""Operator-level seams: GPU stand-ins for the reference's optional native hooks (`*_impl` imports guarded by
try/except ImportError), batched over many inputs.

  get_pixel_footprint   utilities/path_tools.py:101-162       (get_pixel_footprint_impl)
  pose_collides         envs/base/env.py:464-489, utilities/costmap_utils.py:178-203
  normalize_angle       utilities/coordinate_transformations.py:17-36   (normalize_angle_impl)
  world_to_pixel        utilities/coordinate_transformations.py:169-205 (world_to_pixel_impl)
  extract_egocentric_costmap   utilities/costmap_utils.py:25-75 (cv2.getRotationMatrix2D + cv2.warpAffine, nearest)
  robot_step            IRobot.step: tricycle_model.py:478-538 / differential_drive.py:236-265
  is_robot_colliding    utilities/costmap_utils.py:106-164; is_footprint_colliding (is_footprint_colliding_impl, :106-136)
  reward / find_last_reached / path_velocity   envs/base/reward.py:184-259, utilities/path_tools.py:432-448, :298-323
  inflate_costmap       utilities/costmap_inflation.py:73-92 (cv2.distanceTransform + _pixel_distance_to_cost)
  range_scan            no counterpart: distances to the nearest lethal cell along beams (bcp_range_scan)
  goal_field            no counterpart: geodesic cost-to-go of a map to its seed cells (bcp_goal_field)
  scatter_boxes         no counterpart: box obstacles stamped into a batch of maps (bcp_scatter_boxes)
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, boxes, robots
from .api import EnvParams, INDUSTRIAL_TRICYCLE_V1
from .handle import Handle


class NativeOps(Handle):
    """A libbcplan handle used only for the stand-alone operators (no env state bound)."""

    def __init__(self, robot_name=INDUSTRIAL_TRICYCLE_V1, device=0, noise_parameters=None, params=None,
                 footprint_scale=1.0, dynamic_model=True, model_front_column_pid=True, robot_constants=None):
        self.params = EnvParams() if params is None else params
        super(NativeOps, self).__init__(
            robots.make_bcp_params(self.params, robot_name, noise_parameters, footprint_scale, dynamic_model,
                                   model_front_column_pid, robot_constants=robot_constants), 1, device)

    def normalize_angle(self, z):
        zin = self._device_tensor(np.atleast_1d(z) if not isinstance(z, torch.Tensor) else z, torch.float64)
        out = torch.empty_like(zin)
        _lib.check(self._lib.bcp_normalize_angle(self._h, zin.data_ptr(), out.data_ptr(), zin.numel(), self._stream()))
        return out

    def world_to_pixel(self, world_coords, origin, resolution):
        xy = self._device_tensor(world_coords, torch.float64)
        flat = xy.reshape(-1, 2)
        out = torch.empty(flat.shape, dtype=torch.int64, device=self.device)
        org = np.ascontiguousarray(origin, dtype=np.float64)
        _lib.check(self._lib.bcp_world_to_pixel(self._h, flat.data_ptr(), flat.shape[0],
                                                org.ctypes.data_as(C.POINTER(C.c_double)), float(resolution),
                                                out.data_ptr(), self._stream()))
        return out.reshape(xy.shape)

    def get_pixel_footprint(self, angles, map_resolution, side=None):
        """-> (masks uint8 [n, side, side], shape_hw int32 [n, 2]); image i is masks[i, :h, :w]."""
        ang = self._device_tensor(np.atleast_1d(angles) if not isinstance(angles, torch.Tensor) else angles, torch.float64)
        n = ang.numel()
        if side is None:
            side = 2 * int(np.ceil(np.linalg.norm(self.footprint(), axis=1).max() / map_resolution)) + 3
        masks = torch.empty((n, side, side), dtype=torch.uint8, device=self.device)
        shape = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.bcp_pixel_footprint(self._h, ang.data_ptr(), n, float(map_resolution), masks.data_ptr(),
                                                 side, shape.data_ptr(), self._stream()))
        return masks, shape

    def set_costmap(self, data, origin, resolution):
        d = self._device_tensor(data, torch.uint8)
        org = np.ascontiguousarray(origin, dtype=np.float64)
        self._keep["map"] = d
        _lib.check(self._lib.bcp_set_costmaps(self._h, d.data_ptr(), d.shape[0], d.shape[1], 1, None, None,
                                              org.ctypes.data, 0, float(resolution), self._stream()))

    def pose_collides(self, poses):
        """poses [n,3] against the costmap given to set_costmap -> uint8 [n]."""
        p = self._device_tensor(poses, torch.float64)
        out = torch.empty(p.shape[0], dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.bcp_pose_collides(self._h, p.data_ptr(), p.shape[0], out.data_ptr(), self._stream()))
        return out

    def is_robot_colliding(self, poses):
        """is_robot_colliding (costmap_utils.py:106-164) for poses [n,3]: pose_collides, but never when the robot's own
        pixel is off the map -> uint8 [n]."""
        p = self._device_tensor(poses, torch.float64)
        out = torch.empty(p.shape[0], dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.bcp_is_robot_colliding(self._h, p.data_ptr(), p.shape[0], out.data_ptr(), self._stream()))
        return out

    def is_footprint_colliding(self, image_slices, blit_masks, lethal=254):
        """is_footprint_colliding_impl(image_slice, blit_mask, lethal) for n pairs [n, rows, cols] -> uint8 [n]."""
        sl = self._device_tensor(image_slices, torch.uint8)
        mk = self._device_tensor(blit_masks, torch.uint8)
        if sl.dim() == 2:
            sl, mk = sl[None], mk[None]
        assert sl.shape == mk.shape and sl.dim() == 3
        out = torch.empty(sl.shape[0], dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.bcp_is_footprint_colliding(self._h, sl.data_ptr(), mk.data_ptr(), sl.shape[0], sl.shape[1],
                                                        sl.shape[2], int(lethal), out.data_ptr(), self._stream()))
        return out

    def set_path(self, path):
        """The (already refined) path [m,3] the reward operators below score against."""
        p = self._device_tensor(path, torch.float64)
        assert p.dim() == 2 and p.shape[1] == 3
        self._keep["path"] = p
        _lib.check(self._lib.bcp_set_paths(self._h, p.data_ptr(), None, p.shape[0], 1, self._stream()))
        torch.cuda.current_stream(self.device).synchronize()

    def reward(self, poses, min_spat_dist_so_far, target_idx, robot_collided=None):
        """reward_provider.reward(state) / .done(state) (reward.py:184-259) for n (pose, provider state) pairs ->
        (reward float64 [n], new min_spat_dist_so_far [n], new target_idx int32 [n], goal_reached uint8 [n])."""
        p = self._device_tensor(poses, torch.float64)
        n = p.shape[0]
        md = self._device_tensor(min_spat_dist_so_far, torch.float64).clone()
        ti = self._device_tensor(target_idx, torch.int32).clone()
        col = self._device_tensor(robot_collided, torch.uint8) if robot_collided is not None else None
        rew = torch.empty(n, dtype=torch.float64, device=self.device)
        goal = torch.empty(n, dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.bcp_reward(self._h, p.data_ptr(), n, md.data_ptr(), ti.data_ptr(),
                                        col.data_ptr() if col is not None else None, rew.data_ptr(), goal.data_ptr(),
                                        self._stream()))
        return rew, md, ti, goal

    def find_last_reached(self, poses):
        """find_last_reached (path_tools.py:432-448) for poses [n,3] against the path of set_path -> int32 [n], -1 = None."""
        p = self._device_tensor(poses, torch.float64)
        out = torch.empty(p.shape[0], dtype=torch.int32, device=self.device)
        _lib.check(self._lib.bcp_find_last_reached(self._h, p.data_ptr(), p.shape[0], out.data_ptr(), self._stream()))
        return out

    def path_velocity(self, path_txyth):
        """path_velocity (path_tools.py:298-323): rows of (t, x, y, angle) -> (v, w) of the n - 1 segments; raises like
        the reference on corrupted angle data / non-increasing time stamps."""
        p = self._device_tensor(path_txyth, torch.float64)
        n = p.shape[0]
        v = torch.empty(n - 1, dtype=torch.float64, device=self.device)
        w = torch.empty(n - 1, dtype=torch.float64, device=self.device)
        err = torch.zeros(n - 1, dtype=torch.int32, device=self.device)
        _lib.check(self._lib.bcp_path_velocity(self._h, p.data_ptr(), n, v.data_ptr(), w.data_ptr(), err.data_ptr(),
                                               self._stream()))
        e = err.cpu().numpy()
        assert not (e & _lib.ERR_TIME_ORDER).any()
        if (e & _lib.ERR_ANGLE_JUMP).any():
            raise Exception("Path has missing/corrupted angle data at indices: %s." % ((e & _lib.ERR_ANGLE_JUMP).nonzero(),))
        return v, w

    def device_normals(self, n_envs, first_step=0, n_steps=1, first_env=0):
        """The standard normals the step kernels would draw (bcp_device_normals) -> float64 [n_steps, n_envs, 3]."""
        out = torch.empty((int(n_steps), int(n_envs), 3), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.bcp_device_normals(self._h, int(first_env), int(n_envs), int(first_step), int(n_steps),
                                                out.data_ptr(), self._stream()))
        return out

    def extract_egocentric_costmap(self, poses, resulting_origin=None, resulting_size=None, border_value=0, pool=1):
        """The costmap given to set_costmap seen from each of poses [n,3] -> uint8 [n, rows, cols] (robot at (0, 0)
        heading +x; resulting_origin / resulting_size in metres, both or neither).  pool > 1: the maximum of every
        pool x pool block of that image instead, [n, ceil(rows / pool), ceil(cols / pool)]
        (bcp_egocentric_costmaps_pooled)."""
        p = self._device_tensor(np.atleast_2d(poses) if not isinstance(poses, torch.Tensor) else poses, torch.float64)
        f64p = C.POINTER(C.c_double)
        org = sz = None
        if resulting_origin is not None:
            org = np.ascontiguousarray(resulting_origin, dtype=np.float64)
            sz = np.ascontiguousarray(resulting_size, dtype=np.float64)
        org_p = org.ctypes.data_as(f64p) if org is not None else None
        sz_p = sz.ctypes.data_as(f64p) if sz is not None else None
        shape = (C.c_int32 * 2)()
        if pool == 1:
            _lib.check(self._lib.bcp_egocentric_shape(self._h, sz_p, shape))
        else:
            _lib.check(self._lib.bcp_egocentric_pooled_shape(self._h, sz_p, int(pool), shape))
        out = torch.empty((p.shape[0], shape[0], shape[1]), dtype=torch.uint8, device=self.device)
        if pool == 1:
            _lib.check(self._lib.bcp_egocentric_costmaps(self._h, p.data_ptr(), p.shape[0], org_p, sz_p, int(border_value),
                                                         out.data_ptr(), self._stream()))
        else:
            _lib.check(self._lib.bcp_egocentric_costmaps_pooled(self._h, p.data_ptr(), p.shape[0], org_p, sz_p,
                                                                int(border_value), int(pool), out.data_ptr(), self._stream()))
        return out

    def range_scan(self, poses, beam_angles, max_range, want=()):
        """Range scans of the costmap given to set_costmap from each of poses [n,3] (bcp_range_scan): the distance in
        metres to the nearest lethal (254) cell along each of beam_angles [B], angles from the pose's heading,
        counter-clockwise; max_range where there is none within max_range -> float32 [n, B], or (ranges, *wanted) with
        want from "hit" (int32 [n, B], row * cols + col of the cell, -1 for none) and "heading_cs" (float64 [n, 2]).
        The (cos, sin) table of an angle set is uploaded once."""
        p = self._device_tensor(np.atleast_2d(poses) if not isinstance(poses, torch.Tensor) else poses, torch.float64)
        return self._range_scan(p, p.shape[0], beam_angles, max_range, want, lambda n, b, shapes, names: {
            name: torch.empty(shapes[name][0], dtype=shapes[name][1], device=self.device) for name in names})

    def inflate_costmap(self, data, resolution, cost_scaling_factor, footprint=None, inscribed_radius=None,
                        valid_rows=None, valid_cols=None, return_distance=False):
        """inflate_costmap(costmap, cost_scaling_factor, footprint).get_data() (costmap_inflation.py:73-92) for one map
        [rows, cols] or a batch [n, rows, cols], numpy or torch -> uint8 device tensor of the same shape
        (bcp_inflate_costmaps).  The robot enters through `inscribed_radius`, or through `footprint` [k, 2]
        (robots.inscribed_radius of it); neither = the handle's own footprint.  valid_rows / valid_cols int32 [n]: the
        true shape of every entry of a padded batch; the padding is ignored and comes out 0.  return_distance: also the
        float32 distance in cells to the nearest lethal cell (+inf on a map without one)."""
        d = self._device_tensor(data, torch.uint8)
        maps = d[None] if d.dim() == 2 else d
        assert maps.dim() == 3
        if inscribed_radius is None:
            inscribed_radius = robots.inscribed_radius(self.footprint() if footprint is None else footprint)
        assert (valid_rows is None) == (valid_cols is None)
        vr = self._device_tensor(valid_rows, torch.int32) if valid_rows is not None else None
        vc = self._device_tensor(valid_cols, torch.int32) if valid_cols is not None else None
        assert vr is None or (vr.shape == (maps.shape[0],) and vc.shape == (maps.shape[0],))
        out = torch.empty_like(maps)
        dist = torch.empty(maps.shape, dtype=torch.float32, device=self.device) if return_distance else None
        _lib.check(self._lib.bcp_inflate_costmaps(
            self._h, maps.data_ptr(), maps.shape[0], maps.shape[1], maps.shape[2],
            vr.data_ptr() if vr is not None else None, vc.data_ptr() if vc is not None else None, float(resolution),
            float(inscribed_radius), float(cost_scaling_factor), out.data_ptr(),
            dist.data_ptr() if dist is not None else None, self._stream()))
        out = out.reshape(d.shape)
        return (out, dist.reshape(d.shape)) if return_distance else out

    def goal_field(self, data, seeds, clearance_d2, valid=None, max_passes=0, want_info=False, extra_of_cost=None):
        """The geodesic cost-to-go of bcp_goal_field for one map [rows, cols] or a batch [n, rows, cols], numpy or torch ->
        uint16 device tensor of the same shape: min(length of the cheapest route through free space to the nearest seed,
        GOAL_FAR) in steps of GOAL_ORTHO / GOAL_DIAG, GOAL_NONE where there is none.  seeds: int32 (row, col) pairs, [S, 2]
        for one map or [n, S, 2] for a batch; one map with seeds [n, S, 2] is shared by n seed sets and gives n fields.
        clearance_d2: a cell is blocked iff an obstacle cell (== 254) lies within that squared distance in cells.
        valid: optional (valid_rows, valid_cols) int32 [n] each, the true shapes of a padded batch.  max_passes: 0 = as
        many as it takes.  want_info: also int32 [n, 2] = (cells with a value, gave_up).  extra_of_cost: None, or 256
        integers in [0, GOAL_MAX_EXTRA] indexed by the map's byte (bcp_goal_field_cost): entering a free cell c then costs
        the step plus extra_of_cost[data[c]], and the values are costs to go; goal_field.cost_table(w) makes the table for
        an inflated map.  A table of zeros gives the plain field."""
        d = self._device_tensor(data, torch.uint8)
        s = self._device_tensor(seeds, torch.int32)
        maps = d[None] if d.dim() == 2 else d
        assert maps.dim() == 3
        shared = d.dim() == 2 and s.dim() == 3
        s3 = s[None] if s.dim() == 2 else s
        n = s3.shape[0]
        assert s3.dim() == 3 and s3.shape[2] == 2 and (shared or n == maps.shape[0])
        vr = vc = None
        if valid is not None:
            vr, vc = (self._device_tensor(v, torch.int32, (n,)) for v in valid)
        out = torch.empty((n,) + tuple(maps.shape[1:]), dtype=torch.uint16, device=self.device)
        info = torch.zeros((n, 2), dtype=torch.int32, device=self.device) if want_info else None
        from .goal_field import call_fields, checked_table
        table = checked_table(extra_of_cost) if extra_of_cost is not None else None
        call_fields(self._lib, self._h, self._stream(), maps, shared, vr, vc, s3, clearance_d2, max_passes, out, info, table)
        self._alive["goal_field"] = (maps, s3, vr, vc)
        out = out[0] if d.dim() == 2 and s.dim() == 2 else out
        return (out, info) if want_info else out

    def scatter_boxes(self, data, origins, resolution, frame, yaw_cs, n_boxes, half_size, along=(0.2, 0.8), keep=None,
                      valid=None, seed=0, max_attempts=32):
        """Box obstacles stamped into a batch of maps (bcp_scatter_boxes, one launch): data uint8 [n, rows, cols] -- a
        contiguous tensor on the handle's device is written IN PLACE, anything else is copied there first -- with origins
        [n, 2] at `resolution`.  Entry m tries attempts 0 .. max_attempts - 1 and keeps the first n_boxes that are not
        rejected: a box with centre frame[m][0:2] + t * frame[m][2:4] + l * frame[m][4:6] (t uniform in `along`, l in
        (-1, 1)), half sizes uniform in `half_size` (metres) and one of the yaws of yaw_cs [n_yaws, 2] = (cos, sin); rejected
        when a corner leaves the entry's valid shape (valid = (valid_rows, valid_cols), None = the whole plane) or a cell of
        it lies within squared distance d2 of a keep-out (row, col, d2) of keep int32 [n, K, 3] (d2 < 0: unused).  The
        draws are Philox words of (seed, m, attempt): the same call gives the same boxes.
        -> (data, boxes int32 [n, n_boxes, 9] = (attempt, four (x, y) corners in cells), counts int32 [n]); the slots
        behind counts[m] are zeros.  Device tensors, no sync."""
        d = self._device_tensor(data, torch.uint8)
        assert d.dim() == 3
        bx, counts = boxes.scatter_boxes(self, d, origins, resolution, frame, yaw_cs, n_boxes, half_size, along, keep, valid,
                                         seed, max_attempts)
        return d, bx, counts

    def robot_step(self, state7, actions, noise_z=None):
        """state7 [n,7] rows {x,y,angle,v,w,steering_motor_command,wheel_angle}, actions [n,2] -> (new [n,7], err)."""
        st = self._device_tensor(state7, torch.float64).t().contiguous()  # SoA [7, n]
        a = self._device_tensor(actions, torch.float64)
        n = a.shape[0]
        z = self._device_tensor(noise_z, torch.float64) if noise_z is not None else None
        err = torch.zeros(n, dtype=torch.int32, device=self.device)
        _lib.check(self._lib.bcp_robot_step(self._h, st.data_ptr(), n, a.data_ptr(),
                                            z.data_ptr() if z is not None else None, err.data_ptr(), self._stream()))
        return st.t().contiguous(), err

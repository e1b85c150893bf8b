"""Box obstacles stamped into batches of maps (bcp_scatter_boxes, one launch): the raw call on caller tensors, and
BatchedPlanEnv.scatter_obstacles with what it derives from an env's binding before the call -- the frame of every entry's
path, the keep-outs about its start and goal, the table of yaws.  The reference has no counterpart: its obstacle-avoidance scenario
(rw_randomized_corridor_3_boxes.py) reads maps that exist only as a download."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .api import CostMap2D


def yaw_table(n_yaws):
    """float64 [n_yaws, 2]: (cos, sin) of the multiples of 2 pi / n_yaws"""
    ang = np.arange(int(n_yaws), dtype=np.float64) * (2.0 * np.pi / int(n_yaws))
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


def path_frames(starts, goals, lateral):
    """frame float64 [n, 6] = (start, goal - start, lateral * unit normal) of paths from starts [n, >= 2] to goals: a box
    centre is start + t * (goal - start) + l * lateral * normal with l in (-1, 1).  A path without extent gets no normal."""
    starts, goals = np.asarray(starts, dtype=np.float64), np.asarray(goals, dtype=np.float64)
    d = goals[:, :2] - starts[:, :2]
    norm = np.hypot(d[:, 0], d[:, 1])
    norm = np.where(norm > 0, norm, 1.0)
    normal = np.stack([-d[:, 1], d[:, 0]], axis=1) / norm[:, None]
    return np.ascontiguousarray(np.concatenate([starts[:, :2], d, float(lateral) * normal], axis=1))


def cells_of(points, origins, resolution):
    """(row, col) int64 [n, 2] of world points [n, >= 2] on maps with origins [n, 2]: world_to_pixel's expression"""
    inv = np.float64(1.0) / np.float64(resolution)
    col = np.rint((points[:, 0] - origins[:, 0]) * inv)
    row = np.rint((points[:, 1] - origins[:, 1]) * inv)
    return np.stack([row, col], axis=1).astype(np.int64)


def keep_outs(cells, d2):
    """keep int32 [n, K, 3] from K lists of cells [n, 2], all with squared radius d2"""
    keep = np.zeros((len(cells[0]), len(cells), 3), dtype=np.int32)
    for k, c in enumerate(cells):
        keep[:, k, :2] = c
    keep[:, :, 2] = int(d2)
    return keep


def scatter_boxes(handle, data, origins, resolution, frame, yaw_cs, n_boxes, half_size, along=(0.2, 0.8), keep=None,
                  valid=None, seed=0, max_attempts=32):
    """bcp_scatter_boxes on the device tensors of `handle`'s device: data uint8 [n, rows, cols] (contiguous, written in
    place), origins float64 [n, 2], frame float64 [n, 6], yaw_cs float64 [n_yaws, 2], keep int32 [n, K, 3] or None, valid
    (valid_rows, valid_cols) int32 [n] or None -> (boxes int32 [n, n_boxes, 9], counts int32 [n]); no sync."""
    assert data.dtype == torch.uint8 and data.dim() == 3 and data.is_contiguous() and data.device == handle.device
    n = int(data.shape[0])
    org = handle._device_tensor(origins, torch.float64, (n, 2))
    fr = handle._device_tensor(frame, torch.float64, (n, 6))
    yaw = handle._device_tensor(yaw_cs, torch.float64)
    assert yaw.dim() == 2 and yaw.shape[1] == 2
    kp = None
    if keep is not None:
        kp = handle._device_tensor(keep, torch.int32)
        assert kp.dim() == 3 and kp.shape[0] == n and kp.shape[2] == 3
    vr = vc = None
    if valid is not None and valid[0] is not None:
        vr, vc = (handle._device_tensor(v, torch.int32, (n,)) for v in valid)
    p = _lib.BcpScatterParams()
    p.n_boxes, p.max_attempts, p.n_yaws, p.seed = int(n_boxes), int(max_attempts), int(yaw.shape[0]), int(seed) & (2 ** 64 - 1)
    p.along[0], p.along[1] = float(along[0]), float(along[1])
    p.half_size[0], p.half_size[1] = float(half_size[0]), float(half_size[1])
    slots = min(max(int(n_boxes), 1), 64)   # (a refused n_boxes must not size an allocation)
    boxes = torch.empty((n, slots, 9), dtype=torch.int32, device=handle.device)
    counts = torch.empty((n,), dtype=torch.int32, device=handle.device)
    opt = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    _lib.check(handle._lib.bcp_scatter_boxes(
        handle._h, data.data_ptr(), n, int(data.shape[1]), int(data.shape[2]), opt(vr), opt(vc), org.data_ptr(),
        float(resolution), C.byref(p), fr.data_ptr(), opt(kp), int(kp.shape[1]) if kp is not None else 0, yaw.data_ptr(),
        boxes.data_ptr(), counts.data_ptr(), handle._stream()))
    handle._alive["scatter_boxes"] = (data, org, fr, yaw, kp, vr, vc)
    return boxes, counts


def scatter_obstacles(env, n_boxes, half_size, along=(0.2, 0.8), lateral=1.0, keep_clear=None, n_yaws=16, seed=0,
                      max_attempts=32, ensure_route=True, clearance=None):
    """BatchedPlanEnv.scatter_obstacles: see there."""
    if env.endless:
        raise RuntimeError("scatter_obstacles: not supported on endless=True pools -- refresh() re-samples bare worlds "
                           "into the pool")
    if env._shared_path or env._shared_map:
        raise RuntimeError("scatter_obstacles: needs private maps with private paths (a pool, or a map and a path per env)")
    if env._inflated:
        raise RuntimeError("scatter_obstacles: the costmaps of this env are inflated already -- scatter first, then inflate")
    data, vr, vc, _shared = env._bound_maps()
    origins = env._bound_origins()
    pts, lens = env._keep["path"], env._keep["lens"]
    n = int(data.shape[0])
    last = (lens.to(torch.int64) - 1).clamp(min=0)
    starts = pts[:, 0, :].cpu().numpy()
    goals = pts[torch.arange(n, device=env.device), last].cpu().numpy()
    org = origins.cpu().numpy()
    start_cells, goal_cells = cells_of(starts, org, env.resolution), cells_of(goals, org, env.resolution)
    if keep_clear is None:
        keep_clear = float(np.linalg.norm(env.footprint(), axis=1).max())
    d2 = (int(np.ceil(float(keep_clear) / env.resolution)) + 1) ** 2
    original = data.clone()
    bx, counts = scatter_boxes(env, data, origins, env.resolution, path_frames(starts, goals, lateral), yaw_table(n_yaws),
                               n_boxes, half_size, along, keep_outs([start_cells, goal_cells], d2), (vr, vc), seed, max_attempts)
    status = (counts < int(n_boxes)).to(torch.int32) * _lib.SCATTER_SHORT
    if ensure_route:
        fields = env.goal_field(clearance)
        sc = torch.from_numpy(start_cells).to(env.device)
        rows, cols = int(data.shape[1]), int(data.shape[2])
        inside = (sc[:, 0] >= 0) & (sc[:, 0] < rows) & (sc[:, 1] >= 0) & (sc[:, 1] < cols)
        # (uint16 planes cannot be indexed: as int16, GOAL_NONE reads -1)
        at = fields.field.view(torch.int16)[torch.arange(n, device=env.device), sc[:, 0].clamp(0, rows - 1),
                                            sc[:, 1].clamp(0, cols - 1)]
        cut = ~inside | (at == _lib.GOAL_NONE - 65536)
        data.copy_(torch.where(cut[:, None, None], original, data))
        status = status | cut.to(torch.int32) * _lib.SCATTER_REVERTED
    env._rebind_costmaps()
    if env._device_pool is None:   # the host copies behind envs[i].get_state().costmap: one per entry from now on
        host_maps, now = env._map_host, data.cpu().numpy()
        shapes = (np.stack([vr.cpu().numpy(), vc.cpu().numpy()], axis=1) if vr is not None
                  else np.tile(now.shape[1:], (n, 1)))
        old = [host_maps.of_entry(k) for k in range(n)]
        host_maps.replace([CostMap2D(now[k, :shapes[k][0], :shapes[k][1]].copy(), c.get_resolution(), c.get_origin())
                           for k, c in enumerate(old)])
    env.reset()
    return status, counts, bx

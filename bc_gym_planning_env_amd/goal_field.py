"""Goal fields for the whole batch: the geodesic cost-to-go of every bound map to its path's goal (bcp_goal_field, one
launch per build) and what it says at a pose -- distance to go and the direction of the route -- per env and step
(bcp_goal_field_sample, one tiny launch).  The terminal cost of a sampling planner, the dense shaping term and the
"direction to goal" feature of a navigation policy.  follow_refresh=True builds the fields from the handle's own binding
(bcp_goal_field_bound) and, on an endless pool, has every refresh() rebuild the fields of the entries it re-samples
(bcp_refresh_goal_fields).  cost_weight / extra_of_cost weigh the field by the costs of an inflated map
(bcp_goal_field_cost): routes then run down the middle of free space where there is room.  route_paths() makes the routes
down the fields the env's paths (bcp_goal_route_bound), smooth() / route_paths(smooth=...) pulls them taut and blends their
corners (bcp_smooth_route).  The reference has no
counterpart; the shape of the wrapper follows BatchedRangeScan (range_scan.py)."""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, robots
from .handle import SCAN_CACHE_ENTRIES, cached
from .wrappers import BatchedObservationWrapper


def clearance_cells_squared(clearance, resolution):
    """clearance in metres -> clearance_d2 of bcp_goal_field: floor((clearance / resolution)^2) in float64 (151 for the
    tricycle's inscribed radius at 0.03)."""
    return int(np.floor((np.float64(clearance) / np.float64(resolution)) ** 2))


def cost_table(cost_weight):
    """The table of bcp_goal_field_cost for a weight w >= 0: extra[c] = rint(w * 12 * c / 252) for the inflation layer's
    costs c <= 252, extra[253] = extra[252], extra[254] = extra[255] = 0 -- entering a cell of cost 252 costs 1 + w cells
    of travel, a cell of cost 0 the bare step.  uint16 [256]; ValueError for a weight that is negative, not finite, or so
    large that an entry would pass GOAL_MAX_EXTRA (w > 341.25)."""
    w = np.float64(cost_weight)
    if not np.isfinite(w) or w < 0:
        raise ValueError("cost_weight must be finite and >= 0, got %r" % (cost_weight,))
    extra = np.zeros(256, dtype=np.float64)
    extra[:253] = np.rint(w * 12.0 * np.arange(253, dtype=np.float64) / 252.0)
    extra[253] = extra[252]
    return checked_table(extra, "cost_weight %r" % (cost_weight,))


def checked_table(extra_of_cost, what="extra_of_cost"):
    """-> a contiguous uint16 [256] copy of the table, or ValueError: 256 integers in [0, GOAL_MAX_EXTRA]"""
    t = np.asarray(extra_of_cost)
    if t.shape != (256,) or not np.all(np.isfinite(t)) or np.any(t != np.rint(t)) or t.min() < 0 or t.max() > _lib.GOAL_MAX_EXTRA:
        raise ValueError("%s: the table must hold 256 integers in [0, %d]" % (what, _lib.GOAL_MAX_EXTRA))
    return np.ascontiguousarray(t, dtype=np.uint16)


class GoalField(object):
    """The fields of one owner's map binding (a BatchedPlanEnv, or a NativeOps after set_costmap): `field` uint16
    [entries, rows, cols] on the device (GOAL_NONE = no route; else route length in units of resolution / GOAL_ORTHO),
    `clearance_d2`, and `info` int32 [entries, 2] = (cells with a value, gave_up).  entries is 1 (every row reads field 0)
    or the owner's entry count (pool entries, else n_envs).  `extra_of_cost`: None for a plain field, else the uint16 [256]
    table the field was weighted with (bcp_goal_field_cost); the values are then costs to go, not lengths: metres() and
    sample()[..., 0] are the cost to go in metre-equivalents (a cell of extra e counts as 1 + e / 12 cells of travel)."""

    def __init__(self, owner, field, clearance_d2, info=None, keep=(), resolution=None, extra_of_cost=None):
        assert field.dtype == torch.uint16 and field.dim() == 3 and field.is_contiguous()
        self.owner, self.field, self.clearance_d2, self.info = owner, field, int(clearance_d2), info
        self.extra_of_cost = extra_of_cost
        self.resolution = float(owner.resolution if resolution is None else resolution)
        self.max_passes = 0         # of the build: what a following refresh() rebuilds with (build_bound)
        self._keep = keep           # the inputs of the build, alive until the stream has consumed them
        self._buffers = OrderedDict()
        self._route_cache = OrderedDict()   # route() / route_bound(): outputs per (n, max_len)
        self._smooth_cache = OrderedDict()  # smooth(): outputs per (n, max_len)

    def _call(self, final, poses, n, row_env, carrot_cells, max_dist, out3, cell_value, carrot):
        o, f = self.owner, self.field
        opt = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        if final:
            _lib.check(o._lib.bcp_final_goal_field_sample(o._h, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2], int(carrot_cells),
                                                          float(max_dist), out3.data_ptr(), opt(cell_value), opt(carrot), o._stream()))
        else:
            _lib.check(o._lib.bcp_goal_field_sample(o._h, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2], opt(poses), n,
                                                    opt(row_env), int(carrot_cells), float(max_dist), out3.data_ptr(),
                                                    opt(cell_value), opt(carrot), o._stream()))

    def sample(self, poses=None, row_env=None, carrot_cells=8, max_dist=np.inf, want=()):
        """bcp_goal_field_sample: poses None = every env's current pose (the delayed one under pose_delay), or [n, 3]; row i
        belongs to env row_env[i] (int32 [n]), or i % n_envs.  -> out3 float32 [n, 3] = (min(distance to go in metres,
        max_dist) -- on a weighted field the cost to go in metre-equivalents --, direction to the carrot in the robot frame), or (out3, *wanted) with want from "cell_value" (int32 [n],
        GOAL_NONE for a row without a result) and "carrot" (int32 [n, 2] = (row, col), (-1, -1) likewise).  The carrot is
        the cell reached by at most carrot_cells steps down the field.  Device tensors, no sync; the outputs are cached per
        n (the SCAN_CACHE_ENTRIES most recently used), so a caller that samples every tick allocates nothing."""
        o = self.owner
        unknown = set(want) - {"cell_value", "carrot"}
        if unknown:
            raise ValueError("sample: unknown outputs %s" % sorted(unknown))
        if poses is not None:
            poses = o._device_tensor(poses, torch.float64)
            assert poses.dim() == 2 and poses.shape[1] == 3
        if row_env is not None:
            row_env = o._device_tensor(row_env, torch.int32, (int(poses.shape[0]),))
        n = int(poses.shape[0]) if poses is not None else int(getattr(o, "n_envs", 1))
        shapes = {"out3": ((n, 3), torch.float32), "cell_value": ((n,), torch.int32), "carrot": ((n, 2), torch.int32)}
        buf = cached(self._buffers, n, dict, SCAN_CACHE_ENTRIES)
        for name in ["out3"] + list(want):
            if name not in buf:
                buf[name] = torch.zeros(shapes[name][0], dtype=shapes[name][1], device=o.device)
        self._call(False, poses, n, row_env, carrot_cells, max_dist, buf["out3"], buf.get("cell_value") if "cell_value" in want else None,
                   buf.get("carrot") if "carrot" in want else None)
        o._alive["goal_field_sample"] = (poses, row_env)
        return buf["out3"] if not want else (buf["out3"],) + tuple(buf[w] for w in want)

    def _route_buffers(self, n, max_len, want):
        shapes = {"paths": ((n, max_len, 3), torch.float64), "lens": ((n,), torch.int32), "status": ((n,), torch.int32),
                  "init": ((n, 2), torch.float64)}
        buf = cached(self._route_cache, (n, max_len), dict, SCAN_CACHE_ENTRIES)
        for name in ["paths", "lens", "status"] + list(want):
            if name not in buf:
                buf[name] = torch.zeros(shapes[name][0], dtype=shapes[name][1], device=self.owner.device)
        return buf

    def _bound_max_len(self):
        pts = self.owner._keep.get("path")
        if pts is None:
            raise ValueError("route: max_len=None needs an owner with paths bound")
        return int(pts.shape[-2])

    def route(self, poses=None, row_env=None, goals=None, stride=2, max_len=None, want=()):
        """bcp_goal_route: the route down the field from each row's pose to its goal, as a path.  Rows as for sample():
        poses None = every env's current pose, or [n, 3], row i on the map of env row_env[i] (or i % n_envs).  goals: [n, 3],
        or None = the last way point of the path bound for the row's entry.  A way point is written for the pose, for every
        stride-th cell of the walk, and for the goal; interior way points head for their successor.  max_len: the slots per
        row, None = the binding's max_len.  -> (paths float64 [n, max_len, 3] with zeros behind each row's way points, lens
        int32 [n], status int32 [n]: a mask of _lib.ROUTE_LONG / ROUTE_TOO_CLOSE / ROUTE_NO_ROUTE / ROUTE_STUCK), plus init
        float64 [n, 2] = (min_spat_dist_so_far, target_idx) of the owner's reward provider on each path with want=("init",).
        Device tensors, no sync; the outputs are cached per (n, max_len), so the next call with the same sizes overwrites
        them."""
        o, f = self.owner, self.field
        unknown = set(want) - {"init"}
        if unknown:
            raise ValueError("route: unknown outputs %s" % sorted(unknown))
        if poses is not None:
            poses = o._device_tensor(poses, torch.float64)
            assert poses.dim() == 2 and poses.shape[1] == 3
        n = int(poses.shape[0]) if poses is not None else int(getattr(o, "n_envs", 1))
        if row_env is not None:
            row_env = o._device_tensor(row_env, torch.int32, (n,))
        if goals is not None:
            goals = o._device_tensor(goals, torch.float64, (n, 3))
        max_len = self._bound_max_len() if max_len is None else int(max_len)
        buf = self._route_buffers(n, min(max(max_len, 1), 32766), want)
        opt = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        _lib.check(o._lib.bcp_goal_route(o._h, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2], opt(poses), n, opt(row_env),
                                         opt(goals), int(stride), max_len, buf["paths"].data_ptr(), buf["lens"].data_ptr(),
                                         buf["init"].data_ptr() if "init" in want else None, buf["status"].data_ptr(),
                                         o._stream()))
        o._alive["goal_route"] = (poses, row_env, goals)
        return (buf["paths"], buf["lens"], buf["status"]) + tuple(buf[w] for w in want)

    def route_bound(self, stride=2, max_len=None, want=()):
        """bcp_goal_route_bound: row m is entry m of the owner's own binding, from its bound path's first way point to its
        last.  Needs private maps with private paths and a field per entry.  Returns what route() returns."""
        o, f = self.owner, self.field
        unknown = set(want) - {"init"}
        if unknown:
            raise ValueError("route_bound: unknown outputs %s" % sorted(unknown))
        max_len = self._bound_max_len() if max_len is None else int(max_len)
        buf = self._route_buffers(int(f.shape[0]), min(max(max_len, 1), 32766), want)
        _lib.check(o._lib.bcp_goal_route_bound(o._h, f.data_ptr(), f.shape[1], f.shape[2], int(stride), max_len,
                                               buf["paths"].data_ptr(), buf["lens"].data_ptr(),
                                               buf["init"].data_ptr() if "init" in want else None, buf["status"].data_ptr(),
                                               o._stream()))
        return (buf["paths"], buf["lens"], buf["status"]) + tuple(buf[w] for w in want)

    def smooth(self, paths, lens, row_env=None, entries=False, look=64, blend=0.3, delta=0.05, halvings=2, max_len=None,
               want=()):
        """bcp_smooth_route: the way points paths float64 [n, max_len_in, 3] / lens int32 [n] -- a route at stride 1 -- pulled
        taut over the field (an anchor keeps the farthest of its next `look` way points it sees over passable cells) and
        every corner blended over `blend` metres of each leg (halved up to `halvings` times where the blend would leave the
        passable cells), written out every `delta` metres.  Rows as for route(): row i on the map of env row_env[i] (or
        i % n_envs); entries=True: row m is entry m of the owner's binding, as for route_bound().  max_len: the slots per
        row, None = max_len_in.  -> (paths float64 [n, max_len, 3] with zeros behind each row's way points, lens int32 [n],
        status int32 [n]: a mask of _lib.ROUTE_LONG / ROUTE_TOO_CLOSE / ROUTE_NO_ROUTE / SMOOTH_BLOCKED), plus, with want from
        "init" (float64 [n, 2], as route()'s) and "info" (int32 [n, 4] = vertices kept, corners blended at full size, at a
        reduced size, left sharp).  Device tensors, no sync; the outputs are cached per (n, max_len)."""
        o, f = self.owner, self.field
        unknown = set(want) - {"init", "info"}
        if unknown:
            raise ValueError("smooth: unknown outputs %s" % sorted(unknown))
        paths = o._device_tensor(paths, torch.float64)
        assert paths.dim() == 3 and paths.shape[2] == 3
        n, max_len_in = int(paths.shape[0]), int(paths.shape[1])
        lens = o._device_tensor(lens, torch.int32, (n,))
        if row_env is not None:
            row_env = o._device_tensor(row_env, torch.int32, (n,))
        max_len = max_len_in if max_len is None else int(max_len)
        buf = cached(self._smooth_cache, (n, min(max(max_len, 1), 4096)), dict, SCAN_CACHE_ENTRIES)
        shapes = {"paths": ((n, min(max(max_len, 1), 4096), 3), torch.float64), "lens": ((n,), torch.int32),
                  "status": ((n,), torch.int32), "init": ((n, 2), torch.float64), "info": ((n, 4), torch.int32)}
        for name in ["paths", "lens", "status"] + list(want):
            if name not in buf:
                buf[name] = torch.zeros(shapes[name][0], dtype=shapes[name][1], device=o.device)
        prm = _lib.BcpSmoothParams(int(look), int(halvings), float(blend), float(delta))
        _lib.check(o._lib.bcp_smooth_route(o._h, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2], paths.data_ptr(),
                                           lens.data_ptr(), max_len_in, n, row_env.data_ptr() if row_env is not None else None,
                                           int(bool(entries)), prm, max_len, buf["paths"].data_ptr(), buf["lens"].data_ptr(),
                                           buf["init"].data_ptr() if "init" in want else None, buf["status"].data_ptr(),
                                           buf["info"].data_ptr() if "info" in want else None, o._stream()))
        o._alive["smooth_route"] = (paths, lens, row_env)
        return (buf["paths"], buf["lens"], buf["status"]) + tuple(buf[w] for w in want)

    def metres(self):
        """float32 [entries, rows, cols]: the fields in metres -- on a weighted field (extra_of_cost) the cost to go in
        metre-equivalents --, inf where there is no route."""
        f = self.field.to(torch.int32)
        scale = self.resolution / _lib.GOAL_ORTHO
        return torch.where(f == _lib.GOAL_NONE, torch.full((), float("inf"), device=f.device), f.to(torch.float32) * scale)


def path_seeds(env, which):
    """int32 [fields, S, 2] (row, col) seeds from the paths the env has bound, by world_to_pixel on each entry's origin:
    "goal" = the last way point of each entry's path, "path" = every way point, filled with (-1, -1) up to max_len."""
    if which not in ("goal", "path"):
        raise ValueError('seeds must be "goal" or "path", got %r' % (which,))
    pts, lens = env._keep["path"], env._keep["lens"]
    dev = env.device
    if lens is None:
        pts, lens = pts[None], torch.full((1,), int(pts.shape[0]), dtype=torch.int32, device=dev)
    origins = env._bound_origins()
    inv_res = 1.0 / float(env.resolution)
    cells = torch.round((pts[..., :2] - origins[:, None, :]) * inv_res)       # [fields, L, 2] = (col, row), half to even
    cells = torch.nan_to_num(cells, nan=-1.0).clamp(-1.0, 1e9).to(torch.int32)
    n_fields, length = int(cells.shape[0]), int(cells.shape[1])
    lens = lens.to(torch.int64).expand(n_fields)
    rc = torch.stack([cells[..., 1], cells[..., 0]], dim=-1)
    if which == "goal":
        last = (lens - 1).clamp(min=0)
        return rc[torch.arange(n_fields, device=dev), last][:, None, :].contiguous()
    if length > 4096:
        raise ValueError('seeds="path": paths of more than 4096 way points are not supported (max_len %d)' % length)
    beyond = torch.arange(length, device=dev)[None, :] >= lens[:, None]
    return torch.where(beyond[..., None], torch.full((), -1, dtype=torch.int32, device=dev), rc).contiguous()


def call_fields(lib, handle, stream, maps, shared, vr, vc, seeds, d2, max_passes, out, info, table=None):
    """The one call of bcp_goal_field -- or, with a checked table (checked_table, cost_table), bcp_goal_field_cost -- on
    device tensors: maps uint8 [., rows, cols], seeds int32 [n, S, 2], vr / vc int32 [n] or None, out uint16 [n, rows, cols],
    info int32 [n, 2] or None.  The table is read during the call: a launch carries its own copy."""
    head = (handle, maps.data_ptr(), int(seeds.shape[0]), int(maps.shape[1]), int(maps.shape[2]), int(bool(shared)),
            vr.data_ptr() if vr is not None else None, vc.data_ptr() if vc is not None else None, seeds.data_ptr(),
            int(seeds.shape[1]), int(d2), int(max_passes))
    tail = (out.data_ptr(), info.data_ptr() if info is not None else None, stream)
    if table is None:
        _lib.check(lib.bcp_goal_field(*(head + tail)))
    else:
        _lib.check(lib.bcp_goal_field_cost(*(head + (table.ctypes.data,) + tail)))


def build_bound(env, d2, max_passes):
    """The fields of every entry of the env's own binding, seeds derived on the device (bcp_goal_field_bound); on an
    endless env the GoalField is registered with it, and every refresh() rebuilds the fields of the entries it re-samples."""
    if env.endless:
        env.finish_refresh()
    data, _vr, _vc, shared = env._bound_maps()
    if shared:
        raise _lib.BcpError("goal_field(follow_refresh=True): needs private maps with private paths (a pool, or a map "
                            "and a path per env); a shared map is served by the default build")
    n, rows, cols = (int(v) for v in data.shape)
    field = torch.empty((n, rows, cols), dtype=torch.uint16, device=env.device)
    info = torch.zeros((n, 2), dtype=torch.int32, device=env.device)
    _lib.check(env._lib.bcp_goal_field_bound(env._h, None, None, n, d2, int(max_passes), field.data_ptr(), info.data_ptr(),
                                             env._stream()))
    fields = GoalField(env, field, d2, info, keep=(data,))
    fields.max_passes = int(max_passes)
    if env.endless:
        env._follow_goal_fields(fields)
    return fields


def build(env, clearance=None, seeds="goal", max_passes=0, follow_refresh=False, cost_weight=None, extra_of_cost=None):
    """BatchedPlanEnv.goal_field: see there."""
    if cost_weight is not None and extra_of_cost is not None:
        raise ValueError("goal_field: pass one of cost_weight and extra_of_cost")
    weighted = cost_weight is not None or extra_of_cost is not None
    if weighted and follow_refresh:
        raise ValueError("goal_field: cost_weight / extra_of_cost do not go with follow_refresh=True -- the worlds of an "
                         "endless pool are not inflated, so there are no costs to weigh")
    table = None
    if cost_weight is not None:
        table = cost_table(cost_weight)
        if not env._inflated:
            raise RuntimeError("goal_field(cost_weight=...): the costmaps of this env were never inflated, so every cost "
                               "is 0 or 254 -- call inflate_costmaps() first (an explicit extra_of_cost is taken on any map)")
    elif extra_of_cost is not None:
        table = checked_table(extra_of_cost)
    if env.endless and not follow_refresh:
        raise RuntimeError("goal_field: refused on endless=True pools unless follow_refresh=True -- refresh() re-samples "
                           "worlds into the pool, which would leave stale fields")
    if follow_refresh and seeds != "goal":
        if seeds not in ("goal", "path"):
            raise ValueError('seeds must be "goal" or "path", got %r' % (seeds,))
        raise ValueError('goal_field(follow_refresh=True) needs seeds="goal": the way-point seed set is not derived on the '
                         'device')
    if clearance is None:
        clearance = robots.inscribed_radius(env.footprint())
    d2 = clearance_cells_squared(clearance, env.resolution)
    if follow_refresh:
        return build_bound(env, d2, max_passes)
    s = path_seeds(env, seeds)
    data, vr, vc, shared = env._bound_maps()
    n, rows, cols = int(s.shape[0]), int(data.shape[1]), int(data.shape[2])
    assert shared or n == int(data.shape[0])   # (one path for private maps: its way points on every entry's origin)
    field = torch.empty((n, rows, cols), dtype=torch.uint16, device=env.device)
    info = torch.zeros((n, 2), dtype=torch.int32, device=env.device)
    call_fields(env._lib, env._h, env._stream(), data, shared and n > 1, vr, vc, s, d2, max_passes, field, info, table)
    return GoalField(env, field, d2, info, keep=(s, data, vr, vc), extra_of_cost=table)


def route_paths(env, fields=None, stride=2, max_len=None, clearance=None, cost_weight=None, smooth=None):
    """BatchedPlanEnv.route_paths: see there."""
    if env.endless:
        raise RuntimeError("route_paths: not supported on endless=True pools -- refresh() re-samples worlds with "
                           "straight paths into the pool")
    if env._shared_path or env._shared_map:
        raise RuntimeError("route_paths: needs private maps with private paths (a pool, or a map and a path per env)")
    if fields is not None and clearance is not None:
        raise ValueError("route_paths: clearance belongs to the build of the fields; pass one of fields and clearance")
    if fields is not None and cost_weight is not None:
        raise ValueError("route_paths: cost_weight belongs to the build of the fields; pass one of fields and cost_weight")
    if fields is None:
        fields = env.goal_field(clearance, cost_weight=cost_weight)
    data, old_pts, old_lens = env._keep["map"], env._keep["path"], env._keep["lens"]
    if fields.owner is not env or tuple(fields.field.shape) != tuple(data.shape):
        raise ValueError("route_paths: fields must be this env's, one per entry: %s expected, got %s"
                         % (tuple(data.shape), tuple(fields.field.shape)))
    old_len = int(old_pts.shape[1])
    max_len = old_len if max_len is None else int(max_len)
    if smooth is None:
        paths, lens, status, init = fields.route_bound(stride, max_len, want=("init",))
        status = status.clone()
        ok = status == 0
    else:   # the route at stride 1 into a scratch buffer, and that smoothed: an entry needs both to succeed
        prm = dict(smooth)
        route_len = int(prm.pop("route_len", 1024))
        unknown = set(prm) - {"look", "blend", "delta", "halvings"}
        if unknown:
            raise ValueError("route_paths: unknown smooth parameters %s" % sorted(unknown))
        cells, cell_lens, route_status = fields.route_bound(1, route_len)
        paths, lens, status, init = fields.smooth(cells, cell_lens, entries=True, max_len=max_len, want=("init",), **prm)
        status = status | route_status
        ok = (status & ~_lib.SMOOTH_BLOCKED) == 0
    length = max(max_len, old_len)
    new_pts = torch.zeros((int(old_pts.shape[0]), length, 3), dtype=torch.float64, device=env.device)
    new_pts[:, :old_len] = old_pts
    routed = torch.zeros_like(new_pts)
    routed[:, :max_len] = paths
    new_pts = torch.where(ok[:, None, None], routed, new_pts).contiguous()
    new_lens = torch.where(ok, lens, old_lens).contiguous()
    if length == old_len:   # nothing grows: the bound tensors themselves (a device pool's own) take the routes
        new_pts, new_lens = old_pts.copy_(new_pts), old_lens.copy_(new_lens)
    first = env._initial_state
    first.min_spat_dist_so_far.copy_(torch.where(ok, init[:, 0], first.min_spat_dist_so_far))
    first.target_idx.copy_(torch.where(ok, init[:, 1].to(torch.int32), first.target_idx))
    env._bind_paths(new_pts, new_lens)
    env._bind(first, env._lib.bcp_bind_initial_state)
    dp = env._device_pool
    if dp is not None:   # (env._paths hands out copies of these on demand)
        dp.path_points, dp.lens = new_pts, new_lens
        dp.init.copy_(torch.stack([first.min_spat_dist_so_far, first.target_idx.to(torch.float64)], dim=1))
    else:   # the host copies behind path_of(i): one per entry from now on
        host = env._path_host
        pts_host, lens_host, ok_host = new_pts.cpu().numpy(), new_lens.cpu().numpy(), ok.cpu().numpy()
        host.replace([pts_host[k, :lens_host[k]].copy() if ok_host[k] else host.of_entry(k) for k in range(host.n_entries)])
    env.reset()
    return status


class BatchedGoalField(BatchedObservationWrapper):
    """Observation wrapper around a BatchedPlanEnv (or a pool env): step() / reset() return
    OrderedDict(goal_field=float32 [N, 3, 1], goal_n_state=float32 [N, 9, 1]) device tensors (8 rows for a diff-drive
    robot).  goal_field is (min(distance to go, max_dist) in metres, dir_x, dir_y) straight from bcp_goal_field_sample: the
    unit vector, in the robot frame, towards the cell carrot_cells steps down the field.  The fields are built once, in the
    constructor (env.goal_field(clearance)); an observation costs two launches.  goal_n_state is the egocentric wrapper's
    vector with world size (max_dist, max_dist).
    follow_refresh=True: the fields are built by env.goal_field(clearance, follow_refresh=True) -- on an endless=True env
    every refresh() then rebuilds the fields of the entries it re-samples, and the observation follows worlds that never
    repeat.
    final_observation=True: step() adds info["final_observation"] (BatchedObservationWrapper), sampled at every ended
    episode's final pose on the field of the map it ran on."""

    def __init__(self, env, carrot_cells=8, clearance=None, max_dist=10.0, final_observation=False, follow_refresh=False):
        super(BatchedGoalField, self).__init__(env)
        self.carrot_cells, self.max_dist = int(carrot_cells), float(max_dist)
        self.fields = env.goal_field(clearance, follow_refresh=True) if follow_refresh else env.goal_field(clearance)
        self._world = np.array([self.max_dist, self.max_dist], dtype=np.float64)
        self.goal_field = self._vector(env.n_envs)
        self.goal_n_state = self._goal_vector(env.n_envs)
        self._obs = OrderedDict((('goal_field', self.goal_field), ('goal_n_state', self.goal_n_state)))
        self._init_final(final_observation)

    def _vector(self, rows):
        return torch.zeros((rows, 3, 1), dtype=torch.float32, device=self.env.device)

    def observation(self, _observation=None):
        """Refresh and return the observation of the envs' current state (device tensors, no sync)."""
        e = self.env
        self.fields._call(False, None, e.n_envs, None, self.carrot_cells, self.max_dist, self.goal_field, None, None)
        _lib.check(self._lib.bcp_goal_n_state(e._h, self._world.ctypes.data_as(_lib._f64p), self.goal_n_state.data_ptr(),
                                              self._stream()))
        return self._obs

    def _alloc_final(self, cap):
        self.final_goal_field, self.final_vector = self._vector(cap), self._goal_vector(cap)
        return OrderedDict((('goal_field', self.final_goal_field), ('goal_n_state', self.final_vector)))

    def _draw_final(self, stream):
        e = self.env
        self.fields._call(True, None, 0, None, self.carrot_cells, self.max_dist, self.final_goal_field, None, None)
        _lib.check(self._lib.bcp_final_goal_n_state(e._h, self._world.ctypes.data_as(_lib._f64p),
                                                    self.final_vector.data_ptr(), stream))

"""What every owner of a libbcplan handle shares (BatchedPlanEnv, NativeOps, mini_env.PoseCollider): the library, the
bcp_handle and its device, the launch stream, the way inputs reach the device, tuning, seeding, range scans, and the
handle's end."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

SCAN_CACHE_ENTRIES = 8   # beam tables / output buffer sets of range_scan kept per handle (least recently used go first)


def cached(cache, key, make, limit=None):
    """cache[key] (an OrderedDict, least recently used first), made by make() on first use; with a limit, the entries
    used longest ago beyond it go -- a caller that sweeps keys does not pile up device memory."""
    if key in cache:
        cache.move_to_end(key)
    else:
        cache[key] = make()
        while limit is not None and len(cache) > limit:
            cache.popitem(last=False)
    return cache[key]


def beam_table_cached(tables, beam_angles, device):
    """The device table [B, 2] of (cos, sin) of beam_angles for bcp_range_scan, from `tables` (an OrderedDict keyed by the
    angles' bytes, least recently used first) or uploaded and added to it; at most SCAN_CACHE_ENTRIES tables are kept."""
    angles = np.ascontiguousarray(beam_angles.detach().cpu().numpy() if isinstance(beam_angles, torch.Tensor) else beam_angles,
                                  dtype=np.float64).reshape(-1)
    return cached(tables, angles.tobytes(), lambda: torch.from_numpy(
        np.stack([np.cos(angles), np.sin(angles)], axis=1)).to(device).contiguous(), SCAN_CACHE_ENTRIES)


class Handle(object):
    """A bcp_handle for `n_envs` envs on `device`, created from BcpParams; destroyed by close() or with the object."""

    # set_tuning's knobs, in the order they are applied
    TUNING = OrderedDict((
        ("exact_mode", _lib.TUNE_EXACT_MODE), ("dense_threshold", _lib.TUNE_DENSE_THRESHOLD), ("cull", _lib.TUNE_CULL),
        ("defer", _lib.TUNE_DEFER), ("edt_lds", _lib.TUNE_EDT_LDS), ("fused", _lib.TUNE_FUSED),
        ("ego_sparse", _lib.TUNE_EGO_SPARSE), ("local_pairs", _lib.TUNE_LOCAL_PAIRS),
        ("ego_list_stride", _lib.TUNE_EGO_LIST_STRIDE), ("near_dilate", _lib.TUNE_NEAR_DILATE),
        ("near_shift", _lib.TUNE_NEAR_SHIFT), ("local_shared", _lib.TUNE_LOCAL_SHARED)))
    _h = None   # (close() may run on an object whose constructor raised)

    def __init__(self, bcp_params, n_envs, device, env_id_base=0, needs_gpu=None):
        self._lib = _lib.load()  # raises when libbcplan.so is missing: no fallback
        if not torch.cuda.is_available():
            raise RuntimeError("%s needs a GPU (libbcplan has no CPU path)" % (needs_gpu or type(self).__name__))
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._bcp_params = bcp_params
        self._keep = {}            # device buffers the library holds pointers to
        self._alive = {}           # call name -> the inputs of its last launch, alive until the stream has consumed them
        self._beam_tables = OrderedDict()
        self._h = C.c_void_p()
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self._lib.bcp_create(C.byref(bcp_params), int(n_envs), index, int(env_id_base), C.byref(self._h)))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _device_tensor(self, x, dtype=None, shape=None):
        """A tensor, or anything numpy can wrap, on the handle's device and contiguous.  dtype None keeps float32 / float64
        and widens everything else to float64; a shape, if given, is asserted."""
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if dtype is None:
            dtype = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float64
        x = x.to(self.device).to(dtype).contiguous()
        assert shape is None or tuple(x.shape) == shape
        return x

    def footprint(self):
        """The footprint [n_verts, 2] in metres the handle was created with (footprint_scale applied)."""
        p = self._bcp_params
        return np.array([[p.verts[k][0], p.verts[k][1]] for k in range(p.n_verts)], dtype=np.float64)

    def seed(self, seed=None):
        """Seeds the on-device odometry-noise stream (the reference draws from numpy's global RNG)."""
        if seed is not None:
            _lib.check(self._lib.bcp_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_tuning(self, **knobs):
        """Execution knobs of libbcplan (bcp_set_tuning), the keys of TUNING; results never depend on them.  (`cull` must be
        chosen before the costmaps are bound; near_shift takes effect when they are bound the next time.)"""
        unknown = set(knobs) - set(self.TUNING)
        if unknown:
            raise TypeError("set_tuning() got unexpected keyword arguments %s" % sorted(unknown))
        for name, key in self.TUNING.items():
            if knobs.get(name) is not None:
                _lib.check(self._lib.bcp_set_tuning(self._h, key, int(knobs[name])))

    def _range_scan(self, poses, n, beam_angles, max_range, want, alloc):
        """bcp_range_scan from poses [n, 3] (None: every env's current pose) into alloc(n, B, shapes, names), a dict of
        buffers for `names`, shapes[name] = (shape, dtype).  The (cos, sin) table of an angle set is uploaded once.
        Returns ranges, or (ranges, *wanted in the order given)."""
        table = beam_table_cached(self._beam_tables, beam_angles, self.device)
        unknown = set(want) - {"hit", "heading_cs"}
        if unknown:
            raise ValueError("range_scan: unknown outputs %s" % sorted(unknown))
        b = int(table.shape[0])
        out = alloc(n, b, {"ranges": ((n, b), torch.float32), "hit": ((n, b), torch.int32),
                           "heading_cs": ((n, 2), torch.float64)}, ["ranges"] + list(want))
        _lib.check(self._lib.bcp_range_scan(
            self._h, poses.data_ptr() if poses is not None else None, n, table.data_ptr(), b, float(max_range),
            out["ranges"].data_ptr(), out["hit"].data_ptr() if "hit" in out else None,
            out["heading_cs"].data_ptr() if "heading_cs" in out else None, self._stream()))
        self._alive["range_scan"] = (table, poses)
        return out["ranges"] if not want else (out["ranges"],) + tuple(out[w] for w in want)

    def path_speed(self, paths, lens, v_max, a_lat, w_max, a_dec, a_acc, v_start=None, v_end=None, v_min=0.0, span=1, want=()):
        """A speed per way point of any paths (bcp_path_speed, one launch, nothing of the handle changes): paths float64
        [n, max_len, 3] with lens [n] way points each, e.g. what GoalField.route() or GoalField.smooth() return.  No faster
        than v_max, than sqrt(a_lat / kappa) and than w_max / kappa at a way point of curvature kappa (the Menger curvature
        of the way points `span` before and behind), no slower than v_min for curvature's sake; at most v_start / v_end
        (None: v_max) at the two ends; braking with at most a_dec and accelerating with at most a_acc along the path.
        want: optional outputs from "kappa" and "v_limit".  Returns a speed_profile.SpeedProfile of device tensors, no sync."""
        from . import speed_profile
        p = self._device_tensor(paths, torch.float64)
        assert p.dim() == 3 and p.shape[2] == 3
        return speed_profile.path_speed(self, p, self._device_tensor(lens, torch.int32, (int(p.shape[0]),)),
                                        speed_profile.speed_params(v_max, a_lat, w_max, a_dec, a_acc, v_start, v_end, v_min, span),
                                        want)

    def close(self):
        if self._h:
            self._lib.bcp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

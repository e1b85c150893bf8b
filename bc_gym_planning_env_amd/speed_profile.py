"""Speed profiles of paths (bcp_path_speed): a speed per way point that slows for curvature, brakes in time for what lies
ahead and accelerates no harder than allowed -- what BatchedPlanEnv.track(speed_profile=...) and TrackingPlanner follow.
The contract is in include/bcplan.h; the arithmetic in csrc/bcp_speed_cell.h."""
import ctypes as C

import torch

from . import _lib

WANT = ("kappa", "v_limit")


class SpeedProfile(object):
    """What path_speed() / BatchedPlanEnv.speed_profile() return: device tensors, no sync.  `speed` float64 [n, max_len]
    ([max_len] for an env's shared path) in m/s, +0.0 behind a row's way points; `status` int32 [n], 0 or
    _lib.SPEED_NO_PATH (the row is zeros); optional, None unless asked for: `kappa` (1/m, the curvature read at every way
    point) and `v_limit` (m/s, what the way point alone allows).  `params`: the dict of the parameters used.  `owner` and
    `epoch`: the env whose bound paths the profile was made for and the count of its path bindings at that moment
    (None, None for a profile of other paths): track() refuses a profile of an earlier binding."""

    def __init__(self, speed, status, params, kappa=None, v_limit=None, owner=None, epoch=None):
        self.speed, self.status, self.params = speed, status, params
        self.kappa, self.v_limit = kappa, v_limit
        self.owner, self.epoch = owner, epoch

    @property
    def max_len(self):
        return int(self.speed.shape[-1])


def speed_params(v_max, a_lat, w_max, a_dec, a_acc, v_start=None, v_end=None, v_min=0.0, span=1):
    """-> (the dict a SpeedProfile keeps, the bcp_speed_params of it); v_start / v_end None: v_max"""
    prm = dict(span=int(span), v_max=float(v_max), v_min=float(v_min), a_lat=float(a_lat), w_max=float(w_max),
               a_dec=float(a_dec), a_acc=float(a_acc), v_start=float(v_max if v_start is None else v_start),
               v_end=float(v_max if v_end is None else v_end))
    p = _lib.BcpSpeedParams()
    for name, value in prm.items():
        setattr(p, name, value)
    return prm, p


def path_speed(handle, paths, lens, prm, want=(), owner=None, epoch=None):
    """The one call of bcp_path_speed on device tensors: paths float64 [n, max_len, 3], lens int32 [n]; prm: speed_params'
    pair.  -> SpeedProfile with speed [n, max_len]."""
    unknown = set(want) - set(WANT)
    if unknown:
        raise ValueError("path_speed: unknown outputs %s" % sorted(unknown))
    assert paths.dim() == 3 and paths.shape[2] == 3 and tuple(lens.shape) == (paths.shape[0],)
    n, max_len = int(paths.shape[0]), int(paths.shape[1])
    out = {name: torch.empty((n, max_len), dtype=torch.float64, device=handle.device) for name in ("speed",) + tuple(
        w for w in WANT if w in want)}
    status = torch.empty(n, dtype=torch.int32, device=handle.device)
    _lib.check(handle._lib.bcp_path_speed(handle._h, paths.data_ptr(), lens.data_ptr(), max_len, n, C.byref(prm[1]),
                                          out["speed"].data_ptr(), out["kappa"].data_ptr() if "kappa" in out else None,
                                          out["v_limit"].data_ptr() if "v_limit" in out else None, status.data_ptr(),
                                          handle._stream()))
    handle._alive["path_speed"] = (paths, lens)   # alive until the stream has consumed them
    return SpeedProfile(out["speed"], status, prm[0], out.get("kappa"), out.get("v_limit"), owner, epoch)

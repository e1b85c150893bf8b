"""The contract of bcp_goal_field_bound / bcp_refresh_goal_fields restated in numpy: the seed cell of a bound path's last
way point and the order of the refusals.  The fields themselves are tests/goal_field_ref.py's."""
import numpy as np

NO_CELL = -12345        # what tests/c_abi/goal_seed_main.cpp leaves in (row, col) of a refused seed


def seed_of_path(x, y, ox, oy, inv_res, vr, vc):
    """-> (usable, row, col): numpy.rint (half to even) of ((x - ox) * inv_res, (y - oy) * inv_res) and a range test made
    on the float64 values; a way point that is not finite, or whose cell lies outside (vr, vc), gives no seed"""
    with np.errstate(all="ignore"):
        fc = np.rint((np.float64(x) - np.float64(ox)) * np.float64(inv_res))
        fr = np.rint((np.float64(y) - np.float64(oy)) * np.float64(inv_res))
    if not (np.isfinite(x) and np.isfinite(y)) or not (0.0 <= fc < float(vc) and 0.0 <= fr < float(vr)):
        return 0, NO_CELL, NO_CELL
    return 1, int(fr), int(fc)


def check_bound_args(have_handle, have_field, n_list, n_entries, have_entries, have_count, clearance_d2, max_passes, have_map,
                     have_path, shared_map, shared_path, rows, cols, refresh_form, refresh_pending):
    """goal_bound_check_args: 1 .. 6 are BCP_E_INVALID, 7 .. 10 BCP_E_STATE"""
    if not have_handle:
        return 1
    if not have_field:
        return 2
    if not refresh_form and (n_list < 0 or n_list > n_entries):
        return 3
    if not refresh_form and have_count and not have_entries:
        return 4
    if clearance_d2 < 0 or clearance_d2 > 127 * 127:
        return 5
    if max_passes < 0:
        return 6
    if not have_map or not have_path:
        return 7
    if shared_map or shared_path:
        return 8
    if rows < 1 or rows > 2048 or cols < 1 or cols > 2048:
        return 9
    if refresh_form and not refresh_pending:
        return 10
    return 0

"""ctypes binding of libbcplan.so (include/bcplan.h).  There is no fallback: if the HIP library is missing or no
GPU is visible, creating an env raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbcplan.so")

ABI_VERSION = 2
MAX_VERTS = 32
MODEL_TRICYCLE, MODEL_DIFFDRIVE = 0, 1
REWARD_CONTINUOUS, REWARD_PURE_PURSUIT = 0, 1
STEP_AUTO_RESET, STEP_ACTIONS_F32 = 1, 2
LOOKAHEAD_PER_ENV = 1 << 8
ERR_ANGLE_JUMP, ERR_TIME_ORDER, ERR_INTERNAL = 1, 2, 4
DONE_GOAL, DONE_TIMEOUT, DONE_COLLIDED = 1, 2, 4
TUNE_EXACT_MODE, TUNE_DENSE_THRESHOLD, TUNE_CULL, TUNE_DEFER, TUNE_EDT_LDS, TUNE_FUSED, TUNE_EGO_SPARSE, TUNE_NEAR_DILATE = 0, 1, 2, 3, 4, 5, 6, 7
TUNE_LOCAL_PAIRS, TUNE_EGO_LIST_STRIDE, TUNE_NEAR_SHIFT, TUNE_INFLATE_ROUTE, TUNE_GOAL_ROUTE = 8, 9, 10, 11, 12
TUNE_LOCAL_SHARED = 13
GOAL_ORTHO, GOAL_DIAG, GOAL_FAR, GOAL_NONE = 12, 17, 65534, 65535
GOAL_MAX_EXTRA = 4095
ROUTE_LONG, ROUTE_TOO_CLOSE, ROUTE_NO_ROUTE, ROUTE_STUCK = 1, 2, 4, 8
SMOOTH_BLOCKED = 16   # bcp_smooth_route's status bit beside the ROUTE_* ones
SPEED_NO_PATH = 4     # bcp_path_speed's status of a row without a path
SCATTER_SHORT, SCATTER_REVERTED = 1, 2   # BatchedPlanEnv.scatter_obstacles' status bits
E_NO_DEVICE = -2
OPT_DIFFDRIVE_NOISE = 1
EGO_KERNELS = {0: "none", 1: "ego_sparse_kernel", 2: "ego_costmap_kernel<staged>", 3: "ego_costmap_binned_kernel",
               4: "ego_costmap_window_kernel", 5: "ego_costmap_kernel<global>", 6: "ego_pooled_sparse_kernel",
               7: "ego_pooled_sampled_kernel"}

_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


class BcpParams(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32), ("n_verts", C.c_int32), ("dynamic_model", C.c_int32),
        ("model_front_column_pid", C.c_int32), ("noise_on", C.c_int32), ("iteration_timeout", C.c_int32),
        ("options", C.c_int32),
        ("verts", (C.c_double * 2) * MAX_VERTS),
        ("dt", C.c_double), ("front_wheel_from_axis", C.c_double), ("max_front_wheel_angle", C.c_double),
        ("max_front_wheel_speed", C.c_double), ("max_linear_acceleration", C.c_double),
        ("max_angular_acceleration", C.c_double), ("front_column_p_gain", C.c_double),
        ("alpha", C.c_double * 6),
        ("spatial_precision", C.c_double), ("angular_precision", C.c_double),
        ("spatial_progress_multiplier", C.c_double),
        ("reward_provider", C.c_int32), ("control_delay", C.c_int32), ("pose_delay", C.c_int32),
        ("state_delay", C.c_int32),
    ]


class BcpState(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("angle", C.c_void_p), ("v", C.c_void_p), ("w", C.c_void_p),
        ("steering_motor_command", C.c_void_p), ("wheel_angle", C.c_void_p), ("min_spat_dist_so_far", C.c_void_p),
        ("target_idx", C.c_void_p), ("current_iter", C.c_void_p), ("robot_collided", C.c_void_p),
        ("pose_seen", C.c_void_p), ("robot_state_seen", C.c_void_p), ("control_queue", C.c_void_p),
        ("poses_queue", C.c_void_p), ("robot_state_queue", C.c_void_p),
    ]


class BcpMiniWorldParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in (
        "inner_h", "inner_w", "mid_margin", "out_margin", "min_obstacle_angle", "max_obstacle_angle", "lim_euc_dist",
        "lim_ang_dist", "angular_pose_noise_scale", "resolution", "goal_spat_dist", "goal_ang_dist")]


class BcpAisleWorldParams(C.Structure):
    _fields_ = [(k, C.c_double * 2) for k in (
        "main_corridor_length", "turn_corridor_length", "turn_corridor_angle", "main_corridor_width",
        "turn_corridor_width")] + [(k, C.c_double) for k in ("margin", "resolution", "path_delta")]


class BcpStepIO(C.Structure):
    _fields_ = [
        ("actions", C.c_void_p), ("noise_z", C.c_void_p), ("noise_z_out", C.c_void_p), ("reward", C.c_void_p),
        ("done", C.c_void_p), ("collided_now", C.c_void_p), ("err", C.c_void_p),
    ]


class BcpEpisodeRecord(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64), ("reason", C.c_void_p), ("ret", C.c_void_p), ("count", C.c_void_p),
        ("env_id", C.c_void_p), ("geom", C.c_void_p), ("final_ret", C.c_void_p), ("final", BcpState),
    ]


class BcpLookaheadIO(C.Structure):
    _fields_ = [
        ("actions", C.c_void_p), ("noise_z", C.c_void_p), ("mask", C.c_void_p),
        ("horizon", C.c_int32), ("n_candidates", C.c_int32),
        ("ret", C.c_void_p), ("steps", C.c_void_p), ("reason", C.c_void_p), ("final_pose", C.c_void_p),
        ("final_target_idx", C.c_void_p), ("err", C.c_void_p), ("best", C.c_void_p), ("best_action", C.c_void_p),
    ]


class BcpMppiParams(C.Structure):
    _fields_ = [
        ("horizon", C.c_int32), ("n_candidates", C.c_int32), ("iterations", C.c_int32),
        ("sigma", C.c_double * 2), ("low", C.c_double * 2), ("high", C.c_double * 2),
        ("lambda_", C.c_double), ("collision_penalty", C.c_double), ("seed", C.c_uint64), ("draw_index", C.c_uint64),
    ]


class BcpMppiIO(C.Structure):
    _fields_ = [
        ("mean", C.c_void_p), ("action", C.c_void_p), ("mask", C.c_void_p), ("eps_in", C.c_void_p), ("eps_out", C.c_void_p),
        ("draw_index", C.c_void_p), ("iter_mean", C.c_void_p), ("iter_ret", C.c_void_p), ("iter_reason", C.c_void_p),
        ("err", C.c_void_p),
    ]


class BcpMppiTerminal(C.Structure):
    _fields_ = [
        ("field", C.c_void_p), ("n_fields", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("weight", C.c_double),
        ("iter_value", C.c_void_p), ("iter_score", C.c_void_p),
    ]


class BcpMppiWidths(C.Structure):
    """bcp_mppi_widths: the widths of bcp_mppi_adapt"""
    _fields_ = [
        ("sigma", C.c_void_p), ("sigma_min", C.c_double * 2), ("sigma_max", C.c_double * 2), ("rate", C.c_double),
        ("iter_sigma", C.c_void_p),
    ]


class BcpTrackParams(C.Structure):
    _fields_ = [
        ("horizon", C.c_int32), ("n_candidates", C.c_int32), ("low", C.c_double * 2), ("high", C.c_double * 2),
        ("max_curvature", C.c_double),
    ]


class BcpTrackIO(C.Structure):
    _fields_ = [
        ("gains", C.c_void_p), ("mask", C.c_void_p), ("actions", C.c_void_p), ("ret", C.c_void_p), ("steps", C.c_void_p),
        ("reason", C.c_void_p), ("final_pose", C.c_void_p), ("final_target_idx", C.c_void_p), ("err", C.c_void_p),
        ("trace", C.c_void_p), ("best", C.c_void_p), ("best_plan", C.c_void_p), ("best_action", C.c_void_p),
    ]


class BcpScatterParams(C.Structure):
    """bcp_scatter_params: what bcp_scatter_boxes draws from"""
    _fields_ = [
        ("n_boxes", C.c_int32), ("max_attempts", C.c_int32), ("n_yaws", C.c_int32), ("reserved", C.c_int32),
        ("seed", C.c_uint64), ("along", C.c_double * 2), ("half_size", C.c_double * 2),
    ]


class BcpSmoothParams(C.Structure):
    """bcp_smooth_params: the pull's reach and the blend of bcp_smooth_route"""
    _fields_ = [("look", C.c_int32), ("halvings", C.c_int32), ("blend", C.c_double), ("delta", C.c_double)]


class BcpSpeedParams(C.Structure):
    """bcp_speed_params: the limits bcp_path_speed makes a speed profile from"""
    _fields_ = [("span", C.c_int32)] + [(k, C.c_double) for k in (
        "v_max", "v_min", "a_lat", "w_max", "a_dec", "a_acc", "v_start", "v_end")]


class BcpTrackProfileIO(C.Structure):
    """bcp_track_profile_io: the speeds bcp_track_profile reads, laid out as the bound paths"""
    _fields_ = [("speed", C.c_void_p), ("max_len", C.c_int32)]


BcpMppiAdapt = BcpMppiWidths   # (the argument of bcp_mppi_adapt, by the function's name)


# every symbol include/bcplan.h declares: (restype, argtypes)
_H = C.c_void_p
SYMBOLS = {
    "bcp_last_error": (C.c_char_p, []),
    "bcp_abi_version": (C.c_int, []),
    "bcp_create": (C.c_int, [C.POINTER(BcpParams), C.c_int64, C.c_int, C.c_int64, C.POINTER(_H)]),
    "bcp_destroy": (C.c_int, [_H]),
    "bcp_seed": (C.c_int, [_H, C.c_uint64]),
    "bcp_set_tuning": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "bcp_set_geometry_pool": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p]),
    "bcp_set_costmaps": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_double, C.c_void_p]),
    "bcp_set_paths": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "bcp_bind_state": (C.c_int, [_H, C.POINTER(BcpState)]),
    "bcp_bind_initial_state": (C.c_int, [_H, C.POINTER(BcpState)]),
    "bcp_declare_uniform_initial_state": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "bcp_reset_masked": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "bcp_broadcast_state": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p]),
    "bcp_step": (C.c_int, [_H, C.POINTER(BcpStepIO), C.c_uint32, C.c_void_p]),
    "bcp_rollout": (C.c_int, [_H, C.POINTER(BcpStepIO), C.c_int32, C.c_uint32, C.c_void_p]),
    "bcp_lookahead": (C.c_int, [_H, C.POINTER(BcpLookaheadIO), C.c_uint32, C.c_void_p]),
    "bcp_mppi": (C.c_int, [_H, C.POINTER(BcpMppiParams), C.POINTER(BcpMppiIO), C.c_uint32, C.c_void_p]),
    "bcp_mppi_field": (C.c_int, [_H, C.POINTER(BcpMppiParams), C.POINTER(BcpMppiIO), C.POINTER(BcpMppiTerminal), C.c_uint32,
                                 C.c_void_p]),
    "bcp_mppi_adapt": (C.c_int, [_H, C.POINTER(BcpMppiParams), C.POINTER(BcpMppiIO), C.POINTER(BcpMppiWidths),
                                 C.POINTER(BcpMppiTerminal), C.c_uint32, C.c_void_p]),
    "bcp_track": (C.c_int, [_H, C.POINTER(BcpTrackParams), C.POINTER(BcpTrackIO), C.c_uint32, C.c_void_p]),
    "bcp_track_profile": (C.c_int, [_H, C.POINTER(BcpTrackParams), C.POINTER(BcpTrackIO), C.POINTER(BcpTrackProfileIO),
                                    C.c_uint32, C.c_void_p]),
    "bcp_expired_waits": (C.c_int, [_H, C.POINTER(C.c_int64), C.c_void_p]),
    "bcp_parked_poses": (C.c_int, [_H, C.POINTER(C.c_int64), C.c_void_p]),
    "bcp_side_stream": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p)]),
    "bcp_robot_step": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_pose_collides": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bcp_is_robot_colliding": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bcp_is_footprint_colliding": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint8,
                                             C.c_void_p, C.c_void_p]),
    "bcp_reward": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "bcp_find_last_reached": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bcp_path_velocity": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_pixel_footprint": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p]),
    "bcp_pack_mask_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bcp_unpack_mask_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bcp_normalize_angle": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bcp_world_to_pixel": (C.c_int, [_H, C.c_void_p, C.c_int64, _f64p, C.c_double, C.c_void_p, C.c_void_p]),
    "bcp_egocentric_shape": (C.c_int, [_H, _f64p, _i32p]),
    "bcp_egocentric_costmaps": (C.c_int, [_H, C.c_void_p, C.c_int64, _f64p, _f64p, C.c_uint8, C.c_void_p,
                                          C.c_void_p]),
    "bcp_egocentric_route": (C.c_int, [_H, _i32p]),
    "bcp_egocentric_pooled_shape": (C.c_int, [_H, _f64p, C.c_int32, _i32p]),
    "bcp_egocentric_costmaps_pooled": (C.c_int, [_H, C.c_void_p, C.c_int64, _f64p, _f64p, C.c_uint8, C.c_int32, C.c_void_p,
                                                 C.c_void_p]),
    "bcp_goal_n_state": (C.c_int, [_H, _f64p, C.c_void_p, C.c_void_p]),
    "bcp_goal_direction_state": (C.c_int, [_H, _f64p, C.c_void_p, C.c_void_p]),
    "bcp_mini_world_seed": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bcp_sample_mini_worlds": (C.c_int, [_H, C.POINTER(BcpMiniWorldParams), C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_get_distance_field": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "bcp_get_near_field": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "bcp_plan_mini_worlds": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_refresh_mini_worlds": (C.c_int, [_H, C.POINTER(BcpMiniWorldParams)] + [C.c_void_p] * 6 + [C.c_double] +
                                [C.c_void_p] * 3),
    "bcp_release_mini_worlds": (C.c_int, [_H, C.c_void_p]),
    "bcp_mini_world_paths": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "bcp_sample_aisle_worlds": (C.c_int, [_H, C.POINTER(BcpAisleWorldParams), C.c_void_p, C.c_int64, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_render_aisle_worlds": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p]),
    "bcp_aisle_world_paths": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_device_normals": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]),
    "bcp_step_form": (C.c_int, [_H]),
    "bcp_step_shared_variant": (C.c_int, [_H]),
    "bcp_step_uniform_reset": (C.c_int, [_H]),
    "bcp_time_step_kernels": (C.c_int, [_H, C.POINTER(BcpStepIO), C.c_uint32, C.c_int32, C.c_void_p,
                                        C.POINTER(C.c_float)]),
    "bcp_time_steps": (C.c_int, [_H, C.POINTER(BcpStepIO), C.c_uint32, C.c_int32, C.c_void_p, C.POINTER(C.c_float)]),
    "bcp_bind_episode_record": (C.c_int, [_H, C.POINTER(BcpEpisodeRecord)]),
    "bcp_episode_record_overflows": (C.c_int, [_H, C.POINTER(C.c_int64), C.c_void_p]),
    "bcp_final_egocentric_costmaps": (C.c_int, [_H, _f64p, _f64p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bcp_final_egocentric_costmaps_pooled": (C.c_int, [_H, _f64p, _f64p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "bcp_final_goal_n_state": (C.c_int, [_H, _f64p, C.c_void_p, C.c_void_p]),
    "bcp_final_goal_direction_state": (C.c_int, [_H, _f64p, C.c_void_p, C.c_void_p]),
    "bcp_inflate_costmaps": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                       C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_range_scan": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "bcp_final_range_scan": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "bcp_goal_field": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_goal_field_bound": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "bcp_refresh_goal_fields": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (extra_of_cost: a HOST uint16 [256]; pass table.ctypes.data of a contiguous numpy array)
    "bcp_goal_field_cost": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "bcp_goal_field_cost_bound": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_goal_field_sample": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_final_goal_field_sample": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_goal_route": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_goal_route_bound": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_smooth_route": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                   C.c_void_p, C.c_int32, C.POINTER(BcpSmoothParams), C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_path_speed": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.POINTER(BcpSpeedParams), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcp_scatter_boxes": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_double, C.POINTER(BcpScatterParams), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


class BcpError(RuntimeError):
    """A libbcplan call returned a negative status."""


def load():
    """dlopen libbcplan.so and type every exported symbol.  Raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libbcplan.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (hipcc, gfx950); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError here means header and library disagree
            fn.restype = res
            fn.argtypes = args
        if L.bcp_abi_version() != ABI_VERSION:
            raise ImportError("libbcplan ABI %d != binding ABI %d" % (L.bcp_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise BcpError("libbcplan error %d: %s" % (rc, load().bcp_last_error().decode("utf-8", "replace")))

// bcplan.hip -- libbcplan.so: batched PlanEnv.step() for MI355X (gfx950).  C ABI in include/bcplan.h.
//
// One translation unit.  The device code is in bcp_device.h, bcp_raster.h, bcp_coop.h and bcp_step.h with the bcp_step_*.h it includes (the step: robot model ->
// collision classification / exact rasteriser -> rollback -> reward provider -> done -> optional reset -> state write-back),
// bcp_lookahead.h, bcp_mppi.h and bcp_track.h (the planners; the tracker's law: bcp_track_law.h, no HIP in it),
// bcp_ego.h (egocentric views), bcp_sample.h and bcp_aisle.h (world samplers),
// bcp_inflate.h (costmap inflation), bcp_scan.h (range scans; the walk: bcp_scan_march.h, no HIP in it), bcp_goal.h (goal
// fields; a cell's arithmetic: bcp_goal_cell.h, and the plan of a launch: bcp_goal_plan.h, no HIP in either), bcp_boxes.h (box obstacles; the rule: bcp_boxes_cell.h, no HIP
// in it; bcp_philox.h and bcp_outline.h hold the generator and the edge walk for host and device).  The host side is split by
// subsystem:
//   bcp_host.h         errors, the handle and the owners of its state (device buffers are DevBuf, events and streams Owned:
//                      bcp_devbuf.h), EgoCells, the launch helpers
//   bcp_field_plan.h   footprint geometry and the plan of a map binding: every shape and size, no HIP in it
//   bcp_field.h        distance field and tiles: kernels, DistanceField, the launchers of what is derived from maps and paths
//   bcp_step_host.h    step forms, the step's parameter block and launcher, Parking, WaitWatchdog, bcp_step / bcp_rollout
//   bcp_plan_host.h    the planners: bcp_lookahead / bcp_mppi / bcp_mppi_field / bcp_mppi_adapt
//   bcp_track_host.h   bcp_track / bcp_track_profile (kernels: bcp_track.h)
//   bcp_ego_host.h     egocentric costmaps (routed by bcp_ego_route.h, which has no HIP in it), goal-state vectors, the
//                      episode record and its final observations
//   bcp_worlds_host.h  mini-world and aisle-world entry points
//   bcp_inflate_host.h bcp_inflate_costmaps (kernel: bcp_inflate.h)
//   bcp_scan_host.h    bcp_range_scan / bcp_final_range_scan (kernel: bcp_scan.h)
//   bcp_goal_host.h    goal fields (kernels: bcp_goal.h): bcp_goal_field / bcp_goal_field_cost, their forms on the binding
//                      bcp_goal_field_bound / bcp_goal_field_cost_bound / bcp_refresh_goal_fields -- one launch path for the
//                      five, planned by bcp_goal_plan.h --, bcp_goal_field_sample / bcp_final_goal_field_sample, and
//                      bcp_goal_route / bcp_goal_route_bound
//   bcp_smooth_host.h  bcp_smooth_route (kernel: bcp_smooth.h; a row's arithmetic: bcp_smooth_cell.h, no HIP in it)
//   bcp_speed_host.h   bcp_path_speed (kernel: bcp_speed.h; a way point's arithmetic and the passes: bcp_speed_cell.h, no HIP in it)
//   bcp_boxes_host.h   bcp_scatter_boxes (kernel: bcp_boxes.h)
//   bcp_seams_host.h   bind / reset / broadcast of the state and the operator seams (their small kernels: bcp_seams.h)
// This file holds create / destroy / seed / pool / tuning / side stream, bcp_set_costmaps with the two reads of the distance
// field, and bcp_set_paths.
// Compiled with -ffp-contract=off (numpy rounds every product and sum separately).  No CPU path exists here.
#include <hip/hip_runtime.h>
#include <mutex>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <utility>
#include <vector>

#include "bcp_device.h"
#include "bcp_raster.h"
#include "bcp_coop.h"
#include "bcp_step.h"
#include "bcp_lookahead.h"
#include "bcp_mppi.h"
#include "bcp_track.h"
#include "bcp_ego.h"
#include "bcp_sample.h"
#include "bcp_aisle.h"
#include "bcp_inflate.h"
#include "bcp_scan.h"
#include "bcp_goal.h"
#include "bcp_smooth.h"
#include "bcp_speed.h"
#include "bcp_boxes.h"

using namespace bcp;

#include "bcp_host.h"

extern "C" const char* bcp_last_error(void) { return g_err; }
extern "C" int bcp_abi_version(void) { return BCP_ABI_VERSION; }

static void fill_dev_params(bcp_handle* h)
{
    const bcp_params& p = h->params;
    DevParams& d = h->dev;
    memset(&d, 0, sizeof(d));
    d.model = p.model;
    d.n_verts = p.n_verts;
    d.dynamic_model = p.dynamic_model;
    d.model_front_column_pid = p.model_front_column_pid;
    d.noise_on = p.noise_on;
    d.iteration_timeout = p.iteration_timeout;
    d.dt = p.dt;
    d.L = p.front_wheel_from_axis;
    d.max_wheel_angle = p.max_front_wheel_angle;
    d.max_wheel_speed = p.max_front_wheel_speed;
    d.max_lin_acc = p.max_linear_acceleration;
    d.max_ang_acc = p.max_angular_acceleration;
    d.p_gain = p.front_column_p_gain;
    d.inv_dt = 1.0 / p.dt;                       // (correctly rounded: what div_by_const needs)
    d.inv_L = 1.0 / p.front_wheel_from_axis;
    for (int k = 0; k < 6; ++k) d.alpha[k] = p.alpha[k];
    d.sp = p.spatial_precision;
    d.ap = p.angular_precision;
    d.progress_mult = p.spatial_progress_multiplier;
    d.par_thr = -p.spatial_precision / 9;
    d.ap_cos_min = p.angular_precision >= 3.14159265358979 ? -2.0f : (float)(std::cos(p.angular_precision) - 1e-4);
    d.sp_prune = std::nextafter(std::nextafter(p.spatial_precision, INFINITY), INFINITY);
    d.sp2_lo = p.spatial_precision * p.spatial_precision * (1.0 - 1e-13);
    d.sp2_hi = p.spatial_precision * p.spatial_precision * (1.0 + 1e-13);
    d.reward_provider = p.reward_provider;
    d.control_delay = p.control_delay;
    d.pose_delay = p.pose_delay;
    d.state_delay = p.state_delay;
    const double res = h->resolution > 0 ? h->resolution : 1.0;
    scale_footprint(d, p, res);
}

// ------------------------------------------------------------------------------------------------ the subsystems
// (each needs the ones before it, and the helpers above)
#include "bcp_field.h"
#include "bcp_step_host.h"
#include "bcp_plan_host.h"
#include "bcp_track_host.h"
#include "bcp_seams.h"
#include "bcp_seams_host.h"
#include "bcp_ego_host.h"
#include "bcp_worlds_host.h"
#include "bcp_inflate_host.h"
#include "bcp_scan_host.h"
#include "bcp_goal_host.h"
#include "bcp_smooth_host.h"
#include "bcp_speed_host.h"
#include "bcp_boxes_host.h"

// ------------------------------------------------------------------------------------------------ host API
extern "C" int bcp_create(const bcp_params* params, int64_t n_envs, int device, int64_t env_id_base, bcp_handle** out)
{
    if (!params || !out) return fail(BCP_E_INVALID, "bcp_create: null argument");
    if (params->abi_version != BCP_ABI_VERSION)
        return fail(BCP_E_INVALID, "bcp_create: abi_version %d != %d", params->abi_version, BCP_ABI_VERSION);
    if (n_envs <= 0) return fail(BCP_E_INVALID, "bcp_create: n_envs must be positive");
    if (params->n_verts < 3 || params->n_verts > BCP_MAX_VERTS)
        return fail(BCP_E_INVALID, "bcp_create: n_verts %d outside [3, %d]", params->n_verts, BCP_MAX_VERTS);
    for (int k = 0; k < params->n_verts; ++k)
        if (!std::isfinite(params->verts[k][0]) || !std::isfinite(params->verts[k][1]))
            return fail(BCP_E_INVALID, "bcp_create: footprint vertex %d is not finite", k);
    if (params->model != BCP_MODEL_TRICYCLE && params->model != BCP_MODEL_DIFFDRIVE)
        return fail(BCP_E_INVALID, "bcp_create: unknown robot model %d", params->model);
    if (!(params->dt > 0)) return fail(BCP_E_INVALID, "bcp_create: dt must be > 0 (path_tools.py:307)");
    {   // div_by_const (bcp_device.h) divides by dt and by the wheel base through their reciprocals; the sequence is the IEEE
        // quotient for every divisor but those whose significand is all ones (0.99999999999999989 and its like)
        const auto all_ones = [](double d) {
            uint64_t bits;
            memcpy(&bits, &d, sizeof(bits));
            return (bits & 0x000FFFFFFFFFFFFFull) == 0x000FFFFFFFFFFFFFull;
        };
        if (all_ones(params->dt) || (params->model == BCP_MODEL_TRICYCLE && all_ones(params->front_wheel_from_axis)))
            return fail(BCP_E_INVALID, "bcp_create: dt / front_wheel_from_axis with an all-ones significand is not supported");
    }
    if (params->model == BCP_MODEL_DIFFDRIVE && params->noise_on && !(params->options & BCP_OPT_DIFFDRIVE_NOISE))
        return fail(BCP_E_INVALID, "bcp_create: the reference's DiffDriveRobot raises IndexError with noise_parameters "
                                   "(differential_drive.py:73); set BCP_OPT_DIFFDRIVE_NOISE in bcp_params.options to opt in to "
                                   "the unpinned 1-pose analogue");
    if (params->reward_provider != BCP_REWARD_CONTINUOUS && params->reward_provider != BCP_REWARD_PURE_PURSUIT)
        return fail(BCP_E_INVALID, "bcp_create: unknown reward provider %d", params->reward_provider);
    if (params->control_delay < 0 || params->pose_delay < 0 || params->state_delay < 0)
        return fail(BCP_E_INVALID, "bcp_create: delays must be >= 0");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(BCP_E_NO_DEVICE, "bcp_create: no HIP device available (%s); libbcplan has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(BCP_E_INVALID, "bcp_create: device %d of %d", device, count);
    HIP_TRY(hipSetDevice(device));
    bcp_handle* h = new (std::nothrow) bcp_handle();   // (the defaults are the member initialisers: bcp_host.h)
    if (!h) return fail(BCP_E_INVALID, "bcp_create: out of host memory");
    h->params = *params;
    h->n = n_envs;
    h->device = device;
    h->env_id_base = env_id_base;
    h->tune = Tuning::from_environment();
    fill_dev_params(h);
    if (h->tick.reserve(kTickWords) != hipSuccess || hipMemset(h->tick.get(), 0, kTickWords * sizeof(uint64_t)) != hipSuccess) {
        delete h;
        return fail(BCP_E_HIP, "bcp_create: cannot allocate device memory");
    }
    *out = h;
    return BCP_OK;
}

extern "C" int bcp_destroy(bcp_handle* h)
{
    if (!h) return BCP_OK;
    (void)hipSetDevice(h->device);   // (the owners' destructors free on this device)
    delete h;
    return BCP_OK;
}

extern "C" int bcp_seed(bcp_handle* h, uint64_t seed)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_seed: null handle");
    h->seed = seed;
    // The noise stream restarts: step counter 0 again.  The alternating counter sets of the parking scheme are keyed
    // by the counter's parity, so they are re-armed with it (rare call: synchronous).
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const uint64_t tick[4] = {0, 0, seed, 0};
    HIP_TRY(hipMemcpy(h->tick.get(), tick, sizeof(tick), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(h->tick.get() + kTickLocalTicket, 0, sizeof(uint64_t)));
    BCP_TRY(h->parking.arm(h->tune.dense_threshold, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return BCP_OK;
}

extern "C" int bcp_set_geometry_pool(bcp_handle* h, int32_t n_geoms, int32_t* geom_of_env, const int32_t* next_geom)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_set_geometry_pool: null handle");
    if (n_geoms < 0 || (n_geoms > 0 && !geom_of_env))
        return fail(BCP_E_INVALID, "bcp_set_geometry_pool: n_geoms > 0 needs geom_of_env");
    if ((n_geoms > 0) != (h->n_geoms > 0) || (n_geoms > 0 && n_geoms != h->n_geoms)) {
        // the non-shared arrays change their entry count: they have to be given again
        h->have_map = h->have_path = h->have_init = false;
    }
    h->n_geoms = n_geoms;
    h->geom_of_env = n_geoms > 0 ? geom_of_env : nullptr;
    h->next_geom = n_geoms > 0 ? next_geom : nullptr;
    h->static_dirty = true;
    return BCP_OK;
}

extern "C" int bcp_set_tuning(bcp_handle* h, int32_t key, int32_t value)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_set_tuning: null handle");
    h->static_dirty = true;
    switch (key) {
        case BCP_TUNE_EXACT_MODE:
            if (value < 0 || value > 3) return fail(BCP_E_INVALID, "bcp_set_tuning: exact mode must be 0, 1, 2 or 3");
            h->tune.exact_mode = value;
            return BCP_OK;
        case BCP_TUNE_DENSE_THRESHOLD:
            h->tune.dense_threshold = value;
            h->tune.adaptive = 0;   // an explicit threshold is taken as is
            return BCP_OK;
        case BCP_TUNE_DEFER:
            h->tune.defer = value ? 1 : 0;
            return BCP_OK;
        case BCP_TUNE_EDT_LDS:
            h->tune.edt_in_lds = value ? 1 : 0;
            return BCP_OK;
        case BCP_TUNE_NEAR_DILATE:
            if (value < 0 || value > 2) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_NEAR_DILATE takes 0, 1 or 2");
            h->tune.near_dilate = value;
            return BCP_OK;
        case BCP_TUNE_EGO_SPARSE:
            if (value < 0) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_EGO_SPARSE takes 0, 1 or a limit of cells per map");
            if (value != h->tune.ego_sparse) h->ego_cells.invalidate();   // (the lists are sized for the limit in force)
            h->tune.ego_sparse = value;
            return BCP_OK;
        case BCP_TUNE_EGO_LIST_STRIDE:
            if (value < 0 || (value & 63)) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_EGO_LIST_STRIDE takes 0 or a multiple of 64");
            if (value != h->tune.ego_stride) h->ego_cells.invalidate();
            h->tune.ego_stride = value;
            return BCP_OK;
        case BCP_TUNE_FUSED:
            h->tune.fused = value ? 1 : 0;
            return BCP_OK;
        case BCP_TUNE_NEAR_SHIFT:
            if (value < -1 || value > 3) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_NEAR_SHIFT takes -1 (default), 0, 1, 2 or 3");
            h->tune.near_shift = value;   // (in force from the next bcp_set_costmaps on)
            return BCP_OK;
        case BCP_TUNE_LOCAL_PAIRS:
            if (value != 0 && value != 1 && value != 2 && value != 4)
                return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_LOCAL_PAIRS takes 0 (default), 1, 2 or 4");
            h->tune.local_pairs = value;
            return BCP_OK;
        case BCP_TUNE_LOCAL_SHARED:
            if (value != 0 && value != 1) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_LOCAL_SHARED takes 0 or 1");
            h->tune.local_shared = value;
            return BCP_OK;
        case BCP_TUNE_INFLATE_ROUTE:
            if (value != 0 && value != 2) return fail(BCP_E_INVALID, "bcp_set_tuning: BCP_TUNE_INFLATE_ROUTE takes 0 or 2");
            h->tune.inflate_route = value;
            return BCP_OK;
        case BCP_TUNE_GOAL_ROUTE:
            return goal_set_route(h, value);
        case BCP_TUNE_CULL:
            h->tune.cull = value ? 1 : 0;
            h->cull.on = (value && h->cull.edt) ? 1 : 0;
            return BCP_OK;
        default:
            return fail(BCP_E_INVALID, "bcp_set_tuning: unknown key %d", key);
    }
}

extern "C" int bcp_side_stream(bcp_handle* h, int32_t cu_percent, void** stream)
{
    if (!h || !stream) return fail(BCP_E_INVALID, "bcp_side_stream: null argument");
    if (cu_percent < 1 || cu_percent > 100) return fail(BCP_E_INVALID, "bcp_side_stream: cu_percent must be 1 .. 100");
    HIP_TRY(hipSetDevice(h->device));
    if (h->side_stream && h->side_share != cu_percent) {
        HIP_TRY(hipStreamSynchronize(h->side_stream.get()));
        HIP_TRY(h->side_stream.reset());
    }
    if (!h->side_stream) {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        // one bit per CU; the enabled ones are spread evenly (every k-th bit, whatever order the driver numbers the CUs of
        // the shader engines and XCDs in, every one of them keeps the same share)
        const int words = (cus + 31) / 32;
        std::vector<uint32_t> mask((size_t)std::max(words, 1), 0u);
        int enabled = 0;
        for (int c = 0; c < cus; ++c)
            if ((int64_t)(c + 1) * cu_percent / 100 > (int64_t)c * cu_percent / 100) {
                mask[(size_t)c / 32] |= 1u << (c % 32);
                ++enabled;
            }
        if (enabled == 0) mask[0] |= 1u;
        if (hipExtStreamCreateWithCUMask(h->side_stream.put(), (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BCP_E_HIP, "bcp_side_stream: the runtime refused a CU-masked stream");
        }
        h->side_share = cu_percent;
    }
    *stream = (void*)h->side_stream.get();
    return BCP_OK;
}

// the maps as bits: room for them, the descriptor, the footprint at this resolution, and the packing launch
static int bind_maps(bcp_handle* h, const MapBinding& b, const FieldPlan& plan, const uint8_t* data, const int32_t* valid_rows,
                     const int32_t* valid_cols, const double* origins, int32_t origins_per_env, hipStream_t s)
{
    HIP_TRY(h->bitmap.reserve(plan.n_bitmap));
    HIP_TRY(h->map_tiles.reserve(plan.n_map_tiles));
    h->resolution = b.resolution;
    h->map_data = data;
    h->map_valid_rows = valid_rows;
    h->map_valid_cols = valid_cols;
    fill_dev_params(h);
    h->wide = plan.wide;
    MapDesc& m = h->map;
    m.bits = h->bitmap.get();
    m.tiles = h->map_tiles.get();
    m.rows = b.rows;
    m.cols = b.cols;
    m.wpr = plan.wpr;
    m.shared = b.shared ? 1 : 0;
    m.env_stride = b.shared ? 0 : (int64_t)b.rows * plan.wpr;
    m.inv_res = 1.0 / b.resolution;  // anti_resolution = 1./resolution (coordinate_transformations.py:204)
    m.origins = origins_per_env ? origins : nullptr;
    m.ox = origins_per_env ? 0 : origins[0];
    m.oy = origins_per_env ? 0 : origins[1];
    m.in_lds = plan.in_lds;
    const EntrySelect all_maps = {nullptr, nullptr, plan.n_maps};
    launch_pack_bitmap(h, all_maps, plan.n_maps, s);
    HIP_TRY(hipGetLastError());
    return BCP_OK;
}

// validate, plan (bcp_field_plan.h: every shape and size that follows from the binding), bind the maps, the distance field
// and the parking slots, launch
extern "C" int bcp_set_costmaps(bcp_handle* h, const uint8_t* data, int32_t rows, int32_t cols, int32_t shared,
                                const int32_t* valid_rows, const int32_t* valid_cols, const double* origins,
                                int32_t origins_per_env, double resolution, void* stream)
{
    if (!h || !data || !origins) return fail(BCP_E_INVALID, "bcp_set_costmaps: null argument");
    if (rows <= 0 || cols <= 0 || !(resolution > 0)) return fail(BCP_E_INVALID, "bcp_set_costmaps: bad shape/resolution");
    if (!check_kernel_size(h->params, resolution))
        return fail(BCP_E_INVALID, "bcp_set_costmaps: footprint radius / resolution exceeds %d px", BCP_MAX_KERNEL_HALF);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int wpr = map_wpr(cols);
    const MapBinding binding = {rows, cols, shared != 0, n_slots(h), resolution, h->tune.near_shift, h->tune.cull != 0,
                                collision_lds_bytes(h->params.n_verts, 1, rows, wpr), map_tile_words(rows, wpr)};
    const FieldPlan plan = plan_field(h->params, binding);
    BCP_TRY(bind_maps(h, binding, plan, data, valid_rows, valid_cols, origins, origins_per_env, s));
    // The distance field for the O(1) pre-classification, and the parking slots of the steps that use it.  Many private maps
    // under the single-launch step: only the 1-bit tiles are read, so they are made directly from the lethal masks
    // (near_dilate_kernel) and the uint8 fields are left to whoever asks for them (ensure_fields) -- what a pool refresh
    // has done since round 3.  65 536 maps of 256 x 256: 75 ms of edt_lds_kernel -> a few ms (round 4).
    BCP_TRY(h->field.bind(h, plan, s));
    if (plan.field) {
        const EntrySelect all_maps = {nullptr, nullptr, plan.n_maps};
        BCP_TRY(h->field.rebuild(h, all_maps, plan.n_maps, s, DistanceField::bind_reads_tiles_only(h, plan)));
        HIP_TRY(hipGetLastError());
        BCP_TRY(h->parking.bind(h->n, h->tune.dense_threshold, s));
    }
    h->have_map = true;
    h->static_dirty = true;
    if (h->have_path && !h->path.shared) {   // the path records carry the origins
        const int64_t n_paths = n_slots(h);
        const EntrySelect all_paths = {nullptr, nullptr, n_paths};
        launch_world_records(h, all_paths, n_paths, s);
        HIP_TRY(hipGetLastError());
    }
    return BCP_OK;
}

extern "C" int bcp_get_distance_field(bcp_handle* h, int64_t first_entry, int64_t n_entries, uint8_t* out, int32_t* shape,
                                      void* stream)
{
    if (!h || !shape) return fail(BCP_E_INVALID, "bcp_get_distance_field: null argument");
    if (!h->have_map || !h->cull.edt) return fail(BCP_E_STATE, "bcp_get_distance_field: no distance field (no costmap, or culling off)");
    const CullDesc& C = h->cull;
    shape[0] = C.height;
    shape[1] = C.width;
    shape[2] = C.pad;
    shape[3] = C.clamp;
    if (!out) return BCP_OK;
    const int64_t n_maps = h->map.shared ? 1 : n_slots(h);
    if (first_entry < 0 || n_entries <= 0 || first_entry + n_entries > n_maps)
        return fail(BCP_E_INVALID, "bcp_get_distance_field: entries out of range");
    HIP_TRY(hipSetDevice(h->device));
    return h->field.copy_field(h, first_entry, n_entries, out, (hipStream_t)stream);
}

extern "C" int bcp_get_near_field(bcp_handle* h, int64_t first_entry, int64_t n_entries, uint32_t* out, int32_t* shape,
                                  void* stream)
{
    if (!h || !shape) return fail(BCP_E_INVALID, "bcp_get_near_field: null argument");
    if (!h->have_map || !h->cull.near) return fail(BCP_E_STATE, "bcp_get_near_field: no distance field (no costmap, or culling off)");
    const CullDesc& C = h->cull;
    shape[0] = h->field.planned().tiles_y;
    shape[1] = C.near_tx;
    shape[2] = C.t_out;
    if (!out) return BCP_OK;
    const int64_t n_maps = h->map.shared ? 1 : n_slots(h);
    if (first_entry < 0 || n_entries <= 0 || first_entry + n_entries > n_maps)
        return fail(BCP_E_INVALID, "bcp_get_near_field: entries out of range");
    HIP_TRY(hipSetDevice(h->device));
    return h->field.copy_near(first_entry, n_entries, out, (hipStream_t)stream);
}

extern "C" int bcp_set_paths(bcp_handle* h, const double* xytheta, const int32_t* lens, int32_t max_len, int32_t shared,
                             void* stream)
{
    if (!h || !xytheta) return fail(BCP_E_INVALID, "bcp_set_paths: null argument");
    if (max_len <= 0) return fail(BCP_E_INVALID, "bcp_set_paths: max_len must be positive");
    if (!shared && !lens) return fail(BCP_E_INVALID, "bcp_set_paths: per-env paths need lens");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (shared ? 1 : n_slots(h)) * (int64_t)max_len;
    HIP_TRY(h->path5.reserve((size_t)total * 5));
    HIP_TRY(h->path_pre.reserve(shared ? 0 : (size_t)total * 2));
    const int64_t n_paths = shared ? 1 : n_slots(h);
    HIP_TRY(h->path_bbox.reserve((size_t)n_paths * kBoxDoubles));
    HIP_TRY(h->path_index.reserve((size_t)4 * kPathBuckets));   // (a shared path's tables; private ones live in the records)
    if (max_len > 32766) return fail(BCP_E_INVALID, "bcp_set_paths: paths longer than 32766 way points are not supported");
    h->path.pts = h->path5.get();
    h->path.pre = shared ? nullptr : h->path_pre.get();
    h->path.bbox = h->path_bbox.get();
    h->path.index = h->path_index.get();
    h->path.lens = shared ? nullptr : lens;
    h->path.max_len = max_len;
    h->path.shared = shared ? 1 : 0;
    h->path_src = xytheta;
    const EntrySelect all_paths = {nullptr, nullptr, n_paths};
    launch_path_data(h, all_paths, n_paths, s);
    HIP_TRY(hipGetLastError());
    h->have_path = true;
    h->static_dirty = true;
    return BCP_OK;
}


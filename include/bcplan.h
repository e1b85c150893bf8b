/*
 * bcplan.h -- C ABI of libbcplan.so: batched, MI355X-native PlanEnv.step() (gfx950 HIP kernels).
 *
 * This is the drop-in boundary for the ONE hot path of braincorp/bc-gym-planning-env:
 *     PlanEnv.step()                         envs/base/env.py:334-361
 *       -> _env_step / pose_collides         envs/base/env.py:442-489
 *       -> TricycleRobot.step                robot_models/tricycle_model.py:478-538
 *          DiffDriveRobot.step               robot_models/differential_drive.py:236-265
 *       -> get_pixel_footprint (+fillPoly)   utilities/path_tools.py:122-162
 *       -> ContinuousRewardProvider.reward   envs/base/reward.py:214-259
 * The reference has no FFI layer of its own; what it does have is a set of optional native hooks
 * (`try: from brain.shining_utils... import *_impl`, see below).  Every entry point here cites the
 * reference interface it replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C symbols, no exceptions, no torch types.  Return 0 on success, a negative BCP_E_* code
 *     otherwise; bcp_last_error() returns a thread-local message for the last failure.
 *   - Unless a parameter says "host", every pointer is a DEVICE pointer on the handle's GPU
 *     (e.g. torch_tensor.data_ptr()); buffers are caller-owned and must outlive their use.
 *   - All launches are asynchronous on the `stream` argument (a hipStream_t, NULL = default stream).
 *     bcp_step()/bcp_reset_masked() never synchronise or copy to the host and allocate nothing once the first step
 *     has run (the first call after a re-bind uploads a 2 KB parameter block; bcp_egocentric_costmaps() allocates its
 *     scratch on first use).  The step counter (noise stream key, parity of the alternating counter sets) and the
 *     noise seed live on the device and are advanced by the kernels themselves: a step's launch arguments depend only
 *     on the pointers in bcp_step_io and the flags, so steps captured into a hipGraph (after one ordinary step has
 *     uploaded the parameter block) can be replayed.
 *   - One handle per GPU / process rank.  A handle is not thread-safe; different handles are independent.
 *   - There is NO CPU fallback in this library: without a GPU bcp_create() fails with BCP_E_NO_DEVICE.
 */
#ifndef BCPLAN_H
#define BCPLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCP_ABI_VERSION 2
#define BCP_MAX_VERTS 32
#define BCP_LETHAL 254 /* CostMap2D.LETHAL_OBSTACLE, utilities/costmap_2d.py:20-22 */
#define BCP_MAX_KERNEL_HALF 127 /* footprint mask is at most 255x255 px (circumscribed radius / resolution) */

enum { BCP_MODEL_TRICYCLE = 0, BCP_MODEL_DIFFDRIVE = 1 };
/* EnvParams.reward_provider_name (envs/base/reward_provider_examples.py:13-16) */
enum { BCP_REWARD_CONTINUOUS = 0, BCP_REWARD_PURE_PURSUIT = 1 };

enum {
    BCP_OK = 0,
    BCP_E_INVALID = -1,   /* bad argument / unsupported configuration */
    BCP_E_NO_DEVICE = -2, /* no usable GPU: the product has no CPU path */
    BCP_E_HIP = -3,       /* a HIP runtime call failed (message has the hipError string) */
    BCP_E_STATE = -4,     /* call order violated (e.g. step before costmaps/paths/state were bound) */
    BCP_E_INTERNAL = -5   /* bcp_step's watchdog: a bounded hand-off wait inside an EARLIER step launch gave up (see
                             bcp_expired_waits); the steps since then ran, but results of the affected workgroups are
                             unreliable -- a defect of the library, never of the data */
};

/* per-env error bits written to bcp_step_io.err (mirror of the reference's Python exceptions) */
enum {
    BCP_ERR_ANGLE_JUMP = 1, /* path_velocity raises when |dtheta| >= pi, utilities/path_tools.py:319-322 */
    BCP_ERR_TIME_ORDER = 2, /* path_velocity's `assert (dt > 0).all()`, utilities/path_tools.py:307 (bcp_path_velocity only) */
    BCP_ERR_INTERNAL = 4    /* no counterpart in the reference: a wait inside the step kernel ran into its iteration limit (a hand-off
                               between wavefronts never arrived); the step finished, its results for this workgroup are unreliable */
};

/* bcp_step flags */
enum {
    BCP_STEP_AUTO_RESET = 1, /* after outputs are written, envs with done=1 are restored to the bound initial
                                state (what a VecEnv does: scripts/rl_runners/ppo_runner.py:35-36) */
    BCP_STEP_ACTIONS_F32 = 2 /* actions are float32[N,2] (action_space dtype, envs/base/env.py:237-240);
                                otherwise float64[N,2].  float32 is widened to float64 before any arithmetic */
};

/* bcp_params.options */
enum {
    BCP_OPT_DIFFDRIVE_NOISE = 1 /* DiffDriveRobot with noise_parameters raises IndexError in the reference itself
                                   (robot_models/differential_drive.py:73: new_pose[:, 2] on a 1-D pose), so there is no
                                   reference behaviour to match: bcp_create refuses model = BCP_MODEL_DIFFDRIVE with noise_on
                                   (BCP_E_INVALID) unless this bit opts in to the UNPINNED 1-pose analogue of
                                   kinematic_body_pose_motion_step_with_noise */
};

/* POD flattening of EnvParams (envs/base/params.py:14-42), RewardParams (envs/base/reward.py:162-171),
 * the TricycleRobot switches (robot_models/tricycle_model.py:296-300) and the robot constants
 * (robot_models/robot_dimensions_examples.py:108-188).  host struct. */
typedef struct bcp_params {
    int32_t abi_version;            /* = BCP_ABI_VERSION */
    int32_t model;                  /* BCP_MODEL_* */
    int32_t n_verts;                /* footprint vertices, <= BCP_MAX_VERTS */
    int32_t dynamic_model;          /* TricycleRobot._dynamic_model */
    int32_t model_front_column_pid; /* TricycleRobot._model_front_column_pid */
    int32_t noise_on;               /* noise_parameters is not None (env.py:226-232) */
    int32_t iteration_timeout;      /* EnvParams.iteration_timeout */
    int32_t options;                /* BCP_OPT_* bits, 0 = none */
    double verts[BCP_MAX_VERTS][2]; /* metres, robot frame, already multiplied by footprint_scale */
    double dt;
    double front_wheel_from_axis;
    double max_front_wheel_angle;
    double max_front_wheel_speed;
    double max_linear_acceleration;
    double max_angular_acceleration;
    double front_column_p_gain;
    double alpha[6];                /* alpha1..alpha6 of the odometry noise model (differential_drive.py:55-74) */
    double spatial_precision;       /* RewardParams */
    double angular_precision;
    double spatial_progress_multiplier;
    int32_t reward_provider;        /* BCP_REWARD_*: ContinuousRewardProvider (reward.py:174-288) or
                                       ContinuousRewardPurePursuitProvider (reward.py:291-371) */
    int32_t control_delay;          /* EnvParams.control_delay / pose_delay / state_delay (params.py:28-30): FIFO delays */
    int32_t pose_delay;             /* of the action, of State.pose and of State.robot_state (env.py:27-49, 363-398) */
    int32_t state_delay;
} bcp_params;

/* Struct-of-arrays env state, caller-owned device memory, n_envs elements per array.
 * Field names follow State / TricycleRobotState / ContinuousRewardProviderState
 * (envs/base/env.py:52-68, robot_models/tricycle_model.py:234-244, envs/base/reward.py:12-23).
 * `current_time` is not stored: it is the running float64 sum of dt over current_iter steps (env.py:382) and the
 * host layer rebuilds it bit-exactly from current_iter. */
typedef struct bcp_state {
    double *x, *y, *angle;            /* robot pose == State.pose (delays 0) */
    double *v, *w;                    /* measured velocities */
    double *steering_motor_command;   /* tricycle only (may alias a dummy array for diff-drive) */
    double *wheel_angle;              /* tricycle only */
    double *min_spat_dist_so_far;     /* reward provider */
    int32_t *target_idx;              /* reward provider */
    int32_t *current_iter;
    uint8_t *robot_collided;          /* sticky */
    /* Only with delays > 0 (NULL otherwise).  x/y/angle/... above are always the robot's TRUE state.  The k-th element
     * pushed into a queue since the last reset (k = current_iter + 1) lives in slot (k - 1) % delay. */
    double *pose_seen;                /* [3][N] State.pose when pose_delay > 0: what the reward provider and the
                                         observation see (env.py:377-394) */
    double *robot_state_seen;         /* [7][N] State.robot_state when state_delay > 0 (field order as above) */
    double *control_queue;            /* [control_delay][2][N]  State.control_queue */
    double *poses_queue;              /* [pose_delay][3][N]     State.poses_queue */
    double *robot_state_queue;        /* [state_delay][7][N]    State.robot_state_queue */
} bcp_state;

/* per-step inputs/outputs, device pointers, N = n_envs */
typedef struct bcp_step_io {
    const void *actions;     /* [N,2] (wheel_v, wheel_angle) tricycle / (v, w) diff-drive; dtype by flag */
    const double *noise_z;   /* [N,3] standard normals in slot order, or NULL: then, if params.noise_on, normals
                                come from the on-device Philox4x32-10 stream keyed (seed, env, step counter) */
    double *noise_z_out;     /* optional [N,3]: the normals this step used (NaN where no draw happened) */
    double *reward;          /* [N] */
    uint8_t *done;           /* [N] goal reached | timed out | robot_collided (env.py:407-419) */
    uint8_t *collided_now;   /* optional [N]: this step's pose_collides verdict (return of _env_step) */
    int32_t *err;            /* optional [N]: BCP_ERR_* bits */
} bcp_step_io;

typedef struct bcp_handle bcp_handle;

/* ---- lifetime ----------------------------------------------------------------------------------------- */
const char *bcp_last_error(void);
int bcp_abi_version(void);
/* replaces PlanEnv.__init__ (env.py:219-249) for a batch of n_envs envs on GPU `device`.
 * env_id_base: global index of this handle's env 0 (rank * n_envs when sharded); keys the RNG stream. */
int bcp_create(const bcp_params *params /*host*/, int64_t n_envs, int device, int64_t env_id_base, bcp_handle **out);
int bcp_destroy(bcp_handle *h);
/* PlanEnv.seed / np.random.seed for the noise stream (differential_drive.py:50 uses the global numpy RNG) */
int bcp_seed(bcp_handle *h, uint64_t seed);

/* Execution knobs; none of them changes any result (tests run every combination against the oracle).
 *   BCP_TUNE_EXACT_MODE       0 = auto, 1 = always the wave-cooperative exact rasteriser, 2 = always the per-thread one,
 *                             3 = wave-cooperative, cell by cell (the lethal cells under the image tested one by one)
 *   BCP_TUNE_DENSE_THRESHOLD  auto mode: more undecided poses than this in one wavefront -> settle them inside the
 *                             step kernel (cooperatively with a distance field, per thread without one)
 *   BCP_TUNE_CULL             0 = skip the distance-field pre-classification (every in-map pose is rasterised)
 *   BCP_TUNE_DEFER            0 = settle undecided poses inside the step kernel instead of the second, load-balanced
 *                             kernel (only relevant with a distance field and exact mode auto)
 *   BCP_TUNE_EDT_LDS          0 = build distance fields with the two-pass global-memory kernels even where a map fits
 *                             into LDS (takes effect at the next bcp_set_costmaps)
 *   BCP_TUNE_FUSED            0 = settle the parked poses in a second launch (step_fast_pair_kernel + step_pending_kernel)
 *                             instead of inside the step launch itself (step_local_kernel, the default)
 *   BCP_TUNE_EGO_SPARSE       0 = egocentric views always sample the costmap pixel by pixel; 1 (default) = sparse maps with
 *                             border value 0 are drawn as a zero fill plus one patch per non-zero source cell, "sparse"
 *                             decided by a cost model from the largest number of non-zero cells any map entry holds;
 *                             >= 2 = the same with this explicit limit of cells per map (tests, sweeps)
 *   BCP_TUNE_NEAR_DILATE      how the 1-bit tiles of the distance field (bcp_get_near_field) are made: 0 = always by
 *                             thresholding the uint8 field; 1 (default) = a pool refresh (bcp_refresh_mini_worlds) under the
 *                             single-launch step dilates the lethal mask by the sample disc instead and leaves the uint8
 *                             fields of those entries to be computed when something asks for them (the other step forms,
 *                             bcp_pose_collides, bcp_get_distance_field); 2 = bcp_set_costmaps also overwrites its
 *                             thresholded tiles with dilated ones (tests: the two must agree bit for bit)
 *   BCP_TUNE_LOCAL_PAIRS      workgroup size of the single-launch step: 4 = 16 wavefronts / 256 envs (one workgroup per CU),
 *                             2 = 8 wavefronts / 128 envs (two per CU), 1 = 4 wavefronts / 64 envs (four per CU); 0 (default)
 *                             = the library's choice for the configuration.  Same results bit for bit in every size.
 *                             (The environment variable BCP_LOCAL_PAIRS = 1 | 2 | 4, read by bcp_create, sets this knob's
 *                             initial value for every handle of the process: the whole test suite runs under each size.)
 *   BCP_TUNE_EGO_LIST_STRIDE  0 (default) = the cell lists of the sparse egocentric route are sized from the counted cells;
 *                             a multiple of 64 = this many cells per map entry: an entry with more is drawn pixel by pixel
 *                             inside the same launch (what happens to a pool entry that is re-sampled with more cells than
 *                             the lists were sized for; the knob lets tests reach that path)
 *   BCP_TUNE_NEAR_SHIFT       resolution of the 1-bit tiles the single-launch step classifies poses on when the costmaps are
 *                             private: 0 = the tiles of bcp_get_near_field, 1 / 2 / 3 = a copy at 1/2, 1/4, 1/8 of the resolution (a
 *                             bit is the OR of the 2 x 2 / 4 x 4 / 8 x 8 cells it stands for: fewer lines of memory per pose, a few more
 *                             poses left to the exact test); -1 (default) = the library's choice.  In force from the next
 *                             bcp_set_costmaps on; results are the same bit for bit.  (Environment variable BCP_NEAR_SHIFT,
 *                             read by bcp_create: the knob's initial value.)
 *   BCP_TUNE_INFLATE_ROUTE    where bcp_inflate_costmaps keeps its 16-bit intermediate plane: 0 (default) = in LDS when the
 *                             map fits, else in the handle's global scratch; 2 = always in global scratch (lets tests
 *                             compare the two routes on one map; the bytes are the same)
 *   BCP_TUNE_GOAL_ROUTE       where bcp_goal_field keeps its bit masks and its 16-bit working plane: 0 (default) = in LDS
 *                             when they fit, else the masks in the handle's global scratch and the plane in `out` itself;
 *                             2 = always in global memory (the bytes are the same on both routes)
 *   BCP_TUNE_LOCAL_SHARED     which variant of the single-launch step runs: 1 (default) = the library's choice -- a variant
 *                             compiled for shared geometry where the handle has one costmap and one path for all envs, both
 *                             small enough for LDS, no geometry pool, no per-env origins, and 16-wavefront workgroups; the
 *                             generic variant otherwise; 0 = always the generic variant.  Same results bit for bit (the knob
 *                             lets both run against each other on one handle). */
enum { BCP_TUNE_EXACT_MODE = 0, BCP_TUNE_DENSE_THRESHOLD = 1, BCP_TUNE_CULL = 2, BCP_TUNE_DEFER = 3, BCP_TUNE_EDT_LDS = 4,
       BCP_TUNE_FUSED = 5, BCP_TUNE_EGO_SPARSE = 6, BCP_TUNE_NEAR_DILATE = 7, BCP_TUNE_LOCAL_PAIRS = 8,
       BCP_TUNE_EGO_LIST_STRIDE = 9, BCP_TUNE_NEAR_SHIFT = 10, BCP_TUNE_INFLATE_ROUTE = 11,
       BCP_TUNE_GOAL_ROUTE = 12, BCP_TUNE_LOCAL_SHARED = 13 };
int bcp_set_tuning(bcp_handle *h, int32_t key, int32_t value);

/* ---- static per-episode inputs ------------------------------------------------------------------------ */
/* Geometry pool: RandomMiniEnv.reset() with draw_new_turn_on_reset (envs/mini_env.py:469-481) as a batched, masked
 * re-initialisation from n_geoms pre-generated (costmap, path, initial state) entries -- see
 * bc_gym_planning_env_amd/mini_env.py for the sampler (mini_env.py:269-361).  With a pool in effect every
 * NON-shared array given to bcp_set_costmaps / bcp_set_paths / bcp_bind_initial_state has n_geoms entries instead of
 * n_envs, and env i uses entry geom_of_env[i].
 *   geom_of_env  int32 [N], caller-owned device memory, values in [0, n_geoms); read by every step and REWRITTEN by
 *                resets (BCP_STEP_AUTO_RESET and bcp_reset_masked): a reset env moves to next_geom[geom_of_env[i]]
 *                and takes that entry's initial state.
 *   next_geom    int32 [n_geoms] successor table (e.g. g+1 within an env's chain of sampled geometries, or any
 *                permutation), device memory; NULL = stay on the same entry (draw_new_turn_on_reset=False).
 * Call before the arrays are set (changing the entry count invalidates them); n_geoms = 0 turns the pool off. */
int bcp_set_geometry_pool(bcp_handle *h, int32_t n_geoms, int32_t *geom_of_env, const int32_t *next_geom);
/* (bcp_plan_mini_worlds / bcp_release_mini_worlds are the only calls that write next_geom) */
/* (below, N = n_envs, or n_geoms when a geometry pool is in effect)
 * CostMap2D (utilities/costmap_2d.py:13-37).  data: uint8 [rows, cols] when shared, else [N, rows, cols]
 * (row-major, `rows`/`cols` is the padded allocation).  valid_rows/valid_cols (optional, [N] int32) give each
 * env's true map shape for the bounds test of env.py:483-484; NULL => rows/cols.  origins: host double[2] when
 * origins_per_env == 0, else device double [N,2].  Builds the library-owned 1-bit lethal mask
 * (cell == 254) that the step kernel reads and, for a shared map, the distance transform of the lethal cells used
 * to settle most poses without rasterising; call again whenever the costmap content changes. */
int bcp_set_costmaps(bcp_handle *h, const uint8_t *data, int32_t rows, int32_t cols, int32_t shared,
                     const int32_t *valid_rows, const int32_t *valid_cols, const double *origins,
                     int32_t origins_per_env, double resolution, void *stream);

/* Introspection (tests, debugging): the distance field bcp_set_costmaps derived for the pre-classification of poses --
 * floor(min(clamp, Euclidean distance in cells to the nearest lethal cell)) over the map padded by `pad` cells.
 * shape (host int32 [4]) receives {rows + 2 pad, cols + 2 pad, pad, clamp}; out (device uint8 [n_entries][shape0][shape1],
 * or NULL to ask for the shape only) the fields of entries first_entry .. first_entry + n_entries - 1 (entry 0 of a
 * shared map). */
int bcp_get_distance_field(bcp_handle *h, int64_t first_entry, int64_t n_entries, uint8_t *out, int32_t *shape /*host*/,
                           void *stream);
/* The same field as the step's outer test reads it: one bit per cell, set where the field value is < t_out (a lethal
 * cell may touch a footprint whose sample disc is centred there), in tiles of 32 x 32 cells -- bit (x & 31) of word
 * ((y >> 5) * tiles_x + (x >> 5)) * 32 + (y & 31) is cell (y, x) of the padded field.  shape (host int32 [3]) receives
 * {tiles_y, tiles_x, t_out}; out (device uint32 [n_entries][tiles_y * tiles_x * 32], or NULL for the shape only). */
int bcp_get_near_field(bcp_handle *h, int64_t first_entry, int64_t n_entries, uint32_t *out, int32_t *shape /*host*/,
                       void *stream);
/* Static path of the reward provider (ContinuousRewardProviderState.path, reward.py:17-18), already refined.
 * xytheta: double [max_len,3] when shared, else [N,max_len,3]; lens: NULL when shared (then len = max_len) else
 * int32 [N].  Precomputes cos/sin of the waypoint headings (path_tools.py:405) on the device. */
int bcp_set_paths(bcp_handle *h, const double *xytheta, const int32_t *lens, int32_t max_len, int32_t shared,
                  void *stream);

/* ---- state -------------------------------------------------------------------------------------------- */
/* PlanEnv.set_state / get_state (env.py:278-291): the library reads and writes the caller's SoA arrays in
 * place, so "get_state" is reading these tensors and "set_state" is writing them. */
int bcp_bind_state(bcp_handle *h, const bcp_state *state /*host struct of device pointers*/);
/* PlanEnv._initial_state (env.py:247): the snapshot reset()/auto-reset restores (one entry per env, or per pool
 * geometry). */
int bcp_bind_initial_state(bcp_handle *h, const bcp_state *initial /*host struct of device pointers*/);
/* Declares that every env has the SAME initial state (one shared path: make_initial_state depends on the path and the
 * parameters only).  on = 1: the eleven bound arrays x .. robot_collided (n entries each) are copied to the host on `stream`,
 * the stream is synchronised -- bind-time work, not for a captured stream -- and every entry is compared with entry 0 bit for
 * bit (doubles as 64-bit words: a NaN payload or a -0.0 that differs counts; steering_motor_command and wheel_angle are not
 * looked at for the diff-drive model).  If all agree the handle keeps entry 0 as a snapshot and is "declared": steps with
 * BCP_STEP_AUTO_RESET that run the shared-geometry variant of the step kernel (bcp_step_shared_variant) then reset from the
 * snapshot instead of loading the arrays; every other step reads the arrays as before.  Results are the same either way.
 * If an entry differs: BCP_E_INVALID, the message names the first env and the field, and the handle is left undeclared.
 * BCP_E_STATE: no initial state bound, or the handle has a geometry pool.  on = 0 drops the declaration.
 * The snapshot is a VALUE taken at the call: a caller who later rewrites the arrays in place must declare again, or the
 * declared steps keep resetting to the old values.  Any later bcp_bind_initial_state drops the declaration (a plain bind
 * never reads device memory, its arrays may be filled afterwards). */
int bcp_declare_uniform_initial_state(bcp_handle *h, int on, void *stream);
/* PlanEnv.reset (env.py:293-303) for every env with mask[i] != 0 (mask NULL = all). */
int bcp_reset_masked(bcp_handle *h, const uint8_t *mask, void *stream);

/* Monte-Carlo fan-out ("you need to run many rollouts from one state", README.md:45-61): every env with mask[i] != 0
 * (mask NULL = all) takes over env `src`'s complete state -- robot, reward provider, iteration counter, collision
 * flag, geometry-pool entry, delay queues.  The batched form of `s = env.get_state(); other.set_state(s)`. */
int bcp_broadcast_state(bcp_handle *h, int64_t src, const uint8_t *mask, void *stream);

/* ---- the hot path ------------------------------------------------------------------------------------- */
/* PlanEnv.step (env.py:334-361) for all envs: one fused kernel launch. */
int bcp_step(bcp_handle *h, const bcp_step_io *io /*host struct*/, uint32_t flags, void *stream);

/* ---- operator-level seams (the reference's optional native hooks) -------------------------------------- */
/* IRobot.step for n robots (tricycle_model.py:478 / differential_drive.py:236): kinematics only, no collision.
 * state7_io: [7][n] SoA {x,y,angle,v,w,steering_motor_command,wheel_angle}; actions float64 [n,2]. */
int bcp_robot_step(bcp_handle *h, double *state7_io, int64_t n, const double *actions, const double *noise_z,
                   int32_t *err, void *stream);
/* pose_collides(x, y, angle, robot, costmap) (env.py:464-489; twin costmap_utils.py:178-203) for n poses
 * [n,3]; pose i is tested against env (i % n_envs)'s current costmap.  out: uint8 [n]. */
int bcp_pose_collides(bcp_handle *h, const double *poses, int64_t n, uint8_t *out, void *stream);
/* is_robot_colliding(robot_pose, footprint, costmap_data, origin, resolution) (utilities/costmap_utils.py:106-164):
 * pose_collides, except that a robot whose own pixel lies outside the map never collides (in_costmap_bounds, :127-130).
 * Same arguments as bcp_pose_collides. */
int bcp_is_robot_colliding(bcp_handle *h, const double *poses, int64_t n, uint8_t *out, void *stream);
/* is_footprint_colliding_impl(image_slice, blit_mask, lethal) (the native hook of utilities/costmap_utils.py:106-136;
 * Python fallback :163-164: np.any(values == LETHAL)) for n (slice, mask) pairs of one shape: image_slices, blit_masks
 * uint8 [n, rows, cols] (mask: non-zero = footprint cell); out uint8 [n] = any(slice[mask] == lethal). */
int bcp_is_footprint_colliding(bcp_handle *h, const uint8_t *image_slices, const uint8_t *blit_masks, int64_t n,
                               int32_t rows, int32_t cols, uint8_t lethal, uint8_t *out, void *stream);
/* The reward-provider seam (envs/base/reward.py:184-259): reward_provider.reward(state) and .done(state) for n
 * (pose, provider state) pairs against the paths given to bcp_set_paths (pose i: the path of env i % n_envs), with this
 * handle's provider (RewardParams / BCP_REWARD_*).  poses double [n,3]; min_spat_dist_so_far double [n] and target_idx
 * int32 [n] are the provider state, updated in place; robot_collided uint8 [n] or NULL (only the pure-pursuit provider
 * reads it); reward double [n]; goal_reached uint8 [n] or NULL = provider.done(). */
int bcp_reward(bcp_handle *h, const double *poses, int64_t n, double *min_spat_dist_so_far, int32_t *target_idx,
               const uint8_t *robot_collided, double *reward, uint8_t *goal_reached, void *stream);
/* find_last_reached(pose, segment, spatial_precision, angular_precision) (utilities/path_tools.py:432-448) for n poses
 * against the bound paths: out int32 [n] = index of the last way point reached, -1 for None. */
int bcp_find_last_reached(bcp_handle *h, const double *poses, int64_t n, int32_t *out, void *stream);
/* path_velocity(path) (utilities/path_tools.py:298-323): path_txyth double [n_rows,4] rows of (t, x, y, angle) ->
 * v, w double [n_rows - 1]; err int32 [n_rows - 1] or NULL: BCP_ERR_* bits where the reference raises / asserts. */
int bcp_path_velocity(bcp_handle *h, const double *path_txyth, int64_t n_rows, double *v, double *w, int32_t *err,
                      void *stream);
/* get_pixel_footprint_impl(angle, footprint, resolution, fill=True) (path_tools.py:101-162) for n angles.
 * masks: uint8 [n, side, side] (side >= 2*half+1 for every angle), zero-filled then 255 inside; the kernel
 * image of angle i occupies the top-left shape_hw[i] = {2*half_y+1, 2*half_x+1} corner. */
int bcp_pixel_footprint(bcp_handle *h, const double *angles, int64_t n, double resolution, uint8_t *masks,
                        int32_t side, int32_t *shape_hw, void *stream);
/* Done masks as bits, for a job sharded over several GPUs (bc_gym_planning_env_amd/distributed.py: DoneGather(packed=True),
 * bench.py): the only data that crosses GPUs is each rank's done mask, and it crosses as one bit per env --
 * bits[w] bit b = (mask[32 w + b] != 0), n envs -> (n + 31) / 32 words -- an eighth of the bytes an RCCL all-gather has to
 * move while it shares the compute units with the steps.  Device pointers of the current device, asynchronous on `stream`,
 * no handle.  bcp_unpack_mask_bits writes zeros and ones.  No counterpart in the reference (its envs are independent objects,
 * envs/base/env.py; its only vectorised call site, scripts/rl_runners/ppo_runner.py:35-36, runs them in one process). */
int bcp_pack_mask_bits(const uint8_t *mask, int64_t n, uint32_t *bits, void *stream);
int bcp_unpack_mask_bits(const uint32_t *bits, int64_t n, uint8_t *mask, void *stream);

/* normalize_angle_impl (coordinate_transformations.py:17-36) */
int bcp_normalize_angle(bcp_handle *h, const double *in, double *out, int64_t n, void *stream);
/* world_to_pixel_impl (coordinate_transformations.py:169-205): xy [n,2] -> int64 [n,2]; origin host double[2] */
int bcp_world_to_pixel(bcp_handle *h, const double *xy, int64_t n, const double *origin, double resolution,
                       int64_t *out, void *stream);

/* ---- egocentric observation (what envs/egocentric.py:102-160 feeds a policy) ------------------------------ */
/* extract_egocentric_costmap(costmap, pose, resulting_origin, resulting_size, border_value)
 * (utilities/costmap_utils.py:25-75: cv2.getRotationMatrix2D + cv2.warpAffine, INTER_NEAREST) for all envs in one
 * launch: image i = the costmap of env (i % n_envs) seen from poses[i] ([n,3] device doubles; NULL = the bound
 * state's current poses, n = n_envs), robot at (0, 0) heading along +x.  window_origin / window_size: host double[2] in metres (both or neither; NULL = output has
 * the costmap's shape and only the rotation is applied).  out: uint8 [n, shape_hw[0], shape_hw[1]] as reported by
 * bcp_egocentric_shape.  Reads the RAW uint8 costmaps last given to bcp_set_costmaps, which must still be alive
 * (shared maps: the allocation must be readable up to the next multiple of 4 bytes). */
int bcp_egocentric_shape(bcp_handle *h, const double *window_size /*host, or NULL*/, int32_t *shape_hw /*host [2]*/);
int bcp_egocentric_costmaps(bcp_handle *h, const double *poses, int64_t n, const double *window_origin /*host*/,
                            const double *window_size /*host*/, uint8_t border_value, uint8_t *out, void *stream);
/* Which kernel the last bcp_egocentric_costmaps call of this handle ran (no reference counterpart: measurement and tests
 * name the route instead of guessing it).  info4 (host int32[4]): BCP_EGO_* kernel, largest number of non-zero cells of
 * any map entry (-1: not counted), stride of the cell lists, the limit of cells the route decision compared it with. */
enum { BCP_EGO_NONE = 0, BCP_EGO_SPARSE = 1 /* ego_sparse_kernel */, BCP_EGO_STAGED = 2 /* ego_costmap_kernel, shared map in LDS */,
       BCP_EGO_BINNED = 3 /* ego_costmap_binned_kernel */, BCP_EGO_WINDOW = 4 /* ego_costmap_window_kernel */,
       BCP_EGO_GLOBAL = 5 /* ego_costmap_kernel sampling global memory */,
       BCP_EGO_POOLED_SPARSE = 6 /* ego_pooled_sparse_kernel */, BCP_EGO_POOLED_SAMPLED = 7 /* ego_pooled_sampled_kernel */ };
int bcp_egocentric_route(bcp_handle *h, int32_t *info4 /*host*/);
/* The pooled egocentric observation (no reference counterpart; what a resize wrapper around the env would compute, made
 * without the full image ever reaching memory).  Let full[i] be the image bcp_egocentric_costmaps writes for the same
 * arguments, H x W = bcp_egocentric_shape.  Then
 *   out[i][R][C] = max{ full[i][y][x] : R pool <= y < min((R + 1) pool, H),  C pool <= x < min((C + 1) pool, W) },
 * out: uint8 [n, ceil(H / pool), ceil(W / pool)] = bcp_egocentric_pooled_shape.  Edge blocks are partial: nothing outside the
 * image takes part.  Everything else is as for the full-resolution call: poses == NULL means the bound state's poses (the
 * delayed ones under pose_delay), window origin and size go together, a NULL window means the costmap's shape, windows
 * narrower than 4 px are refused; bcp_final_egocentric_costmaps_pooled draws the record's slots j < min(*count, capacity)
 * and leaves the rest untouched.  The call is asynchronous and allocates nothing after first use; the first sparse call
 * after a (re)bind does the counting pass and its read-back.  Cell lists and counts belong to the handle and are shared
 * with bcp_egocentric_costmaps: whichever call runs first builds them, and a pool refresh keeps them valid for both.
 * pool must be in [1, 64] (BCP_E_INVALID otherwise); pool == 1 forwards to the full-resolution routine, identical bytes.
 * Under a maximum 255 (NO_INFORMATION) outranks 254 (LETHAL): a block that holds both reads 255.  (The env families of this
 * library hold only 0 and 254.)  bcp_egocentric_route reports BCP_EGO_POOLED_SPARSE / BCP_EGO_POOLED_SAMPLED for pool > 1. */
int bcp_egocentric_pooled_shape(bcp_handle *h, const double *window_size /*host, or NULL*/, int32_t pool,
                                int32_t *shape_hw /*host [2]*/);
int bcp_egocentric_costmaps_pooled(bcp_handle *h, const double *poses, int64_t n, const double *window_origin /*host*/,
                                   const double *window_size /*host*/, uint8_t border_value, int32_t pool,
                                   uint8_t *out /*[n][ceil(H/pool)][ceil(W/pool)]*/, void *stream);
/* EgocentricCostmap.observation's `goal_n_state` (envs/egocentric.py:140-160) for all envs: the next way point in
 * the robot frame (from_global_to_egocentric, coordinate_transformations.py:341-362) with its position divided by
 * world_size (host double[2] = CostMap2D.world_size() of the egocentric map) and clipped to [-1, 1], followed by
 * robot_state.to_numpy_array().  out: float32 [N, 3 + 6] (tricycle) / [N, 3 + 5] (diff-drive); zeros for envs whose
 * path is exhausted. */
int bcp_goal_n_state(bcp_handle *h, const double *world_size /*host*/, float *out, void *stream);
/* ColoredEgoCostmapRandomAisleTurnEnv's `goal` vector (envs/synth_turn_env.py:412-420) for all envs: the LAST way
 * point in the robot frame divided by world_size and normalised to unit length, then the robot's egocentric state
 * (v, w, wheel_angle; 0 for a diff-drive robot).  out: float64 [N, 5]. */
int bcp_goal_direction_state(bcp_handle *h, const double *world_size /*host*/, double *out, void *stream);

/* ---- RandomMiniEnv worlds sampled on the device ------------------------------------------------------------ */
/* RandomMiniEnvParams (envs/mini_env.py:30-47) + the EnvParams fields the sampler reads.  host struct. */
typedef struct bcp_mini_world_params {
    double inner_h, inner_w, mid_margin, out_margin;
    double min_obstacle_angle, max_obstacle_angle;
    double lim_euc_dist, lim_ang_dist, angular_pose_noise_scale;
    double resolution;      /* EnvParams.resolution */
    double goal_spat_dist;  /* EnvParams.goal_spat_dist / goal_ang_dist: start and goal must not be this close */
    double goal_ang_dist;
} bcp_mini_world_params;
/* numpy.random.RandomState(seed) for n_chains independent streams: mt_state is uint32 [n_chains][625] device memory
 * (624 MT19937 words + the position), seeds int64 [n_chains] device memory (0 <= seed < 2^32, mt19937_seed). */
int bcp_mini_world_seed(bcp_handle *h, const int64_t *seeds, int64_t n_chains, uint32_t *mt_state, void *stream);
/* _sample_mini_env_params (envs/mini_env.py:328-359) `episodes` times in a row for every stream, one wavefront per
 * stream: same draw order as the reference, two 1-px walls (cv2.line), pose_collides of both path ends with this
 * handle's footprint, "not too close" test; the streams continue where they stopped.  Outputs (device):
 *   worlds  double [n_chains * episodes][14] = start(3), end(3), obstacle_a(2), obstacle_o(2), obstacle_b(2), h, w
 *   maps    uint8  [n_chains * episodes][rows][cols]  (rows, cols as CostMap2D.create_empty gives them for (h, w))
 *   status  int32  [n_chains]  0, or 1 where the reference would raise "the sampling space looks empty"
 * Transcendentals are the device's: a world can differ from numpy's in the last bit of a coordinate. */
int bcp_sample_mini_worlds(bcp_handle *h, const bcp_mini_world_params *p /*host*/, uint32_t *mt_state, int64_t n_chains,
                           int32_t episodes, int32_t rows, int32_t cols, double *worlds, uint8_t *maps, int32_t *status,
                           void *stream);

/* make_initial_state (envs/base/env.py:179-214) for sampled worlds, on the device: refine_path of each world's coarse
 * (start, end) path (utilities/path_tools.py:178-240) and the initial state of this handle's reward provider
 * (reward.py:261-288 / :355-371).  worlds as bcp_sample_mini_worlds writes them; paths: double [n_worlds][max_len][3];
 * lens: int32 [n_worlds]; init: double [n_worlds][2] = (min_spat_dist_so_far, target_idx); status: int32 [n_worlds],
 * 0 = ok, 1 = the refined path does not fit max_len, 2 = "Goal pose too close to initial pose". */
int bcp_mini_world_paths(bcp_handle *h, const double *worlds, int64_t n_worlds, double path_delta, int32_t max_len,
                         double *paths, int32_t *lens, double *init, int32_t *status, void *stream);

/* A pool that never runs out: RandomMiniEnv.reset() draws a NEW world every time (envs/mini_env.py:441-459), a pool
 * of `episodes` entries per stream would wrap around.  For a handle whose geometry pool has n_envs x episodes entries,
 * env c on the entries c * episodes .. + episodes - 1 of stream c (mt_state [n_envs][625], worlds / maps / paths / lens
 * / init as produced by bcp_sample_mini_worlds + bcp_mini_world_paths and handed to bcp_set_costmaps / bcp_set_paths /
 * bcp_bind_initial_state), three calls top the pool up behind the envs without a host round trip.  World number j of
 * stream c lives in entry c * episodes + j % episodes; next_geom (the array given to bcp_set_geometry_pool, WRITTEN
 * here) is a ring with one guard: the entry of the newest world points to itself, so an env that gets there before new
 * worlds are ready repeats that world instead of wrapping onto an old one (set next_geom[c * episodes + episodes - 1]
 * to itself before the first step).
 *   1. bcp_plan_mini_worlds     looks where every env is, marks the entries of the worlds it has left as free and
 *                               closes the ring behind the last of them (the next guard).
 *        generated  int64 [n_envs] device, in/out: worlds drawn from each stream so far (`episodes` after the first fill)
 *        info       int32 [4] device, out: {entries freed, envs found waiting on their guard entry, 0, 0}
 *   2. bcp_refresh_mini_worlds  samples the next worlds of each stream into the free entries: costmap, path, lens, init
 *                               and initial state are rewritten in place and the handle's derived data (lethal masks,
 *                               distance fields, path index) is rebuilt for exactly those entries.
 *        status  int32 [n_envs]: as bcp_sample_mini_worlds;  path_status int32 [n_envs * episodes]: as bcp_mini_world_paths
 *   3. bcp_release_mini_worlds  opens the previous guard: the envs can walk on into the new worlds.
 * 1 and 3 belong on the stream of the steps.  Sampling a world is a latency-bound job for one wavefront (~0.3 ms, with
 * a long tail), so 2 may run on a SIDE stream while steps go on -- they neither read nor reach an entry that is being
 * rewritten: make the side stream wait for 1 and the stream of the steps wait for 2 before 3 (events).  With one
 * plan-refresh-release round per `episodes - 1` episodes of the fastest env no world is ever repeated. */
int bcp_plan_mini_worlds(bcp_handle *h, int32_t episodes, int64_t *generated, int32_t *info, void *stream);
int bcp_refresh_mini_worlds(bcp_handle *h, const bcp_mini_world_params *p /*host*/, uint32_t *mt_state, double *worlds,
                            uint8_t *maps, double *paths, int32_t *lens, double *init, double path_delta, int32_t *status,
                            int32_t *path_status, void *stream);
int bcp_release_mini_worlds(bcp_handle *h, void *stream);

/* ---- the on-device noise stream (introspection) --------------------------------------------------------------- */
/* A stream of the handle that may only use `cu_percent` % of the device's compute units, spread evenly over the chip
 * (hipExtStreamCreateWithCUMask).  For work that runs BESIDE the steps: the single-launch step wants whole compute units
 * (one 1024-thread workgroup each), and behind a kernel of small long-running workgroups on an ordinary side stream -- the
 * world sampler of bcp_refresh_mini_worlds -- a step launch can wait until that kernel has drained (measured: 18 ms).  On a
 * masked stream such a kernel leaves the other compute units to the steps.  Measured in round 3: with 50 %
 * the endless pool ran SLOWER (0.078 against 0.064 ms per step) -- the refresh takes twice as long and the steps' own
 * workgroups still land on the masked units too -- so the Python layer defaults to an ordinary stream; the entry point is
 * kept for callers whose side work is lighter.  The stream belongs to the handle (destroyed
 * with it; asking for another share replaces it after a synchronisation).  BCP_E_HIP when the runtime refuses: use an
 * ordinary stream.  No counterpart in the reference. */
int bcp_side_stream(bcp_handle *h, int32_t cu_percent, void **stream);

/* n_steps steps in one call, for callers that hold the actions of a whole rollout (open-loop Monte-Carlo rollouts from one
 * state, the use the reference documents in its README; no counterpart function in the reference, whose PlanEnv.step takes
 * one action).  Every array of bcp_step_io has a leading [n_steps] dimension: actions [n_steps][N][2], noise_z /
 * noise_z_out [n_steps][N][3], reward / done / collided_now / err [n_steps][N]; row k is what the k-th of n_steps calls of
 * bcp_step would read and write, and the state ends where those calls would leave it -- bit for bit, in-kernel resets and
 * the on-device noise stream included.  With the single-launch step form (bcp_step_form() == 3) the steps are ONE launch:
 * the workgroups advance independently and launch, argument fetch and staging are paid once; other forms are stepped one
 * launch at a time. */
int bcp_rollout(bcp_handle *h, const bcp_step_io *io, int32_t n_steps, uint32_t flags, void *stream);

/* Health of the step kernel's internal hand-offs.  The single-launch step passes undecided poses between the wavefronts of a
 * workgroup through LDS; every wait on such a hand-off is bounded (~10^7 cycles against the ~2 * 10^4 a step lasts).  A
 * wait that runs into its limit gives up -- the step still finishes; an env whose verdict never arrived is finished as
 * "free" with BCP_ERR_INTERNAL in `err` -- and is counted here.  *count = waits that gave up since bcp_create (host
 * pointer; the call synchronises `stream`).  Anything but 0 means a defect of the library, never of the caller's data.
 * bcp_step also watches this counter by itself, without ever waiting for the GPU: every 256 calls it copies the counter to
 * pinned host memory behind the step it has just launched, and a later bcp_step that finds the copy landed and the counter
 * grown returns BCP_E_INTERNAL (once per growth; the step of that call has been launched all the same).  Steps replayed
 * from a captured hipGraph do not pass through bcp_step: such callers ask here.  No counterpart in the reference. */
int bcp_expired_waits(bcp_handle *h, int64_t *count, void *stream);
/* Poses the single-launch step (step_local_kernel) could not clear by its distance-field classification and handed to the
 * exact footprint test (pose_collides proper, envs/base/env.py:464-489), summed over all steps since bcp_create: the
 * "parked-pose fraction" of a workload is the growth of this counter over a run / (n_envs * steps).  Host pointer; the call
 * synchronises `stream`.  The other step forms do not count.  No counterpart in the reference (measurement only). */
int bcp_parked_poses(bcp_handle *h, int64_t *count, void *stream);

/* The standard normals a step draws when bcp_step_io.noise_z is NULL (the stand-in for np.random.normal of
 * robot_models/differential_drive.py:43-52): out double [n_steps][n_envs][3] = the three slots of envs first_env ..
 * first_env + n_envs - 1 of this handle at step counters first_step .. first_step + n_steps - 1, for the handle's seed
 * and env_id_base.  (A step consumes slot k only when variance_k > 0, like the reference.)  Any n_envs, not only the
 * handle's. */
int bcp_device_normals(bcp_handle *h, int64_t first_env, int64_t n_envs, uint64_t first_step, int32_t n_steps, double *out,
                       void *stream);

/* ---- RandomAisleTurnEnv worlds made on the device ---------------------------------------------------------- */
/* The ranges RandomAisleTurnEnv._draw_random_turn_params draws from (envs/synth_turn_env.py:317-332; low, high each),
 * TurnParams.margin (:31) and the EnvParams fields the world needs.  host struct. */
typedef struct bcp_aisle_world_params {
    double main_corridor_length[2], turn_corridor_length[2], turn_corridor_angle[2];
    double main_corridor_width[2], turn_corridor_width[2];
    double margin;
    double resolution;   /* EnvParams.resolution: below 0.025 m the walls would be 2 px thick -> BCP_E_INVALID */
    double path_delta;   /* EnvParams.path_delta: only the refined path length of the record depends on it */
} bcp_aisle_world_params;
/* _draw_random_turn_params (envs/synth_turn_env.py:317-332) `episodes` times in a row for every stream (mt_state as
 * bcp_mini_world_seed makes it; the streams continue where they stopped), and what path_and_costmap_from_config
 * (:110-192) computes before it draws: one wavefront per stream.  World k of stream c is entry c * episodes + k.
 * Outputs (device):
 *   worlds  double [n_chains * episodes][44]: [0, 8) turn params (main / turn corridor length, turn angle, main / turn
 *           corridor width, flip_arnd_oy, flip_arnd_ox as 0 / 1, rot_theta), [8, 10) world origin, [10, 30) corners
 *           A .. J (:42-79), [30, 42) oriented way points B, K, L, F (:82-97) after rotation and flips, [42] the length
 *           of the refined path (utilities/path_tools.py:178-240), [43] 0
 *   shapes  int32  [n_chains * episodes][2] = (rows, cols) of the world's map (CostMap2D.create_empty,
 *           utilities/costmap_2d.py:58-69)
 * There is no rejection: the reference tests nothing.  Transcendentals are the device's: a coordinate can differ from
 * numpy's in its last bit. */
int bcp_sample_aisle_worlds(bcp_handle *h, const bcp_aisle_world_params *p /*host*/, uint32_t *mt_state, int64_t n_chains,
                            int32_t episodes, double *worlds, int32_t *shapes, void *stream);
/* The five 1-px walls of every world (:174-190, Wall.render -> cv2.line, envs/base/maps.py:28-44) into padded pool
 * entries, one workgroup per world: maps uint8 [n_worlds][rows][pitch] (device, 16-byte aligned) is zeroed entry by
 * entry and each world is drawn into its own shapes[g] = (rows_g, cols_g) corner; the padding stays 0.  pitch must be a
 * multiple of 16, and rows / pitch at least every world's rows / cols: a world that does not fit is left empty. */
int bcp_render_aisle_worlds(bcp_handle *h, const double *worlds, const int32_t *shapes, int64_t n_worlds,
                            double resolution, int32_t rows, int32_t pitch, uint8_t *maps, void *stream);
/* make_initial_state (envs/base/env.py:179-214) for aisle worlds: refine_path of the coarse path B K L F
 * (utilities/path_tools.py:178-240: np.linspace arithmetic, inserted points carry their segment's first heading) and the
 * initial state of this handle's reward provider (reward.py:261-288 / :355-371).  paths / lens / init / status as
 * bcp_mini_world_paths (max_len: at least the largest record[42]). */
int bcp_aisle_world_paths(bcp_handle *h, const double *worlds, int64_t n_worlds, double path_delta, int32_t max_len,
                          double *paths, int32_t *lens, double *init, int32_t *status, void *stream);

/* ---- episode ends under auto-reset ---------------------------------------------------------------------- */
/* Why an env's episode ended: the three terms of PlanEnv's done (envs/base/env.py:400-419 -- goal reached, current_iter >=
 * iteration_timeout, robot_collided); several may be set at once.  A time-out alone is a truncation (the episode was cut,
 * its last state is not terminal: a learner bootstraps V(s_T) there); goal and collision are terminal. */
enum { BCP_DONE_GOAL = 1, BCP_DONE_TIMEOUT = 2, BCP_DONE_COLLIDED = 4 };

/* Where the step leaves every env whose episode ends (done = 1), before BCP_STEP_AUTO_RESET restores its initial state:
 * what the reference's caller sees from step() before it calls reset() (env.py:334-361, 293-303).  Host struct of device
 * pointers, caller-owned; N = n_envs. */
typedef struct bcp_episode_record {
    int64_t capacity;      /* slots in the [capacity] arrays */
    uint8_t *reason;       /* [N] BCP_DONE_* bits of the last step, 0 where done = 0 (written for every env) */
    double *ret;           /* [N] running float64 sum of this episode's rewards in step order (the rewards of
                              reward.py:66-69 / :144-153), or NULL = not kept.  Zeroed by every reset (auto-reset,
                              bcp_reset_masked); bcp_broadcast_state and writes of the state arrays leave it alone */
    int32_t *count;        /* [1] envs that ended in the last step (may exceed capacity: overflow) */
    int32_t *env_id;       /* [capacity] which env ended, one slot per ended env, order unspecified */
    int32_t *geom;         /* [capacity] pool entry the episode ran on (-1 without a geometry pool) */
    double *final_ret;     /* [capacity] the episode's return (needs ret) */
    bcp_state final;       /* [capacity] each: the State the env held after its last step, BEFORE the reset -- x ..
                              robot_collided (current_iter = episode length); pose_seen [3][capacity] / robot_state_seen
                              [7][capacity] when pose_delay / state_delay > 0; the queue pointers must be NULL */
} bcp_episode_record;

/* Binds (rec != NULL) or unbinds (NULL) the episode record.  From then on every step -- every step form, with and without
 * BCP_STEP_AUTO_RESET -- gives each env with done = 1 exactly one slot (without auto-reset an env that is not reset ends
 * again on every step, as the reference's done stays true), and its final state is bit for bit the state a handle without
 * auto-reset holds after the same step.  *count is published on the device by the step itself: no host synchronisation,
 * no extra launch, the same launch arguments from step to step (captured steps replay).  Without a record the step kernels
 * do not look at one.  bcp_rollout refuses to run with a record bound (BCP_E_STATE).  Binding synchronises the device (it
 * re-arms the library's counters, which steps still in flight on any stream may be using) and does not touch `ret`: the
 * caller zeroes it, and a record bound in the middle of episodes returns partial sums for them. */
int bcp_bind_episode_record(bcp_handle *h, const bcp_episode_record *rec /*host struct of device pointers; NULL = unbind*/);
/* Steps whose count exceeded the capacity since the last call (or the bind): *steps, host pointer; synchronises `stream`.
 * Slots beyond the capacity are counted but not written. */
int bcp_episode_record_overflows(bcp_handle *h, int64_t *steps /*host*/, void *stream);
/* The observations of the episodes that ended in the last step (SB3's terminal_observation, gymnasium's final_obs), drawn
 * from the record on the device: slot j < min(*count, capacity) from final state j on pool entry geom[j] (private maps
 * without a pool: env_id[j]); slots beyond are left untouched.  No host synchronisation.  Same outputs as
 * bcp_egocentric_costmaps / bcp_goal_n_state / bcp_goal_direction_state with [capacity] rows. */
int bcp_final_egocentric_costmaps(bcp_handle *h, const double *window_origin /*host*/, const double *window_size /*host*/,
                                  int32_t border_value, uint8_t *out /*[capacity][H][W]*/, void *stream);
/* the pooled images of those slots (bcp_egocentric_costmaps_pooled) */
int bcp_final_egocentric_costmaps_pooled(bcp_handle *h, const double *window_origin /*host*/, const double *window_size /*host*/,
                                         int32_t border_value, int32_t pool, uint8_t *out /*[capacity][..][..]*/, void *stream);
int bcp_final_goal_n_state(bcp_handle *h, const double *world_size /*host*/, float *out, void *stream);
int bcp_final_goal_direction_state(bcp_handle *h, const double *world_size /*host*/, double *out, void *stream);

/* ---- range observation: distances to the nearest obstacle along beams fixed to the robot ------------------ */
/* A planar range scan per row, by an exact walk over the grid (no reference counterpart: the reference's observations are
 * images; this is what a navigation learner is usually fed instead).  One launch, asynchronous on `stream`, no allocation,
 * no host synchronisation; the launch arguments depend only on the pointers and numbers given, so a call can be captured
 * into a HIP graph -- after one ordinary call with the same maps bound: with a shared map staged in LDS the first call on a
 * device may have to raise the kernel's dynamic-LDS limit, which is not a stream operation.
 * Rows: exactly those of bcp_egocentric_costmaps.  poses is [n,3] device doubles, row i is seen on the map entry of env
 * i % n_envs (geom_of_env under a pool); poses == NULL requires n == n_envs and means the bound state's pose (pose_seen when
 * pose_delay > 0).  bcp_final_range_scan draws slots j < min(*count, capacity) of the bound episode record on entry geom[j]
 * (private maps without a pool: env_id[j]) and leaves the other rows untouched, in every output.
 * Beams: beam_cs[b] = (cos phi_b, sin phi_b), phi_b the beam's angle from the robot's heading, counter-clockwise: a device
 * table [n_beams][2] the caller makes and owns.  The library computes no transcendental per beam.
 * Obstacles: a cell is an obstacle exactly where the lethal mask is set, data == 254 inside the entry's valid shape -- the
 * set bcp_pose_collides tests.  255, 253 and inflated costs are free space, and so is everything outside the valid shape,
 * padding included: inflating the maps changes no range.
 * Arithmetic: float64 throughout, every product, quotient and sum rounded on its own.  For a row with pose (x, y, theta)
 * on an entry with origin (ox, oy):
 *   (c, s) = (cos theta, sin theta)                  the device's; written to heading_cs_out[row] when given
 *   u = (x - ox) * inv_res + 0.5                     inv_res = 1 / resolution as bcp_set_costmaps rounds it
 *   v = (y - oy) * inv_res + 0.5                     cell (row, col) covers [col, col + 1) x [row, row + 1)
 *   R = max_range * inv_res
 *   for each beam b with (cb, sb):
 *     dx = c*cb - s*sb ;  dy = s*cb + c*sb
 *     col = floor(u), row = floor(v)
 *     sx = dx > 0 ? 1 : -1,  sy likewise
 *     tdx = dx != 0 ? |1.0 / dx| : +inf,  tdy likewise
 *     tmx = dx > 0 ? (col + 1 - u) / dx : dx < 0 ? (col - u) / dx : +inf        tmy likewise with row, v, dy
 *     t = 0.0
 *     while t < R:
 *         if 0 <= row < valid_rows and 0 <= col < valid_cols and lethal(row, col):
 *             -> ranges = (float)(t * resolution), hit = row * cols + col ; done
 *         if tmx < tmy: t = tmx; tmx += tdx; col += sx
 *         else:         t = tmy; tmy += tdy; row += sy          (a tie steps in y)
 *     -> ranges = (float)max_range, hit = -1
 * A start cell that is lethal gives range 0; a pose outside the map walks free space until it enters the map or reaches R.
 * The loop crosses one grid line per trip and is cut after 2 * ceil(R) + 4 trips (a miss), which no ray of unit direction
 * reaches.  Rows whose pose has a non-finite component, or with |u| or |v| >= 2^30, get max_range / -1 in every beam, and
 * their heading_cs_out is unspecified.  A ray that passes exactly through the shared corner of two diagonally adjacent wall
 * cells may slip through an 8-connected wall (a cv2.line wall); every other ray cannot: the walk visits every cell the ray
 * touches.
 * ranges: float32 [n][n_beams] in metres; hit: optional int32 [n][n_beams]; heading_cs_out: optional float64 [n][2].
 * BCP_E_INVALID: NULL h, beam_cs or ranges; n_beams outside [1, 1024]; n <= 0, or n != n_envs without poses; max_range not
 * finite, not > 0, or max_range * inv_res > 4096.  BCP_E_STATE: no costmaps bound; no state bound with poses == NULL; no
 * record bound (bcp_final_range_scan). */
int bcp_range_scan(bcp_handle *h, const double *poses, int64_t n, const double *beam_cs /*device [n_beams][2]*/,
                   int32_t n_beams, double max_range, float *ranges /*[n][n_beams]*/, int32_t *hit /*optional [n][n_beams]*/,
                   double *heading_cs_out /*optional [n][2]*/, void *stream);
int bcp_final_range_scan(bcp_handle *h, const double *beam_cs, int32_t n_beams, double max_range,
                         float *ranges /*[capacity][n_beams]*/, int32_t *hit, double *heading_cs_out, void *stream);

/* ---- look-ahead: score K candidate plans per env without stepping it ------------------------------------- */
/* bcp_lookahead flags (it also takes BCP_STEP_ACTIONS_F32) */
enum {
    BCP_LOOKAHEAD_PER_ENV = 1 << 8 /* actions are [H][N][K][2]: every env has candidates of its own; otherwise [H][K][2],
                                      one candidate library shared by all envs */
};

/* Inputs / outputs of bcp_lookahead.  Host struct of device pointers, caller-owned; N = n_envs, H = horizon,
 * K = n_candidates.  No counterpart struct in the reference: it is what a planner's `.act(obs)` (README "motion planning
 * challenge", bc_gym_planning_env/run_the_challange.py) works out with get_state / set_state and H x K calls of PlanEnv.step. */
typedef struct bcp_lookahead_io {
    const void *actions;       /* [H][K][2], or [H][N][K][2] with BCP_LOOKAHEAD_PER_ENV: step t of candidate k; float64, or
                                  float32 with BCP_STEP_ACTIONS_F32, widened before any arithmetic as in bcp_step */
    const double *noise_z;     /* NULL: the noise-free forward model (the arithmetic of a handle created with noise_on = 0,
                                  whatever this handle's setting), or [H][N][K][3] standard normals in slot order, consumed
                                  as bcp_step_io.noise_z is (needs params.noise_on).  The on-device Philox stream is never
                                  used and never advanced */
    const uint8_t *mask;       /* optional [N]: rows of envs with mask[i] == 0 are left untouched in every output */
    int32_t horizon;           /* H >= 1 */
    int32_t n_candidates;      /* K >= 1; N * K * H * 3 must stay below 2^62 (the element offsets are 64-bit) */
    double *ret;               /* [N][K] float64 sum of the rewards of the steps taken, added in step order from 0.0 (the rule
                                  of bcp_episode_record.ret; rewards of reward.py:66-69 / :144-153) */
    int32_t *steps;            /* [N][K] steps taken: index of the first step with done = 1 (env.py:407-419) plus one, else H */
    uint8_t *reason;           /* [N][K] BCP_DONE_* bits of that done step (as bcp_episode_record.reason), 0 if none was done */
    double *final_pose;        /* optional [N][K][3]: State.pose after the last step taken (after the roll-back of
                                  env.py:458-459 where it collided) */
    int32_t *final_target_idx; /* optional [N][K]: the reward provider's target_idx after the last step taken */
    int32_t *err;              /* optional [N][K]: OR of the BCP_ERR_* bits of the steps taken */
    int32_t *best;             /* optional [N]: the candidate with the largest key (reason & BCP_DONE_COLLIDED ? 0 : 1, ret),
                                  compared lexicographically; ties go to the lowest k */
    void *best_action;         /* optional [N][2], dtype of `actions` (needs best): step 0 of candidate best[i] for env i --
                                  can be passed to bcp_step as it is */
} bcp_lookahead_io;

/* For every env i and candidate k: a private copy of env i's state (x .. robot_collided, its map / path / pool entry) is
 * stepped `horizon` times with the candidate's actions, WITHOUT auto-reset, stopping after the first step whose done is 1
 * -- PlanEnv.step (envs/base/env.py:334-361) H times on a copy made with get_state / set_state (env.py:305-330).  An env
 * that is already done takes its first step, which is done, like the reference's.  Nothing of the handle changes: no state
 * array, not geom_of_env, not the step counter or the noise stream, not a bound episode record.  Asynchronous on `stream`,
 * no allocation, no synchronisation; the launch arguments depend only on the pointers given, so a call can be captured into
 * a HIP graph (on a pool whose maps are refreshed by bcp_refresh_mini_worlds, capture after the refresh: the call settles
 * stale distance fields on its stream like bcp_pose_collides).
 * Refused with BCP_E_INVALID: control_delay, pose_delay or state_delay > 0 (every candidate would need private delay
 * queues), horizon < 1, n_candidates < 1, noise_z on a handle without noise_on, best_action without best.  There is no
 * other limit on H or K: a candidate is one lane, K may be smaller or larger than a wavefront. */
int bcp_lookahead(bcp_handle *h, const bcp_lookahead_io *io, uint32_t flags, void *stream);

/* ---- plan refinement by sampling (MPPI): sample, roll out, weight, update -- I times in one launch -------- */
/* Parameters of bcp_mppi, passed to the kernel by value. */
typedef struct bcp_mppi_params {
    int32_t horizon, n_candidates, iterations;   /* H, K, I */
    double  sigma[2];           /* std of the perturbation per action component, >= 0 */
    double  low[2], high[2];    /* the action box (action_space.low / high widened to float64) */
    double  lambda_;            /* temperature, > 0 */
    double  collision_penalty;  /* subtracted from the score of a candidate whose reason has BCP_DONE_COLLIDED */
    uint64_t seed, draw_index;  /* perturbation stream; draw_index is used when io.draw_index is NULL */
} bcp_mppi_params;

/* Host struct of device pointers, caller-owned; N = n_envs. */
typedef struct bcp_mppi_io {
    double *mean;               /* [N][H][2] in: the plan to refine (warm start); out: after I iterations */
    void   *action;             /* [N][2]: step 0 of the refined mean, float64, or float32 with BCP_STEP_ACTIONS_F32 */
    const uint8_t *mask;        /* optional [N]; mask 0: mean / action rows (and every optional output's) untouched */
    const float *eps_in;        /* optional [I][N][K][H][2]: parity mode, the perturbations to use (candidate 0's are ignored) */
    float  *eps_out;            /* optional, same shape: the perturbations used (replay) */
    const uint64_t *draw_index; /* optional device word: read by the kernel instead of params.draw_index */
    double *iter_mean;          /* optional [I][N][H][2]: the mean going INTO iteration j */
    double *iter_ret;           /* optional [I][N][K] */
    uint8_t *iter_reason;       /* optional [I][N][K] */
    int32_t *err;               /* optional [N]: OR of the candidates' err bits */
} bcp_mppi_io;

/* Refines one plan per env by model-predictive path integral control.  All arithmetic is float64, each product and sum
 * rounded on its own.  For iteration j, env i, candidate k, step t, component d:
 *     u = min(max(mean_j[i][t][d] + sigma[d] * (double)eps_j[i][k][t][d], low[d]), high[d])
 * Candidate 0 is the unperturbed mean (eps = 0, written as 0 to eps_out).  Every candidate is rolled out exactly as
 * bcp_lookahead with noise_z = NULL rolls out per-env float64 actions u: a private copy of env i's state, the noise-free
 * forward model, no auto-reset, stop after the first done step, ret added in step order from 0.0.  Then
 *     s_k = ret_k - collision_penalty * [reason_k & BCP_DONE_COLLIDED]
 *     w_k = exp((s_k - max_k s) / lambda_) / sum_k exp((s_k - max_k s) / lambda_)
 *     mean_{j+1}[i][t][d] = sum_k w_k * u_k[t][d]        (steps after a candidate's done step count with their u)
 * After the last iteration `mean` holds mean_I and action[i] = mean_I[i][0] (rounded to float32 under the flag): it can be
 * passed to bcp_step as it is.  The order of the sum over k is unspecified (partial sums per lane, then a butterfly).
 * Perturbations: read from eps_in, or drawn on the device -- Philox4x32-10 keyed by `seed` on a counter made of (env index,
 * draw_index, j, k, t), one float32 Box-Muller pair for the two components: deterministic, |eps| <= 5.89, the same values
 * for the same (seed, draw_index); distinct streams for draw_index < 2^52 and I * H <= 2^32.  The step's own noise stream
 * is never read or advanced.
 * Nothing of the handle changes (as for bcp_lookahead): no step kernel runs, no state array, step counter, noise stream or
 * episode record is touched.  One kernel launch, asynchronous on `stream`, no allocation, no synchronisation; the launch
 * arguments are the caller's pointers and *p by value, so a call can be captured into a HIP graph, and with io->draw_index
 * successive replays draw fresh perturbations once the caller has changed that word.
 * Refused with BCP_E_INVALID:
 *   - control_delay, pose_delay or state_delay > 0 (every candidate would need private delay queues);
 *   - horizon < 1 or iterations < 1;
 *   - n_candidates not a power of two in [8, 1024] (the K candidates of an env share a wavefront, or K / 64 passes of one);
 *   - lambda_ not > 0 (or not finite);
 *   - a negative or non-finite sigma;
 *   - low[d] > high[d]; a non-finite low, high or collision_penalty;
 *   - 5 * I * N * K * H >= 2^62 (the element offsets are 64-bit);
 *   - flag bits other than BCP_STEP_ACTIONS_F32; mean or action NULL. */
int bcp_mppi(bcp_handle *h, const bcp_mppi_params *p, const bcp_mppi_io *io, uint32_t flags, void *stream);

/* The terminal cost of bcp_mppi_field: a goal field of the handle's map binding (bcp_goal_field, below) and what a metre
 * of distance to go costs.  Host struct of device pointers, caller-owned. */
typedef struct bcp_mppi_terminal {
    const uint16_t *field;   /* [n_fields][rows][cols], as bcp_goal_field wrote it */
    int64_t n_fields;        /* 1, or the handle's entry count (pool entries, else n_envs) */
    int32_t rows, cols;      /* must equal the map binding's */
    double  weight;          /* reward per metre of distance to go, finite, >= 0 */
    int32_t *iter_value;     /* optional [I][N][K]: the field value read for the candidate (65535 = none) */
    double  *iter_score;     /* optional [I][N][K]: s_k as weighted */
} bcp_mppi_terminal;

/* bcp_mppi with the distance to go at a candidate's final pose in its score: what the H steps of the roll-out cannot see.
 * Everything bcp_mppi specifies holds unchanged -- sampling, roll-outs, iter_ret / iter_reason (the pure return and reason),
 * the weights and the update from the scores, one launch, nothing of the handle written, capture into a HIP graph, every
 * refusal -- and only s_k differs.  For candidate k let (x, y) be its pose after the last step taken (after the roll-back
 * where it collided: bcp_lookahead's final_pose) and g its env's slot (geom_of_env[i], else i):
 *     (col, row) = half-to-even of ((x - ox) * inv_res, (y - oy) * inv_res), with the origin, inv_res and valid shape that
 *                  bcp_goal_field_sample uses for that env's entry (entry 0 when the map is shared)
 *     v   = field[n_fields == 1 ? 0 : g][row][col], or BCP_GOAL_NONE if x or y is not finite or the cell is outside the
 *           valid shape
 *     d   = ((double)(v == BCP_GOAL_NONE ? BCP_GOAL_FAR : v) * resolution) / 12.0      (float64, never through float32)
 *     s_k = ret_k; if reason_k & BCP_DONE_COLLIDED: s_k = s_k - collision_penalty; then s_k = s_k - weight * d
 * every product and sum rounded on its own, in that order.  With weight == 0 every output of bcp_mppi is the same bit for
 * bit (d is always finite).  The read is one 2-byte load per live candidate and iteration.
 * Refused with BCP_E_INVALID (messages prefixed "bcp_mppi_field: "): everything bcp_mppi refuses; term or term->field NULL;
 * weight negative or not finite; rows / cols other than the binding's; n_fields neither 1 nor the entry count. */
int bcp_mppi_field(bcp_handle *h, const bcp_mppi_params *p, const bcp_mppi_io *io, const bcp_mppi_terminal *term,
                   uint32_t flags, void *stream);

/* The widths of bcp_mppi_adapt.  Host struct of device pointers, caller-owned.  (Named for what it holds: a C tag may share
 * its name with a function, a typedef name may not.) */
typedef struct bcp_mppi_widths {
    double *sigma;          /* [N][H][2] in / out: std of the perturbation per env, step and component */
    double sigma_min[2];    /* finite, >= 0 */
    double sigma_max[2];    /* finite, >= sigma_min */
    double rate;            /* in [0, 1]: how far a width moves towards the weighted spread per iteration */
    double *iter_sigma;     /* optional [I][N][H][2]: the widths going INTO iteration j (after the entry clamp) */
} bcp_mppi_widths;

/* bcp_mppi (term == NULL) or bcp_mppi_field (term given) with a sampling width per env, step and component that follows the
 * weights, CEM-style: a plan the weights agree on is perturbed less the next time, one they spread over keeps its width.
 * Everything bcp_mppi specifies holds -- the sampling stream, eps_in / eps_out, candidate 0, the roll-outs, iter_ret /
 * iter_reason, the scores (with term exactly bcp_mppi_field's, iter_value / iter_score included), the weights and the mean
 * update, one launch, nothing of the handle written, capture into a HIP graph with io->draw_index -- and two things differ.
 * The width used.  Let clampd(s) = !(s >= sigma_min[d]) ? sigma_min[d] : (s > sigma_max[d] ? sigma_max[d] : s): a NaN goes
 * to the minimum.  On entry sigma_0[i][t][d] = clampd(sigma[i][t][d]), and for iteration j
 *     u = min(max(mean_j[i][t][d] + sigma_j[i][t][d] * (double)eps_j[i][k][t][d], low[d]), high[d])
 * p->sigma is checked as bcp_mppi checks it and is otherwise not read.
 * The width update.  With the weights w_k and the new mean row m' = mean_{j+1}[i][t][d], in float64, every difference,
 * product, root and sum rounded on its own (the order of the sum over k unspecified, as for the mean):
 *     v  = sum_k w_k * ((u_k - m') * (u_k - m'))
 *     sd = sqrt(v)
 *     sigma_{j+1}[i][t][d] = clampd(sigma_j + rate * (sd - sigma_j))
 * After the last iteration `sigma` holds sigma_I.  Rows of envs with mask 0 are untouched, in sigma and iter_sigma as
 * everywhere else.
 * With rate == 0 and every sigma[i][t][d] == p->sigma[d] inside the clamps, every output that bcp_mppi has (bcp_mppi_field,
 * when term is given) is the same bit for bit, and the bytes of sigma do not change.
 * Refused with BCP_E_INVALID (messages prefixed "bcp_mppi_adapt: "), in this order: h, p or io NULL; ad or ad->sigma NULL;
 * rate NaN or outside [0, 1]; per component d = 0, 1 a negative or non-finite sigma_min[d], the same of sigma_max[d],
 * sigma_min[d] > sigma_max[d]; term given with term->field NULL; then everything bcp_mppi refuses and, with term,
 * everything bcp_mppi_field refuses. */
int bcp_mppi_adapt(bcp_handle *h, const bcp_mppi_params *p, const bcp_mppi_io *io, const bcp_mppi_widths *ad,
                   const bcp_mppi_terminal *term /* NULL = no goal field */, uint32_t flags, void *stream);

/* ---- path tracking: K gain settings of a pure-pursuit tracker per env, rolled out through the forward model */
/* Parameters of bcp_track, passed to the kernel by value. */
typedef struct bcp_track_params {
    int32_t horizon, n_candidates;   /* H >= 1, K >= 1 */
    double  low[2], high[2];         /* the action box (action_space.low / high widened to float64) */
    double  max_curvature;           /* 1/m, finite, > 0: the clamp of the arc's curvature */
} bcp_track_params;

/* Host struct of device pointers, caller-owned; N = n_envs, H = horizon, K = n_candidates. */
typedef struct bcp_track_io {
    const double *gains;        /* [K][2] (speed, reach), or [N][K][2] with BCP_LOOKAHEAD_PER_ENV */
    const uint8_t *mask;        /* optional [N]; 0: every output row of the env untouched */
    double  *actions;           /* [N][K][H][2]: the commands taken; after the done step the last one repeated */
    double  *ret;               /* [N][K] */
    int32_t *steps;             /* [N][K] */
    uint8_t *reason;            /* [N][K] */
    double  *final_pose;        /* optional [N][K][3] */
    int32_t *final_target_idx;  /* optional [N][K] */
    int32_t *err;               /* optional [N][K] */
    double  *trace;             /* optional [N][K][H][6]: x, y, th, wheel_angle, target_idx, carrot index as the
                                   law READ them at step t (doubles); rows after the done step zeros */
    int32_t *best;              /* optional [N] */
    double  *best_plan;         /* optional [N][H][2] (needs best): actions[i][best[i]] -- the layout of bcp_mppi_io.mean */
    void    *best_action;       /* optional [N][2] (needs best): float64, or float32 with BCP_STEP_ACTIONS_F32 */
} bcp_track_io;

/* A feedback controller rolled out through the forward model.  For env i and setting k with gains (speed, reach), a private
 * copy of env i's state takes up to H trips exactly as bcp_lookahead with noise_z = NULL takes them (the noise-free forward
 * model, no auto-reset, stop after the first done step, ret added in step order from 0.0; ret, steps, reason, final_pose,
 * final_target_idx and err mean what they mean in bcp_lookahead_io), but the command of trip t is computed from the state
 * trip t - 1 left.  All arithmetic is float64, every product, quotient and sum rounded on its own.  With the pose
 * (x, y, th), the wheel angle wa (0 for the diff-drive), the provider's target_idx, the env's m way points pts and the
 * lane's previous carrot index c_prev (target_idx before the first trip):
 *   1. carrot: j0 = min(max(c_prev, target_idx), m - 1); the carrot is the first j >= j0 with dx * dx + dy * dy >=
 *      reach * reach, dx = pts[j].x - x, dy = pts[j].y - y, or m - 1 if there is none.  It never goes backwards.
 *   2. robot frame: lx = c * dx + s * dy, ly = -s * dx + c * dy, (c, s) = (cos th, sin th).
 *   3. curvature: d2 = lx * lx + ly * ly; kappa = d2 < 1e-12 ? 0 : 2 * ly / d2, clamped to [-max_curvature, max_curvature].
 *   4. desired body motion: v = speed, w = speed * kappa.
 *   5. command: (v, w) for the diff-drive; for the tricycle diff_drive_control_to_tricycle(v, w, wa, max_front_wheel_angle,
 *      front_wheel_from_axis) of robot_models/tricycle_model.py:191-231 -- the wheel speed and the wheel angle.
 *   6. each component clipped to [low[d], high[d]].
 * The tracker is the reference's "planner helper" put to use; the reference has no counterpart of the roll-out.
 * best: the setting with the largest key of bcp_lookahead_io.best (free before collided, then ret, lowest k on ties);
 * best_plan = actions[i][best[i]], best_action = its step 0 (rounded to float32 under the flag): both can be passed on as
 * they are, best_plan as bcp_mppi_io.mean.
 * Gains are device data and are not checked on the host: a lane whose speed or reach is not finite, whose speed < 0 or
 * whose reach <= 0 takes no trip -- steps = 0, reason = 0, ret = 0, zeros in its rows of actions and trace, final_pose /
 * final_target_idx as the env holds them -- and comes last in the key of `best`, behind every collided setting.
 * Nothing of the handle changes: no state array, step counter, noise stream or episode record.  Asynchronous on `stream`,
 * no allocation, no synchronisation; the launch arguments are the caller's pointers and *p by value, so a call can be
 * captured into a HIP graph after one ordinary call.
 * Refused with BCP_E_INVALID, nothing written:
 *   - h, p or io NULL; flag bits other than BCP_STEP_ACTIONS_F32 and BCP_LOOKAHEAD_PER_ENV;
 *   - control_delay, pose_delay or state_delay > 0;
 *   - the pure-pursuit reward provider (the law reads target_idx as "the next way point to reach", which only the
 *     continuous provider keeps);
 *   - horizon < 1 or n_candidates < 1; max_curvature not finite or not > 0; a non-finite low or high; low[d] > high[d];
 *   - gains, actions, ret, steps or reason NULL; best_plan or best_action without best;
 *   - 6 * N * K * H >= 2^62 (the element offsets are 64-bit). */
int bcp_track(bcp_handle *h, const bcp_track_params *p, const bcp_track_io *io, uint32_t flags, void *stream);

/* ---- costmap inflation ------------------------------------------------------------------------------------ */
/* inflate_costmap (utilities/costmap_inflation.py:73-92) for n_maps maps in one call: the ROS inflation layer.  Per map
 * `data` [rows][cols] with valid shape (vr, vc) = (valid_rows[m], valid_cols[m]) clamped to [0, rows] x [0, cols], or the
 * full shape when both pointers are NULL:
 *   - a cell is an obstacle exactly where data == 254 inside the valid shape (:83: 254 - data wraps, and the distance is
 *     to the nearest zero pixel; 255, 253 and every other value are free space);
 *   - d = (float32) sqrt(d2), correctly rounded, d2 the exact squared Euclidean distance in cells to the nearest obstacle
 *     cell, never clamped (:84, cv2.distanceTransform(DIST_L2, DIST_MASK_PRECISE));
 *   - _pixel_distance_to_cost (:47-70) in float64 on that d, every product and sum rounded on its own:
 *     pir = inscribed_radius / resolution, psf = cost_scaling_factor * resolution;
 *     d < pir / 1000.0 -> 254; otherwise d <= pir -> 253; otherwise (uint8) trunc(252.0 * exp(-psf * ((double)d - pir)));
 *   - a map without an obstacle cell has every d = +inf and every cost 0;
 *   - cells outside the valid shape are not read; cost 0 (and d 0) is written there.
 * inscribed_radius is path_tools.py:519-528 of the footprint (the caller computes it).  Exactly the lethal cells come out
 * as 254, so a handle bound to the inflated maps steps bit for bit like one bound to the raw maps (env.py:464-489).
 * Independent of what the handle has bound: the handle names the device and owns the scratch (allocated on first use, grown
 * only when a later call needs more, freed by bcp_destroy).  Asynchronous on `stream`, no host synchronisation.  `out`
 * may be `data` itself: every read of a map is finished before any of its cells is written.
 * Refused with BCP_E_INVALID: NULL h; n_maps < 0; NULL data or out with n_maps > 0; rows or cols outside [1, 2048] (which
 * keeps d2 < 2^24: the float holds it exactly); resolution, inscribed_radius or cost_scaling_factor not finite or not > 0;
 * only one of valid_rows / valid_cols; out overlapping data without being equal to it.  n_maps == 0 succeeds and does
 * nothing. */
int bcp_inflate_costmaps(bcp_handle *h, const uint8_t *data, int64_t n_maps, int32_t rows, int32_t cols,
                         const int32_t *valid_rows, const int32_t *valid_cols,   /* device [n_maps], both or neither */
                         double resolution, double inscribed_radius, double cost_scaling_factor,
                         uint8_t *out,          /* [n_maps][rows][cols]; may be `data` itself (in place) */
                         float *distance_out,   /* optional [n_maps][rows][cols]: d in cells, +inf / 0 as above */
                         void *stream);

/* ---- goal field: geodesic cost-to-go per map, sampled per env ---------------------------------------------- */
/* A navigation function (no reference counterpart; the other half of the ROS costmap stack that inflation starts): for
 * every free cell of a map the length of the cheapest route through free space to the nearest seed cell, as an integer
 * fixed point that does not depend on the order of evaluation. */
#define BCP_GOAL_ORTHO 12          /* cost of a step to an edge neighbour */
#define BCP_GOAL_DIAG  17          /* ... to a corner neighbour (17/12 = 1.4167) */
#define BCP_GOAL_FAR   65534       /* min(true cost, 65534): the arithmetic saturates */
#define BCP_GOAL_NONE  65535       /* blocked, outside the valid shape, or not connected to a seed */

/* bcp_goal_field: fields of n_maps maps in one launch.  Independent of what the handle has bound: the handle names the
 * device and owns the scratch of the global route (allocated on first use, grown only when a later call needs more, freed
 * by bcp_destroy).  Asynchronous on `stream`, no host synchronisation.
 * Maps: `data` is [n_maps][rows][cols]; with shared != 0 it is ONE map [rows][cols] used for all n_maps seed sets, and the
 * valid pointers must be NULL.  The valid shape (valid_rows[m], valid_cols[m]) is clamped to [0, rows] x [0, cols] as
 * bcp_inflate_costmaps clamps it; both pointers NULL = the full shape.  A cell is an obstacle exactly where data == 254
 * inside the valid shape -- the set bcp_pose_collides tests -- so inflating a map changes no field.
 * Blocked cells: a cell of the valid shape is blocked iff some obstacle cell lies at squared cell distance <= clearance_d2
 * (clearance_d2 = 0 blocks the obstacle cells alone).  Cells outside the valid shape are never entered and come out
 * BCP_GOAL_NONE.
 * Seeds: `seeds` is device int32 [n_maps][n_seeds][2] = (row, col).  A seed inside the valid shape is a source of cost 0
 * and counts as a free cell for every purpose, even where it was blocked; a seed outside the valid shape, (-1, -1)
 * included, is ignored; a map with no usable seed comes out all BCP_GOAL_NONE.
 * Graph: from a free cell to each of its eight neighbours that is free and inside the valid shape, at BCP_GOAL_ORTHO or
 * BCP_GOAL_DIAG.  A diagonal move is admissible only if BOTH edge neighbours it passes between are free: nothing slips
 * through an 8-connected wall (a cv2.line wall) at clearance 0.
 * Result: out = min(length of the cheapest admissible route to any seed, BCP_GOAL_FAR), or BCP_GOAL_NONE where there is
 * none.  Exact, and unique: the weights are positive integers and the saturating addition is monotone, so the Bellman
 * equations have one solution, whatever order the cells are relaxed in.
 * info (optional, device int32 [n_maps][2]): {cells with out != BCP_GOAL_NONE, gave_up}.
 * max_passes: the field is found by passes of a pull relaxation over the map, separated by workgroup barriers, until a
 * pass changes nothing.  Every pass finalises at least one more edge of every cheapest route, so rows * cols passes always
 * suffice: that is what 0 means.  A positive value caps the passes; when the cap ends the work, gave_up = 1 and every
 * value is BCP_GOAL_NONE or the length of SOME admissible route, i.e. an upper bound.  The loop is bounded in every case.
 * Refused with BCP_E_INVALID: NULL h; n_maps < 0; rows or cols outside [1, 2048]; n_seeds outside [1, 4096]; clearance_d2
 * outside [0, 16129] (BCP_MAX_KERNEL_HALF squared); max_passes < 0; only one of valid_rows / valid_cols; valid pointers
 * together with shared; NULL data, seeds or out with n_maps > 0.  n_maps == 0 succeeds and does nothing. */
int bcp_goal_field(bcp_handle *h, const uint8_t *data, int64_t n_maps, int32_t rows, int32_t cols, int32_t shared,
                   const int32_t *valid_rows, const int32_t *valid_cols,      /* device [n_maps], both or neither */
                   const int32_t *seeds, int32_t n_seeds,                     /* device [n_maps][n_seeds][2] = (row, col) */
                   int32_t clearance_d2, int32_t max_passes,
                   uint16_t *out,                                             /* [n_maps][rows][cols] */
                   int32_t *info,                                             /* optional [n_maps][2] */
                   void *stream);

/* bcp_goal_field_bound: fields of the handle's OWN map / path binding, seeds derived on the device (the goal of each
 * entry's path).  For private maps with private paths -- a geometry pool, or one map and one path per env -- and n_entries
 * = the handle's entry count (the pool's entries, else n_envs).  One launch, asynchronous on `stream`, no host
 * synchronisation, no upload; it allocates nothing after first use (the scratch of the global route is the handle's, one of
 * its own beside bcp_goal_field's, grown only when a re-bind needs more).  A field kernel whose LDS passes 64 KB has its
 * limit raised on first use, which is not a stream operation: one ordinary call must precede a capture.
 * Data: the raw costmaps given to bcp_set_costmaps, entry m, with the binding's valid_rows / valid_cols when present,
 * clamped as bcp_goal_field clamps them.
 * Seed, one per entry: the last way point (x, y) = paths[m][lens[m] - 1] of the path given to bcp_set_paths (lens[m] above
 * max_len counts as max_len), at
 *   (col, row) = half-to-even of ((x - ox) * inv_res, (y - oy) * inv_res)        the rule of bcp_goal_field_sample
 * on entry m's origin.  lens[m] < 1, an x or y that is not finite, or a cell outside the valid shape: no seed, the field is
 * all BCP_GOAL_NONE and info = (0, 0).  A usable seed is free, whatever stood there.
 * Result: field[m] and info[m] are byte for byte what bcp_goal_field writes for map m of the binding with that one seed.
 * Entries: entries == NULL = entries 0 .. n_list - 1.  Otherwise `entries` is device int32 [n_list] -- room for n_list ids,
 * which cannot be checked -- and the first min(max(*count, 0), n_list) of them are worked on (count == NULL = n_list); both
 * are read on the device, in stream order, and the grid never depends on *count.  An id outside [0, n_entries) is skipped:
 * nothing is read or written for it.  Listed ids are expected to be distinct.  field[m] and info[m] of every entry that is
 * not worked on are left untouched.
 * field: [n_entries][rows][cols] of the binding; info: optional [n_entries][2].  max_passes and clearance_d2: as above.
 * BCP_E_INVALID: NULL h or field; n_list < 0 or above the entry count; count without entries; clearance_d2 outside
 * [0, 16129]; max_passes < 0.  n_list == 0 succeeds and does nothing.  BCP_E_STATE: costmaps or paths not bound; a shared
 * map or a shared path (bcp_goal_field serves those); bound maps beyond 2048 x 2048.  Refusals carry the entry point's name
 * as a prefix.  Calls of the two entry points on different streams must not run beside each other (they share the scratch);
 * either may run beside a bcp_goal_field. */
int bcp_goal_field_bound(bcp_handle *h, const int32_t *entries /*device [n_list], or NULL = entries 0..n_list-1*/,
                         const int32_t *count /*device word, or NULL = n_list*/, int64_t n_list,
                         int32_t clearance_d2, int32_t max_passes,
                         uint16_t *field /*[n_entries][rows][cols] of the binding*/, int32_t *info /*optional [n_entries][2]*/,
                         void *stream);
/* bcp_refresh_goal_fields: the same for exactly the entries the pending bcp_refresh_mini_worlds re-sampled -- the list
 * bcp_plan_mini_worlds made, and the count the refresh used, both still in the handle.  A refresh is pending after
 * bcp_refresh_mini_worlds and before bcp_release_mini_worlds; otherwise BCP_E_STATE.  The call belongs on the refresh's
 * stream, or one ordered after it, and must be ordered before the bcp_release_mini_worlds that opens those entries to the
 * envs: whoever waits for the worlds then waits for the fields too.  It may be called once per field tensor while the
 * refresh is pending.  Everything else -- contract, refusals, capture -- as bcp_goal_field_bound. */
int bcp_refresh_goal_fields(bcp_handle *h, int32_t clearance_d2, int32_t max_passes, uint16_t *field, int32_t *info,
                            void *stream);

/* bcp_goal_field_cost / bcp_goal_field_cost_bound: the same fields, weighted by the map's costs -- what makes a route run
 * down the middle of free space where there is room and still squeeze through where there is not (the potential of ROS's
 * navfn, which pays for every cell's cost).  With e(c) = extra_of_cost[data[c]]:
 *   v(seed) = 0;   v(c) = min over admissible neighbours n of sat(v(n) + step(n, c) + e(c))  for every free, non-seed cell c
 * The extra belongs to the cell that is ENTERED on the way from the goal.  Everything else is bcp_goal_field's (and
 * bcp_goal_field_bound's), word for word: obstacles (== 254 only), clearance_d2, seeds (cost 0 and free whatever stood
 * there; a seed's own extra is never charged), the valid shape (bytes outside it are never looked up), the corner rule,
 * 12 / 17, the saturation at BCP_GOAL_FAR, BCP_GOAL_NONE, max_passes / gave_up (rows * cols passes still always suffice),
 * info, the two routes, the scratch they share with their plain counterparts and the stream rules that follow from it.
 * The result is exact and unique for the same reason, and an all-zero table gives the plain call's bytes.
 * A weighted field is a goal field for every consumer: e(c) is the same for every neighbour of c, so the neighbour that
 * minimises field + step is the true successor, and bcp_goal_field_sample, bcp_goal_route*, and bcp_mppi_field read it
 * unchanged.  Its values are costs to go in units of resolution / 12 "metre-equivalents", not lengths.
 * extra_of_cost: HOST uint16 [256], indexed by the map's byte, every entry <= BCP_GOAL_MAX_EXTRA.  It is copied by value
 * into the launch arguments: no upload, no allocation, no host synchronisation, and the caller may overwrite it as soon as
 * the call returns.  A call can be captured after one ordinary call with the same shapes; a captured call keeps the table
 * it was captured with.
 * Refused: everything the plain entry point refuses, in its order, with this entry point's name as prefix; then, with
 * BCP_E_INVALID, a NULL table; then an entry above BCP_GOAL_MAX_EXTRA (all 256 are checked, 254 and 255 too, although 254
 * is never looked up).  n_maps == 0 (n_list == 0) succeeds and does nothing -- behind the checks.
 * There is no refresh form: the worlds of an endless pool are not inflated, so there are no costs to weigh. */
#define BCP_GOAL_MAX_EXTRA 4095
int bcp_goal_field_cost(bcp_handle *h, const uint8_t *data, int64_t n_maps, int32_t rows, int32_t cols, int32_t shared,
                        const int32_t *valid_rows, const int32_t *valid_cols, const int32_t *seeds, int32_t n_seeds,
                        int32_t clearance_d2, int32_t max_passes, const uint16_t extra_of_cost[256] /*host*/,
                        uint16_t *out, int32_t *info, void *stream);
int bcp_goal_field_cost_bound(bcp_handle *h, const int32_t *entries, const int32_t *count, int64_t n_list,
                              int32_t clearance_d2, int32_t max_passes, const uint16_t extra_of_cost[256] /*host*/,
                              uint16_t *field, int32_t *info, void *stream);

/* bcp_goal_field_sample: what the fields say at a pose, per row -- distance to go, and the direction of the route.
 * One launch, asynchronous on `stream`, no allocation, no host synchronisation; the launch arguments depend only on the
 * pointers and numbers given, so a call can be captured into a HIP graph after one ordinary call.
 * Rows: exactly those of bcp_range_scan.  poses is [n,3] device doubles; poses == NULL requires n == n_envs and row_env ==
 * NULL and means the bound state's pose (pose_seen when pose_delay > 0).  Row i belongs to env row_env[i] (device int32
 * [n]), or i % n_envs when row_env is NULL, and reads the map entry of its env: geom_of_env under a pool, the env index
 * for private maps, 0 for a shared map.  Origins, inv_res and valid shapes are the handle's map binding; rows / cols must
 * equal that binding's.  n_fields is 1 (every row reads field 0) or the handle's entry count -- the pool's entries, or
 * n_envs without a pool -- and a row then reads the field of its env's entry (with a shared map and private paths: a field
 * per env, all read with the one map's origin).  bcp_final_goal_field_sample draws slots j < min(*count, capacity) of the bound episode record on entry geom[j]
 * (private maps without a pool: env_id[j]) and leaves the other rows untouched, in every output.
 * Per row with pose (x, y, theta) on an entry with origin (ox, oy):
 *   (col, row) = half-to-even of ((x - ox) * inv_res, (y - oy) * inv_res)        the handle's world-to-pixel rule
 *   v = field[row][col]
 * A row has no result if its cell is outside the valid shape, its pose is not finite, its row_env is out of range, or v is
 * BCP_GOAL_NONE: out3 = (max_dist, 0, 0), cell_value = 65535, carrot = (-1, -1).  Otherwise
 *   out3[0] = (float) min(((double)v * resolution) / 12.0, max_dist)
 *   cell_value = v
 * and the carrot walk takes at most carrot_cells steps from (row, col): each step moves to the admissible neighbour k that
 * minimises field[neighbour] + w_k, neighbours in the order E, NE, N, NW, W, SW, S, SE with (dcol, drow) = (1,0), (1,1),
 * (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1), ties to the lowest k.  A neighbour is admissible if it is inside the valid
 * shape, its value is not BCP_GOAL_NONE and, for a diagonal, both edge cells' values are not BCP_GOAL_NONE (on a finished
 * field that is "free").  The walk stops on a cell of value 0, or where no neighbour is admissible.
 *   carrot = (row, col) of the cell reached
 *   (out3[1], out3[2]) = the unit vector from (x, y) to that cell's centre (ox + col * resolution, oy + row * resolution),
 *   turned into the robot frame: (ux * c + uy * s, uy * c - ux * s) with the device's (c, s) = (cos theta, sin theta);
 *   float64 with every product, quotient, root and sum rounded on its own, then (float).  (0, 0) when the walk did not
 *   leave the pose's cell.
 * out3: float32 [n][3]; cell_value: optional int32 [n]; carrot: optional int32 [n][2] = (row, col).
 * BCP_E_INVALID: NULL h, field or out3; carrot_cells outside [1, 256]; max_dist NaN or not > 0 (+inf is allowed); n <= 0, or
 * n != n_envs without poses; row_env without poses; rows / cols other than the binding's; n_fields neither 1 nor the
 * handle's entry count.  BCP_E_STATE: no costmaps bound; no state bound with poses == NULL; no record bound (the final
 * variant). */
int bcp_goal_field_sample(bcp_handle *h, const uint16_t *field, int64_t n_fields, int32_t rows, int32_t cols,
                          const double *poses, int64_t n, const int32_t *row_env, int32_t carrot_cells, double max_dist,
                          float *out3 /*[n][3]*/, int32_t *cell_value /*optional [n]*/, int32_t *carrot /*optional [n][2]*/,
                          void *stream);
int bcp_final_goal_field_sample(bcp_handle *h, const uint16_t *field, int64_t n_fields, int32_t rows, int32_t cols,
                                int32_t carrot_cells, double max_dist, float *out3, int32_t *cell_value, int32_t *carrot,
                                void *stream);

/* bcp_goal_route: the route down a field from a pose to the goal, per row, written as a path that bcp_set_paths takes.
 * One launch (one lane per row), asynchronous on `stream`, no allocation, no upload, no host synchronisation; the launch
 * arguments depend only on the pointers and numbers given, so a call can be captured into a HIP graph after one ordinary
 * call.  Nothing of the handle changes.
 * Rows, fields and shapes: exactly those of bcp_goal_field_sample -- poses [n,3] or NULL (n == n_envs, row_env NULL: the
 * bound state's pose, pose_seen when pose_delay > 0); row i belongs to env row_env[i], or i % n_envs; it stands on the map
 * entry of its env and reads field 0 (n_fields == 1) or the field of its env's entry.
 * goals: device [n][3], or NULL = the last way point paths_bound[e][min(lens_bound[e], max_len_bound) - 1] of the path given
 * to bcp_set_paths for the row's entry e (a shared path: its last way point).
 * Per row with start pose s and goal pose g on an entry with origin (ox, oy):
 *   (col, row) = half-to-even of ((s.x - ox) * inv_res, (s.y - oy) * inv_res),  v = field[row][col]
 *   way point 0 = s, bit for bit
 *   while v != 0: one step of bcp_goal_field_sample's carrot walk (the admissible neighbour k that minimises field + w_k, ties
 *     to the lowest k); STUCK if no neighbour is admissible or the neighbour's value is not below v (the plane is not a goal
 *     field there) -- the walk then ends where it stands; otherwise move, and after every stride-th step that did not arrive
 *     on a cell of value 0 append the centre (ox + col * resolution, oy + row * resolution) of the cell reached.  If that way
 *     point would take the last slot, max_len - 1, it is not written and the walk ends: LONG.
 *   the last way point = g, bit for bit
 * Every trip ends the walk or lowers v, a uint16: the loop is bounded whatever the plane holds.
 * Headings: way point 0 keeps s.theta, the last one g.theta; interior way point j gets atan2(y[j+1] - y[j], x[j+1] - x[j])
 * over the written coordinates, or g.theta where both differences are zero.  float64, every operation rounded on its own.
 * paths: [n][max_len][3]; slots lens[i] .. max_len - 1 of a row are written as zeros, so the output is a function of the
 * input alone.  lens: [n], 2 <= lens[i] <= max_len for a row with a path.
 * status: [n], a bit mask --
 *   1 LONG       truncated: the first max_len - 1 way points, then the goal
 *   2 TOO_CLOSE  the reward provider's "Goal pose too close to initial pose" on the written path (find_last_reached of way
 *                point 0 is the last way point); evaluated for every row that has a path.  init is then (distance to the
 *                goal, lens[i] - 1)
 *   4 NO_ROUTE   the start or the goal pose is not finite, the start's cell is outside the valid shape, the field there is
 *                BCP_GOAL_NONE, the row's env or entry is out of range, or (goals NULL) the entry's bound path has lens < 1:
 *                lens[i] = 0, every slot zero, init = (0, 0)
 *   8 STUCK
 * init: optional [n][2] = (min_spat_dist_so_far, (double)target_idx) of this handle's reward provider on the written path
 * (ContinuousRewardProvider.generate_initial_state, reward.py:261-288; :355-371 for pure pursuit), what
 * bcp_bind_initial_state takes beside pose = way point 0.
 * BCP_E_INVALID: NULL h, field, paths, lens or status; stride outside [1, 64]; max_len outside [2, 32766]; n <= 0, or
 * n != n_envs without poses; row_env without poses; rows / cols other than the binding's; n_fields neither 1 nor the handle's
 * entry count (the bound form: not the entry count) -- tested in that order.  BCP_E_STATE: no costmaps bound; no goals and
 * no paths bound; no poses and no state bound; `paths` or `lens` being the arrays given to bcp_set_paths while the call
 * reads them.  Refusals carry the entry point's name as a prefix.
 *
 * bcp_goal_route_bound: row m is entry m of the handle's own binding -- from its bound path[m][0] to its last way point
 * (lens[m] above max_len_bound counts as max_len_bound; lens[m] < 1: NO_ROUTE), on map m and field m.  For private maps
 * with private paths (a geometry pool, or a map and a path per env), as bcp_goal_field_bound; field is
 * [n_entries][rows][cols], paths [n_entries][max_len][3], lens / status [n_entries], init optional [n_entries][2].  A shared
 * map or path: BCP_E_STATE.  No state needs to be bound. */
int bcp_goal_route(bcp_handle *h, const uint16_t *field, int64_t n_fields, int32_t rows, int32_t cols,
                   const double *poses /*[n][3] or NULL*/, int64_t n, const int32_t *row_env /*or NULL*/,
                   const double *goals /*[n][3] or NULL*/, int32_t stride, int32_t max_len,
                   double *paths /*[n][max_len][3]*/, int32_t *lens /*[n]*/, double *init /*optional [n][2]*/,
                   int32_t *status /*[n]*/, void *stream);
int bcp_goal_route_bound(bcp_handle *h, const uint16_t *field, int32_t rows, int32_t cols, int32_t stride, int32_t max_len,
                         double *paths /*[n_entries][max_len][3]*/, int32_t *lens, double *init /*optional*/, int32_t *status,
                         void *stream);
#define BCP_ROUTE_LONG      1
#define BCP_ROUTE_TOO_CLOSE 2
#define BCP_ROUTE_NO_ROUTE  4
#define BCP_ROUTE_STUCK     8

/* bcp_smooth_route: a route's cell chain pulled taut and its corners blended, per row, written as a path that bcp_set_paths
 * takes.  The stage between bcp_goal_route and a tracker: scatter -> inflate -> field -> route -> smooth -> track / plan.
 * One launch (one wave per row), asynchronous on `stream`, no allocation, no upload, no host synchronisation; *p is read
 * during the call and travels by value in the launch arguments, so a call can be captured into a HIP graph after one
 * ordinary call.  Nothing of the handle changes.
 * Rows.  rows_are_entries == 0: bcp_goal_route's rows -- row i belongs to env row_env[i], or i % n_envs, stands on the map
 * entry of its env and reads field 0 (n_fields == 1) or the field of its env's entry; no state needs to be bound.
 * rows_are_entries != 0: row m is entry m of the binding, as in bcp_goal_route_bound; n and n_fields are the entry count,
 * row_env is NULL, and the maps are private.
 * Input: the first m = min(lens_in[i], max_len_in) way points of paths_in[i].
 * Passable: a cell is passable iff it lies inside its entry's valid shape and field[row][col] != BCP_GOAL_NONE; the field
 * thereby carries the clearance, and a seed is passable.  The cell of a point (x, y) is bcp_goal_field_sample's: (col, row) =
 * half-to-even of ((x - ox) * inv_res, (y - oy) * inv_res); a point that is not finite, or whose cell lies outside the valid
 * shape, has no cell.
 * clear(a, b), exact in integers, between the CENTRES of cells a and b (a start or goal pose lies within half a cell of its
 * cell's centre, as with the first leg of bcp_goal_route): with dc = b.col - a.col, dr = b.row - a.row, ax = |dc|, ay = |dr|,
 * signs sx, sy and counters i = j = 0, while i < ax or j < ay:
 *   j == ay, or i < ax and j < ay and (2i+1) * ay < (2j+1) * ax:  col += sx, ++i
 *   i == ax, or i < ax and j < ay and (2i+1) * ay > (2j+1) * ax:  row += sy, ++j
 *   equality (the segment passes exactly through a cell corner): the edge neighbours (row, col + sx) and (row + sy, col)
 *   must both be passable -- the field's own corner rule --; then col += sx, row += sy, ++i, ++j
 * clear is true iff both ends have a cell and a, every cell stepped on (b among them) and every corner's edge neighbours
 * are passable.  The cells stepped on are exactly those whose open unit square meets the segment, and the walk visits the
 * same cells and corners from either end.  The products stay below 2^24 for maps up to 2048 x 2048.
 * Pull: anchors k_0 = 0; k_next = the largest j in (k, min(k + look, m - 1)] with clear(cell[k], cell[j]); if there is none,
 * k_next = k + 1 and the row's status gets BLOCKED; the pull ends at m - 1.  The vertices V_0 .. V_M are the kept way points
 * with their input coordinates, bit for bit.
 * Blend, at every interior vertex V with neighbours P and N (float64, every operation rounded on its own, per coordinate):
 *   lp = sqrt(dx*dx + dy*dy) with (dx, dy) = P - V, ln likewise for N;  d = blend; if (lp / 3.0 < d) d = lp / 3.0;
 *   if (ln / 3.0 < d) d = ln / 3.0.  Sizes d, d / 2.0, ... (at most `halvings` halvings) are tried in turn:
 *   A = V + ((P - V) * (d / lp))      B = V + ((N - V) * (d / ln))      q = pieces(2.0 * d, delta)
 *   Q_k = ((A * ((1-t)*(1-t))) + (V * ((2.0*t)*(1-t)))) + (B * (t*t)),  t = (double)k / (double)q,  k = 0 .. q -- every
 *   one of them by this formula, Q_0 and Q_q too
 *   the size is accepted iff clear(cell(Q_k), cell(Q_k+1)) for every k < q
 *   pieces(l, s) = max(1, (int)ceil(l / s)); a quotient that is a NaN gives 1, and one above 4096 counts as 4097: a blend
 *   size of 4097 pieces is refused untested (no row could hold it), a stretch of 4097 makes the row LONG.
 * If every size is refused, if blend == 0, or if lp or ln is 0, the corner stays sharp: V itself is the one way point there.
 * Output: way point 0 is V_0 bit for bit, heading included.  Each straight stretch runs from S = the previous corner's B
 * (its V when sharp; V_0) to E = the next corner's A (its V when sharp; V_M); with l = sqrt over E - S and q = pieces(l,
 * delta) it writes S + ((E - S) * ((double)i / (double)q)) for i = 1 .. q - 1 and then E itself.  A blended corner's Q_1 ..
 * Q_q follow its A.  The last way point is V_M bit for bit, heading included; every other heading is bcp_goal_route's:
 * atan2 to the successor over the written coordinates, or the last input way point's heading where both differences are
 * zero.  Slots behind a row's way points are written as +0.0.
 * The way points are counted before anything is written; more than max_len: LONG, lens = 0, every slot zero.
 * status: [n], bcp_goal_route's bits and one more --
 *   1 LONG       as above; init = (0, 0), info is still written
 *   2 TOO_CLOSE  as bcp_goal_route's, evaluated on the written path; init likewise
 *   4 NO_ROUTE   m < 2, a number among the row's 3 m is not finite, or the row's env or entry is out of range: lens = 0,
 *                every slot zero, init = (0, 0), info = (0, 0, 0, 0)
 *   16 BLOCKED   the pull found an anchor that sees none of its successors; the path is still written
 * init: optional [n][2], as bcp_goal_route's, on the written path (the same function).
 * info: optional [n][4] = (vertices after the pull, corners blended at full d, corners blended at a reduced d, corners
 * left sharp).
 * Refusals, tested in this order.  BCP_E_INVALID: NULL h, field, paths_in, lens_in, paths, lens, status or p; look outside
 * [1, 4096]; halvings outside [0, 8]; blend NaN, negative or infinite; delta NaN, not > 0 or infinite; max_len_in outside
 * [2, 4096]; max_len outside [2, 4096]; n <= 0; row_env together with rows_are_entries; with costmaps bound: rows / cols
 * other than the binding's; n_fields neither 1 nor the entry count (rows_are_entries: not the entry count); n not the entry
 * count with rows_are_entries.  BCP_E_STATE: no costmaps bound; a shared map with rows_are_entries; paths or lens sharing a
 * byte with paths_in or lens_in; paths or lens being the arrays given to bcp_set_paths.  Refusals carry the entry point's
 * name as a prefix, and a refused call writes nothing. */
typedef struct bcp_smooth_params {
    int32_t look;       /* way points the pull looks ahead, 1 .. 4096 */
    int32_t halvings;   /* halved blend sizes tried after the full one, 0 .. 8 */
    double blend;       /* the blend's length along each leg, metres; 0: every corner stays sharp */
    double delta;       /* spacing of the written way points, metres */
} bcp_smooth_params;
int bcp_smooth_route(bcp_handle *h, const uint16_t *field, int64_t n_fields, int32_t rows, int32_t cols,
                     const double *paths_in /*[n][max_len_in][3]*/, const int32_t *lens_in /*[n]*/, int32_t max_len_in,
                     int64_t n, const int32_t *row_env /*or NULL*/, int32_t rows_are_entries,
                     const bcp_smooth_params *p /*host*/, int32_t max_len,
                     double *paths /*[n][max_len][3]*/, int32_t *lens, double *init /*optional [n][2]*/,
                     int32_t *status, int32_t *info /*optional [n][4]*/, void *stream);
#define BCP_SMOOTH_BLOCKED 16

/* ---- speed profile: a speed per way point that slows for curvature, and the tracker that follows it ------------ */
/* bcp_path_speed: for every row of `paths` a speed per way point -- no faster than the curvature there allows, braking in
 * time for what lies ahead and accelerating no harder than allowed.  One launch (one wave per row), asynchronous on
 * `stream`; nothing is allocated or uploaded, nothing synchronises with the host, *p travels by value in the launch
 * arguments (a call can be captured into a HIP graph after one ordinary call), and nothing of the handle changes: no
 * binding is needed, the handle names the device.  The reference has no counterpart (its path_velocity measures a speed).
 * All arithmetic is float64, every product, quotient, root and sum rounded on its own.
 * Row i has m = min(lens[i], max_len) way points P_0 .. P_{m-1} (x, y of [n][max_len][3]; the heading is not read).
 *   Curvature kappa[j], the Menger curvature of a triple: a = max(j - span, 0), b = min(j + span, m - 1); kappa[j] = 0 if
 *     a == j or b == j; otherwise with A = P_j - P_a, B = P_b - P_j, C = P_b - P_a: la = sqrt(Ax*Ax + Ay*Ay), lb, lc likewise,
 *     den = (la * lb) * lc, cr = |Ax*By - Ay*Bx|, kappa = den < 1e-18 ? 0 : (2.0 * cr) / den.
 *   Limit u_lim[j], a squared speed: u = v_max * v_max; if kappa > 0: t = a_lat / kappa, if (t < u) u = t; s = w_max / kappa,
 *     s2 = s * s, if (s2 < u) u = s2; then f = v_min * v_min, if (u < f) u = f; at j == 0 u = min(u, v_start * v_start); at
 *     j == m - 1 u = min(u, v_end * v_end) (both when m == 1).
 *   Passes, with ds_j = sqrt(dx*dx + dy*dy) from P_j to P_{j+1}, cd_j = (2.0 * a_dec) * ds_j, ca_j = (2.0 * a_acc) * ds_j:
 *     backward ub[m-1] = u_lim[m-1], ub[j] = min(u_lim[j], ub[j+1] + cd_j); forward uf[0] = ub[0], uf[j] = min(ub[j],
 *     uf[j-1] + ca_{j-1}); speed[j] = sqrt(uf[j]).
 * kappa and v_limit (= sqrt(u_lim)) are these values bit for bit.  The sequential recurrence DEFINES speed; a pass is a
 * scan of f_j(u) = min(A_j, u + c_j) with the combine (A1, c1) o (A2, c2) = (min(A1, A2 + c1), c1 + c2), and the device
 * associates the sums of the c's in a tree.  Every term is non-negative, so speed is within relative 2 (m + 1) * 2^-52 of
 * the recurrence's value.
 * status[i]: 0, or BCP_SPEED_NO_PATH when lens[i] < 1 or an x or y among the row's first m is not finite; then every slot
 * of the row in speed, kappa and v_limit is +0.0.  Slots behind m are always written as +0.0.
 * Refused with BCP_E_INVALID in this order, nothing written, the message prefixed "bcp_path_speed": h, paths, lens, p,
 * speed or status NULL; max_len outside [1, 4096]; n outside [1, 2^31 - 1]; span outside [1, 64]; v_max, a_lat, w_max,
 * a_dec, a_acc (in this order) not finite or not > 0; v_min, v_start, v_end (in this order) not finite or negative;
 * v_min > v_max; speed, kappa or v_limit sharing a byte with paths. */
typedef struct bcp_speed_params {
    int32_t span;       /* way points between a triple's points, 1 .. 64 */
    double v_max;       /* m/s: the speed of a straight stretch */
    double v_min;       /* m/s: curvature alone never asks for less (the end clamps may) */
    double a_lat;       /* m/s^2: v^2 * kappa stays below it */
    double w_max;       /* rad/s: v * kappa stays below it */
    double a_dec;       /* m/s^2: braking along the path */
    double a_acc;       /* m/s^2: acceleration along the path */
    double v_start;     /* m/s: at most this at way point 0 */
    double v_end;       /* m/s: at most this at way point m - 1 */
} bcp_speed_params;
#define BCP_SPEED_NO_PATH 4
int bcp_path_speed(bcp_handle *h, const double *paths /*[n][max_len][3]*/, const int32_t *lens /*[n]*/,
                   int32_t max_len, int64_t n, const bcp_speed_params *p /*host*/,
                   double *speed /*[n][max_len]*/, double *kappa /*optional*/, double *v_limit /*optional, sqrt(u_lim)*/,
                   int32_t *status /*[n]*/, void *stream);

/* bcp_track_profile: bcp_track whose speed follows a profile.  `speed` is laid out as the paths given to bcp_set_paths:
 * [max_len] for a shared path, else [entries][max_len]; a lane reads the row of the slot its env stands on (geom_of_env[i],
 * or i).  Everything bcp_track specifies holds except step 4 of its law, with m the env's way points and `carrot` step 1's:
 *   cap = min(speed_row[min(target_idx, m - 1)], speed_row[carrot])   (a NaN if either is one)
 *   v = the gain's speed; if (cap >= 0 && cap < v) v = cap            (a NaN or negative cap leaves the gain's speed)
 *   w = v * kappa, kappa the pursuit arc's curvature of step 3.
 * A profile of speeds at or above every gain's speed gives bcp_track's outputs bit for bit.  Refused with BCP_E_INVALID:
 * prof or prof->speed NULL; prof->max_len other than the bound paths' max_len; then everything bcp_track refuses, in its
 * order (BCP_E_STATE where nothing is bound).  The messages carry "bcp_track_profile" as a prefix. */
typedef struct bcp_track_profile_io {
    const double *speed;   /* device: a speed per way point slot of the bound paths */
    int32_t max_len;       /* the slots of a row: the bound paths' max_len */
} bcp_track_profile_io;
int bcp_track_profile(bcp_handle *h, const bcp_track_params *p, const bcp_track_io *io,
                      const bcp_track_profile_io *prof, uint32_t flags, void *stream);

/* ---- box obstacles ------------------------------------------------------------------------------------ */
/* bcp_scatter_boxes: rectangular obstacles stamped into every map of a batch, reproducibly.  One launch (one 256-thread
 * workgroup per entry), asynchronous on `stream`, no allocation, no upload, no host synchronisation; the launch arguments
 * depend only on the pointers and numbers given, so a call can be captured into a HIP graph after one ordinary call.
 * Nothing of the handle changes: the maps are the caller's (bind them again if they are the ones bound).
 * Everything below is float64 + - *, rint (half to even) and integers, every operation rounded on its own; there is no
 * sin, cos, sqrt or division on the device.
 * Draws: for entry m and attempt a, Philox4x32-10 with key (seed low word, seed high word): counter (m_lo, m_hi, a, 0) gives
 * w0 .. w3 and counter (m_lo, m_hi, a, 1) gives v0;  u_i = ((double)w_i + 0.5) * 2^-32.
 * Candidate box of (m, a), with frame[m] = (ax, ay, dx, dy, nx, ny) -- anchor, along-vector, lateral vector:
 *   t = along[0] + u0 * (along[1] - along[0])        l = 2 * u1 - 1
 *   hx = half_size[0] + u2 * (half_size[1] - half_size[0])      hy likewise from u3
 *   k = ((uint64)v0 * n_yaws) >> 32      (c, s) = yaw_cs[k], the caller's table of cosines and sines
 *   cx = (ax + t * dx) + l * nx          cy = (ay + t * dy) + l * ny
 *   for the corner signs (sx, sy) = (+,+), (-,+), (-,-), (+,-):
 *     wx = (cx + (sx * hx) * c) - (sy * hy) * s       wy = (cy + (sx * hx) * s) + (sy * hy) * c
 *     px = rint((wx - ox) * inv_res)   py = rint((wy - oy) * inv_res)     (world_to_pixel; inv_res = 1.0 / resolution)
 * The four integer vertices V are the candidate; its pixel set is exactly what cv2.fillPoly(img, [V], 254) writes for that
 * contour: the four edges by the 8-connected LineIterator plus the even-odd spans in 16.16 fixed point.  Degenerate
 * contours come out as fillPoly draws them: half sizes of 0 give a single pixel, one of them 0 a line.
 * A candidate is rejected when a vertex lies outside [0, valid_cols[m]) x [0, valid_rows[m]) (NULL: cols, rows; a vertex
 * that is not a finite number lies outside), or when a cell (r, c) of its pixel set has (r - kr)^2 + (c - kc)^2 <= d2 for
 * a keep-out (kr, kc, d2) of keep[m]; d2 < 0 is an unused slot.
 * The accepted boxes of an entry are the first n_boxes attempts, in attempt order, of 0 .. max_attempts - 1 that are not
 * rejected.  Overlap with walls or with other boxes is allowed, so a verdict depends on its attempt alone.  Every cell of
 * an accepted box becomes 254; no other byte of `data` changes.
 * boxes: [n_maps][n_boxes][9] = (attempt, V0.x, V0.y, .. V3.x, V3.y) per accepted box, x a column and y a row; the slots
 * behind counts[m] are zeros.  counts: [n_maps].
 * BCP_E_INVALID, tested in this order: NULL h; NULL p; n_maps < 0; rows or cols outside [1, 2048]; resolution not a finite
 * number > 0; n_boxes outside [1, 64]; max_attempts outside [1, 4096]; n_yaws outside [1, 4096]; n_keep outside [0, 16];
 * along not finite or along[0] > along[1]; half_size not finite, negative or half_size[0] > half_size[1]; a largest box
 * that need not fit the map, (4 * half_size[1]) * inv_res + 2 > min(rows, cols); one of valid_rows / valid_cols without
 * the other; n_maps > 0 with a NULL data, origins, frame, yaw_cs, boxes or counts, or with n_keep > 0 and a NULL keep. */
typedef struct bcp_scatter_params {
    int32_t n_boxes;        /* boxes wanted per entry */
    int32_t max_attempts;   /* attempts 0 .. max_attempts - 1 are tried */
    int32_t n_yaws;         /* rows of yaw_cs */
    int32_t reserved;       /* 0 */
    uint64_t seed;
    double along[2];        /* the range of t */
    double half_size[2];    /* the range of hx and hy, in metres */
} bcp_scatter_params;
int bcp_scatter_boxes(bcp_handle *h, uint8_t *data /*[n_maps][rows][cols]*/, int64_t n_maps, int32_t rows, int32_t cols,
                      const int32_t *valid_rows /*[n_maps] or NULL*/, const int32_t *valid_cols,
                      const double *origins /*[n_maps][2]*/, double resolution, const bcp_scatter_params *p /*host*/,
                      const double *frame /*[n_maps][6]*/, const int32_t *keep /*[n_maps][n_keep][3] or NULL*/, int32_t n_keep,
                      const double *yaw_cs /*[n_yaws][2]*/, int32_t *boxes /*[n_maps][n_boxes][9]*/, int32_t *counts /*[n_maps]*/,
                      void *stream);

/* ---- measurement -------------------------------------------------------------------------------------- */
/* Which kernels a bcp_step() of this handle launches, as configured now: 0 = step_kernel alone (no distance field, or a
 * forced mode), 1 = step_fast_pair_kernel alone (every undecided pose settled in place), 2 = step_fast_pair_kernel +
 * step_pending_kernel, 3 = step_local_kernel (one launch).  Negative: BCP_E_*. */
int bcp_step_form(bcp_handle *h);
/* 1 when the last step of this handle ran step_local_kernel's shared-geometry variant (BCP_TUNE_LOCAL_SHARED), 0 when it
 * ran anything else or no step has run.  Negative: BCP_E_*. */
int bcp_step_shared_variant(bcp_handle *h);
/* 1 when the last step of this handle took its resets from the declared uniform initial state
 * (bcp_declare_uniform_initial_state: declared, shared-geometry variant, BCP_STEP_AUTO_RESET), 0 otherwise.  Negative: BCP_E_*. */
int bcp_step_uniform_reset(bcp_handle *h);
/* Runs `steps` bcp_step() launches back to back on `stream` bracketed by HIP events recorded on that stream and
 * returns the average kernel-launch duration in milliseconds (synchronises).  Used by bench.py for
 * roofline.achieved. */
int bcp_time_steps(bcp_handle *h, const bcp_step_io *io, uint32_t flags, int32_t steps, void *stream, float *avg_ms);
/* Per-kernel split of a step.  Single-launch forms (bcp_step_form 0, 1, 3 -- the default is 3): kernel_ms[0] = the average
 * step, kernel_ms[1] = 0; the envs advance by `steps` steps.  Two-launch form (2): kernel_ms[0] = average duration of
 * kernel 1 (a second loop of `steps` launches of kernel 1 alone), kernel_ms[1] = average full step minus kernel_ms[0], i.e.
 * step_pending_kernel plus the launch boundary.  Coarse: the kernel-1-only loop re-parks the same poses without settling
 * them; profiles/ (rocprofv3 kernel trace) is the reference for per-kernel durations. */
int bcp_time_step_kernels(bcp_handle *h, const bcp_step_io *io, uint32_t flags, int32_t steps, void *stream,
                          float *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* BCPLAN_H */

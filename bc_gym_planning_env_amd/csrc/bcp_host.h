// bcp_host.h -- what every host-side piece of libbcplan shares: the error record, the handle with the owners of its state,
// and the few helpers that launch kernels.  Included by bcplan.hip after the device headers and before the subsystems (bcp_field.h,
// bcp_step_host.h, bcp_plan_host.h, bcp_seams.h + bcp_seams_host.h, bcp_ego_host.h, bcp_worlds_host.h, bcp_inflate_host.h, bcp_scan_host.h,
// bcp_goal_host.h).
#pragma once

// The library exports its C entry points and nothing else: the member functions of the host-side types stay inside.
#pragma GCC visibility push(hidden)

#include "bcp_devbuf.h"
#include "bcp_field_plan.h"

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(BCP_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ... and the same for a call that has filed its own error
#define BCP_TRY(expr)                      \
    do {                                   \
        const int rc_ = (expr);            \
        if (rc_ != BCP_OK) return rc_;     \
    } while (0)

// ------------------------------------------------------------------------------------------------ cell lists
struct bcp_handle;

// Sparse egocentric views (ego_sparse_kernel, ego_pooled_sparse_kernel): per map entry the list of its non-zero cells, and
// the counts a call's route is decided from -- a counting pass over the maps on the first candidate call after the maps were
// (re)bound, one read-back of the largest count, lists sized from it; a pool refresh keeps counts and lists of the entries it
// re-samples up to date.  The state is written by the methods alone (defined below the handle).
class EgoCells {
    DevBuf<uint32_t> cells;    // [entries][cap] (empty while the maps count as dense)
    DevBuf<int32_t> counts;    // [entries] + [1] running maximum
    int64_t entries = 0;
    int32_t cap = 0;           // stride of a list, sized from the counting pass
    bool built = false;        // counts (and lists, if any) describe the current maps (rebuilt entry by entry by a pool refresh)
    bool refusal = false;      // allocation failed once: the sampling kernels serve this handle
    int32_t max = -1;          // host copy of the maximum count, -1 = not fetched since the last (re)build
    void launch(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s);
    int fetch_max(hipStream_t s);

public:
    // the maps were re-bound, or the tuning the lists were sized for changed: the next candidate call counts again
    void invalidate() { built = false; }
    // a pool refresh re-sampled the entries of `sel`: their counts and lists again, in stream order
    void recount(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s);
    // counts and (if the largest is within `limit`) lists of `n_entries` map entries, whatever state they were in
    int ensure(bcp_handle* h, int64_t n_entries, int32_t limit, hipStream_t s);
    // lists exist, describe the maps, and no entry has more cells than `limit`
    bool usable(int32_t limit) const { return cells.get() && built && max >= 0 && max <= limit; }
    // what a launch and bcp_egocentric_route read
    const uint32_t* lists() const { return cells.get(); }
    const int32_t* list_counts() const { return counts.get(); }
    int32_t stride() const { return cap; }
    int32_t largest() const { return max; }
    bool refused() const { return refusal; }
};

// ------------------------------------------------------------------------------------------------ owners
// Each group of the handle's state that has an invariant of its own has an owner: private members, and a few named methods
// that are the only writers.  The handle holds them by value, so the classes are defined here; their methods are defined
// in the subsystem that uses them (bcp_field.h, bcp_step_host.h), below the handle.

// The tuning knobs (bcp_set_tuning) with their defaults.
struct Tuning {
    int32_t defer = 1;              // settle undecided envs in a second kernel (shared map with distance field)
    int32_t exact_mode = 0;         // 0 auto, 1 cooperative only, 2 per-thread only, 3 cooperative cell by cell
    int32_t dense_threshold = 6;    // auto: more ambiguous lanes than this in a wave -> per-thread rasteriser
    int32_t adaptive = 1;           // the threshold above is only the fallback: kernel 2 re-decides every step
    int32_t cull = 1;               // BCP_TUNE_CULL: build and use the distance field
    int32_t fused = 1;              // settle parked poses inside the step launch (step_local_kernel) instead of a second launch
    int32_t local_pairs = 0;        // BCP_TUNE_LOCAL_PAIRS: workgroup size of step_local_kernel (0 = default, 1, 2, 4 x 64 envs)
    int32_t local_shared = 1;       // BCP_TUNE_LOCAL_SHARED: 1 = step_local_kernel's shared-geometry variant where the handle allows it, 0 = never
    int32_t near_shift = -1;        // BCP_NEAR_SHIFT / BCP_TUNE_NEAR_SHIFT: resolution of step_near for private maps (-1: the library's rule)
    int32_t near_dilate = 1;        // BCP_TUNE_NEAR_DILATE: 0 never, 1 pool refreshes (default), 2 every build (after the field: tests)
    int32_t edt_in_lds = 1;         // distance transform of maps that fit: the LDS-resident kernel (BCP_TUNE_EDT_LDS)
    int32_t ego_sparse = 1;         // BCP_TUNE_EGO_SPARSE: 0 never, 1 cost model, >= 2 explicit limit of cells per map
    int32_t ego_stride = 0;         // BCP_TUNE_EGO_LIST_STRIDE: 0 = lists sized from the counts, else this many cells per entry (tests)
    int32_t inflate_route = 0;      // BCP_TUNE_INFLATE_ROUTE: 0 by size, 2 always the global plane
    int32_t goal_route = 0;         // BCP_TUNE_GOAL_ROUTE: 0 by size, 2 masks and plane always in global memory

    // the defaults of a new handle: the initialisers above, and what the environment says for every handle of the process
    static Tuning from_environment()
    {
        Tuning t;
        if (const char* e = getenv("BCP_NEAR_SHIFT")) {
            const int v = atoi(e);
            if (v >= 0 && v <= 3) t.near_shift = v;
        }
        if (const char* e = getenv("BCP_LOCAL_PAIRS")) {
            const int v = atoi(e);
            if (v == 1 || v == 2 || v == 4) t.local_pairs = v;
        }
        return t;
    }
};

// Everything derived from the lethal masks for the O(1) pre-classification (bcp_field.h): the uint8 distance field with the
// scratch of its transform, its 1-bit tiles and their coarse copy, and the marks of the entries whose uint8 field a tiles-only
// rebuild has left behind.  It is bound from a FieldPlan and keeps it: tiles_y, cty and the sizes are read from there.
class DistanceField {
    DevBuf<uint8_t> edt;            // distance transform of the costmap(s) (padded)
    DevBuf<uint8_t> edt_col;        // scratch of the transform
    DevBuf<uint32_t> near;          // the field as 1-bit tiles (CullDesc::near)
    DevBuf<uint32_t> near_coarse;   // CullDesc::step_near when it is not the tiles themselves
    // The pair exists together or not at all (reserve_marks); the marks' capacity is the number of entries of both.
    DevBuf<uint8_t> stale;          // [entries] 1 = the entry's uint8 field does not describe its map (tiles do)
    DevBuf<int32_t> stale_list;     // [entries] + [1] count, scratch of ensure_fields
    bool lazy = false;              // a rebuild has left stale fields behind since the last full build
    FieldPlan plan = {};            // of the last bind
    hipError_t reserve_marks(size_t entries);
    size_t near_dilate_lds() const;
    void launch_edt(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s);
    void launch_near_tiles(EntrySelect sel, int64_t max_entries, hipStream_t s);
    void launch_near_dilate(bcp_handle* h, EntrySelect sel, int64_t max_entries, uint8_t* marks, hipStream_t s);
    void launch_near_coarse(EntrySelect sel, int64_t max_entries, hipStream_t s);

public:
    // room for what `f` plans, h->cull as `f` describes it with the buffers' addresses, no entry marked stale
    int bind(bcp_handle* h, const FieldPlan& f, hipStream_t s);
    // distance field + tiles of the selected entries; `tiles_only`: see the two predicates
    int rebuild(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s, bool tiles_only = false);
    // before anything reads the uint8 field: the transform of the entries a tiles-only rebuild has left stale
    int ensure_fields(bcp_handle* h, hipStream_t s);
    bool has_stale_fields() const { return lazy; }
    // "The steps of this handle read only the tiles", asked where the fields are (re)built.  At the bind it is asked of the
    // tuning alone -- the parking slots may not exist yet -- and only many private maps under the default BCP_TUNE_NEAR_DILATE
    // are worth it; a pool refresh asks whether the single-launch form can run at all (its slots exist), whatever the count.
    static bool bind_reads_tiles_only(const bcp_handle* h, const FieldPlan& f);
    static bool refresh_reads_tiles_only(const bcp_handle* h);
    // the reads behind bcp_get_distance_field / bcp_get_near_field (`entries` checked by the caller)
    int copy_field(bcp_handle* h, int64_t first_entry, int64_t n_entries, uint8_t* out, hipStream_t s);
    int copy_near(int64_t first_entry, int64_t n_entries, uint32_t* out, hipStream_t s);
    const FieldPlan& planned() const { return plan; }
};

// Parking and adaptation state of the two-launch step form (bcp_step_host.h): the slots of the parked envs, the two
// alternating sets of counters, the thresholds, and the form of the last step launched.
class Parking {
    DevBuf<Pending> pending;        // [kShards][cap]
    DevBuf<int32_t> pending_count;  // two alternating sets of kShards counters
    int32_t cap = 0;                // parking slots per shard
    DevBuf<int32_t> adapt;          // [2] thresholds + [2][kShards] in-place counters, alternating by step parity
    DevBuf<RecPark> rec_park;       // [kShards][cap] (two-launch form with an episode record)
    int32_t last_form = -1;         // step_form() of the last step launched, -1: none yet

public:
    // the first bind of a map with a distance field: slots for `n_envs`, armed (a later bind changes nothing)
    int bind(int64_t n_envs, int32_t threshold, hipStream_t s);
    // both counter sets zero, both thresholds `threshold`: in stream order, nothing on the host to wait for
    int arm(int32_t threshold, hipStream_t s);
    // a step of `form` is about to be launched: parking that resumes after another form is re-armed first
    int step_takes_form(int form, int32_t threshold, hipStream_t s);
    int record_slots(bool defer, RecPark** out);   // the record's parking slots of the two-launch form (nullptr without deferral)
    Pending* slots() const { return pending.get(); }
    int32_t* counters() const { return pending_count.get(); }
    int32_t* thresholds() const { return adapt.get(); }
    int32_t slots_per_shard() const { return cap; }
};

// Watchdog of the step kernel's bounded waits: every kWatchdogSteps calls bcp_step copies tick[4] to pinned host memory
// behind the step (no synchronisation) and a later call looks at what arrived (bcp_step_host.h).
class WaitWatchdog {
    PinnedWord host;
    OwnedEvent event;
    bool in_flight = false;
    uint64_t seen = 0;
    uint32_t steps_since_probe = 0;

public:
    int after_step(bcp_handle* h, hipStream_t s);
};

// ------------------------------------------------------------------------------------------------ handle
// Parameters, what the caller owns (plain pointers), the descriptors the kernels get, and the owners of everything the library
// allocates: a DevBuf grows when a re-bind needs more room, and the handle's destructor gives everything back.
struct bcp_handle {
    // ---- parameters
    bcp_params params = {};
    DevParams dev = {};
    int64_t n = 0;
    int device = 0;
    int64_t env_id_base = 0;
    uint64_t seed = 0;
    double resolution = 0;
    Tuning tune;
    bool have_map = false, have_path = false, have_state = false, have_init = false;
    // ---- the caller's arrays
    const uint8_t* map_data = nullptr;    // raw costmap(s) as given to bcp_set_costmaps (egocentric views read them)
    const int32_t* map_valid_rows = nullptr;
    const int32_t* map_valid_cols = nullptr;
    int32_t n_geoms = 0;                  // > 0: geometry pool of that many entries
    int32_t* geom_of_env = nullptr;       // device int32 [n]
    const int32_t* next_geom = nullptr;   // device int32 [n_geoms] or nullptr
    const double* path_src = nullptr;     // way points [.,max_len,3] as given to bcp_set_paths
    bool have_rec = false;                // episode record (bcp_bind_episode_record): the caller's arrays ...
    EpisodeRec rec = {};
    DevBuf<uint32_t> rec_work;            // ... and the library's [3] words: slots taken in the running step, ticket of the parties that
                                          // publish the count, steps that overflowed the capacity since bcp_episode_record_overflows last looked
    // ---- descriptors (kernel arguments) and the derived data they point to
    MapDesc map = {};
    DevBuf<uint32_t> bitmap;
    DevBuf<uint32_t> map_tiles;     // the bitmap once more in tiles of 32 x 32 cells (MapDesc::tiles)
    int32_t wide = 0;               // kernel image may exceed 96 px: 8-word row masks in the cooperative path
    CullDesc cull = {};             // written by DistanceField::bind; BCP_TUNE_CULL switches `on`
    DistanceField field;
    PathDesc path = {};
    DevBuf<double> path5;
    DevBuf<uint32_t> path_pre;      // [paths][max_len][2] {x, y as uint16 steps | cos, sin as int16}: the prefilter record of private paths
    DevBuf<double> path_bbox;
    DevBuf<int16_t> path_index;
    DevState st = {}, init = {};
    // ---- the step
    DevBuf<uint64_t> tick;          // step counter (two views), noise seed, ticket -- see StepArgs::tick; [4]: waits that gave up
    StepStatic host_static = {};    // host image of the device-resident step parameters
    StepHot host_hot = {};          // ... and of the copy of them that travels with a step's arguments (upload_step_static)
    DevBuf<StepStatic> dev_static;
    bool static_dirty = true;       // host_static must be rebuilt and uploaded before the next step
    Parking parking;
    DevBuf<uint64_t> parked_slots;  // a word per workgroup of step_local_kernel, its parked poses so far (bcp_parked_poses)
    WaitWatchdog watchdog;
    int32_t last_local_shared = 0;  // the last step ran step_local_kernel's shared-geometry variant (bcp_step_shared_variant)
    // ---- a declared uniform initial state (bcp_declare_uniform_initial_state): entry 0 of the arrays as they were at the call
    bool init_declared = false;
    InitUniform init_snapshot = {};
    int32_t last_uniform_reset = 0; // the last step took its resets from the snapshot (bcp_step_uniform_reset)
    // ---- egocentric views
    DevBuf<int32_t> ego_bins;       // [2][capacity / 2] image counts / first slots per map entry
    DevBuf<int32_t> ego_order;      // [2][capacity / 2] rank within the bin / images grouped by map entry
    EgoCells ego_cells;             // sparse views: the lists of non-zero cells
    int32_t ego_route[4] = {};      // what the last bcp_egocentric_costmaps call ran: kernel, largest count, list stride, limit
    // ---- world ring (bcp_plan / refresh / release_mini_worlds) and the side stream
    DevBuf<unsigned char> ring;     // scratch of bcp_refresh_mini_worlds (bytes: one int64 and three int32 arrays)
    int32_t ring_episodes = 0;      // of the last bcp_plan_mini_worlds
    bool ring_planned = false, ring_refreshed = false;   // plan -> refresh -> release, in that order
    OwnedEvent refresh_done;        // end of the last bcp_refresh_mini_worlds (whoever derives data from the maps on
    bool refresh_recorded = false;  // another stream waits for it first)
    OwnedStream side_stream;        // the CU-masked stream of bcp_side_stream (empty: not created)
    int32_t side_share = 0;         // ... and the share of the CUs it was created with
    // ---- bcp_inflate_costmaps: the 16-bit plane of maps beyond LDS, a slice per workgroup; grown on demand, never shrunk
    DevBuf<uint16_t> inflate_scratch;
    // ---- bcp_goal_field: the two bit masks of maps beyond LDS, a slice per workgroup; grown on demand, never shrunk
    DevBuf<uint32_t> goal_scratch;
    // ---- bcp_goal_field_bound / bcp_refresh_goal_fields: the same, of their own -- a refresh on a side stream may run
    // beside a bcp_goal_field on the steps' stream, and the two must not share mask slices
    DevBuf<uint32_t> goal_bound_scratch;
};

// number of entries of a non-shared map / path / initial-state array
static int64_t n_slots(const bcp_handle* h) { return h->n_geoms > 0 ? h->n_geoms : h->n; }

// ------------------------------------------------------------------------------------------------ cell lists, continued
inline void EgoCells::launch(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    const MapDesc& m = h->map;
    hipLaunchKernelGGL(ego_cells_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(max_entries, 8192))), dim3(256), 0, s,
                       h->map_data, sel, m.rows, m.cols, h->map_valid_rows, h->map_valid_cols, cap, cells.get(), counts.get(),
                       counts.get() + entries);
    max = -1;
}

inline int EgoCells::fetch_max(hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(&max, counts.get() + entries, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BCP_OK;
}

inline void EgoCells::recount(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    if (!built) return;   // (nothing to keep up to date: the next candidate call counts everything)
    if (counts.get()) launch(h, sel, max_entries, s);
    else invalidate();
}

inline int EgoCells::ensure(bcp_handle* h, int64_t n_entries, int32_t limit, hipStream_t s)
{
    if (h->refresh_recorded && (!built || max < 0))
        HIP_TRY(hipStreamWaitEvent(s, h->refresh_done.get(), 0));   // (a refresh on another stream may still be writing the maps / counts)
    if (entries != n_entries || !counts.get()) {
        (void)cells.reset();
        entries = 0;
        cap = 0;
        built = false;
        if (counts.reserve((size_t)n_entries + 1) != hipSuccess) {
            (void)hipGetLastError();
            refusal = true;   // (no room: not an error, the sampling kernels take over)
        } else {
            entries = n_entries;
        }
    }
    if (counts.get() && !built) {
        // counting pass -> largest count -> stride of the lists -> lists
        const EntrySelect all = {nullptr, nullptr, entries};
        (void)cells.reset();   // (the counting pass is the one without lists; they are sized from its result)
        cap = 0;
        HIP_TRY(hipMemsetAsync(counts.get() + entries, 0, sizeof(int32_t), s));
        launch(h, all, entries, s);
        BCP_TRY(fetch_max(s));
        built = true;
        if (max <= limit) {
            // pool entries change under a refresh: leave room for a world with more cells than today's largest
            int64_t stride = std::max<int64_t>(kEgoCellCapMin, ((int64_t)max + 63) & ~(int64_t)63);
            const int64_t budget = (int64_t)1 << 30;   // bytes of lists per handle
            if (entries * stride * 4 > budget) stride = ((int64_t)max + 63) & ~(int64_t)63;
            if (h->tune.ego_stride > 0) stride = h->tune.ego_stride;   // (tests: entries with more cells than this are drawn pixel by pixel)
            if (stride > 0 && entries * stride * 4 <= budget && cells.reserve((size_t)entries * stride) == hipSuccess) {
                cap = (int32_t)stride;
                const int32_t counted = max;
                launch(h, all, entries, s);   // (the same counts again, and the lists)
                max = counted;
            } else {
                (void)hipGetLastError();
                if (stride > 0) refusal = true;
            }
        }
    }
    if (counts.get() && built && max < 0) BCP_TRY(fetch_max(s));   // (a refresh re-counted some entries)
    return BCP_OK;
}

// grid of a grid-stride kernel; a selection's size is only known on the device, so those launches get a chip-filling
// grid that does not grow with the upper bound
constexpr size_t kMaxDynamicLds = 150 * 1024;   // of the 160 KB a gfx950 workgroup can have

static unsigned stride_grid(int64_t work_items, int threads, bool selection = false)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work_items + threads - 1) / threads, selection ? 4096 : 65536));
}

// Lets `fn` be launched with `bytes` of dynamic LDS on `device`.  The attribute belongs to the FUNCTION on a device, not to
// a handle, so it is only ever raised: the largest size any handle of this process has asked for stays set (two live handles
// with different staging sizes would otherwise lower it under each other).
static int raise_dynamic_lds(const void* fn, int device, size_t bytes)
{
    static std::mutex mutex;
    static std::map<std::pair<const void*, int>, size_t> raised;   // (function, device) -> the attribute as it stands
    std::lock_guard<std::mutex> lock(mutex);
    size_t& cur = raised[std::make_pair(fn, device)];
    if (bytes > cur) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        cur = bytes;
    }
    return BCP_OK;
}

// The one way to launch a kernel that exists in several variants: the caller picks the variant's function once, as a
// pointer, and everything that follows -- the LDS attribute, an occupancy query, the launch -- goes through that pointer.
// A workgroup gets 64 KiB of dynamic LDS without asking; more needs the function's attribute raised first.
static int variant_lds(const bcp_handle* h, const void* fn, size_t lds)
{
    return lds > 64 * 1024 ? raise_dynamic_lds(fn, h->device, lds) : BCP_OK;
}

// `args` are the kernel's arguments, each of exactly the parameter's type.  The caller has seen to variant_lds.
template <typename... Args>
static int launch_fn(const void* fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args)
{
    void* kargs[] = {(void*)&args...};
    HIP_TRY(hipLaunchKernel(fn, grid, block, kargs, lds, s));
    return BCP_OK;
}

template <typename... Args>
static int launch_variant(const bcp_handle* h, const void* fn, dim3 grid, dim3 block, size_t lds, hipStream_t s,
                          const Args&... args)
{
    const int rc = variant_lds(h, fn, lds);
    return rc != BCP_OK ? rc : launch_fn(fn, grid, block, lds, s, args...);
}

#pragma GCC visibility pop

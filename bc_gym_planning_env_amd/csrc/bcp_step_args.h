// bcp_step_args.h -- what the host hands the step kernels: the device-resident parameter block (StepStatic), the launch
// arguments (StepArgs, StepHot) and the finishing pass's view of them, the internal flag bits, the episode record's
// helpers and the device-side step counter (resolve_step, advance_step_by_ticket).
#pragma once

#include "bcp_device.h"
#include "bcp_raster.h"
#include "bcp_coop.h"
#include "bcp_init_uniform.h"
#include "bcp_step_layout.h"

using namespace bcp;

struct DevState {
    double *x, *y, *angle, *v, *w, *steer, *wheel, *min_dist;
    int32_t *target_idx, *cur_iter;
    uint8_t* collided;
    double *pose_seen, *state_seen;         // [3][n] / [7][n], delays > 0 only
    double *control_q, *pose_q, *state_q;   // [delay][width][n]
};

struct MapDesc {
    const uint32_t* bits;  // lethal bitmap, [rows][wpr] shared or [N][rows][wpr]
    const uint32_t* tiles; // the same bits in tiles of 32 x 32 cells, [tile_words] per entry (pack_bitmap_kernel, CoopCollisionSink)
    int32_t rows, cols, wpr;
    int32_t shared;
    int32_t in_lds;        // shared bitmap small enough to be staged in LDS
    int64_t env_stride;    // words per env (0 when shared)
    const double* origins; // device [N,2] when per-env, else NULL
    double ox, oy, inv_res;
};

struct PathDesc {
    const double* pts;   // [len][5] = x, y, theta, cos(theta), sin(theta); shared or [N][max_len][5]
    const uint32_t* pre; // private paths: [N][max_len][2] = x, y (uint16 each, in steps from the box corner) and cos, sin of theta
                         // (int16, / 32767) -- the 8-byte prefilter record of
                         // the way-point scan (16 bytes: four way points per 64-byte sector); nullptr for a shared path
    const double* bbox;  // [kBoxDoubles] per path, one 128-byte record: box of the way points and bucket grid as eight f32,
                         // the costmap origin, the path length and, for private paths, the bucket tables -- see kBoxDoubles
    const int16_t* index; // shared path: [2 axes][kPathBuckets][2] = first / last way point index that can be reached from a bucket
    const int32_t* lens;
    int32_t max_len, shared;
};

struct Pending;

// The episode record (bcp_bind_episode_record): where the step kernels leave each env whose episode ends.  It lies at the END
// of StepStatic and is NOT part of what step_local_kernel stages in LDS (kStaticChunks): the kernels read it through the
// global block a.S, behind the internal flag kStepRecord, and only where an env is finished.
// Two-launch step with a record: what kernel 2's redo of a parked env needs from kernel 1, one per parking slot
struct RecPark {
    double ret_before;      // the env's return before this step
    int32_t slot, pad;      // the record slot kernel 1 gave the env (-1: none)
};

// How finalize_env_from finishes an env: first time (on = false), or kernel 2 redoing an env kernel 1 finished optimistically
struct RecRedo {
    double ret_before;
    int32_t slot;
    bool on;
};

struct EpisodeRec {
    uint8_t* reason;        // [N] BCP_DONE_* bits of the last step
    double* ret;            // [N] running return of the episode, or nullptr
    int32_t* count;         // [1] envs that ended in the last step (published by the last party of the step)
    int32_t* env_id;        // [capacity]
    int32_t* geom;          // [capacity] pool entry the episode ran on (-1 without a pool)
    double* final_ret;      // [capacity] (with ret)
    DevState fin;           // [capacity] final states: x .. collided, pose_seen / state_seen with delays, queues nullptr
    int64_t capacity;
    uint32_t* work;         // library-owned [3]: slots taken so far in this step, ticket of the publishing parties, steps
                            // whose count exceeded the capacity (bcp_episode_record_overflows)
    RecPark* park;          // library-owned [kShards][pending_cap] (two-launch form), indexed like StepStatic::pending
};

// Everything a step needs that only changes when the caller re-binds something.  It lives in DEVICE memory (uploaded
// when dirty) and the kernels get a pointer: kernel arguments sit in host memory on this platform, and a kernel that
// takes kilobytes of arguments by value pays a PCIe-latency scalar load every time it touches a new field.
struct StepStatic {
    DevParams P;
    MapDesc map;
    CullDesc cull;
    PathDesc path;
    DevState st, init;
    int64_t n;
    int64_t env_id_base;
    int32_t exact_mode, dense_threshold, wide;
    int32_t pending_cap;       // slots per shard
    int32_t lds_path_doubles;  // > 0: the shared path (max_len * 5 doubles) is staged in LDS by the fast step kernel
    struct Pending* pending;   // [kShards][pending_cap] parking slots for undecided envs (nullptr: no second kernel)
    // geometry pool (bcp_set_geometry_pool): env i uses entry geom_of_env[i] of the non-shared map / path / initial
    // state arrays; a reset moves it to next_geom[entry].  nullptr: env i uses entry i.
    int32_t* geom_of_env;
    const int32_t* next_geom;
    // A declared uniform initial state (bcp_declare_uniform_initial_state): the one entry every env is reset to.  Directly in
    // front of the record, so it is the last of what step_local_kernel stages in LDS; read there behind kStepInitUniform only.
    alignas(16) InitUniform init_uniform;
    EpisodeRec rec;            // (last: not staged in LDS, see EpisodeRec)
};
static_assert(offsetof(StepStatic, init_uniform) % 16 == 0 && offsetof(StepStatic, rec) == offsetof(StepStatic, init_uniform) + sizeof(InitUniform),
              "the uniform initial state is whole 16-byte pieces of *S, the last ones in front of the record");

// What a wave needs before anything else -- where its state, its path and (kernel 2) its parked poses are -- travels
// with the kernel arguments: the first vector loads then depend on the argument fetch alone and overlap the (cold, the
// kernel boundary emptied the L2) scalar fetch of *S instead of queueing behind it.  A copy of the corresponding *S fields.
struct StepHot {
    DevState st;               // (x .. collided first: what every configuration loads; the five delay-queue arrays last)
    // ---- the rest of what step_local_kernel's prologue uses, contiguous (fetched in one go: fetch / pin_words)
    int64_t n;
    int64_t env_id_base;
    int32_t* geom_of_env;
    const double* path_pts;
    const uint32_t* path_pre;
    const double* path_bbox;
    const int16_t* path_index;
    const uint32_t* map_bits;
    const double* qverts;      // = &S->P.qverts[0][0]
    const double* map_origins; // per-entry map origins [.,2] or nullptr
    int32_t model, lds_path_doubles, path_shared, path_max_len;
    int32_t map_rows, map_cols, map_wpr, map_shared;
    int32_t noise_on, n_verts, control_delay, pose_delay, state_delay;
    int32_t dynamic_model, model_front_column_pid;
    int32_t noise_slot0;       // alpha1 > 0 or alpha2 > 0: the noise model can consume slot 0 (differential_drive.py:62)
    int32_t pending_cap;
    // (copies of StepArgs::flags / actions / noise_z / tick: with them here everything step_local_kernel's prologue fetches
    //  lies in the first five 64-byte lines of the launch arguments instead of being spread over seven -- a cold argument
    //  fetch costs ~160 cycles per further line, at the very start of every wave)
    uint32_t io_flags;
    const void* io_actions;
    const double* io_noise_z;
    uint64_t* io_tick;
    // ---- used later in a step
    const uint32_t* near;
    int64_t map_env_stride;
    struct Pending* pending;
};
constexpr int kHotStateWords = 11 * 2;                                   // x .. collided
constexpr int kHotPrologueWords = (10 * 8 + 18 * 4 + 3 * 8) / 4;        // n .. io_tick
static_assert(offsetof(DevState, collided) == 10 * 8 && offsetof(StepHot, st) == 0, "x .. collided lead DevState");
static_assert(offsetof(StepHot, io_tick) + 8 - offsetof(StepHot, n) == kHotPrologueWords * 4, "the prologue block of StepHot");

constexpr int kShards = 64;  // a wave parks into shard (block index % kShards)

// Per-launch kernel arguments (small).
struct StepArgs {
    const StepStatic* S;
    StepHot hot;
    const void* actions;
    const double* noise_z;
    double* noise_z_out;
    double* reward;
    uint8_t* done;
    uint8_t* collided_now;
    int32_t* err;
    int32_t* pending_count;    // [kShards] this step's counters of parked envs (one per shard: no hot atomic)
    int32_t* pending_next;     // [kShards] the next step's counters (the two sets alternate); kernel 1 zeroes them
    // adaptive split between "settle in place" and "park for kernel 2" (nullptr: S->dense_threshold is used as is):
    // kernel 2 of step t counts the undecided poses of step t and picks the threshold of step t + 1
    const int32_t* threshold_now;
    int32_t* threshold_next;
    int32_t* inplace_count;    // [kShards] undecided poses settled inside kernel 1 this step (the parked ones are in
                               // pending_count); sharded like the parking counters: no hot atomic
    int32_t* inplace_next;     // [kShards] next step's counters; kernel 1 zeroes them
    uint64_t seed, step_counter;
    uint32_t flags;
    // The step counter (parity of the alternating counter sets above, counter of the noise stream) and the noise seed
    // live on the DEVICE, so that the launch arguments of a step never change and a captured hipGraph of steps can be
    // replayed: the kernels fill in the eight fields above themselves (resolve_step).  tick[0] = counter as kernel 1 (or
    // the single-kernel step) reads it, tick[1] = as kernel 2 reads it, tick[2] = seed, tick[3] = ticket of the
    // single-kernel step.  Two-kernel step: kernel 1 copies tick[0] to tick[1], kernel 2 stores tick[1] + 1 to tick[0]
    // -- each word is only written while no kernel that reads it is running.  Single-kernel step: the last workgroup
    // to finish (ticket) advances tick[0].  tick[4] counts the bounded waits of step_local_kernel that gave up (bcp_expired_waits).
    // step_local_kernel draws its ticket from tick[8], a cache line of its own (see there) -- tick has 16 words.
    uint64_t* tick;
    int32_t* pending_base;     // [2][kShards] or nullptr
    int32_t* adapt_base;       // [2] thresholds + [2][kShards] in-place counters, or nullptr (no adaptation)
    uint64_t* parked_slots;    // [workgroups of step_local_kernel] parked poses so far, a word per workgroup (bcp_parked_poses)
    int32_t rollout_steps;     // step_local_kernel<.., ROLL = true> (bcp_rollout): steps per launch; actions / noise_z / outputs are [steps][N]..
    const uint32_t* map_tiles; // MapDesc::tiles: what step_local_kernel's exact tests read when the map is not staged in LDS
};
// The per-launch words finalize_env_from uses, as they lie in StepArgs (noise_z_out .. err), and the flags.  The shared-
// geometry variant of step_local_kernel keeps this launch's copy in LDS, behind its copy of *S (kFinishSlotBytes).
struct FinishWords {
    double* noise_z_out;
    double* reward;
    uint8_t* done;
    uint8_t* collided_now;
    int32_t* err;
    uint32_t flags, pad;
};
constexpr int kFinishPtrWords = 5 * 2;
constexpr int kFinishSlotBytes = 64;
static_assert(offsetof(StepArgs, err) + 8 - offsetof(StepArgs, noise_z_out) == kFinishPtrWords * 4 &&
              offsetof(FinishWords, flags) == kFinishPtrWords * 4 && sizeof(FinishWords) <= kFinishSlotBytes, "noise_z_out .. err are adjacent");

// What finalize_env_from takes from a launch, under StepArgs' member names, as VALUES: the movers of step_local_kernel's
// shared-geometry variant read them from LDS in one batch (FinishWords and the state arrays of the LDS copy of *S), into vector
// registers -- every store of the finishing pass has a per-lane 64-bit address anyway -- instead of fetching each from the
// launch arguments where it is first used, one scalar round trip after the other at the very end of the workgroup.
struct FinishArgs {
    const __attribute__((address_space(4))) StepArgs* launch;   // (for the global block *S: the episode record)
    struct {
        DevState st;   // (x .. collided)
    } hot;
    double* noise_z_out;
    double* reward;
    uint8_t* done;
    uint8_t* collided_now;
    int32_t* err;
    uint32_t flags;    // (wave-uniform, one scalar register)
};

// the parameter block in global memory (finalize_env_from: the episode record, which no LDS copy holds)
template <typename A>
__device__ __forceinline__ const StepStatic* global_block(const A& a) { return a.S; }
__device__ __forceinline__ const StepStatic* global_block(const FinishArgs& a) { return a.launch->S; }

constexpr int kTickWords = 16;
constexpr int kTickLocalTicket = 8;   // step_local_kernel's ticket: not on the line the prologues read the counter and the seed from

constexpr uint32_t kStepAdvances = 1u << 24;   // internal flag: this launch is the last kernel of its step
constexpr uint32_t kStepRecord = 1u << 25;     // internal flag: an episode record is bound (StepStatic::rec)
constexpr uint32_t kStepInitUniform = 1u << 26;   // internal flag: resets take StepStatic::init_uniform from the LDS copy of *S
                                                  // (set by launch_step for step_local_kernel's shared-geometry variant alone)

// The step's count of ended envs, by the last party of the step (every slot has been taken): published, counter re-armed
__device__ __forceinline__ void record_store_count(const EpisodeRec& R)
{
    const uint32_t taken = atomicExch(R.work, 0u);
    *R.count = (int32_t)taken;
    if ((int64_t)taken > R.capacity) atomicAdd(R.work + 2, 1u);
}

// The last of `parties` to get here (each after its own slots were taken) publishes the count.  One lane per party.
__device__ __forceinline__ void record_publish(const StepStatic* S, unsigned int parties)
{
    uint32_t* work = S->rec.work;
    __threadfence();
    if (atomicAdd(work + 1, 1u) == parties - 1) {
        work[1] = 0u;
        record_store_count(S->rec);
    }
}

// which: 0 = kernel 1 / single-kernel step, 1 = kernel 2
__device__ __forceinline__ StepArgs resolve_step(const StepArgs& in, int which)
{
    StepArgs a = in;
    const uint64_t step = in.tick[which];
    a.step_counter = step;
    a.seed = in.tick[2];
    const int p = (int)(step & 1u);
    a.pending_count = in.pending_base ? in.pending_base + p * kShards : nullptr;
    a.pending_next = in.pending_base ? in.pending_base + (p ^ 1) * kShards : nullptr;
    a.threshold_now = in.adapt_base ? in.adapt_base + p : nullptr;
    a.threshold_next = in.adapt_base ? in.adapt_base + (p ^ 1) : nullptr;
    a.inplace_count = in.adapt_base ? in.adapt_base + 2 + p * kShards : nullptr;
    a.inplace_next = in.adapt_base ? in.adapt_base + 2 + (p ^ 1) * kShards : nullptr;
    return a;
}

// end of a kernel that is the last one of its step (flag kStepAdvances): the last workgroup to get here moves the
// counter on.  Every workgroup has read tick[0] long before it takes its ticket.
__device__ __forceinline__ void advance_step_by_ticket(const StepArgs& a)
{
    if (!(a.flags & kStepAdvances) || threadIdx.x != 0) return;
    unsigned int* ticket = reinterpret_cast<unsigned int*>(a.tick + 3);
    __threadfence();
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
        *ticket = 0u;
        a.tick[0] = a.step_counter + 1;
        // (every workgroup finished its envs -- in the wave that drew its ticket -- before it drew)
        if (a.flags & kStepRecord) record_store_count(a.S->rec);
    }
}

// bcp_step_layout.h -- the limits of the step kernels' LDS staging and the layout of their dynamic LDS, once, for the launcher
// that sizes an allocation (bcp_step_host.h), the kernel that carves it up, and the tests.  Plain C++ with no HIP in it:
// tests/c_abi/step_layout_main.cpp includes this header alone and prints what the compiler saw.
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef BCP_HD_INLINE   // (bcp_philox.h has the same one)
#if defined(__HIPCC__)
#define BCP_HD_INLINE __host__ __device__ __forceinline__
#else
#define BCP_HD_INLINE inline
#endif
#endif

namespace bcp {

constexpr int kBlock = 64;  // one wavefront per workgroup

// ---- limits ----------------------------------------------------------------------------------------------------------
constexpr int kLocalPairsMax = 4;
constexpr int kScanItems = 1024;       // candidates of a pair's 64 envs that the flat scan list holds (bytes of LDS)
constexpr int kHandDoubles = 8;   // per pair and env: pose [3], score / noise [3], cos / sin of the old heading [2]
constexpr int kLocalMapWords = 4096;   // a shared lethal bitmap of up to 16 KB is staged in LDS for the exact tests
constexpr int kWayPointDoubles = 5;    // x, y, theta, cos(theta), sin(theta)
constexpr int kPathLdsBytes = 24 * 1024;   // a shared path of at most this many bytes is staged in LDS
constexpr int kPairStageRegs = 4;      // step_fast_pair_kernel: path doubles each of its 2 * kBlock threads stages from registers ...
constexpr int kPairStageDoubles = kPairStageRegs * 2 * kBlock;   // ... 512 in all; a loop takes over from there
constexpr int kPendingWaves = 4;  // wave = 2 * (row-chunk slot) + (edge slot)
constexpr int kCtlWords = 16;
static_assert((2 * kBlock + kScanItems / 4) * 4 <= 3 * kBlock * 8, "the flat scan list lies in the score / noise part of a hand-off block");

// What the layouts take from the device headers, restated: bcp_step.h static_asserts every one against the real thing.
struct StepLdsConsts {
    int parked_pose_bytes;   // sizeof(ParkedPose)
    int sparse_lds_words;    // kSparseLdsWords
    int static_chunks;       // kStaticChunks: 16-byte pieces of StepStatic in front of its episode record
    int finish_slot_bytes;   // kFinishSlotBytes
};
constexpr StepLdsConsts kStepLds = {64, 257, 97, 64};

// the threads of step_local_kernel that stage path and bitmap (everybody but the movers): 768 / 384 / 192
constexpr int local_stagers(int pairs) { return (4 * pairs - pairs) * kBlock; }
// ... and the bitmap words each of them holds at most: 6 / 11 / 22
constexpr int local_map_per_stager(int pairs) { return (kLocalMapWords + local_stagers(pairs) - 1) / local_stagers(pairs); }

// words of a shared lethal bitmap that step_local_kernel stages in LDS for its exact tests (0: they read global memory)
BCP_HD_INLINE int staged_map_words(bool shared, int rows, int wpr)
{
    return (shared & (rows * wpr <= kLocalMapWords)) ? rows * wpr : 0;
}

// ---- step_local_kernel -----------------------------------------------------------------------------------------------
// the 16 control words, zeroed by the last wave in front of barrier 0
enum LocalCtl {
    kCtlParked = 0,         // parked poses of the workgroup
    kCtlTicket = 1,         // tickets drawn for them
    kCtlMoversParked = 2,   // movers that have parked theirs
    kCtlMoversDone = 3,     // movers that have finished (the last one draws the step's ticket)
    kCtlScansDone = 4,      // [pairs] scan results in hand
    kCtlListReady = 8       // [pairs] the flat scan list is built: candidates + 1
};

// [footprint][path][hand-off blocks: pairs][box: 8 doubles][bucket index: 128 words][control words: 16] | [parked poses]
// [cell lists: one per wave][staged map] | [*S][finish slot][delay stash, PLAIN = false].  The front part, all doubles or
// pairs of words, is counted in doubles from the start (the footprint is at 0); the rest in bytes.  `|`: aligned to 16 bytes.
// In two parts, so that the kernel can form its pointers in the order it always did, the map's size last; local_lds_plan is both.
struct LocalLds {
    int path, hand, box, index, ctl;                                      // (doubles)
    uint32_t rec, cells, map, stat, finish, stash, bytes;                 // (bytes)
};

// the regions in front of the staged map, the only one whose size a launch does not know from its template arguments ...
BCP_HD_INLINE LocalLds local_lds_front(int n_verts, int lds_path_doubles, int pairs)
{
    LocalLds o = {};
    o.path = 2 * n_verts;
    o.hand = o.path + lds_path_doubles;
    o.box = o.hand + pairs * kHandDoubles * kBlock;
    o.index = o.box + 8;
    o.ctl = o.index + kBlock;   // (128 words)
    o.rec = (uint32_t)((((size_t)(o.path + lds_path_doubles + pairs * kHandDoubles * kBlock + 8) * sizeof(double) +
                         2 * kBlock * sizeof(uint32_t) + kCtlWords * sizeof(int32_t)) + 15) & ~(size_t)15);
    o.cells = o.rec + (uint32_t)(pairs * kBlock * kStepLds.parked_pose_bytes);
    o.map = o.cells + (uint32_t)(4 * pairs * kStepLds.sparse_lds_words * sizeof(uint32_t));   // a cell list per wave (coop_collides_sparse)
    return o;
}

// ... and the regions behind it
BCP_HD_INLINE LocalLds local_lds_rear(LocalLds o, int map_words, bool plain, int pairs)
{
    o.stat = (uint32_t)(((size_t)o.map + (size_t)map_words * sizeof(uint32_t) + 15) & ~(size_t)15);
    o.finish = o.stat + kStepLds.static_chunks * 16;   // the parameter block *S, then this launch's FinishWords (the shared-geometry variant)
    o.stash = o.finish + kStepLds.finish_slot_bytes;
    // delay queues: what the step's pushes will hand back
    o.bytes = o.stash + (plain ? 0u : (uint32_t)(10 * pairs * kBlock * sizeof(double)));
    return o;
}

BCP_HD_INLINE LocalLds local_lds_plan(int n_verts, int lds_path_doubles, int map_words, bool plain, int pairs)
{
    return local_lds_rear(local_lds_front(n_verts, lds_path_doubles, pairs), map_words, plain, pairs);
}

// ---- step_fast_pair_kernel: [qverts][shared path][64 x {x, y, theta}][64 x {reward, min_dist, target}][box][bucket index]
struct PairLds {
    int path, hand_pose, hand_score, box, index;   // (doubles)
    uint32_t bytes;
};

BCP_HD_INLINE PairLds pair_lds_plan(int n_verts, int lds_path_doubles)
{
    PairLds o;
    o.path = 2 * n_verts;
    o.hand_pose = o.path + lds_path_doubles;
    o.hand_score = o.hand_pose + 3 * kBlock;
    o.box = o.hand_score + 3 * kBlock;
    o.index = o.box + 8;
    o.bytes = (uint32_t)((size_t)o.index * sizeof(double) + 2 * kBlock * sizeof(uint32_t));
    return o;
}

// ---- step_pending_kernel: the exchange buffer of coop_collides_quad, two rounds of a row mask per lane and wave (8 or 3 words:
// that function's NW, repeated here); the kernel hands it over whole
BCP_HD_INLINE uint32_t pending_lds_bytes(bool wide) { return (uint32_t)(2 * kPendingWaves * (wide ? 8 : 3) * kBlock * sizeof(uint32_t)); }

// ---- step_kernel and the other callers of collision_lds_setup (collides_wave):
//   [lethal bitmap words (when the shared map is staged)] [qverts: n_verts * 2 doubles] [vertex scratch of the
//   per-thread rasteriser: n_verts * 2 * kBlock words] [cell list of the cell-by-cell exact test]
// (the words each region takes, not where it begins: collision_lds_setup adds them up one pointer after the other, as it did)
struct CollisionLdsPlan {
    int map, qverts, scratch, cells;   // words each region takes, in this order
    size_t bytes;
};

BCP_HD_INLINE constexpr CollisionLdsPlan collision_lds_plan(int n_verts, int map_words)
{
    CollisionLdsPlan o = {};
    o.map = (map_words + 1) & ~1;  // 8-byte alignment for the doubles
    o.qverts = 4 * n_verts;
    o.scratch = 2 * n_verts * kBlock;
    o.cells = kStepLds.sparse_lds_words;
    o.bytes = ((size_t)o.map + o.qverts + o.scratch + o.cells) * sizeof(uint32_t);
    return o;
}

inline size_t collision_lds_bytes(int n_verts, int in_lds, int rows, int wpr)
{
    return collision_lds_plan(n_verts, in_lds ? rows * wpr : 0).bytes;
}

}  // namespace bcp

// The step kernels' staging limits and LDS layouts as the compiler sees them: csrc/bcp_step_layout.h alone -- it has no HIP in
// it -- in a program of its own for AddressSanitizer and UBSan (tests/test_staging_host.py).
//   step_layout_main [PLAN...]   first every named limit as "limit NAME VALUE", then per PLAN one line, every offset in BYTES:
//       local:N_VERTS,PATH_DOUBLES,MAP_WORDS,PLAIN,PAIRS   step_local_kernel (local_lds_plan)
//       pair:N_VERTS,PATH_DOUBLES                          step_fast_pair_kernel (pair_lds_plan)
//       pending:WIDE                                       step_pending_kernel (pending_lds_bytes)
//       collision:N_VERTS,MAP_WORDS                        step_kernel (collision_lds_plan)
// Ends with "step layout ok".
#include <cstdio>
#include <cstring>

#include "bcp_step_layout.h"

using namespace bcp;

static void limit(const char* name, long long value) { printf("limit %s %lld\n", name, value); }

static int plan(const char* arg)
{
    int v[5] = {0, 0, 0, 0, 0};
    const unsigned d = (unsigned)sizeof(double), w = (unsigned)sizeof(uint32_t);
    if (sscanf(arg, "local:%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4]) == 5) {
        const LocalLds o = local_lds_plan(v[0], v[1], v[2], v[3] != 0, v[4]);
        printf("%s footprint=0 path=%u hand=%u box=%u index=%u ctl=%u rec=%u cells=%u map=%u stat=%u finish=%u stash=%u bytes=%u\n", arg,
               o.path * d, o.hand * d, o.box * d, o.index * d, o.ctl * d, o.rec, o.cells, o.map, o.stat, o.finish, o.stash, o.bytes);
    } else if (sscanf(arg, "pair:%d,%d", &v[0], &v[1]) == 2) {
        const PairLds o = pair_lds_plan(v[0], v[1]);
        printf("%s footprint=0 path=%u hand_pose=%u hand_score=%u box=%u index=%u bytes=%u\n", arg, o.path * d, o.hand_pose * d,
               o.hand_score * d, o.box * d, o.index * d, o.bytes);
    } else if (sscanf(arg, "pending:%d", &v[0]) == 1) {
        printf("%s bytes=%u\n", arg, pending_lds_bytes(v[0] != 0));
    } else if (sscanf(arg, "collision:%d,%d", &v[0], &v[1]) == 2) {
        const CollisionLdsPlan o = collision_lds_plan(v[0], v[1]);
        printf("%s map=0 qverts=%u scratch=%u cells=%u bytes=%zu\n", arg, o.map * w, (o.map + o.qverts) * w, (o.map + o.qverts + o.scratch) * w, o.bytes);
    } else {
        return 2;
    }
    return 0;
}

int main(int argc, char** argv)
{
    limit("kBlock", kBlock);
    limit("kLocalPairsMax", kLocalPairsMax);
    limit("kLocalMapWords", kLocalMapWords);
    limit("kScanItems", kScanItems);
    limit("kHandDoubles", kHandDoubles);
    limit("kPathLdsBytes", kPathLdsBytes);
    limit("kWayPointDoubles", kWayPointDoubles);
    limit("kPairStageRegs", kPairStageRegs);
    limit("kPairStageDoubles", kPairStageDoubles);
    limit("kPendingWaves", kPendingWaves);
    limit("kCtlWords", kCtlWords);
    for (int pairs = 1; pairs <= kLocalPairsMax; pairs *= 2) {
        char name[48];
        snprintf(name, sizeof(name), "local_stagers(%d)", pairs);
        limit(name, local_stagers(pairs));
        snprintf(name, sizeof(name), "local_map_per_stager(%d)", pairs);
        limit(name, local_map_per_stager(pairs));
    }
    limit("staged_map_words(1,256,16)", staged_map_words(true, 256, 16));
    limit("staged_map_words(1,241,17)", staged_map_words(true, 241, 17));
    limit("staged_map_words(0,8,8)", staged_map_words(false, 8, 8));
    limit("parked_pose_bytes", kStepLds.parked_pose_bytes);
    limit("sparse_lds_words", kStepLds.sparse_lds_words);
    limit("static_chunks", kStepLds.static_chunks);
    limit("finish_slot_bytes", kStepLds.finish_slot_bytes);
    for (int k = 1; k < argc; ++k) {
        if (plan(argv[k]) != 0) {
            fprintf(stderr, "step_layout_main: %s: not a plan\n", argv[k]);
            return 2;
        }
    }
    printf("step layout ok\n");
    return 0;
}

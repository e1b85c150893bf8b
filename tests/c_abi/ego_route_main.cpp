// The route decision of the egocentric observation (csrc/bcp_ego_route.h) on the host alone: which kernel a call's shape
// leads to and with what launch shape, the sparse route's limit and LDS sizes.  The header has no HIP in it; this program
// includes nothing else of the library and is built with -fsanitize=address,undefined.  Expected values are worked out
// by hand from the formulas (resolution 0.05; windows are rows x cols in pixels).
#include <cstdio>
#include <initializer_list>

#include "bcp_ego_route.h"
#include "host_io.h"

using namespace bcp;


// what the router is told of the cell lists: they exist and describe the maps; the largest count; the limit in force
struct EgoLists {
    bool usable;
    int32_t count, limit;
};
static const EgoLists kNoLists = {false, -1, 0};

static EgoPlan ego_route_of(const EgoCall& c, const EgoLists& lists) { return ego_route_of(c, lists.usable, lists.count, lists.limit); }
static const int64_t kImages = 96;

static EgoCall call_of(bool shared, int rows, int cols, int drows, int dcols, int border = 7, int pool = 1)
{
    const EgoCall c = {rows, cols, shared, drows, dcols, border, pool, kImages};
    return c;
}

static bool same_plan(const EgoPlan& a, const EgoPlan& b)
{
    return a.route == b.route && a.waves == b.waves && a.lds_bytes == b.lds_bytes && a.stage_map == b.stage_map &&
           a.win_lds_bytes == b.win_lds_bytes && a.px == b.px;
}

// lists unusable or a non-zero border, pool = 1: the sampling kernels
static void sampling_routes()
{
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: border 7 with usable lists (which must not matter); pass 1: border 0 without lists
        const int border = pass == 0 ? 7 : 0;
        const EgoLists lists = pass == 0 ? EgoLists{true, 10, 4096} : kNoLists;
        EgoPlan p = ego_route_of(call_of(true, 90, 70, 80, 70, border), lists);
        CHECK(p.route == BCP_EGO_STAGED && p.px == 8 && p.stage_map == 1 && p.waves == 8);
        CHECK(p.lds_bytes == 6624 + 8 * (2 * 80 + 16) * 4);
        p = ego_route_of(call_of(true, 90, 70, 5, 6, border), lists);
        CHECK(p.route == BCP_EGO_STAGED && p.px == 4 && p.stage_map == 1);
        // the whole 330 x 290 map: 107 760 bytes with the four tables of the fits-in-LDS test, 118 576 with the eight of the
        // launch -- above 64 KiB, so the function's LDS attribute has to be raised
        p = ego_route_of(call_of(true, 330, 290, 330, 290, border), lists);
        CHECK(ego_map_bytes(330, 290) + 4 * ego_row_bytes(330) == 107760);
        CHECK(p.route == BCP_EGO_STAGED && p.px == 8 && p.stage_map == 1 && p.lds_bytes == 118576 && p.lds_bytes > 64 * 1024);
        p = ego_route_of(call_of(false, 300, 260, 80, 70, border), lists);
        CHECK(p.route == BCP_EGO_BINNED && p.px == 8 && p.stage_map == 1 && p.waves == 4);
        CHECK(p.lds_bytes == 79128 + 4 * (2 * 80 + 16) * 4 && p.lds_bytes > 64 * 1024);
        p = ego_route_of(call_of(true, 420, 400, 80, 70, border), lists);
        CHECK(p.route == BCP_EGO_WINDOW && p.win_lds_bytes == 12544 && p.px == 8 && p.stage_map == 0 && p.waves == 4);
        CHECK(p.lds_bytes == 12544 + (2 * 80 + 16) * 4);
        p = ego_route_of(call_of(true, 420, 400, 5, 6, border), lists);
        CHECK(p.route == BCP_EGO_WINDOW && p.px == 4 && p.win_lds_bytes == 176);
        p = ego_route_of(call_of(true, 420, 400, 420, 400, border), lists);
        CHECK(p.route == BCP_EGO_GLOBAL && p.px == 8 && p.stage_map == 0 && p.win_lds_bytes == 0 && p.waves == 8);
        CHECK(p.lds_bytes == 8 * (2 * 420 + 16) * 4);
        // window side ceil(250.07) + 5 = 256: 65 536 bytes > 60 KB
        CHECK(ego_win_bytes(250, 6) == 65536);
        p = ego_route_of(call_of(true, 420, 400, 250, 6, border), lists);
        CHECK(p.route == BCP_EGO_GLOBAL && p.px == 4 && p.stage_map == 0);
        CHECK(ego_win_bytes(180, 180) == 260 * 260);
        p = ego_route_of(call_of(true, 420, 400, 180, 180, border), lists);
        CHECK(p.route == BCP_EGO_GLOBAL && p.px == 8);
        // private maps too large for LDS take the window / global routes like a shared one
        p = ego_route_of(call_of(false, 420, 400, 80, 70, border), lists);
        CHECK(p.route == BCP_EGO_WINDOW && p.stage_map == 0);
    }
    // 2^31 images and more cannot be binned (32-bit ranks)
    EgoCall many = call_of(false, 300, 260, 80, 70);
    many.n = (int64_t)1 << 31;
    CHECK(ego_route_of(many, kNoLists).route == BCP_EGO_WINDOW);
    many.n -= 1;
    CHECK(ego_route_of(many, kNoLists).route == BCP_EGO_BINNED);
}

// lists usable, the count at or below the limit, border 0
static void sparse_routes()
{
    const EgoLists at_limit = {true, 1945, 1945}, empty = {true, 0, 1945};
    for (const EgoLists& lists : {at_limit, empty}) {
        EgoPlan p = ego_route_of(call_of(true, 183, 183, 133, 117, 0, 1), lists);
        CHECK(p.route == BCP_EGO_SPARSE && p.waves == 8 && p.lds_bytes == 40576);
        p = ego_route_of(call_of(true, 183, 183, 133, 117, 0, 8), lists);
        CHECK(p.route == BCP_EGO_POOLED_SPARSE && p.waves == 8 && p.lds_bytes == 8 * 6096);
        p = ego_route_of(call_of(true, 183, 183, 133, 117, 0, 4), lists);
        CHECK(p.route == BCP_EGO_POOLED_SPARSE && p.waves == 7 && p.lds_bytes == 7 * 9152);
        p = ego_route_of(call_of(false, 183, 183, 133, 117, 0, 2), lists);
        CHECK(p.route == BCP_EGO_POOLED_SPARSE && p.waves == 3 && p.lds_bytes == 3 * 20888);
        p = ego_route_of(call_of(true, 350, 512, 133, 133, 0, 2), lists);
        CHECK(p.route == BCP_EGO_POOLED_SPARSE && p.waves == 2 && p.lds_bytes == 2 * 23160);
        CHECK(p.lds_bytes <= 64 * 1024);
    }
    CHECK(ego_pooled_sparse_waves(133, 117, 8) == 8 && ego_pooled_sparse_waves(133, 117, 4) == 7);
    CHECK(ego_pooled_sparse_waves(133, 117, 2) == 3 && ego_pooled_sparse_waves(133, 133, 2) == 2);
    // 400 x 300: the tables and held lists of eight waves are 69 376 bytes > 64 KiB -- no candidate, the sampling routes
    const EgoCall big = call_of(true, 420, 400, 400, 300, 0, 1);
    CHECK(ego_sparse_lds_bytes(400, 300, 8) == 69376);
    CHECK(ego_sparse_waves(big) == 0 && !ego_sparse_candidate(big, 1, false) && !ego_sparse_candidate(big, 4096, false));
    CHECK(ego_route_of(big, at_limit).route == BCP_EGO_GLOBAL);
    CHECK(same_plan(ego_route_of(big, at_limit), ego_route_of(big, kNoLists)));
}

static void candidates()
{
    const EgoCall c = call_of(true, 183, 183, 133, 117, 0, 1);
    CHECK(ego_sparse_candidate(c, 1, false) && ego_sparse_candidate(c, 4096, false));
    CHECK(!ego_sparse_candidate(c, 0, false));   // BCP_TUNE_EGO_SPARSE = 0: never
    CHECK(!ego_sparse_candidate(c, 1, true));    // the lists could not be allocated once
    CHECK(!ego_sparse_candidate(call_of(true, 183, 183, 133, 117, 1, 1), 1, false));   // a border value
    CHECK(ego_sparse_candidate(call_of(true, 4095, 4095, 133, 117, 0, 1), 1, false));
    CHECK(!ego_sparse_candidate(call_of(true, 4096, 100, 133, 117, 0, 1), 1, false));   // (a cell packs row and column in 12 bits each)
    CHECK(!ego_sparse_candidate(call_of(true, 100, 4096, 133, 117, 0, 1), 1, false));
    // pooled: a window whose pooled words leave no room for even one wave
    CHECK(ego_pooled_sparse_waves(1000, 1000, 2) == 0);
    CHECK(!ego_sparse_candidate(call_of(true, 1200, 1200, 1000, 1000, 0, 2), 1, false));
}

static void other_cases()
{
    const EgoLists usable = {true, 100, 1945}, over = {true, 1946, 1945}, uncounted = {true, -1, 1945};
    // any pool > 1 with the lists unusable or a border value: the pooled sampling kernel
    for (int pool : {2, 3, 4, 8, 64}) {
        for (bool shared : {true, false}) {
            EgoPlan p = ego_route_of(call_of(shared, 183, 183, 133, 117, 0, pool), kNoLists);
            CHECK(p.route == BCP_EGO_POOLED_SAMPLED && p.waves == 8 && p.lds_bytes == 0);
            p = ego_route_of(call_of(shared, 183, 183, 133, 117, 255, pool), usable);
            CHECK(p.route == BCP_EGO_POOLED_SAMPLED && p.waves == 8 && p.lds_bytes == 0);
            CHECK(ego_route_of(call_of(shared, 183, 183, 133, 117, 0, pool), over).route == BCP_EGO_POOLED_SAMPLED);
            CHECK(ego_route_of(call_of(shared, 420, 400, 133, 117, 0, pool), uncounted).route == BCP_EGO_POOLED_SAMPLED);
        }
    }
    // more cells than the limit: the sampling route of the same shape
    const EgoCall shapes[] = {call_of(true, 183, 183, 133, 117, 0),  call_of(false, 183, 183, 133, 117, 0), call_of(true, 350, 512, 133, 133, 0),
                              call_of(true, 420, 400, 250, 6, 0),    call_of(true, 90, 70, 5, 6, 0),        call_of(true, 183, 183, 133, 117, 0, 4)};
    const int32_t want[] = {BCP_EGO_STAGED, BCP_EGO_BINNED, BCP_EGO_WINDOW, BCP_EGO_GLOBAL, BCP_EGO_STAGED, BCP_EGO_POOLED_SAMPLED};
    for (int k = 0; k < 6; ++k) {
        const EgoPlan p = ego_route_of(shapes[k], over);
        CHECK(p.route == want[k]);
        CHECK(same_plan(p, ego_route_of(shapes[k], kNoLists)));
        CHECK(same_plan(ego_route_of(shapes[k], uncounted), ego_route_of(shapes[k], kNoLists)));
        const int32_t sparse = ego_route_of(shapes[k], usable).route;
        CHECK(sparse == (shapes[k].pool > 1 ? BCP_EGO_POOLED_SPARSE : BCP_EGO_SPARSE));
    }
}

static void limits()
{
    CHECK(ego_sparse_limit(4096, 133 * 117, true) == 4096 && ego_sparse_limit(4096, 30, false) == 4096);
    CHECK(ego_sparse_limit(2, 133 * 117, true) == 2);
    CHECK(ego_fits_lds(183, 183, 133) && !ego_fits_lds(350, 512, 133));
    CHECK(ego_sparse_limit(1, 133 * 117, true) == 1945);
    CHECK(ego_sparse_limit(1, 133 * 117, false) == 7780);
    CHECK(ego_sparse_limit(1, 5 * 6, true) == 512 && ego_sparse_limit(1, 5 * 6, false) == 512);   // the floor, kEgoCellCapMin
    CHECK(ego_sparse_limit(1, 40 * 40, true) == 512 && ego_sparse_limit(1, 40 * 40, false) == 800);
    CHECK(ego_sparse_limit(1, 420 * 400, true) == 16384 && ego_sparse_limit(1, 400 * 300, false) == 16384);   // the ceiling
    CHECK(ego_sparse_limit(1, 400 * 300, true) == 15000);
}

int main()
{
    sampling_routes();
    sparse_routes();
    candidates();
    other_cases();
    limits();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("ego route ok\n");
    return 0;
}

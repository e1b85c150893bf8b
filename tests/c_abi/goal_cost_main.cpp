// The weighted goal field's arithmetic (csrc/bcp_goal_cell.h: goal_relax_cell_cost, goal_cost_check_args, and -- unchanged,
// on weighted fields -- goal_walk_step and goal_route_row) on the host alone: the very functions goal_field_kernel<.., kCost>
// and goal_route_kernel call, over case files that tests/test_goal_cost_host.py writes.  The header has no HIP in it; this
// program includes nothing else of the library and is built with -ffp-contract=off -fsanitize=address,undefined.  Every read
// of a plane goes through a bounds-checked accessor, and the map, the table, the masks and the way points live in heap
// blocks of exactly their size: a relaxation, a lookup or a walk that left its block fails here.
//
//   goal_cost_main relax FILE OUT    FILE (binary, native endian):
//       int32 rows, cols, valid_rows, valid_cols, n_seeds, clearance_d2, max_passes, 0
//       uint8 data[rows * cols]
//       int32 seeds[n_seeds][2]              (row, col)
//       uint16 extra_of_cost[256]
//     the kernel's phases in sequence (host_goal_sweep, goal_sweep.h); phase 4 as in-place sweeps of goal_relax_cell_cost with the extra of the relaxed
//     cell's own byte, looked up for open cells only.  Writes uint16 plane[rows * cols] to OUT, prints
//     "sweeps S gave_up G reached N lookups L" (L: table lookups made)
//   goal_cost_main walk FILE         FILE (binary): int32 rows, cols, valid_rows, valid_cols, n, 0, 0, 0;
//       uint16 field[rows * cols]; int32 cell[n][2]      prints goal_walk_step of every cell, one per line
//   goal_cost_main route FILE        FILE (binary): int32 rows, cols, stride, max_len; double ox, oy, resolution;
//       double start[3], goal[3]; uint16 field[rows * cols]      prints "status S len L" of goal_route_row
//   goal_cost_main args FILE         FILE (text), per line the 13 arguments of goal_field_check_args, then the table: -2 = none,
//       -1 = all zeros, i >= 0 followed by a value = zeros but for entry i.  Prints "W N": W = 0 accepted, 1 refused by
//       goal_field_check_args with N, 2 refused by goal_cost_check_args with N -- the order bcp_goal_field_cost looks in
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bcp_goal_cell.h"
#include "goal_sweep.h"
#include "host_io.h"

using namespace bcp;

static int run_relax(const char* path, const char* out_path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head, seeds;
    std::vector<uint8_t> data;
    std::vector<uint16_t> table;
    bool ok = read_n(f, head, 8);
    ok = ok && head[0] > 0 && head[1] > 0 && head[4] >= 0 && head[5] >= 0 && head[5] <= kGoalMaxClearance && head[6] >= 0;
    ok = ok && read_n(f, data, (size_t)head[0] * head[1]) && read_n(f, seeds, (size_t)head[4] * 2) && read_n(f, table, 256);
    fclose(f);
    if (!ok) return 3;
    int32_t bad = 0;
    if (goal_cost_check_args(table.data(), bad) != kGoalCostOk) return 6;
    const int32_t rows = head[0], cols = head[1], n_seeds = head[4], clearance_d2 = head[5];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const int32_t max_passes = head[6] > 0 ? head[6] : rows * cols;
    HostSweep sw;
    if (!host_goal_sweep(rows, cols, vr, vc, data, seeds, n_seeds, clearance_d2, max_passes, &table, sw)) return 4;
    FILE* o = fopen(out_path, "wb");
    if (!o) return 5;
    const bool wrote = fwrite(sw.plane.data(), sizeof(uint16_t), sw.plane.size(), o) == sw.plane.size();
    fclose(o);
    if (!wrote) return 5;
    printf("sweeps %d gave_up %d reached %lld lookups %lld\n", sw.sweeps, sw.gave_up, sw.reached, sw.lookups);
    return 0;
}

static int run_walk(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head, cells;
    std::vector<uint16_t> field;
    bool ok = read_n(f, head, 8) && head[0] > 0 && head[1] > 0 && head[4] >= 0;
    ok = ok && read_n(f, field, (size_t)head[0] * head[1]) && read_n(f, cells, (size_t)head[4] * 2);
    fclose(f);
    if (!ok) return 3;
    const int32_t rows = head[0], cols = head[1];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const HostPlane get = {&field, cols, rows, cols};
    for (int32_t i = 0; i < head[4]; ++i) printf("%d\n", goal_walk_step(get, vr, vc, cells[(size_t)2 * i], cells[(size_t)2 * i + 1]));
    return 0;
}

static int run_route(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<double> nums;
    std::vector<uint16_t> field;
    bool ok = read_n(f, head, 4) && read_n(f, nums, 9) && head[0] > 0 && head[1] > 0 && head[2] >= 1 && head[3] >= 2;
    ok = ok && read_n(f, field, (size_t)head[0] * head[1]);
    fclose(f);
    if (!ok) return 3;
    const int32_t rows = head[0], cols = head[1], stride = head[2], max_len = head[3];
    const HostPlane get = {&field, cols, rows, cols};
    std::unique_ptr<double[]> wp(new double[(size_t)max_len * 3]);
    int32_t len = -1;
    double init[2] = {0.0, 0.0};
    const int32_t st = goal_route_row(get, rows, cols, &nums[3], &nums[6], true, nums[0], nums[1], 1.0 / nums[2], nums[2], stride,
                                      max_len, 0.0, 0.0, 1, HostNormalizeAngle(), wp.get(), len, init);
    if (len < 0 || len > max_len) return 4;
    printf("status %d len %d\n", st, len);
    return 0;
}

static int run_args(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        long long n_maps;
        int a[12], which = -2, value = 0;
        const int got = sscanf(line, "%d %lld %d %d %d %d %d %d %d %d %d %d %d %d %d", &a[0], &n_maps, &a[1], &a[2], &a[3], &a[4],
                               &a[5], &a[6], &a[7], &a[8], &a[9], &a[10], &a[11], &which, &value);
        if (got < 14 || which < -2 || which > 255 || value < 0 || value > 65535) {
            fclose(f);
            return 3;
        }
        std::vector<uint16_t> table(256, (uint16_t)0);
        if (which >= 0) table[(size_t)which] = (uint16_t)value;
        const int plain = goal_field_check_args(a[0] != 0, n_maps, a[1] != 0, a[2] != 0, a[3] != 0, a[4], a[5], a[6], a[7], a[8],
                                                a[9] != 0, a[10] != 0, a[11] != 0);
        int32_t bad = -1;
        const int cost = plain ? 0 : goal_cost_check_args(which == -2 ? nullptr : table.data(), bad);
        if (cost == kGoalCostEntry && bad != which) {
            fclose(f);
            return 4;
        }
        printf("%d %d\n", plain ? 1 : (cost ? 2 : 0), plain ? plain : cost);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 1;
    int rc = 1;
    if (strcmp(argv[1], "relax") == 0 && argc == 4) rc = run_relax(argv[2], argv[3]);
    else if (strcmp(argv[1], "walk") == 0 && argc == 3) rc = run_walk(argv[2]);
    else if (strcmp(argv[1], "route") == 0 && argc == 3) rc = run_route(argv[2]);
    else if (strcmp(argv[1], "args") == 0 && argc == 3) rc = run_args(argv[2]);
    if (rc == 0) printf("goal cost ok\n");
    return rc;
}

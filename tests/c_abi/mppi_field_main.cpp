// The terminal read of bcp_mppi_field (csrc/bcp_goal_cell.h: goal_value_at, goal_metres) on the host alone: the very
// functions mppi_kernel<.., FIELD> and goal_sample_row call, over a case file that tests/test_mppi_field_host.py writes.
// The header has no HIP in it; this program includes nothing else of the library and is built with -ffp-contract=off
// -fsanitize=address,undefined.  Every read of the plane goes through a bounds-checked accessor: a cell that left the
// valid shape aborts.
//
//   mppi_field_main FILE      FILE (binary, native endian):
//       int32 rows, cols, valid_rows, valid_cols, n_rows, 0, 0, 0
//       double ox, oy, resolution
//       uint16 field[rows * cols]
//       double pose[n_rows][2]               x, y
//     prints per row "value metres" -- metres = goal_metres(value == kGoalNone ? kGoalFar : value) as uint64 hex
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bcp_goal_cell.h"
#include "host_io.h"

using namespace bcp;

int main(int argc, char** argv)
{
    if (argc != 2) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<double> nums, poses;
    std::vector<uint16_t> field;
    bool ok = read_n(f, head, 8) && read_n(f, nums, 3);
    ok = ok && head[0] > 0 && head[1] > 0 && head[4] >= 0;
    ok = ok && read_n(f, field, (size_t)head[0] * head[1]) && read_n(f, poses, (size_t)head[4] * 2);
    fclose(f);
    if (!ok) return 3;
    const int32_t rows = head[0], cols = head[1], n_rows = head[4];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const double ox = nums[0], oy = nums[1], resolution = nums[2];
    const double inv_res = 1.0 / resolution;   // (as bcp_set_costmaps has it)
    const double lim = 1.7976931348623157e308;
    const HostPlane get = {&field, cols, vr, vc};   // (the helper reads inside the valid shape only)
    for (int32_t i = 0; i < n_rows; ++i) {
        const double x = poses[(size_t)2 * i], y = poses[(size_t)2 * i + 1];
        const bool finite = x >= -lim && x <= lim && y >= -lim && y <= lim;
        int32_t r = -1, c = -1;
        const int32_t v = goal_value_at(get, vr, vc, x, y, finite, ox, oy, inv_res, r, c);
        if (v != goal_value_at(get, vr, vc, x, y, finite, ox, oy, inv_res)) return 4;   // the two forms agree
        if (v != kGoalNone && (r < 0 || r >= vr || c < 0 || c >= vc || v != (int32_t)field[(size_t)r * cols + c])) return 5;
        const double metres = goal_metres(v == kGoalNone ? kGoalFar : v, resolution);
        uint64_t bits;
        memcpy(&bits, &metres, sizeof(bits));
        printf("%d %016llx\n", v, (unsigned long long)bits);
    }
    printf("mppi field ok\n");
    return 0;
}

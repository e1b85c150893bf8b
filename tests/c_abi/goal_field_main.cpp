// The goal field's arithmetic (csrc/bcp_goal_cell.h) on the host alone: the very functions goal_field_kernel and
// goal_sample_kernel call, over case files that tests/test_goal_field_host.py writes.  The header has no HIP in it; this
// program includes nothing else of the library and is built with -ffp-contract=off -fsanitize=address,undefined.  Every read
// of a plane goes through a bounds-checked accessor: a relaxation or a walk that left the map throws.
//
//   goal_field_main relax FILE OUT   FILE (binary, native endian):
//       int32 rows, cols, valid_rows, valid_cols, n_seeds, clearance_d2, max_passes, 0
//       uint8 data[rows * cols]
//       int32 seeds[n_seeds][2]              (row, col)
//     the kernel's phases in sequence (host_goal_sweep, goal_sweep.h): lethal mask, closed mask by goal_half_width /
//     goal_widen_word, plane and seeds, then in-place sweeps of goal_relax_cell until one changes nothing (or max_passes > 0
//     sweeps were made).
//     writes uint16 plane[rows * cols] to OUT, prints "sweeps S gave_up G reached N"
//   goal_field_main sample FILE      FILE (binary):
//       int32 rows, cols, valid_rows, valid_cols, n_rows, carrot_cells, 0, 0
//       double ox, oy, resolution, max_dist
//       uint16 field[rows * cols]
//       double pose[n_rows][5]               x, y, theta, cos theta, sin theta (the caller's cos / sin)
//     prints per row "out3[0] out3[1] out3[2] (as uint32 hex) cell_value carrot_row carrot_col"
//   goal_field_main args FILE        FILE (text), per line the 13 arguments of goal_field_check_args
//   goal_field_main sargs FILE       FILE (text), per line the 16 arguments of goal_sample_check_args (max_dist as strtod reads it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    bool ok = read_n(f, head, 8);
    ok = ok && head[0] > 0 && head[1] > 0 && head[4] >= 0 && head[5] >= 0 && head[5] <= kGoalMaxClearance && head[6] >= 0;
    ok = ok && read_n(f, data, (size_t)head[0] * head[1]) && read_n(f, seeds, (size_t)head[4] * 2);
    fclose(f);
    if (!ok) return 3;
    const int32_t rows = head[0], cols = head[1], n_seeds = head[4], clearance_d2 = head[5];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const int32_t max_passes = head[6] > 0 ? head[6] : rows * cols;
    HostSweep sw;
    if (!host_goal_sweep(rows, cols, vr, vc, data, seeds, n_seeds, clearance_d2, max_passes, nullptr, sw)) return 4;
    FILE* o = fopen(out_path, "wb");
    if (!o) return 5;
    const bool wrote = fwrite(sw.plane.data(), sizeof(uint16_t), sw.plane.size(), o) == sw.plane.size();
    fclose(o);
    if (!wrote) return 5;
    printf("sweeps %d gave_up %d reached %lld\n", sw.sweeps, sw.gave_up, sw.reached);
    return 0;
}

static int run_sample(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<double> nums, poses;
    std::vector<uint16_t> field;
    bool ok = read_n(f, head, 8) && read_n(f, nums, 4);
    ok = ok && head[0] > 0 && head[1] > 0 && head[4] >= 0;
    ok = ok && read_n(f, field, (size_t)head[0] * head[1]) && read_n(f, poses, (size_t)head[4] * 5);
    fclose(f);
    if (!ok) return 3;
    const int32_t rows = head[0], cols = head[1], n_rows = head[4], carrot_cells = head[5];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const double ox = nums[0], oy = nums[1], resolution = nums[2], max_dist = nums[3];
    const double inv_res = 1.0 / resolution;   // (as bcp_set_costmaps has it)
    const double lim = 1.7976931348623157e308;
    const HostPlane get = {&field, cols, rows, cols};
    for (int32_t i = 0; i < n_rows; ++i) {
        const double* p = &poses[(size_t)i * 5];
        const bool finite = p[0] >= -lim && p[0] <= lim && p[1] >= -lim && p[1] <= lim && p[2] >= -lim && p[2] <= lim;
        const GoalSample s = goal_sample_row(get, vr, vc, p[0], p[1], p[3], p[4], finite, ox, oy, inv_res, resolution, carrot_cells,
                                             max_dist);
        uint32_t bits[3];
        memcpy(bits, s.out3, sizeof(bits));
        printf("%08x %08x %08x %d %d %d\n", bits[0], bits[1], bits[2], s.cell_value, s.carrot_row, s.carrot_col);
    }
    return 0;
}

static int run_args(const char* path, bool sample)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        if (!sample) {
            long long n_maps;
            int a[12];
            if (sscanf(line, "%d %lld %d %d %d %d %d %d %d %d %d %d %d", &a[0], &n_maps, &a[1], &a[2], &a[3], &a[4], &a[5], &a[6],
                       &a[7], &a[8], &a[9], &a[10], &a[11]) != 13) {
                fclose(f);
                return 3;
            }
            printf("%d\n", goal_field_check_args(a[0] != 0, n_maps, a[1] != 0, a[2] != 0, a[3] != 0, a[4], a[5], a[6], a[7], a[8],
                                                 a[9] != 0, a[10] != 0, a[11] != 0));
        } else {
            int h, fld, out3, carrot, have_poses, have_row_env, final_form, rows, cols, map_rows, map_cols;
            long long n, n_envs, n_fields, n_entries;
            char dist_text[64];
            if (sscanf(line, "%d %d %d %d %63s %lld %lld %d %d %d %d %d %d %d %lld %lld", &h, &fld, &out3, &carrot, dist_text, &n,
                       &n_envs, &have_poses, &have_row_env, &final_form, &rows, &cols, &map_rows, &map_cols, &n_fields,
                       &n_entries) != 16) {
                fclose(f);
                return 3;
            }
            printf("%d\n", goal_sample_check_args(h != 0, fld != 0, out3 != 0, carrot, strtod(dist_text, nullptr), n, n_envs,
                                                  have_poses != 0, have_row_env != 0, final_form != 0, rows, cols, map_rows, map_cols,
                                                  n_fields, n_entries));
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 1;
    int rc = 1;
    if (strcmp(argv[1], "relax") == 0 && argc == 4) rc = run_relax(argv[2], argv[3]);
    else if (strcmp(argv[1], "sample") == 0 && argc == 3) rc = run_sample(argv[2]);
    else if (strcmp(argv[1], "args") == 0 && argc == 3) rc = run_args(argv[2], false);
    else if (strcmp(argv[1], "sargs") == 0 && argc == 3) rc = run_args(argv[2], true);
    if (rc == 0) printf("goal field ok\n");
    return rc;
}

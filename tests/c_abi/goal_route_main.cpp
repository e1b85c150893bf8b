// The route of one row (csrc/bcp_goal_cell.h: goal_route_row, goal_route_check_args, and through them goal_walk_step,
// goal_value_at and csrc/bcp_path_init.h's path_initial_reward) on the host alone: the very functions goal_route_kernel
// calls, over case files that tests/test_goal_route_host.py writes.  The headers have no HIP in them; this program includes
// nothing else of the library and is built with -ffp-contract=off -fsanitize=address,undefined.  Every read of a plane goes
// through a bounds-checked accessor, and every row's way points live in a heap block of exactly max_len * 3 doubles: a walk
// that left the map aborts, a way point written past the row's slots is AddressSanitizer's.
//
//   goal_route_main route FILE OUT   FILE (binary, native endian):
//       int32 rows, cols, valid_rows, valid_cols, n_rows, stride, max_len, pure_pursuit
//       double ox, oy, resolution, spatial_precision, angular_precision
//       uint16 field[rows * cols]
//       double row[n_rows][6]                start x, y, theta, goal x, y, theta
//     writes to OUT double paths[n_rows][max_len][3], double init[n_rows][2], int32 lens[n_rows], int32 status[n_rows]
//   goal_route_main args FILE        FILE (text), per line the 18 arguments of goal_route_check_args
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bcp_goal_cell.h"
#include "host_io.h"

using namespace bcp;

static int run_route(const char* path, const char* out_path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<double> nums, poses;
    std::vector<uint16_t> field;
    bool ok = read_n(f, head, 8) && read_n(f, nums, 5);
    ok = ok && head[0] > 0 && head[1] > 0 && head[4] >= 0 && head[5] >= 1 && head[5] <= kGoalRouteMaxStride && head[6] >= 2 &&
         head[6] <= kGoalRouteMaxLen;
    ok = ok && read_n(f, field, (size_t)head[0] * head[1]) && read_n(f, poses, (size_t)head[4] * 6);
    fclose(f);
    if (!ok) return 3;
    const int32_t rows = head[0], cols = head[1], n_rows = head[4], stride = head[5], max_len = head[6], pure_pursuit = head[7];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const double ox = nums[0], oy = nums[1], resolution = nums[2], sp = nums[3], ap = nums[4];
    const double inv_res = 1.0 / resolution;   // (as bcp_set_costmaps has it)
    const double lim = 1.7976931348623157e308;
    const HostPlane get = {&field, cols, rows, cols};
    std::vector<double> all_paths, all_init;
    std::vector<int32_t> lens, status;
    for (int32_t i = 0; i < n_rows; ++i) {
        const double* p = &poses[(size_t)i * 6];
        bool finite = true;
        for (int k = 0; k < 6; ++k) finite = finite && p[k] >= -lim && p[k] <= lim;
        std::unique_ptr<double[]> wp(new double[(size_t)max_len * 3]);   // exactly the row's slots
        for (int32_t j = 0; j < 3 * max_len; ++j) wp[j] = -7.0;          // (a slot left unwritten shows)
        int32_t len = -1;
        double init[2] = {-7.0, -7.0};
        const int32_t st = goal_route_row(get, vr, vc, p, p + 3, finite, ox, oy, inv_res, resolution, stride, max_len, sp, ap,
                                          pure_pursuit, HostNormalizeAngle(), wp.get(), len, init);
        if (len < 0 || len > max_len) return 4;
        all_paths.insert(all_paths.end(), wp.get(), wp.get() + (size_t)max_len * 3);
        all_init.push_back(init[0]);
        all_init.push_back(init[1]);
        lens.push_back(len);
        status.push_back(st);
    }
    FILE* o = fopen(out_path, "wb");
    if (!o) return 5;
    bool wrote = fwrite(all_paths.data(), sizeof(double), all_paths.size(), o) == all_paths.size();
    wrote = wrote && fwrite(all_init.data(), sizeof(double), all_init.size(), o) == all_init.size();
    wrote = wrote && fwrite(lens.data(), sizeof(int32_t), lens.size(), o) == lens.size();
    wrote = wrote && fwrite(status.data(), sizeof(int32_t), status.size(), o) == status.size();
    fclose(o);
    return wrote ? 0 : 5;
}

static int run_args(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        int a[14];
        long long n, n_envs, n_fields, n_entries;
        if (sscanf(line, "%d %d %d %d %d %d %d %lld %lld %d %d %d %d %d %d %d %lld %lld", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5],
                   &a[6], &n, &n_envs, &a[7], &a[8], &a[9], &a[10], &a[11], &a[12], &a[13], &n_fields, &n_entries) != 18) {
            fclose(f);
            return 3;
        }
        printf("%d\n", goal_route_check_args(a[0] != 0, a[1] != 0, a[2] != 0, a[3] != 0, a[4] != 0, a[5], a[6], n, n_envs, a[7] != 0,
                                             a[8] != 0, a[9] != 0, a[10], a[11], a[12], a[13], n_fields, n_entries));
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 1;
    int rc = 1;
    if (strcmp(argv[1], "route") == 0 && argc == 4) rc = run_route(argv[2], argv[3]);
    else if (strcmp(argv[1], "args") == 0 && argc == 3) rc = run_args(argv[2]);
    if (rc == 0) printf("goal route ok\n");
    return rc;
}

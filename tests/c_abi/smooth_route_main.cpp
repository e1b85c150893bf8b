// One row of bcp_smooth_route (csrc/bcp_smooth_cell.h: smooth_row, smooth_clear, smooth_check_args, and through them the
// pull, the blends, the pieces and csrc/bcp_path_init.h's path_initial_reward) on the host alone: the very functions
// smooth_kernel calls, over case files that tests/test_smooth_route_host.py writes.  The header has no HIP in it; this
// program includes nothing else of the library and is built with -ffp-contract=off -fsanitize=address,undefined.  Every
// read of a plane goes through a bounds-checked accessor, and every row's input, cells, vertices and way points live in heap
// blocks of exactly their sizes.
//
//   smooth_route_main smooth FILE OUT   FILE (binary, native endian):
//       int32 rows, cols, valid_rows, valid_cols, n_rows, max_len_in, max_len, pure_pursuit, look, halvings
//       double ox, oy, resolution, spatial_precision, angular_precision, blend, delta
//       uint16 field[rows * cols]
//       int32 lens_in[n_rows]
//       double paths_in[n_rows][max_len_in][3]
//     writes to OUT double paths[n_rows][max_len][3], double init[n_rows][2], int32 lens[n_rows], status[n_rows], info[n_rows][4]
//   smooth_route_main clear FILE        FILE (binary): int32 rows, cols, valid_rows, valid_cols, n_pairs; uint16 field[rows * cols];
//       int32 pair[n_pairs][4] = r0, c0, r1, c1 (a negative r: no cell).  Prints per pair: the verdict, the number of cells
//       asked for, and those cells (row col) in the order the walk asked for them.
//   smooth_route_main args FILE         FILE (text), per line the 20 arguments of smooth_check_args
//   smooth_route_main layout            prints sizeof(SmoothParams) and the offsets of look, halvings, blend, delta
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "bcp_smooth_cell.h"
#include "host_io.h"

using namespace bcp;

struct RowIn {
    const double* p;
    int32_t m;
    double operator()(int32_t k, int32_t e) const
    {
        if (k < 0 || k >= m || e < 0 || e > 2) abort();
        return p[3 * k + e];
    }
};

// a map that remembers what it was asked
struct AskedMap {
    SmoothMap<HostPlane> map;
    std::vector<std::pair<int32_t, int32_t>>* asked;
    bool passable(int32_t r, int32_t c) const
    {
        asked->push_back(std::make_pair(r, c));
        return map.passable(r, c);
    }
};

static int run_smooth(const char* path, const char* out_path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head, lens_in;
    std::vector<double> nums;
    std::vector<uint16_t> field;
    bool ok = read_n(f, head, 10) && read_n(f, nums, 7);
    ok = ok && head[0] > 0 && head[1] > 0 && head[4] >= 0 && head[5] >= 2 && head[5] <= kSmoothMaxLen && head[6] >= 2 &&
         head[6] <= kSmoothMaxLen;
    ok = ok && read_n(f, field, (size_t)head[0] * head[1]) && read_n(f, lens_in, (size_t)head[4]);
    if (!ok) {
        fclose(f);
        return 3;
    }
    const int32_t rows = head[0], cols = head[1], n_rows = head[4], max_len_in = head[5], max_len = head[6], pure_pursuit = head[7];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    SmoothParams prm;
    prm.look = head[8];
    prm.halvings = head[9];
    prm.blend = nums[5];
    prm.delta = nums[6];
    const HostPlane plane = {&field, cols, vr, vc};   // (nothing may be read beyond the valid shape)
    SmoothMap<HostPlane> map = {plane, vr, vc, nums[0], nums[1], 1.0 / nums[2]};
    std::vector<double> all_paths, all_init;
    std::vector<int32_t> lens, status, infos;
    for (int32_t i = 0; i < n_rows; ++i) {
        const int32_t m = lens_in[i] < max_len_in ? (lens_in[i] < 0 ? 0 : lens_in[i]) : max_len_in;
        bool read_ok = true;
        std::unique_ptr<double[]> row = read_block<double>(f, (size_t)max_len_in * 3, read_ok);
        if (!read_ok) {
            fclose(f);
            return 3;
        }
        std::unique_ptr<double[]> mine(new double[(size_t)m * 3]);   // exactly the row's m way points
        memcpy(mine.get(), row.get(), sizeof(double) * (size_t)m * 3);
        const RowIn in = {mine.get(), m};
        std::unique_ptr<int16_t[]> cells(new int16_t[(size_t)2 * m]);
        std::unique_ptr<uint16_t[]> vertices(new uint16_t[(size_t)m]);
        std::unique_ptr<double[]> wp(new double[(size_t)max_len * 3]);
        for (int32_t j = 0; j < 3 * max_len; ++j) wp[j] = -7.0;
        int32_t len = -1, info[4] = {-7, -7, -7, -7};
        double init[2] = {-7.0, -7.0};
        const int32_t st = smooth_row(map, in, m, true, prm, max_len, nums[3], nums[4], pure_pursuit, HostNormalizeAngle(),
                                      cells.get(), vertices.get(), wp.get(), len, init, info);
        if (len < 0 || len > max_len) {
            fclose(f);
            return 4;
        }
        all_paths.insert(all_paths.end(), wp.get(), wp.get() + (size_t)max_len * 3);
        all_init.push_back(init[0]);
        all_init.push_back(init[1]);
        lens.push_back(len);
        status.push_back(st);
        infos.insert(infos.end(), info, info + 4);
    }
    fclose(f);
    FILE* o = fopen(out_path, "wb");
    if (!o) return 5;
    bool wrote = fwrite(all_paths.data(), sizeof(double), all_paths.size(), o) == all_paths.size();
    wrote = wrote && fwrite(all_init.data(), sizeof(double), all_init.size(), o) == all_init.size();
    wrote = wrote && fwrite(lens.data(), sizeof(int32_t), lens.size(), o) == lens.size();
    wrote = wrote && fwrite(status.data(), sizeof(int32_t), status.size(), o) == status.size();
    wrote = wrote && fwrite(infos.data(), sizeof(int32_t), infos.size(), o) == infos.size();
    fclose(o);
    return wrote ? 0 : 5;
}

static int run_clear(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head, pairs;
    std::vector<uint16_t> field;
    bool ok = read_n(f, head, 5) && head[0] > 0 && head[1] > 0 && head[4] >= 0;
    ok = ok && read_n(f, field, (size_t)head[0] * head[1]) && read_n(f, pairs, (size_t)head[4] * 4);
    fclose(f);
    if (!ok) return 3;
    const int32_t rows = head[0], cols = head[1];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const HostPlane plane = {&field, cols, vr, vc};
    std::vector<std::pair<int32_t, int32_t>> asked;
    const AskedMap map = {{plane, vr, vc, 0.0, 0.0, 1.0}, &asked};
    for (int32_t i = 0; i < head[4]; ++i) {
        asked.clear();
        const int32_t* p = &pairs[(size_t)i * 4];
        const bool verdict = smooth_clear(map, p[0], p[1], p[2], p[3]);
        printf("%d %d", verdict ? 1 : 0, (int)asked.size());
        for (const auto& rc : asked) printf(" %d %d", rc.first, rc.second);
        printf("\n");
    }
    return 0;
}

static int run_args(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        int a[16];
        double blend, delta;
        long long n, n_fields, n_entries;
        if (sscanf(line, "%d %d %d %d %lf %lf %d %d %lld %d %d %d %d %d %d %lld %lld %d %d %d", &a[0], &a[1], &a[2], &a[3], &blend, &delta,
                   &a[4], &a[5], &n, &a[6], &a[7], &a[8], &a[9], &a[10], &a[11], &n_fields, &n_entries, &a[12], &a[13], &a[14]) != 20) {
            fclose(f);
            return 3;
        }
        printf("%d\n", smooth_check_args(a[0] != 0, a[1] != 0, a[2], a[3], blend, delta, a[4], a[5], n, a[6] != 0, a[7] != 0, a[8], a[9],
                                         a[10], a[11], n_fields, n_entries, a[12] != 0, a[13] != 0, a[14] != 0));
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 1;
    int rc = 1;
    if (strcmp(argv[1], "smooth") == 0 && argc == 4) rc = run_smooth(argv[2], argv[3]);
    else if (strcmp(argv[1], "clear") == 0 && argc == 3) rc = run_clear(argv[2]);
    else if (strcmp(argv[1], "args") == 0 && argc == 3) rc = run_args(argv[2]);
    else if (strcmp(argv[1], "layout") == 0) {
        printf("%d %d %d %d %d\n", (int)sizeof(SmoothParams), (int)offsetof(SmoothParams, look), (int)offsetof(SmoothParams, halvings),
               (int)offsetof(SmoothParams, blend), (int)offsetof(SmoothParams, delta));
        printf("%d %d\n", smooth_overlap(100, 10, 109, 4) ? 1 : 0, smooth_overlap(100, 10, 110, 4) ? 1 : 0);
        rc = 0;
    }
    if (rc == 0) printf("smooth route ok\n");
    return rc;
}

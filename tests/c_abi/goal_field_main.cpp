// The goal field's arithmetic (csrc/bcp_goal_cell.h) on the host alone: the very functions goal_field_kernel and
// goal_sample_kernel call, over case files that tests/test_goal_field_host.py writes.  The header has no HIP in it; this
// program includes nothing else of the library and is built with -ffp-contract=off -fsanitize=address,undefined.  Every read
// of a plane goes through a bounds-checked accessor: a relaxation or a walk that left the map throws.
//
//   goal_field_main relax FILE OUT   FILE (binary, native endian):
//       int32 rows, cols, valid_rows, valid_cols, n_seeds, clearance_d2, max_passes, 0
//       uint8 data[rows * cols]
//       int32 seeds[n_seeds][2]              (row, col)
//     the kernel's phases in sequence: lethal mask, closed mask by goal_half_width / goal_widen_word, plane and seeds, then
//     in-place sweeps of goal_relax_cell until one changes nothing (or max_passes > 0 sweeps were made).
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

using namespace bcp;

struct HostPlane {
    const std::vector<uint16_t>* cells;
    int32_t rows, cols;
    uint16_t operator()(int32_t r, int32_t c) const
    {
        if (r < 0 || r >= rows || c < 0 || c >= cols) abort();   // (the index alone could wrap into the plane)
        return cells->at((size_t)r * cols + c);
    }
};

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

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
    const int32_t rows = head[0], cols = head[1], wpr = (cols + 31) / 32, n_seeds = head[4], clearance_d2 = head[5];
    const int32_t vr = head[2] < 0 ? 0 : (head[2] > rows ? rows : head[2]), vc = head[3] < 0 ? 0 : (head[3] > cols ? cols : head[3]);
    const int32_t max_passes = head[6] > 0 ? head[6] : rows * cols;
    const int32_t reach = goal_isqrt(clearance_d2);
    std::vector<uint32_t> lethal((size_t)rows * wpr, 0u), closed((size_t)rows * wpr, 0u);
    for (int32_t r = 0; r < vr; ++r)
        for (int32_t c = 0; c < vc; ++c)
            if (data[(size_t)r * cols + c] == 254) lethal.at((size_t)r * wpr + (c >> 5)) |= 1u << (c & 31);
    for (int32_t r = 0; r < rows; ++r) {
        for (int32_t w = 0; w < wpr; ++w) {
            const int32_t first = 32 * w;
            const uint32_t inside = r < vr && vc > first ? (vc - first >= 32 ? ~0u : (1u << (vc - first)) - 1u) : 0u;
            uint32_t acc = 0u;
            if (inside) {
                const int32_t lo = r - reach > 0 ? r - reach : 0, hi = r + reach < vr - 1 ? r + reach : vr - 1;
                for (int32_t rr = lo; rr <= hi; ++rr) {
                    const int32_t hw = goal_half_width(clearance_d2, rr > r ? rr - r : r - rr), kw = (hw + 31) >> 5;
                    const int32_t k0 = w - kw > 0 ? w - kw : 0, k1 = w + kw < wpr - 1 ? w + kw : wpr - 1;
                    for (int32_t k = k0; k <= k1; ++k) acc |= goal_widen_word(lethal.at((size_t)rr * wpr + k), 32 * (k - w), hw);
                }
            }
            closed.at((size_t)r * wpr + w) = (acc & inside) | ~inside;
        }
    }
    std::vector<uint16_t> plane((size_t)rows * cols, (uint16_t)kGoalNone);
    for (int32_t s = 0; s < n_seeds; ++s) {
        const int32_t sr = seeds[(size_t)2 * s], sc = seeds[(size_t)2 * s + 1];
        if (sr >= 0 && sr < vr && sc >= 0 && sc < vc) {
            plane.at((size_t)sr * cols + sc) = 0;
            closed.at((size_t)sr * wpr + (sc >> 5)) &= ~(1u << (sc & 31));
        }
    }
    const HostPlane get = {&plane, rows, cols};
    int32_t sweeps = 0, gave_up = 0;
    for (;;) {
        if (sweeps == max_passes) {
            gave_up = 1;
            break;
        }
        ++sweeps;
        bool lowered = false;
        for (int32_t r = 0; r < vr; ++r) {
            for (int32_t c = 0; c < vc; ++c) {
                if ((closed.at((size_t)r * wpr + (c >> 5)) >> (c & 31)) & 1u) continue;
                const int32_t own = plane[(size_t)r * cols + c];
                if (own == 0) continue;
                const int32_t now = goal_relax_cell(get, vr, vc, r, c, own);
                if (now > own || now < 0 || now > kGoalNone) return 4;   // (values only fall)
                if (now != own) {
                    plane[(size_t)r * cols + c] = (uint16_t)now;
                    lowered = true;
                }
            }
        }
        if (!lowered) break;
    }
    long long reached = 0;
    for (uint16_t v : plane) reached += v != (uint16_t)kGoalNone;
    FILE* o = fopen(out_path, "wb");
    if (!o) return 5;
    const bool wrote = fwrite(plane.data(), sizeof(uint16_t), plane.size(), o) == plane.size();
    fclose(o);
    if (!wrote) return 5;
    printf("sweeps %d gave_up %d reached %lld\n", sweeps, gave_up, reached);
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
    const HostPlane get = {&field, rows, cols};
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

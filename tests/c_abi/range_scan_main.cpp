// The range scan's arithmetic (csrc/bcp_scan_march.h) on the host alone: the very functions range_scan_kernel calls, over a
// case file that tests/test_range_scan_host.py writes.  The header has no HIP in it; this program includes nothing else of
// the library and is built with -ffp-contract=off -fsanitize=address,undefined.
//
//   range_scan_main scan FILE    FILE (binary, native endian):
//       int32 rows, cols, wpr, valid_rows, valid_cols, n_rows, n_beams, 0
//       double ox, oy, resolution, max_range
//       uint32 bits[rows * wpr]              the row-major lethal mask
//       double pose[n_rows][5]               x, y, theta, cos theta, sin theta (the caller's cos / sin)
//       double beam[n_beams][2]
//     prints "bound B", then per ray "range-as-uint32-hex hit trips"
//   range_scan_main args FILE    FILE (text), per line: have_handle have_beams have_ranges n_beams n n_envs have_poses
//       final_form max_range inv_res (the doubles as strtod reads them: hex floats, nan, inf)
//     prints scan_check_args' answer per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bcp_scan_march.h"
#include "host_io.h"

using namespace bcp;

struct HostWords {
    const std::vector<uint32_t>* words;
    uint32_t operator()(int32_t k) const { return words->at((size_t)k); }   // (a walk that left the mask throws)
};

static int run_scan(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> head;
    std::vector<double> nums, poses, beams;
    std::vector<uint32_t> bits;
    bool ok = read_n(f, head, 8) && read_n(f, nums, 4);
    ok = ok && head[0] > 0 && head[1] > 0 && head[2] == (head[1] + 31) / 32 && head[5] >= 0 && head[6] >= 0;
    ok = ok && read_n(f, bits, (size_t)head[0] * head[2]) && read_n(f, poses, (size_t)head[5] * 5) &&
         read_n(f, beams, (size_t)head[6] * 2);
    fclose(f);
    if (!ok) return 3;
    const int32_t cols = head[1], wpr = head[2], valid_rows = head[3], valid_cols = head[4], n_rows = head[5], n_beams = head[6];
    const double ox = nums[0], oy = nums[1], resolution = nums[2], max_range = nums[3];
    const double inv_res = 1.0 / resolution;   // (as bcp_set_costmaps has it)
    const double R = max_range * inv_res;
    const int32_t bound = scan_trip_bound(R);
    const HostWords words = {&bits};
    printf("bound %d\n", bound);
    for (int32_t i = 0; i < n_rows; ++i) {
        const double* p = &poses[(size_t)i * 5];
        double u, v, row_R;
        scan_row_start(p[0], p[1], p[2], ox, oy, inv_res, R, &u, &v, &row_R);
        for (int32_t b = 0; b < n_beams; ++b) {
            double dx, dy;
            scan_direction(p[3], p[4], beams[(size_t)2 * b], beams[(size_t)2 * b + 1], &dx, &dy);
            const ScanResult r = scan_march(words, wpr, cols, valid_rows, valid_cols, u, v, dx, dy, row_R, resolution, max_range, bound);
            uint32_t as_bits;
            memcpy(&as_bits, &r.range, sizeof(as_bits));
            printf("%08x %d %d\n", as_bits, r.hit, r.trips);
        }
    }
    return 0;
}

static int run_args(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        int have_h, have_beams, have_ranges, n_beams, have_poses, final_form;
        long long n, n_envs;
        char range_text[64], inv_text[64];
        if (sscanf(line, "%d %d %d %d %lld %lld %d %d %63s %63s", &have_h, &have_beams, &have_ranges, &n_beams, &n, &n_envs,
                   &have_poses, &final_form, range_text, inv_text) != 10) {
            fclose(f);
            return 3;
        }
        printf("%d\n", scan_check_args(have_h != 0, have_beams != 0, have_ranges != 0, n_beams, n, n_envs, have_poses != 0,
                                       final_form != 0, strtod(range_text, nullptr), strtod(inv_text, nullptr)));
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    const int rc = strcmp(argv[1], "scan") == 0 ? run_scan(argv[2]) : (strcmp(argv[1], "args") == 0 ? run_args(argv[2]) : 1);
    if (rc == 0) printf("range scan ok\n");
    return rc;
}

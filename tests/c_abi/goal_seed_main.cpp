// The host half of bcp_goal_field_bound / bcp_refresh_goal_fields: goal_seed_of_path and goal_bound_check_args of
// csrc/bcp_goal_cell.h as goal_field_kernel's bound form and the entry points call them, in a program of its own for
// AddressSanitizer and UBSan (tests/test_goal_field_refresh_host.py).  The header has no HIP in it.
//   goal_seed_main seeds FILE   lines "x y ox oy inv_res vr vc" (strtod: hex floats, nan, inf) -> "usable row col" per line;
//                               row and col start from a sentinel, so a refusal that wrote them shows
//   goal_seed_main args FILE    lines of the 16 arguments of goal_bound_check_args -> the refusal per line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bcp_goal_cell.h"

static int run_seeds(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        double v[5];
        char* p = line;
        for (int k = 0; k < 5; ++k) {
            char* end = nullptr;
            v[k] = strtod(p, &end);
            if (end == p) {
                fclose(f);
                return 3;
            }
            p = end;
        }
        long vr = 0, vc = 0;
        if (sscanf(p, "%ld %ld", &vr, &vc) != 2) {
            fclose(f);
            return 3;
        }
        int32_t row = -12345, col = -12345;
        const bool usable = bcp::goal_seed_of_path(v[0], v[1], v[2], v[3], v[4], (int32_t)vr, (int32_t)vc, row, col);
        printf("%d %d %d\n", usable ? 1 : 0, (int)row, (int)col);
    }
    fclose(f);
    return 0;
}

static int run_args(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        long long a[16];
        if (sscanf(line, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &a[0], &a[1], &a[2],
                   &a[3], &a[4], &a[5], &a[6], &a[7], &a[8], &a[9], &a[10], &a[11], &a[12], &a[13], &a[14], &a[15]) != 16) {
            fclose(f);
            return 3;
        }
        printf("%d\n", bcp::goal_bound_check_args(a[0] != 0, a[1] != 0, (int64_t)a[2], (int64_t)a[3], a[4] != 0, a[5] != 0,
                                                  (int32_t)a[6], (int32_t)a[7], a[8] != 0, a[9] != 0, a[10] != 0, a[11] != 0,
                                                  (int32_t)a[12], (int32_t)a[13], a[14] != 0, a[15] != 0));
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    int rc = 1;
    if (strcmp(argv[1], "seeds") == 0) rc = run_seeds(argv[2]);
    else if (strcmp(argv[1], "args") == 0) rc = run_args(argv[2]);
    if (rc == 0) printf("goal seed ok\n");
    return rc;
}

// The arithmetic of bcp_path_speed (csrc/bcp_speed_cell.h: speed_row, speed_curvature, speed_limit, speed_combine,
// speed_apply, speed_check_args, speed_lds_plan) on the host alone: the very functions speed_kernel calls, over case files
// that tests/test_speed_profile_host.py writes.  The header has no HIP in it; this program includes nothing else of the
// library and is built with -ffp-contract=off -fsanitize=address,undefined.  Every read of a way point goes through a
// bounds-checked accessor, and every row's way points, scratch plane and outputs live in heap blocks of exactly their sizes.
//
//   speed_profile_main row FILE OUT    FILE (binary, native endian):
//       int32 n_rows, max_len, span, 0
//       double v_max, v_min, a_lat, w_max, a_dec, a_acc, v_start, v_end
//       int32 lens[n_rows]
//       double paths[n_rows][max_len][3]
//     writes to OUT double speed[n_rows][max_len], kappa[..], v_limit[..] and int32 status[n_rows]: speed_row, the
//     recurrence that defines the value
//   speed_profile_main scan FILE OUT   the same FILE; writes double speed[n_rows][max_len] and int32 status[n_rows] with the
//     two passes run as speed_kernel runs them: trips of 64 lanes, six doubling steps of speed_combine per trip, a carry
//     across trips (the shuffles are array reads here)
//   speed_profile_main args FILE       FILE (text), per line: have_pointers have_params max_len n span v_max v_min a_lat w_max
//     a_dec a_acc v_start v_end overlap; prints speed_check_args' verdict and `which` per line
//   speed_profile_main layout          sizeof(SpeedParams) and the offsets of span, v_max, v_min, a_lat, w_max, a_dec, a_acc,
//     v_start, v_end; then the LDS plan (u_doubles bytes) of max_len 1, 400 and 4096; then two overlap verdicts
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bcp_speed_cell.h"
#include "host_io.h"

using namespace bcp;

struct RowIn {
    const double* p;
    int32_t m;
    double operator()(int32_t k, int32_t e) const
    {
        if (k < 0 || k >= m || e < 0 || e > 1) abort();
        return p[3 * k + e];
    }
};

struct Case {
    int32_t n_rows, max_len;
    SpeedParams prm;
    std::vector<int32_t> lens;
};

static bool read_head(FILE* f, Case& c)
{
    std::vector<int32_t> head;
    std::vector<double> nums;
    if (!read_n(f, head, 4) || !read_n(f, nums, 8)) return false;
    if (head[0] < 0 || head[1] < 1 || head[1] > kSpeedMaxLen) return false;
    c.n_rows = head[0];
    c.max_len = head[1];
    memset(&c.prm, 0, sizeof(c.prm));
    c.prm.span = head[2];
    c.prm.v_max = nums[0];
    c.prm.v_min = nums[1];
    c.prm.a_lat = nums[2];
    c.prm.w_max = nums[3];
    c.prm.a_dec = nums[4];
    c.prm.a_acc = nums[5];
    c.prm.v_start = nums[6];
    c.prm.v_end = nums[7];
    return read_n(f, c.lens, (size_t)c.n_rows);
}

// the two passes in the kernel's order over a plane u of m doubles that holds u_lim: -> u holds uf
static void scan_passes(const RowIn& in, int32_t m, const SpeedParams& prm, double* u)
{
    SpeedStep f[64];
    double carry = kSpeedInf;
    for (int32_t base = ((m - 1) >> 6) << 6; base >= 0; base -= 64) {
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t j = base + lane;
            f[lane].A = kSpeedInf;
            f[lane].c = 0.0;
            if (j < m) {
                f[lane].A = u[j];
                f[lane].c = j + 1 < m ? speed_gain(prm.a_dec, speed_ds(in, j)) : 0.0;
            }
        }
        for (int off = 1; off < 64; off <<= 1) {
            SpeedStep next[64];
            for (int lane = 0; lane < 64; ++lane) next[lane] = lane + off < 64 ? speed_combine(f[lane], f[lane + off]) : f[lane];
            memcpy(f, next, sizeof(f));
        }
        double first = 0.0;
        for (int lane = 0; lane < 64; ++lane) {
            const double ub = speed_apply(f[lane], carry);
            if (base + lane < m) u[base + lane] = ub;
            if (lane == 0) first = ub;
        }
        carry = first;
    }
    carry = kSpeedInf;
    for (int32_t base = 0; base < m; base += 64) {
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t j = base + lane;
            f[lane].A = kSpeedInf;
            f[lane].c = 0.0;
            if (j < m) {
                f[lane].A = u[j];
                f[lane].c = j > 0 ? speed_gain(prm.a_acc, speed_ds(in, j - 1)) : 0.0;
            }
        }
        for (int off = 1; off < 64; off <<= 1) {
            SpeedStep next[64];
            for (int lane = 0; lane < 64; ++lane) next[lane] = lane >= off ? speed_combine(f[lane], f[lane - off]) : f[lane];
            memcpy(f, next, sizeof(f));
        }
        double last = 0.0;
        for (int lane = 0; lane < 64; ++lane) {
            const double uf = speed_apply(f[lane], carry);
            if (base + lane < m) u[base + lane] = uf;
            if (lane == 63) last = uf;
        }
        carry = last;
    }
}

static int run_rows(const char* path, const char* out_path, bool as_scan)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    Case c;
    if (!read_head(f, c)) {
        fclose(f);
        return 3;
    }
    const int32_t max_len = c.max_len;
    std::vector<double> all_speed, all_kappa, all_limit;
    std::vector<int32_t> status;
    for (int32_t i = 0; i < c.n_rows; ++i) {
        bool read_ok = true;
        std::unique_ptr<double[]> row = read_block<double>(f, (size_t)max_len * 3, read_ok);
        if (!read_ok) {
            fclose(f);
            return 3;
        }
        const int32_t m = speed_row_len(c.lens[i], max_len);
        std::unique_ptr<double[]> mine(new double[(size_t)m * 3]);   // exactly the row's m way points
        memcpy(mine.get(), row.get(), sizeof(double) * (size_t)m * 3);
        const RowIn in = {mine.get(), m};
        std::unique_ptr<double[]> u(new double[(size_t)m]);
        std::unique_ptr<double[]> speed(new double[(size_t)max_len]), kappa(new double[(size_t)max_len]), limit(new double[(size_t)max_len]);
        for (int32_t j = 0; j < max_len; ++j) speed[j] = kappa[j] = limit[j] = -7.0;
        int32_t st = speed_row(in, c.lens[i], max_len, c.prm, u.get(), speed.get(), kappa.get(), limit.get());
        if (as_scan && st == 0) {
            for (int32_t j = 0; j < m; ++j) u[j] = speed_limit(kappa[j], j, m, c.prm);   // u_lim again: speed_row left uf
            scan_passes(in, m, c.prm, u.get());
            for (int32_t j = 0; j < m; ++j) speed[j] = std::sqrt(u[j]);
        }
        all_speed.insert(all_speed.end(), speed.get(), speed.get() + max_len);
        all_kappa.insert(all_kappa.end(), kappa.get(), kappa.get() + max_len);
        all_limit.insert(all_limit.end(), limit.get(), limit.get() + max_len);
        status.push_back(st);
    }
    fclose(f);
    FILE* o = fopen(out_path, "wb");
    if (!o) return 5;
    bool wrote = fwrite(all_speed.data(), sizeof(double), all_speed.size(), o) == all_speed.size();
    if (!as_scan) {
        wrote = wrote && fwrite(all_kappa.data(), sizeof(double), all_kappa.size(), o) == all_kappa.size();
        wrote = wrote && fwrite(all_limit.data(), sizeof(double), all_limit.size(), o) == all_limit.size();
    }
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
        int ptrs, prm, max_len, span, overlap;
        long long n;
        double v[8];
        if (sscanf(line, "%d %d %d %lld %d %lf %lf %lf %lf %lf %lf %lf %lf %d", &ptrs, &prm, &max_len, &n, &span, &v[0], &v[1], &v[2],
                   &v[3], &v[4], &v[5], &v[6], &v[7], &overlap) != 14) {
            fclose(f);
            return 3;
        }
        SpeedParams p;
        memset(&p, 0, sizeof(p));
        p.span = span;
        p.v_max = v[0];
        p.v_min = v[1];
        p.a_lat = v[2];
        p.w_max = v[3];
        p.a_dec = v[4];
        p.a_acc = v[5];
        p.v_start = v[6];
        p.v_end = v[7];
        int which = -1;
        const int rc = speed_check_args(ptrs != 0, prm != 0, max_len, n, p, overlap != 0, &which);
        printf("%d %d\n", rc, which);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 1;
    int rc = 1;
    if (strcmp(argv[1], "row") == 0 && argc == 4) rc = run_rows(argv[2], argv[3], false);
    else if (strcmp(argv[1], "scan") == 0 && argc == 4) rc = run_rows(argv[2], argv[3], true);
    else if (strcmp(argv[1], "args") == 0 && argc == 3) rc = run_args(argv[2]);
    else if (strcmp(argv[1], "layout") == 0) {
        printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(SpeedParams), (int)offsetof(SpeedParams, span), (int)offsetof(SpeedParams, v_max),
               (int)offsetof(SpeedParams, v_min), (int)offsetof(SpeedParams, a_lat), (int)offsetof(SpeedParams, w_max),
               (int)offsetof(SpeedParams, a_dec), (int)offsetof(SpeedParams, a_acc), (int)offsetof(SpeedParams, v_start),
               (int)offsetof(SpeedParams, v_end));
        for (int32_t max_len : {1, 400, 4096}) {
            const SpeedLdsPlan plan = speed_lds_plan(max_len);
            printf("%d %u\n", plan.u_doubles, plan.bytes);
        }
        printf("%d %d\n", speed_overlap(100, 10, 109, 4) ? 1 : 0, speed_overlap(100, 10, 110, 4) ? 1 : 0);
        rc = 0;
    }
    if (rc == 0) printf("speed profile ok\n");
    return rc;
}

// The law of bcp_track (csrc/bcp_track_law.h, the very functions track_kernel calls) as a stand-alone host program, built with
// AddressSanitizer and UBSan by tests/test_track_host.py (tests/host_program.py).  Files hold raw float64.
//   track_main dd2tri IN OUT   IN rows (v, w, wheel_angle, max_wheel_angle, L) -> OUT rows (wheel speed, angle)
//   track_main curv IN OUT     IN rows (lx, ly, max_curvature) -> OUT rows (kappa)
//   track_main law IN OUT      IN cases: 17 doubles (m, x, y, th, wheel_angle, target_idx, c_prev, speed, reach, max_curvature,
//                              tricycle, max_wheel_angle, L, low0, low1, high0, high1) and then m records of 5 doubles, which
//                              the program copies into a heap block of exactly m records -> OUT rows (carrot, cmd0, cmd1)
//   track_main checks          the refusals of track_check_args and their order, track_gains_ok, track_clip
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "bcp_track_law.h"

using namespace bcp;

// the host's side of the law's Math parameter: libm, and numpy's float `%` for normalize_angle
struct HostTrackMath {
    void cos_sin(double a, double& c, double& s) const
    {
        c = std::cos(a);
        s = std::sin(a);
    }
    double atan(double x) const { return std::atan(x); }
    double normalize(double z) const
    {
        const double pi = 3.14159265358979323846, b = 2.0 * pi;
        double r = std::fmod(z + pi, b);
        if (r != 0.0) {
            if (r < 0.0) r += b;
        } else {
            r = 0.0;
        }
        return r - pi;
    }
};

static std::vector<double> read_all(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<double> v((size_t)bytes / sizeof(double));
    if (!v.empty() && fread(v.data(), sizeof(double), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}

static void write_all(const char* path, const std::vector<double>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(double), v.size(), f) != v.size())) exit(2);
    fclose(f);
}

#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static int checks()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    EXPECT(track_gains_ok(0.0, 0.5) && track_gains_ok(1.0, 1e-300) && track_gains_ok(1.7976931348623157e308, 1.0));
    EXPECT(!track_gains_ok(-1e-300, 0.5) && !track_gains_ok(1.0, 0.0) && !track_gains_ok(1.0, -1.0));
    EXPECT(!track_gains_ok(nan, 0.5) && !track_gains_ok(1.0, nan) && !track_gains_ok(inf, 0.5) && !track_gains_ok(1.0, inf));
    EXPECT(!track_gains_ok(-inf, 0.5) && !track_gains_ok(1.0, -inf));
    EXPECT(track_clip(2.0, -1.0, 1.0) == 1.0 && track_clip(-2.0, -1.0, 1.0) == -1.0 && track_clip(0.25, -1.0, 1.0) == 0.25);
    EXPECT(track_clip(1.0, -1.0, 1.0) == 1.0 && track_clip(-1.0, -1.0, 1.0) == -1.0 && track_clip(0.5, 0.5, 0.5) == 0.5);
    const double lo[2] = {0.1, -1.5}, hi[2] = {0.5, 1.5};
    int d = -1;
    EXPECT(track_check_args(1, 1, 1.0, lo, hi, true, false, false, 1, &d) == kTrackOk);
    EXPECT(track_check_args(16, 64, 1e-300, lo, hi, true, true, true, 65536, &d) == kTrackOk);
    // every refusal, and an earlier one hides a later one
    EXPECT(track_check_args(0, 1, nan, lo, hi, false, false, true, 1, &d) == kTrackShape);
    EXPECT(track_check_args(1, 0, 1.0, lo, hi, true, false, false, 1, &d) == kTrackShape);
    EXPECT(track_check_args(-3, 4, 1.0, lo, hi, true, false, false, 1, &d) == kTrackShape);
    for (double bad : {0.0, -1.0, nan, inf, -inf}) EXPECT(track_check_args(1, 1, bad, hi, lo, false, false, true, 1, &d) == kTrackCurvature);
    for (int c = 0; c < 2; ++c) {
        for (double bad : {nan, inf, -inf}) {
            double l2[2] = {lo[0], lo[1]}, h2[2] = {hi[0], hi[1]};
            l2[c] = bad;
            EXPECT(track_check_args(1, 1, 1.0, l2, hi, false, false, true, 1, &d) == kTrackBoxFinite && d == c);
            h2[c] = bad;
            EXPECT(track_check_args(1, 1, 1.0, lo, h2, false, false, true, 1, &d) == kTrackBoxFinite && d == c);
        }
        double l2[2] = {lo[0], lo[1]};
        l2[c] = hi[c] + 1.0;
        EXPECT(track_check_args(1, 1, 1.0, l2, hi, false, false, true, 1, &d) == kTrackBoxOrder && d == c);
    }
    EXPECT(track_check_args(1, 1, 1.0, hi, hi, true, false, false, 1, &d) == kTrackOk);   // low == high is a box
    EXPECT(track_check_args(1, 1, 1.0, lo, hi, false, false, true, 1, &d) == kTrackNull);
    EXPECT(track_check_args(1, 1, 1.0, lo, hi, true, false, true, 1, &d) == kTrackBest);
    EXPECT(track_check_args(1, 1, 1.0, lo, hi, true, true, true, 1, &d) == kTrackOk);
    // 6 * N * K * H against 2^62
    EXPECT(track_check_args(2147483647, 2147483647, 1.0, lo, hi, true, false, false, 8, &d) == kTrackLarge);
    EXPECT(track_check_args(1024, 1024, 1.0, lo, hi, true, false, false, (int64_t)1 << 40, &d) == kTrackLarge);
    EXPECT(track_check_args(1024, 1024, 1.0, lo, hi, true, false, false, (int64_t)1 << 39, &d) == kTrackOk);
    return 0;
}

int main(int argc, char** argv)
{
    const HostTrackMath math;
    if (argc == 2 && !strcmp(argv[1], "checks")) {
        if (checks()) return 1;
    } else if (argc == 4 && !strcmp(argv[1], "dd2tri")) {
        const std::vector<double> in = read_all(argv[2]);
        std::vector<double> out;
        for (size_t r = 0; r + 5 <= in.size(); r += 5) {
            double fw, angle;
            track_diff_drive_to_tricycle(in[r], in[r + 1], in[r + 2], in[r + 3], in[r + 4], math, fw, angle);
            out.push_back(fw);
            out.push_back(angle);
        }
        write_all(argv[3], out);
    } else if (argc == 4 && !strcmp(argv[1], "curv")) {
        const std::vector<double> in = read_all(argv[2]);
        std::vector<double> out;
        for (size_t r = 0; r + 3 <= in.size(); r += 3) out.push_back(track_curvature(in[r], in[r + 1], in[r + 2]));
        write_all(argv[3], out);
    } else if (argc == 4 && !strcmp(argv[1], "law")) {
        const std::vector<double> in = read_all(argv[2]);
        std::vector<double> out;
        size_t at = 0;
        while (at + 17 <= in.size()) {
            const double* h = &in[at];
            const int m = (int)h[0];
            if (m < 1 || at + 17 + (size_t)m * kTrackPointStride > in.size()) return 3;
            double* pts = new double[(size_t)m * kTrackPointStride];   // exactly m records: a read past them is a sanitizer report
            memcpy(pts, h + 17, sizeof(double) * (size_t)m * kTrackPointStride);
            const double low[2] = {h[13], h[14]}, high[2] = {h[15], h[16]};
            const TrackCommand c = track_law((const double*)pts, m, h[1], h[2], h[3], h[4], (int)h[5], (int)h[6], h[7], h[8], h[9],
                                             h[10] != 0.0, h[11], h[12], low, high, math);
            delete[] pts;
            out.push_back((double)c.carrot);
            out.push_back(c.cmd0);
            out.push_back(c.cmd1);
            at += 17 + (size_t)m * kTrackPointStride;
        }
        if (at != in.size()) return 3;
        write_all(argv[3], out);
    } else {
        fprintf(stderr, "usage: track_main checks | dd2tri IN OUT | curv IN OUT | law IN OUT\n");
        return 2;
    }
    printf("track ok\n");
    return 0;
}

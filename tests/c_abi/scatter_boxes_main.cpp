// scatter_boxes_main.cpp -- the box sampler's rule on the host: includes csrc/bcp_boxes_cell.h alone (it has no HIP in it) and
// calls the very functions scatter_boxes_kernel calls.  Built with -fsanitize=address,undefined by
// tests/test_scatter_boxes_host.py; every array lives in a heap block of exactly its stated size and every cell is written
// through a sink that refuses a cell outside the entry's valid shape.
//   scatter_boxes_main scatter IN OUT   one batch: IN as _write_case lays it out, OUT = maps, boxes, counts
//   scatter_boxes_main args FILE        one line of scatter_check_args' 18 arguments per case -> the refusal's number
//   scatter_boxes_main philox           the two published vectors of Philox4x32-10
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bcp_boxes_cell.h"
#include "host_io.h"

using namespace bcp;

static void die(const char* what)
{
    fprintf(stderr, "scatter_boxes_main: %s\n", what);
    exit(2);
}

struct HostFill {
    uint8_t* plane;
    int32_t cols, vr, vc;
    bool span(int32_t r, int32_t ca, int32_t cb) const
    {
        if (r < 0 || r >= vr || ca < 0 || cb >= vc || ca > cb) die("a run leaves the valid shape");
        for (int32_t c = ca; c <= cb; ++c) plane[(size_t)r * cols + c] = kBoxLethal;
        return false;
    }
    bool pixel(int32_t r, int32_t c) const { return span(r, c, c); }
};

static int run_scatter(const char* in, const char* out)
{
    FILE* f = fopen(in, "rb");
    if (!f) die("cannot open the case");
    int32_t head[8];
    uint64_t words[2];   // seed, first entry
    double nums[5];      // resolution, t_lo, t_hi, h_lo, h_hi
    if (fread(head, sizeof(head), 1, f) != 1 || fread(words, sizeof(words), 1, f) != 1 || fread(nums, sizeof(nums), 1, f) != 1)
        die("short header");
    const int32_t n = head[0], rows = head[1], cols = head[2], n_keep = head[6];
    BoxRule R;
    R.n_boxes = head[3];
    R.max_attempts = head[4];
    R.n_yaws = head[5];
    R.seed_lo = (uint32_t)words[0];
    R.seed_hi = (uint32_t)(words[0] >> 32);
    R.t_lo = nums[1];
    R.t_hi = nums[2];
    R.h_lo = nums[3];
    R.h_hi = nums[4];
    if (scatter_check_args(true, true, n, rows, cols, nums[0], R.n_boxes, R.max_attempts, R.n_yaws, n_keep, R.t_lo, R.t_hi, R.h_lo,
                           R.h_hi, true, true, true, true) != kScatterOk)
        die("the case is one the library refuses");
    const double inv_res = 1.0 / nums[0];
    bool ok = true;
    auto valid = read_block<int32_t>(f, (size_t)n * 2, ok);
    auto origins = read_block<double>(f, (size_t)n * 2, ok);
    auto frame = read_block<double>(f, (size_t)n * 6, ok);
    auto keep = read_block<int32_t>(f, (size_t)n * n_keep * 3, ok);
    auto yaw_cs = read_block<double>(f, (size_t)R.n_yaws * 2, ok);
    const size_t cells = (size_t)rows * cols;
    auto data = read_block<uint8_t>(f, (size_t)n * cells, ok);
    fclose(f);
    if (!ok) die("short read");
    std::unique_ptr<int32_t[]> boxes(new int32_t[(size_t)n * R.n_boxes * kBoxWords]);
    std::unique_ptr<int32_t[]> counts(new int32_t[(size_t)n]);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t vr = box_clamp_valid(valid[2 * i], rows), vc = box_clamp_valid(valid[2 * i + 1], cols);
        HostFill fill = {data.get() + (size_t)i * cells, cols, vr, vc};
        // (the entry's keep-outs in a block of their own: a read past them is a read past the block)
        std::unique_ptr<int32_t[]> mine(new int32_t[(size_t)n_keep * 3]);
        if (n_keep) memcpy(mine.get(), keep.get() + (size_t)i * n_keep * 3, sizeof(int32_t) * n_keep * 3);
        counts[i] = scatter_entry(R, words[1] + (uint64_t)i, frame.get() + 6 * i, yaw_cs.get(), origins[2 * i], origins[2 * i + 1],
                                  inv_res, vr, vc, mine.get(), n_keep, fill, boxes.get() + (size_t)i * R.n_boxes * kBoxWords);
    }
    FILE* g = fopen(out, "wb");
    if (!g) die("cannot open the output");
    fwrite(data.get(), 1, (size_t)n * cells, g);
    fwrite(boxes.get(), sizeof(int32_t), (size_t)n * R.n_boxes * kBoxWords, g);
    fwrite(counts.get(), sizeof(int32_t), (size_t)n, g);
    fclose(g);
    return 0;
}

static int run_args(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) die("cannot open the cases");
    for (;;) {
        long long n_maps;
        int hh, hp, rows, cols, nb, na, ny, nk, vr, vc, arr, kp;
        double res, t0, t1, h0, h1;
        const int got = fscanf(f, "%d %d %lld %d %d %lf %d %d %d %d %lf %lf %lf %lf %d %d %d %d", &hh, &hp, &n_maps, &rows, &cols, &res,
                               &nb, &na, &ny, &nk, &t0, &t1, &h0, &h1, &vr, &vc, &arr, &kp);
        if (got != 18) break;
        printf("%d\n", scatter_check_args(hh != 0, hp != 0, n_maps, rows, cols, res, nb, na, ny, nk, t0, t1, h0, h1, vr != 0, vc != 0,
                                          arr != 0, kp != 0));
    }
    fclose(f);
    return 0;
}

static int run_philox()
{
    uint32_t zero[4] = {0u, 0u, 0u, 0u}, ones[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    philox4x32_10(zero, 0u, 0u);
    philox4x32_10(ones, 0xFFFFFFFFu, 0xFFFFFFFFu);
    printf("%08x %08x %08x %08x\n", zero[0], zero[1], zero[2], zero[3]);
    printf("%08x %08x %08x %08x\n", ones[0], ones[1], ones[2], ones[3]);
    return 0;
}

int main(int argc, char** argv)
{
    int rc = 2;
    if (argc == 4 && !strcmp(argv[1], "scatter")) rc = run_scatter(argv[2], argv[3]);
    else if (argc == 3 && !strcmp(argv[1], "args")) rc = run_args(argv[2]);
    else if (argc == 2 && !strcmp(argv[1], "philox")) rc = run_philox();
    else die("usage: scatter IN OUT | args FILE | philox");
    if (rc == 0) printf("scatter boxes ok\n");
    return rc;
}

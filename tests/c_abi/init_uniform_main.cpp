// The host half of bcp_declare_uniform_initial_state: init_uniform_pack of csrc/bcp_init_uniform.h as the entry point calls it, in
// a program of its own for AddressSanitizer and UBSan (tests/test_init_uniform_host.py).  The header has no HIP in it.
//   init_uniform_main FILE...   each FILE: int64 n, int32 tri, int32 0, then the eleven arrays x .. robot_collided as the library
//                               holds them on the host (eight float64 [n], two int32 [n], one uint8 [n])
//                               -> per file one line "env field name" (-1 -1 - : uniform) and the 80 bytes of the snapshot in hex
// Every array is a heap block of exactly n entries; with tri = 0 the two tricycle arrays are handed over as null pointers, so a
// function that read them would fault here.  Ends with "init uniform ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bcp_init_uniform.h"
#include "host_io.h"

static int run(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    int64_t n = 0;
    int32_t head[2] = {0, 0};
    if (fread(&n, sizeof(n), 1, f) != 1 || fread(head, sizeof(int32_t), 2, f) != 2 || n < 1 || n > (1 << 24)) {
        fclose(f);
        return 3;
    }
    const bool tri = head[0] != 0;
    bool ok = true;
    std::unique_ptr<double[]> f64[8];
    for (int k = 0; k < 8; ++k) f64[k] = read_block<double>(f, (size_t)n, ok);
    std::unique_ptr<int32_t[]> target = read_block<int32_t>(f, (size_t)n, ok), iter = read_block<int32_t>(f, (size_t)n, ok);
    std::unique_ptr<uint8_t[]> collided = read_block<uint8_t>(f, (size_t)n, ok);
    fclose(f);
    if (!ok) return 3;
    bcp::InitHostArrays a = {};
    for (int k = 0; k < 8; ++k) {
        const bool tricycle_only = k == bcp::kInitSteer || k == bcp::kInitWheel;
        a.f64[k] = (tricycle_only && !tri) ? nullptr : f64[k].get();
    }
    a.target = target.get();
    a.iter = iter.get();
    a.collided = collided.get();
    std::unique_ptr<bcp::InitUniform> snap(new bcp::InitUniform);
    memset(snap.get(), 0xA5, sizeof(bcp::InitUniform));   // (a byte the function leaves alone would show)
    const bcp::InitDifference d = bcp::init_uniform_pack(a, n, tri, snap.get());
    printf("%lld %d %s ", (long long)d.env, d.field, d.env >= 0 ? bcp::init_field_name(d.field) : "-");
    const unsigned char* raw = (const unsigned char*)snap.get();
    for (size_t k = 0; k < sizeof(bcp::InitUniform); ++k) printf("%02x", raw[k]);
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 1;
    for (int k = 1; k < argc; ++k) {
        const int rc = run(argv[k]);
        if (rc != 0) {
            fprintf(stderr, "init_uniform_main: %s: error %d\n", argv[k], rc);
            return rc;
        }
    }
    printf("init uniform ok\n");
    return 0;
}

// What the stand-alone host programs of this directory share, each written once: the bounds-checked read of a uint16
// plane, the reads of a case file into heap blocks of exactly their size (so AddressSanitizer sees every step beyond one),
// numpy's angle normalisation, and the counting CHECK.  Everything is inline or a template: a program that uses a part of
// it builds under -Wall -Werror.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

// get(r, c) of a plane [.][cols], allowed inside [0, ok_rows) x [0, ok_cols) alone: the plane's shape, or the valid shape
// where a function must not read beyond it.  (The index alone could wrap into the plane.)
struct HostPlane {
    const std::vector<uint16_t>* cells;
    int32_t cols, ok_rows, ok_cols;
    uint16_t operator()(int32_t r, int32_t c) const
    {
        if (r < 0 || r >= ok_rows || c < 0 || c >= ok_cols) abort();
        return cells->at((size_t)r * cols + c);
    }
};

// numpy's (z + pi) % (2 pi) - pi: the remainder takes the divisor's sign
struct HostNormalizeAngle {
    double operator()(double z) const
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

// n elements into a vector whose heap block holds exactly n
template <typename T>
bool read_n(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    v.shrink_to_fit();
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// n elements into a block of their own; a short read clears `ok`
template <typename T>
std::unique_ptr<T[]> read_block(FILE* f, size_t n, bool& ok)
{
    std::unique_ptr<T[]> p(new T[n]);
    if (n && fread(p.get(), sizeof(T), n, f) != n) ok = false;
    return p;
}

// CHECK(cond): says where it does not hold (g_where: the case at hand, if the program names one) and counts
inline int g_failed = 0;
inline char g_where[128] = "";
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "line %d (%s): %s does not hold\n", __LINE__, g_where, #cond); \
            ++g_failed;                                                                      \
        }                                                                                    \
    } while (0)

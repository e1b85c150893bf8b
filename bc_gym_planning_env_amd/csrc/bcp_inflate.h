// bcp_inflate.h -- costmap inflation (utilities/costmap_inflation.py:47-92): an exact Euclidean distance transform of the
// lethal cells followed by the ROS inflation cost law, for many maps in one launch.
//
// Reference semantics, per map `data` [rows][cols] with valid shape (vr, vc):
//   obstacle(r, c)  =  data[r][c] == 254, r < vr, c < vc          (:83: 254 - data wraps; the distance is to a zero pixel)
//   d2(r, c)        =  min over obstacles (r', c') of (r - r')^2 + (c - c')^2, an integer, never clamped
//   d               =  (float32) sqrt(d2), correctly rounded        (cv2.distanceTransform, DIST_L2, DIST_MASK_PRECISE)
//   cost            =  254 if d < pir / 1000, else 253 if d <= pir, else (uint8) trunc(252 exp(-psf (d - pir)))   (:56-69)
// with pir = inscribed_radius / resolution and psf = cost_scaling_factor * resolution, all of it float64 arithmetic on the
// float32 d (the inscribed radius is a float64 scalar, so numpy promotes).  No obstacle: d = +inf, cost 0.  Outside the
// valid shape: nothing is read, cost 0 and d 0 are written.
//
// One workgroup per map, five phases with a barrier between them:
//   0  clear the 1-bit obstacle mask of the map (LDS, [rows][wpr])
//   1  read the map ONCE, four cells per aligned dword; the rare lethal byte sets its bit with an LDS atomic.  After this
//      phase nothing reads the map again, which is what makes out == data safe
//   2  wave 0 lists the rows that hold an obstacle (ballot + running count): `list` [n_list], and per row r `pos[r]` = number
//      of listed rows above r.  Rows without an obstacle cost nothing from here on
//   3  g(r', c) = distance along row r' to its nearest obstacle, for the listed rows only, from the mask with clz / ctz; a
//      wave per row, a lane per cell; 16-bit plane [rows][cols]
//   4  d2(r, c) = min over listed rows r' of (r - r')^2 + g(r', c)^2, walking the list from row r outwards in both directions
//      and abandoning a direction once (r - r')^2 alone reaches the best value; cost law; four cells per thread packed into
//      one aligned dword store of `out` (single bytes at the map's ragged ends)
// The two 1-D passes are the separable form of the exact transform (min over r' of min over c'), so d2 is exact.
// The plane lives in LDS when the map fits (InflateLds) and in a slice of handle-owned global scratch per workgroup
// otherwise (InflateGlobal); the code is the same template, so the bytes are the same.
#pragma once

#include "bcp_device.h"

namespace bcp {

typedef __attribute__((address_space(3))) uint16_t* InflateLdsU16;

struct InflateArgs {
    const uint8_t* data;        // [n_maps][rows][cols]
    uint8_t* out;               // [n_maps][rows][cols], may be `data`
    float* dist;                // optional [n_maps][rows][cols]
    const int32_t* valid_rows;  // optional [n_maps], with valid_cols
    const int32_t* valid_cols;
    int64_t n_maps;
    int32_t rows, cols, wpr;    // wpr = ceil(cols / 32)
    double pir, lethal_below, psf;   // pir, pir / 1000.0, psf
    uint16_t* scratch;          // InflateGlobal: [gridDim.x][rows][cols]
};

constexpr int kInflateFar = 0x7FFF;                       // g of "no obstacle": its square exceeds every real d2 (< 2^24)
constexpr int kInflateNone = kInflateFar * kInflateFar;   // d2 of a map without obstacles

// _pixel_distance_to_cost (:47-70) for one cell.  252 exp(-x) < 1 for x > ln 252 = 5.53: beyond 6 the truncated value is 0
// whatever the last bits of exp() are, and the far field skips the exponential.
__device__ __forceinline__ uint32_t inflate_cost(float d, const InflateArgs& a)
{
    const double dd = (double)d;
    if (dd < a.lethal_below) return 254u;
    if (dd <= a.pir) return 253u;
    const double x = a.psf * (dd - a.pir);   // (-psf) * (d - pir) == -(psf * (d - pir)), exactly
    if (x > 6.0) return 0u;
    return (uint32_t)(int)(252.0 * exp(-x));
}

// distance along a listed row to its nearest obstacle bit (the row holds at least one)
__device__ __forceinline__ int inflate_row_distance(LdsWords row, int wpr, int c)
{
    const int w = c >> 5, b = c & 31;
    int best = kInflateFar;
    uint32_t x = row[w] >> b;   // bit 0 = column c
    if (x) {
        best = __builtin_ctz(x);
    } else {
        for (int k = w + 1; k < wpr; ++k) {
            x = row[k];
            if (x) {
                best = k * 32 + __builtin_ctz(x) - c;
                break;
            }
        }
    }
    x = row[w] << (31 - b);     // bit 31 = column c
    if (x) {
        best = min(best, (int)__builtin_clz(x));
    } else {
        for (int k = w - 1; k >= 0; --k) {
            x = row[k];
            if (x) {
                best = min(best, c - (k * 32 + 31 - (int)__builtin_clz(x)));
                break;
            }
        }
    }
    return best;
}

template <typename Plane>
__device__ __forceinline__ int inflate_d2(Plane plane, InflateLdsU16 list, int n_list, int first_below, int r, int c, int cols)
{
    int best = kInflateNone;
    int dn = first_below, up = first_below - 1;
    while (dn < n_list || up >= 0) {
        if (dn < n_list) {
            const int rr = list[dn], dy = rr - r;
            if (dy * dy < best) {
                const int g = plane[rr * cols + c];
                best = min(best, dy * dy + g * g);
                ++dn;
            } else {
                dn = n_list;
            }
        }
        if (up >= 0) {
            const int rr = list[up], dy = r - rr;
            if (dy * dy < best) {
                const int g = plane[rr * cols + c];
                best = min(best, dy * dy + g * g);
                --up;
            } else {
                up = -1;
            }
        }
    }
    return best;
}

// LDS words of the kernel apart from the plane: mask, list, pos (16-bit each, rounded up to words), n_list
__host__ __device__ inline int inflate_fixed_words(int rows, int wpr) { return rows * wpr + 2 * ((rows + 1) / 2) + 1; }

template <bool kPlaneInLds>
__global__ void __launch_bounds__(1024) inflate_kernel(InflateArgs a)
{
    const int rows = a.rows, cols = a.cols, wpr = a.wpr, cells = rows * cols;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const LdsU32 bits = (LdsU32)lds_dyn;                               // [rows][wpr]
    const InflateLdsU16 list = (InflateLdsU16)(bits + rows * wpr);     // [rows] rows with an obstacle, ascending
    const InflateLdsU16 pos = list + 2 * ((rows + 1) / 2);             // [rows] listed rows above row r
    const LdsU32 n_list_word = (LdsU32)(pos + 2 * ((rows + 1) / 2));
    const InflateLdsU16 plane_lds = (InflateLdsU16)(n_list_word + 1);  // [rows][cols] when it fits
    uint16_t* const plane_glb = kPlaneInLds ? nullptr : a.scratch + (int64_t)blockIdx.x * cells;

    for (int64_t m = blockIdx.x; m < a.n_maps; m += gridDim.x) {
        int vr = rows, vc = cols;
        if (a.valid_rows) {
            vr = min(max(a.valid_rows[m], 0), rows);
            vc = min(max(a.valid_cols[m], 0), cols);
        }
        // ---- 0: clear the mask (the previous map's phase 4 does not read it)
        for (int i = tid; i < rows * wpr; i += nthr) bits[i] = 0u;
        __syncthreads();
        // ---- 1: the map, once.  Dword j of the aligned run that covers the map holds cells 4 j - head .. 4 j - head + 3
        {
            const uint8_t* src = a.data + m * (int64_t)cells;
            const int head = (int)((uintptr_t)src & 3u);
            const uint32_t* words = reinterpret_cast<const uint32_t*>(src - head);
            const int n_words = (cells + head + 3) >> 2;
            for (int j = tid; j < n_words; j += nthr) {
                const uint32_t y = words[j] ^ 0xFEFEFEFEu;   // a zero byte = a lethal cell
                if (((y - 0x01010101u) & ~y & 0x80808080u) == 0u) continue;
                for (int b = 0; b < 4; ++b) {
                    const int p = 4 * j - head + b;          // (bytes before and after the map belong to others: skipped)
                    if (((y >> (8 * b)) & 255u) != 0u || p < 0 || p >= cells) continue;
                    const int r = p / cols, c = p - r * cols;
                    if (r < vr && c < vc)
                        __hip_atomic_fetch_or(bits + r * wpr + (c >> 5), 1u << (c & 31), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // ---- 2: the rows that hold an obstacle
        if (tid < 64) {
            int count = 0;
            for (int base = 0; base < rows; base += 64) {
                const int r = base + tid;
                uint32_t any = 0u;
                if (r < rows)
                    for (int k = 0; k < wpr; ++k) any |= bits[r * wpr + k];
                const uint64_t mask = __ballot(any != 0u);
                const int before = count + (int)__popcll(mask & ((1ull << tid) - 1ull));
                if (r < rows) pos[r] = (uint16_t)before;
                if (any) list[before] = (uint16_t)r;
                count += (int)__popcll(mask);
            }
            if (tid == 0) *n_list_word = (uint32_t)count;
        }
        __syncthreads();
        const int n_list = (int)*n_list_word;
        // ---- 3: g of the listed rows
        for (int li = tid >> 6; li < n_list; li += nthr >> 6) {
            const int r = list[li];
            const LdsWords row = (LdsWords)(bits + r * wpr);
            for (int c = tid & 63; c < cols; c += 64) {
                const uint16_t g = (uint16_t)inflate_row_distance(row, wpr, c);
                if (kPlaneInLds) plane_lds[r * cols + c] = g;
                else plane_glb[r * cols + c] = g;
            }
        }
        __syncthreads();
        // ---- 4: d2, cost, store
        {
            uint8_t* dst = a.out + m * (int64_t)cells;
            float* dist = a.dist ? a.dist + m * (int64_t)cells : nullptr;
            const int head = (int)((uintptr_t)dst & 3u);
            uint32_t* words = reinterpret_cast<uint32_t*>(dst - head);
            const int n_words = (cells + head + 3) >> 2;
            for (int j = tid; j < n_words; j += nthr) {
                const int p0 = 4 * j - head;
                int r = p0 >= 0 ? p0 / cols : 0, c = p0 >= 0 ? p0 - r * cols : p0;   // (p0 < 0: c < 0 until the map begins)
                uint32_t packed = 0u;
                for (int b = 0; b < 4; ++b) {
                    const int p = p0 + b;
                    if (p >= 0 && p < cells) {
                        uint32_t cost = 0u;
                        float d = 0.0f;
                        if (r < vr && c < vc) {
                            const int d2 = kPlaneInLds ? inflate_d2(plane_lds, list, n_list, (int)pos[r], r, c, cols)
                                                       : inflate_d2(plane_glb, list, n_list, (int)pos[r], r, c, cols);
                            // d2 < 2^24: the float holds it exactly, and the double root rounds to the correctly rounded float
                            d = d2 == kInflateNone ? __builtin_huge_valf() : (float)sqrt((double)d2);
                            cost = inflate_cost(d, a);
                        }
                        packed |= cost << (8 * b);
                        if (dist) dist[p] = d;
                    }
                    if (++c == cols) {
                        c = 0;
                        ++r;
                    }
                }
                if (p0 >= 0 && p0 + 3 < cells) {
                    words[j] = packed;
                } else {
                    for (int b = 0; b < 4; ++b)
                        if (p0 + b >= 0 && p0 + b < cells) dst[p0 + b] = (uint8_t)(packed >> (8 * b));
                }
            }
        }
        // (no barrier here: phases 0 and 1 of the next map write the mask only, which phase 4 does not read, and the
        //  barrier after phase 1 keeps list, pos and the plane intact until every thread has left phase 4)
    }
}

}  // namespace bcp

// bcp_bind_kernels.h -- the kernels that derive data from costmaps and paths when they are bound (or a pool is topped up):
// the lethal bitmap, the way points with cos / sin, the 128-byte path records and the bucket tables.  They step nothing.
#pragma once

#include "bcp_step_args.h"

// Which entries of a non-shared array (costmaps, paths, ...) a set-up kernel derives data for: all n of them, or the
// *count entries listed in `list` (both on the device: a pool that is topped up between steps, bcp_refresh_mini_worlds).
// The kernels walk `size() * units-per-entry` work items in a grid-stride loop, so their grids never depend on *count.
struct EntrySelect {
    const int32_t* list;
    const int32_t* count;
    int64_t n;
    __device__ __forceinline__ int64_t size() const { return list ? (int64_t)*count : n; }
    __device__ __forceinline__ int64_t entry(int64_t k) const { return list ? (int64_t)list[k] : k; }
};

// uint8 costmap -> 1-bit lethal mask.  One thread per 32-bit output word.
// (tiles: the same words once more in tiles of 32 x 32 cells, map_tile_words() per entry -- see CoopCollisionSink)
__host__ __device__ __forceinline__ int64_t map_tile_words(int rows, int wpr) { return (int64_t)((rows + 31) & ~31) * wpr; }

__global__ void pack_bitmap_kernel(const uint8_t* __restrict__ data, uint32_t* __restrict__ bits, uint32_t* __restrict__ tiles,
                                   EntrySelect sel, int rows, int cols, int wpr, const int32_t* __restrict__ valid_rows,
                                   const int32_t* __restrict__ valid_cols)
{
    const int64_t total = sel.size() * rows * wpr;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        const int w = (int)(it % wpr);
        const int64_t t = it / wpr;
        const int r = (int)(t % rows);
        const int64_t m = sel.entry(t / rows);
        const int64_t idx = (m * rows + r) * wpr + w;
        const int vr = valid_rows ? valid_rows[m] : rows;
        const int vc = valid_cols ? valid_cols[m] : cols;
        uint32_t word = 0;
        if (r < vr) {
            const uint8_t* src = data + (m * rows + r) * (int64_t)cols + (int64_t)w * 32;
            const int lim = min(32, vc - w * 32);
            if (lim == 32) {
                // the 32 cells as four 8-byte loads (any alignment: the rows of a 183-column map start anywhere) instead of 32
                // byte loads -- the kernel was bound by its load instructions, not by bytes (a pool refresh: 0.11 - 0.4 ms of
                // this kernel for ~7000 maps) --; "byte == LETHAL" for eight bytes at once: the exact zero-byte test of
                // x ^ LETHAL.., then the eight flags gathered into a byte by a multiplication
                typedef uint64_t __attribute__((aligned(1))) PackU64Unaligned;
                constexpr uint64_t kOnes = 0x0101010101010101ull, kLow7 = 0x7F7F7F7F7F7F7F7Full;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint64_t t = reinterpret_cast<const PackU64Unaligned*>(src)[q] ^ ((uint64_t)BCP_LETHAL * kOnes);
                    const uint64_t hit = ~((((t & kLow7) + kLow7) | t) | kLow7);   // 0x80 in every byte of t that is zero
                    word |= (uint32_t)(((hit >> 7) * 0x0102040810204080ull) >> 56) << (8 * q);
                }
            } else {
                for (int b = 0; b < lim; ++b) word |= (uint32_t)(src[b] == BCP_LETHAL) << b;
            }
        }
        bits[idx] = word;
        if (tiles) tiles[m * map_tile_words(rows, wpr) + (((r >> 5) * wpr + w) << 5) + (r & 31)] = word;
    }
}

constexpr int kPathBuckets = 64;          // buckets per axis of a shared path's tables (PathDesc::index, staged in LDS)
constexpr int kPathBucketsCompact = 16;   // ... of a private path's, which live inside its record
// One 128-byte record per path entry -- ONE line of memory: a load that misses L2 fetches the whole line whatever it asks
// for (tools/sector_probe.hip: 128 bytes per lone 4-byte read, and no more for a second word 32 or 64 bytes further), so
// every small per-entry array an env reads from costs it a line per step.  With private paths all of them share this one:
//   floats  [0..3]    xmin, xmax, ymin, ymax of the way points, rounded OUTWARD to f32 (the box only ever prunes: a wider one
//                     hands a few more poses to the bucket tables, whose windows the exact test then walks)
//   floats  [4..7]    the bucket grid x0, 1/wx, y0, 1/wy, as f32 (the tables are built from these very values, below, so a
//                     look-up and the table it reads agree whatever their rounding)
//   doubles [4],[5]   origin of the entry's costmap (world_record_kernel)
//   int32   [12],[13] number of way points; shift of the compact tables' indices (0 unless the paths have > 255 way points)
//   floats  [14],[15] step of the quantised prefilter records (path_trig_kernel) and its reciprocal
//   bytes   [64..127] private paths: the bucket tables, [2 axes][kPathBucketsCompact] {first, last} >> shift as uint8
//                     (path_index_compact_kernel); until round 4 [2][64] int16 pairs in an array of their own, two lines per step
// (rounds 2-3: 128 bytes in two halves -- box and grid as doubles, origin and length -- beside 512 bytes of tables)
constexpr int kBoxDoubles = 16;
constexpr int kBoxOrigin = 4;
constexpr int kBoxLenWord = 12;      // (int32 index; [13]: the index shift)
constexpr int kBoxQuantStep = 14;    // (float index)
constexpr int kBoxIndexU16 = 32;     // (uint16 index of the compact tables: {first | last << 8} per bucket)
constexpr int kQuantSteps = 65000;   // the longer side of the box in steps (uint16 coordinates)
constexpr int kQuantReach = 16384;   // spatial precision in steps, at most: poses the window lets through stay below 2^17 steps

// path [.,3] -> [.,5] with cos/sin of the heading (utilities/path_tools.py:405)
// (pre: the quantised prefilter record of private paths, last_reached_prefiltered -- needs the entry's record, `bbox`,
//  which path_bbox_kernel writes: launched behind it)
__global__ void path_trig_kernel(const double* __restrict__ xyt, double* __restrict__ out, uint32_t* __restrict__ pre,
                                 const double* __restrict__ bbox, EntrySelect sel, int max_len)
{
    const int64_t total = sel.size() * max_len;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = sel.entry(it / max_len) * max_len + it % max_len;
        const double th = xyt[3 * i + 2];
        out[5 * i + 0] = xyt[3 * i + 0];
        out[5 * i + 1] = xyt[3 * i + 1];
        out[5 * i + 2] = th;
        const double c = cos(th), sn = sin(th);
        out[5 * i + 3] = c;
        out[5 * i + 4] = sn;
        if (pre) {
            const float* rec = reinterpret_cast<const float*>(bbox + (i / max_len) * kBoxDoubles);
            const double ox = (double)rec[0], oy = (double)rec[2], step = (double)rec[kBoxQuantStep];
            const uint32_t qx = (uint32_t)fmin(fmax(rint((xyt[3 * i + 0] - ox) / step), 0.0), 65535.0);
            const uint32_t qy = (uint32_t)fmin(fmax(rint((xyt[3 * i + 1] - oy) / step), 0.0), 65535.0);
            const int32_t qc = (int32_t)rint(c * 32767.0), qs = (int32_t)rint(sn * 32767.0);
            pre[2 * i + 0] = qx | (qy << 16);
            pre[2 * i + 1] = ((uint32_t)qc & 0xFFFFu) | ((uint32_t)qs << 16);
        }
    }
}

__device__ __forceinline__ float f32_below(double v)
{
    float f = (float)v;
    return (double)f > v ? nextafterf(f, -INFINITY) : f;
}

__device__ __forceinline__ float f32_above(double v)
{
    float f = (float)v;
    return (double)f < v ? nextafterf(f, INFINITY) : f;
}

// Per path: bounding box of the way points and a 1-D grid of `buckets` buckets per axis over [min - sp, max + sp].
__device__ __forceinline__ void path_bbox_one(const double* __restrict__ xyt, const int32_t* __restrict__ lens, int max_len,
                                              int64_t p, double sp_prune, int buckets, double* __restrict__ bbox)
{
    const int m = lens ? lens[p] : max_len;
    const double* q = xyt + p * (int64_t)max_len * 3;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int j = 0; j < m; ++j) {
        x0 = fmin(x0, q[3 * j]);
        x1 = fmax(x1, q[3 * j]);
        y0 = fmin(y0, q[3 * j + 1]);
        y1 = fmax(y1, q[3 * j + 1]);
    }
    float* o = reinterpret_cast<float*>(bbox + kBoxDoubles * p);
    o[0] = f32_below(x0);
    o[1] = f32_above(x1);
    o[2] = f32_below(y0);
    o[3] = f32_above(y1);
    const double wx = fmax((x1 - x0 + 2.0 * sp_prune) / buckets, 1e-9);
    const double wy = fmax((y1 - y0 + 2.0 * sp_prune) / buckets, 1e-9);
    o[4] = (float)(x0 - sp_prune);
    o[5] = (float)(1.0 / wx);
    o[6] = (float)(y0 - sp_prune);
    o[7] = (float)(1.0 / wy);
    // prefilter records: way points as uint16 steps from the (rounded-down) lower corner of the box
    double extent = fmax(x1 - (double)o[0], y1 - (double)o[2]);
    if (!(extent >= 0.0) || extent > 3e38) extent = 0.0;   // (no way points)
    const float step = (float)fmax(extent / kQuantSteps, sp_prune / kQuantReach);
    o[kBoxQuantStep] = step;
    o[kBoxQuantStep + 1] = 1.0f / step;
    int shift = 0;
    while (((max_len - 1) >> shift) > 254) ++shift;   // (255 marks an empty bucket)
    reinterpret_cast<int32_t*>(o)[kBoxLenWord] = m;
    reinterpret_cast<int32_t*>(o)[kBoxLenWord + 1] = shift;
}

__global__ void path_bbox_kernel(const double* __restrict__ xyt, const int32_t* __restrict__ lens, int max_len,
                                 EntrySelect sel, double sp_prune, int buckets, double* __restrict__ bbox)
{
    const int64_t total = sel.size();
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x)
        path_bbox_one(xyt, lens, max_len, sel.entry(it), sp_prune, buckets, bbox);
}

// the rest of a path entry's record: origin of the entry's costmap (or of the shared one)
__global__ void world_record_kernel(EntrySelect sel, const double* __restrict__ origins, double ox, double oy,
                                    double* __restrict__ bbox)
{
    const int64_t total = sel.size();
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = sel.entry(it);
        double* o = bbox + kBoxDoubles * p;
        o[kBoxOrigin] = origins ? origins[2 * p] : ox;
        o[kBoxOrigin + 1] = origins ? origins[2 * p + 1] : oy;
    }
}

// index[p][axis][b] = {first, last} way point whose coordinate lies within sp of bucket b (widened by a guard band
// that swallows the rounding of the bucket computation); {32767, -1} when there is none.  Any way point with
// |x_j - x| <= sp_prune for a query x that falls into bucket b is inside [first, last].
__device__ __forceinline__ void path_index_one(const double* __restrict__ xyt, const int32_t* __restrict__ lens, int max_len,
                                               int64_t t, double sp_prune, const double* __restrict__ bbox,
                                               int16_t* __restrict__ index)
{
    const int b = (int)(t % kPathBuckets);
    const int axis = (int)((t / kPathBuckets) % 2);
    const int64_t p = t / (2 * kPathBuckets);
    const int m = lens ? lens[p] : max_len;
    const double* q = xyt + p * (int64_t)max_len * 3;
    const float* grid = reinterpret_cast<const float*>(bbox + kBoxDoubles * p) + 4;
    const double o = (double)grid[2 * axis], w = 1.0 / (double)grid[2 * axis + 1];
    const double guard = 1e-6 * w + 1e-12;
    const double lo = o + b * w - sp_prune - guard, hi = o + (b + 1) * w + sp_prune + guard;
    int first = 32767, last = -1;
    for (int j = 0; j < m; ++j) {
        const double v = q[3 * j + axis];
        if (v >= lo && v <= hi) {
            first = min(first, j);
            last = j;
        }
    }
    index[2 * t] = (int16_t)first;
    index[2 * t + 1] = (int16_t)last;
}

__global__ void path_index_kernel(const double* __restrict__ xyt, const int32_t* __restrict__ lens, int max_len,
                                  EntrySelect sel, double sp_prune, const double* __restrict__ bbox,
                                  int16_t* __restrict__ index)
{
    const int64_t total = sel.size() * 2 * kPathBuckets;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x)
        path_index_one(xyt, lens, max_len, sel.entry(it / (2 * kPathBuckets)) * (2 * kPathBuckets) + it % (2 * kPathBuckets),
                       sp_prune, bbox, index);
}

// The same tables for a private path, inside its record: kPathBucketsCompact buckets per axis, {first, last} >> shift as
// uint8 ({255, 0} when there is none).  One thread per bucket.
__global__ void path_index_compact_kernel(const double* __restrict__ xyt, const int32_t* __restrict__ lens, int max_len,
                                          EntrySelect sel, double sp_prune, double* __restrict__ bbox)
{
    const int64_t total = sel.size() * 2 * kPathBucketsCompact;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(it % kPathBucketsCompact), axis = (int)((it / kPathBucketsCompact) % 2);
        const int64_t p = sel.entry(it / (2 * kPathBucketsCompact));
        const int m = lens ? lens[p] : max_len;
        const double* q = xyt + p * (int64_t)max_len * 3;
        const float* rec = reinterpret_cast<const float*>(bbox + kBoxDoubles * p);
        const int shift = reinterpret_cast<const int32_t*>(rec)[kBoxLenWord + 1];
        const double o = (double)rec[4 + 2 * axis], w = 1.0 / (double)rec[5 + 2 * axis];
        const double guard = 1e-6 * w + 1e-12;
        const double lo = o + b * w - sp_prune - guard, hi = o + (b + 1) * w + sp_prune + guard;
        int first = -1, last = -1;
        for (int j = 0; j < m; ++j) {
            const double v = q[3 * j + axis];
            if (v >= lo && v <= hi) {
                if (first < 0) first = j;
                last = j;
            }
        }
        const uint32_t packed = first < 0 ? 255u : (uint32_t)(first >> shift) | ((uint32_t)(last >> shift) << 8);
        reinterpret_cast<uint16_t*>(bbox + kBoxDoubles * p)[kBoxIndexU16 + axis * kPathBucketsCompact + b] = (uint16_t)packed;
    }
}

// bcp_scan.h -- range_scan_kernel: the range observation of bcp_range_scan (include/bcplan.h), one lane per ray.
// The walk itself is scan_march of bcp_scan_march.h, which has no HIP in it and which the host tests run as it stands; this
// file only decides who walks which ray and where the words of the lethal mask come from.
//
// Rays are numbered row-major, ray f = row * n_beams + beam, and a workgroup takes 256 consecutive rays at a time: the
// stores of `ranges` and `hit` are one contiguous run per workgroup whatever the beam count.  What depends on the row alone
// -- (cos, sin) of the heading, the pose in cell units, the entry's words, its valid shape -- is computed once per row by the
// first lanes of the workgroup and handed to the row's rays through LDS (a chunk of 256 rays touches at most 256 rows).
// "Once per row" holds per chunk: a row whose beams straddle a chunk boundary is set up by every chunk that touches it (twice
// at 64 beams where the rows do not divide the chunks, up to five times at 1 024 beams), each time with the same values, and
// its heading_cs_out is stored as often, with the same bytes.
// The shared map's mask is staged in LDS when MapDesc::in_lds; private maps and pool entries are read through the cache.
#pragma once

#include "bcp_scan_march.h"

using namespace bcp;

constexpr int kScanBlock = 256;

struct ScanArgs {
    MapDesc map;
    const int32_t* valid_rows;   // per entry, or nullptr: the allocated shape
    const int32_t* valid_cols;
    const double* poses;         // [n][3] or nullptr: sx, sy, sth
    const double *sx, *sy, *sth;
    const int32_t* entry;        // map entry of row (i % n_envs), or nullptr: the row index itself (one shared map: unused)
    const int32_t* live;         // rows beyond min(*live, n) are left alone, or nullptr
    int64_t n_envs, n;
    const double* beam_cs;       // [n_beams][2]
    int32_t n_beams, trip_bound;
    double max_range, R, resolution;
    float* ranges;
    int32_t* hit;                // or nullptr
    double* heading_cs;          // or nullptr
};

// what a row's rays share
struct ScanRow {
    double c, s, u, v;
    double R;                    // 0 for a row that is not walked (scan_row_ok): every beam is a miss
    int64_t base;                // first word of the entry's mask
    int32_t valid_rows, valid_cols;
};
typedef __attribute__((address_space(3))) ScanRow* LdsScanRow;

constexpr int kScanRowWords = kScanBlock * (int)sizeof(ScanRow) / 4;   // the mask, when staged, follows the row records

struct ScanWordsLds {
    LdsWords p;
    __device__ __forceinline__ uint32_t operator()(int32_t k) const { return p[k]; }
};

struct ScanWordsGlobal {
    const uint32_t* p;
    __device__ __forceinline__ uint32_t operator()(int32_t k) const { return p[k]; }
};

static size_t scan_lds_bytes(const MapDesc& map)
{
    return ((size_t)kScanRowWords + (map.in_lds ? (size_t)map.rows * map.wpr : 0)) * sizeof(uint32_t);
}

template <bool STAGED>
__global__ void __launch_bounds__(kScanBlock) range_scan_kernel(ScanArgs a)
{
    const int tid = threadIdx.x;
    const LdsScanRow rows = (LdsScanRow)lds_dyn;
    if (STAGED) {
        const LdsU32 staged = (LdsU32)lds_dyn + kScanRowWords;
        const int words = a.map.rows * a.map.wpr;
        for (int k = tid; k < words; k += kScanBlock) staged[k] = a.map.bits[k];   // (visible after the loop's first barriers)
    }
    const int64_t n_rows = a.live ? min(a.n, (int64_t)max(*a.live, 0)) : a.n;
    const int64_t total = n_rows * a.n_beams;
    for (int64_t first = (int64_t)blockIdx.x * kScanBlock; first < total; first += (int64_t)gridDim.x * kScanBlock) {
        const int64_t last = min(first + kScanBlock, total) - 1;
        const int64_t row0 = first / a.n_beams;
        const int here = (int)(last / a.n_beams - row0) + 1;   // rows this chunk touches, <= 256
        __syncthreads();   // (the rays of the previous chunk have read their rows)
        if (tid < here) {
            const int64_t i = row0 + tid;
            const int64_t me = i % a.n_envs;
            const int64_t g = a.map.shared ? 0 : (a.entry ? (int64_t)a.entry[me] : me);
            const double ox = a.map.origins ? a.map.origins[2 * g] : a.map.ox;
            const double oy = a.map.origins ? a.map.origins[2 * g + 1] : a.map.oy;
            const double x = a.poses ? a.poses[3 * i] : a.sx[i];
            const double y = a.poses ? a.poses[3 * i + 1] : a.sy[i];
            const double th = a.poses ? a.poses[3 * i + 2] : a.sth[i];
            ScanRow r;
            r.c = cos(th);
            r.s = sin(th);
            scan_row_start(x, y, th, ox, oy, a.map.inv_res, a.R, &r.u, &r.v, &r.R);
            if (a.heading_cs) {
                a.heading_cs[2 * i] = r.c;
                a.heading_cs[2 * i + 1] = r.s;
            }
            r.base = g * a.map.env_stride;
            r.valid_rows = a.valid_rows ? max(0, min(a.valid_rows[g], a.map.rows)) : a.map.rows;
            r.valid_cols = a.valid_cols ? max(0, min(a.valid_cols[g], a.map.cols)) : a.map.cols;
            const LdsScanRow o = rows + tid;   // (member by member: an LDS object has no copy operators)
            o->c = r.c; o->s = r.s; o->u = r.u; o->v = r.v; o->R = r.R;
            o->base = r.base; o->valid_rows = r.valid_rows; o->valid_cols = r.valid_cols;
        }
        __syncthreads();
        const int64_t f = first + tid;
        if (f < total) {
            const uint32_t local = (uint32_t)(first - row0 * a.n_beams) + (uint32_t)tid;   // < n_beams + 256
            const uint32_t rl = local / (uint32_t)a.n_beams, b = local - rl * (uint32_t)a.n_beams;
            const LdsScanRow q = rows + rl;
            ScanRow r;
            r.c = q->c; r.s = q->s; r.u = q->u; r.v = q->v; r.R = q->R;
            r.base = q->base; r.valid_rows = q->valid_rows; r.valid_cols = q->valid_cols;
            const double cb = a.beam_cs[2 * b], sb = a.beam_cs[2 * b + 1];
            double dx, dy;
            scan_direction(r.c, r.s, cb, sb, &dx, &dy);
            ScanResult res;
            if (STAGED) {
                const ScanWordsLds w = {(LdsWords)((LdsU32)lds_dyn + kScanRowWords)};
                res = scan_march(w, a.map.wpr, a.map.cols, r.valid_rows, r.valid_cols, r.u, r.v, dx, dy, r.R, a.resolution,
                                 a.max_range, a.trip_bound);
            } else {
                const ScanWordsGlobal w = {a.map.bits + r.base};
                res = scan_march(w, a.map.wpr, a.map.cols, r.valid_rows, r.valid_cols, r.u, r.v, dx, dy, r.R, a.resolution,
                                 a.max_range, a.trip_bound);
            }
            a.ranges[f] = res.range;
            if (a.hit) a.hit[f] = res.hit;
        }
    }
}


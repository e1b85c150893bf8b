// bcp_boxes.h -- scatter_boxes_kernel: box obstacles stamped into a batch of maps (bcp_scatter_boxes; include/bcplan.h).
// The rule -- draws, candidate, pixel runs, verdict -- is bcp_boxes_cell.h, which has no HIP in it; this file only spreads
// it over a workgroup.  One 256-thread workgroup per entry, in three phases:
//   verdicts   one lane per attempt: its vertices, then its own runs against the entry's keep-outs (in LDS)
//   selection  a ballot per wave and the waves' totals in LDS rank the accepted attempts of a chunk of 256 in attempt
//              order; chunks are taken in order until n_boxes are found or max_attempts is reached
//   fill       per winner, lanes 0 .. 3 draw one edge each and the other lanes take the span rows, 252 apart
// Plain byte stores of 254 (lanes that meet on a cell store the same byte), no atomics, no scratch, bounded loops only.
#pragma once

#include "bcp_boxes_cell.h"

namespace bcp {

struct BoxArgs {
    uint8_t* data;                 // [n_maps][rows][cols]
    const int32_t* valid_rows;     // [n_maps] or null
    const int32_t* valid_cols;
    const double* origins;         // [n_maps][2]
    const double* frame;           // [n_maps][6]
    const int32_t* keep;           // [n_maps][n_keep][3] or null
    const double* yaw_cs;          // [n_yaws][2]
    int32_t* boxes;                // [n_maps][n_boxes][kBoxWords]
    int32_t* counts;               // [n_maps]
    int64_t n_maps;
    int32_t rows, cols, n_keep;
    double inv_res;
    BoxRule rule;
};

// writes the cells of a run; a run of an accepted box lies inside the valid shape, and the clamp to the plane costs nothing
struct BoxFillSink {
    uint8_t* plane;
    int32_t rows, cols;
    __device__ __forceinline__ bool span(int32_t r, int32_t ca, int32_t cb) const
    {
        if ((uint32_t)r >= (uint32_t)rows) return false;
        ca = ca < 0 ? 0 : ca;
        cb = cb >= cols ? cols - 1 : cb;
        for (int32_t c = ca; c <= cb; ++c) plane[(int64_t)r * cols + c] = kBoxLethal;
        return false;
    }
    __device__ __forceinline__ bool pixel(int32_t r, int32_t c) const { return span(r, c, c); }
};

__global__ __launch_bounds__(kBoxChunk) void scatter_boxes_kernel(BoxArgs a)
{
    __shared__ int32_t win[kBoxMaxBoxes * kBoxWords];
    __shared__ int32_t keep_s[kBoxMaxKeep * 3];
    __shared__ int32_t wave_n[kBoxChunk / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BoxRule& R = a.rule;
    for (int64_t m = blockIdx.x; m < a.n_maps; m += gridDim.x) {
        __syncthreads();   // (the entry before is done with win and keep_s)
        if (tid < 3 * a.n_keep) keep_s[tid] = a.keep[m * 3 * a.n_keep + tid];
        const int32_t vr = a.valid_rows ? box_clamp_valid(a.valid_rows[m], a.rows) : a.rows;
        const int32_t vc = a.valid_cols ? box_clamp_valid(a.valid_cols[m], a.cols) : a.cols;
        const double ox = a.origins[2 * m], oy = a.origins[2 * m + 1];
        __syncthreads();

        // ---- verdicts and selection, a chunk of attempts at a time
        int32_t count = 0;   // (the same in every lane)
        for (int32_t base = 0; base < R.max_attempts && count < R.n_boxes; base += kBoxChunk) {
            const int32_t att = base + tid;
            int32_t V[8];
            const bool ok = att < R.max_attempts &&
                            box_accepted(R, (uint64_t)m, att, a.frame + 6 * m, a.yaw_cs, ox, oy, a.inv_res, vr, vc, keep_s,
                                         a.n_keep, V);
            const uint64_t votes = __ballot(ok);
            if (lane == 0) wave_n[wave] = (int32_t)__popcll(votes);
            __syncthreads();
            int32_t rank = count + (int32_t)__popcll(votes & ((1ull << lane) - 1ull)), total = 0;
            for (int w = 0; w < kBoxChunk / 64; ++w) {
                rank += w < wave ? wave_n[w] : 0;
                total += wave_n[w];
            }
            if (ok && rank < R.n_boxes) {
                win[kBoxWords * rank] = att;
                for (int q = 0; q < 8; ++q) win[kBoxWords * rank + 1 + q] = V[q];
            }
            count = count + total < R.n_boxes ? count + total : R.n_boxes;
            __syncthreads();   // (win is complete; wave_n may be written again)
        }

        // ---- fill, and the boxes on their way out
        BoxFillSink fill = {a.data + m * (int64_t)a.rows * a.cols, a.rows, a.cols};
        for (int32_t w = 0; w < count; ++w) {
            int32_t V[8];
            for (int q = 0; q < 8; ++q) V[q] = win[kBoxWords * w + 1 + q];
            if (tid < 4) {
                (void)box_outline(V, tid, fill);
            } else {
                int32_t ymin, ymax;
                box_rows(V, ymin, ymax);
                for (int32_t y = ymin + (tid - 4); y < ymax; y += kBoxChunk - 4) (void)box_span_row(V, y, fill);
            }
        }
        int32_t* out = a.boxes + m * (int64_t)(kBoxWords * R.n_boxes);
        for (int32_t j = tid; j < kBoxWords * R.n_boxes; j += kBoxChunk) out[j] = j < kBoxWords * count ? win[j] : 0;
        if (tid == 0) a.counts[m] = count;
    }
}

}  // namespace bcp

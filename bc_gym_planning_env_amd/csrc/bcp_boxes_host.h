// bcp_boxes_host.h -- the host side of bcp_scatter_boxes: the checks (scatter_check_args of bcp_boxes_cell.h, which the host
// tests run too), the launch arguments, one launch of scatter_boxes_kernel (bcp_boxes.h).  Included by bcplan.hip after
// bcp_goal_host.h.
// Capture: nothing is uploaded or allocated, the kernel's LDS is static and the launch arguments depend only on what the
// caller passes: a call can be captured after one ordinary call.
#pragma once

constexpr int64_t kScatterGrid = 16384;   // workgroups at most; entries beyond are taken in turns

extern "C" int bcp_scatter_boxes(bcp_handle* h, uint8_t* data, int64_t n_maps, int32_t rows, int32_t cols,
                                 const int32_t* valid_rows, const int32_t* valid_cols, const double* origins, double resolution,
                                 const bcp_scatter_params* p, const double* frame, const int32_t* keep, int32_t n_keep,
                                 const double* yaw_cs, int32_t* boxes, int32_t* counts, void* stream)
{
    const bool arrays = data && origins && frame && yaw_cs && boxes && counts;
    switch (scatter_check_args(h != nullptr, p != nullptr, n_maps, rows, cols, resolution, p ? p->n_boxes : 0,
                               p ? p->max_attempts : 0, p ? p->n_yaws : 0, n_keep, p ? p->along[0] : 0.0, p ? p->along[1] : 0.0,
                               p ? p->half_size[0] : 0.0, p ? p->half_size[1] : 0.0, valid_rows != nullptr,
                               valid_cols != nullptr, arrays, keep != nullptr)) {
    case kScatterOk: break;
    case kScatterHandle: return fail(BCP_E_INVALID, "bcp_scatter_boxes: null handle");
    case kScatterParams: return fail(BCP_E_INVALID, "bcp_scatter_boxes: null params");
    case kScatterMaps: return fail(BCP_E_INVALID, "bcp_scatter_boxes: n_maps %lld is negative", (long long)n_maps);
    case kScatterShape: return fail(BCP_E_INVALID, "bcp_scatter_boxes: shape %d x %d outside [1, %d] x [1, %d]", rows, cols,
                                    kBoxMaxSide, kBoxMaxSide);
    case kScatterResolution: return fail(BCP_E_INVALID, "bcp_scatter_boxes: resolution must be a finite number > 0");
    case kScatterBoxes: return fail(BCP_E_INVALID, "bcp_scatter_boxes: n_boxes %d outside [1, %d]", p->n_boxes, kBoxMaxBoxes);
    case kScatterAttempts: return fail(BCP_E_INVALID, "bcp_scatter_boxes: max_attempts %d outside [1, %d]", p->max_attempts,
                                       kBoxMaxAttempts);
    case kScatterYaws: return fail(BCP_E_INVALID, "bcp_scatter_boxes: n_yaws %d outside [1, %d]", p->n_yaws, kBoxMaxYaws);
    case kScatterKeep: return fail(BCP_E_INVALID, "bcp_scatter_boxes: n_keep %d outside [0, %d]", n_keep, kBoxMaxKeep);
    case kScatterAlong: return fail(BCP_E_INVALID, "bcp_scatter_boxes: along must be finite with along[0] <= along[1]");
    case kScatterHalf: return fail(BCP_E_INVALID, "bcp_scatter_boxes: half_size must be finite with 0 <= half_size[0] <= "
                                                  "half_size[1]");
    case kScatterHalfFits: return fail(BCP_E_INVALID, "bcp_scatter_boxes: a box of half size %g m need not fit a map of %d x %d "
                                                      "cells of %g m", p->half_size[1], rows, cols, resolution);
    case kScatterValidPair: return fail(BCP_E_INVALID, "bcp_scatter_boxes: valid_rows and valid_cols go together, both or neither");
    default: return fail(BCP_E_INVALID, "bcp_scatter_boxes: null data / origins / frame / yaw_cs / boxes / counts / keep");
    }
    if (n_maps == 0) return BCP_OK;
    HIP_TRY(hipSetDevice(h->device));

    BoxArgs a;
    memset(&a, 0, sizeof(a));
    a.data = data;
    a.valid_rows = valid_rows;
    a.valid_cols = valid_cols;
    a.origins = origins;
    a.frame = frame;
    a.keep = n_keep > 0 ? keep : nullptr;
    a.yaw_cs = yaw_cs;
    a.boxes = boxes;
    a.counts = counts;
    a.n_maps = n_maps;
    a.rows = rows;
    a.cols = cols;
    a.n_keep = n_keep;
    a.inv_res = 1.0 / resolution;   // anti_resolution (coordinate_transformations.py:204)
    a.rule.n_boxes = p->n_boxes;
    a.rule.max_attempts = p->max_attempts;
    a.rule.n_yaws = p->n_yaws;
    a.rule.seed_lo = (uint32_t)p->seed;
    a.rule.seed_hi = (uint32_t)(p->seed >> 32);
    a.rule.t_lo = p->along[0];
    a.rule.t_hi = p->along[1];
    a.rule.h_lo = p->half_size[0];
    a.rule.h_hi = p->half_size[1];
    return launch_fn((const void*)scatter_boxes_kernel, dim3((unsigned)std::min(n_maps, kScatterGrid)), dim3(kBoxChunk), 0,
                     (hipStream_t)stream, a);
}

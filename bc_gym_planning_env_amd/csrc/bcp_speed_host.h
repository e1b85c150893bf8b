// bcp_speed_host.h -- the host side of bcp_path_speed: the checks (speed_check_args, bcp_speed_cell.h, which the host tests
// run too) and one launch of speed_kernel (bcp_speed.h).  Nothing is uploaded or allocated, the parameters travel by value in
// the launch arguments, and the dynamic LDS (speed_lds_plan: 8 bytes per slot, at most 4096 slots) stays below 64 KB, so no
// attribute is raised: a call can be captured after one ordinary call.  The handle gives the device and is not changed.
// Included by bcplan.hip after bcp_smooth_host.h.
#pragma once

static_assert(sizeof(bcp_speed_params) == sizeof(SpeedParams) && offsetof(bcp_speed_params, span) == offsetof(SpeedParams, span) &&
                  offsetof(bcp_speed_params, v_max) == offsetof(SpeedParams, v_max) &&
                  offsetof(bcp_speed_params, v_end) == offsetof(SpeedParams, v_end),
              "bcp_speed_params is SpeedParams, field for field");
static_assert(BCP_SPEED_NO_PATH == kSpeedNoPath, "one value for the status");

extern "C" int bcp_path_speed(bcp_handle* h, const double* paths, const int32_t* lens, int32_t max_len, int64_t n,
                              const bcp_speed_params* p, double* speed, double* kappa, double* v_limit, int32_t* status,
                              void* stream)
{
    const char* who = "bcp_path_speed";
    static const char* const positive[5] = {"v_max", "a_lat", "w_max", "a_dec", "a_acc"};
    static const char* const non_negative[3] = {"v_min", "v_start", "v_end"};
    const bool pointers = h && paths && lens && speed && status;
    SpeedParams prm;
    memset(&prm, 0, sizeof(prm));
    if (p) {
        prm.span = p->span;
        prm.v_max = p->v_max;
        prm.v_min = p->v_min;
        prm.a_lat = p->a_lat;
        prm.w_max = p->w_max;
        prm.a_dec = p->a_dec;
        prm.a_acc = p->a_acc;
        prm.v_start = p->v_start;
        prm.v_end = p->v_end;
    }
    bool overlap = false;
    if (pointers && n > 0 && n <= 0x7FFFFFFFll && max_len >= 1 && max_len <= kSpeedMaxLen) {
        const uint64_t in_p = (uint64_t)(uintptr_t)paths, in_bytes = (uint64_t)n * max_len * 24, out_bytes = (uint64_t)n * max_len * 8;
        for (const double* out : {(const double*)speed, (const double*)kappa, (const double*)v_limit})
            overlap = overlap || (out && speed_overlap((uint64_t)(uintptr_t)out, out_bytes, in_p, in_bytes));
    }
    int which = 0;
    switch (speed_check_args(pointers, p != nullptr, max_len, n, prm, overlap, &which)) {
    case kSpeedOk: break;
    case kSpeedNull: return fail(BCP_E_INVALID, "%s: null argument", who);
    case kSpeedMaxLenRange: return fail(BCP_E_INVALID, "%s: max_len %d outside [1, %d]", who, max_len, kSpeedMaxLen);
    case kSpeedRows: return fail(BCP_E_INVALID, "%s: n must be in [1, 2^31 - 1]", who);
    case kSpeedSpan: return fail(BCP_E_INVALID, "%s: span %d outside [1, %d]", who, prm.span, kSpeedMaxSpan);
    case kSpeedPositive: return fail(BCP_E_INVALID, "%s: %s must be a finite number > 0", who, positive[which]);
    case kSpeedNonNegative: return fail(BCP_E_INVALID, "%s: %s must be a finite number >= 0", who, non_negative[which]);
    case kSpeedOrder: return fail(BCP_E_INVALID, "%s: v_min > v_max", who);
    default: return fail(BCP_E_INVALID, "%s: speed / kappa / v_limit overlap paths, which the call reads", who);
    }
    HIP_TRY(hipSetDevice(h->device));
    SpeedArgs a;
    memset(&a, 0, sizeof(a));
    a.paths = paths;
    a.lens = lens;
    a.max_len = max_len;
    a.prm = prm;
    a.speed = speed;
    a.kappa = kappa;
    a.v_limit = v_limit;
    a.status = status;
    return launch_fn((const void*)speed_kernel, dim3((unsigned)n), dim3(64), speed_lds_plan(max_len).bytes, (hipStream_t)stream, a);
}

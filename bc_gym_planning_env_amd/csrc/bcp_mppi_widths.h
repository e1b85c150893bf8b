// bcp_mppi_widths.h -- what bcp_mppi_adapt decides about its widths before and inside the launch, as plain functions: the
// checks of the bcp_mppi_adapt struct (mppi_adapt_check_args, the refusals in the order the header lists them), the clamp
// every width goes through (mppi_clamp_width) and the move of a width towards the weighted spread (mppi_next_width).
// No HIP in here: bcp_mppi.h includes it for the kernel and bcp_plan_host.h's checks, and so does a stand-alone host program
// (tests/c_abi/mppi_adapt_main.cpp) that drives the checks through every refusal without a GPU.
#pragma once

#if defined(__HIPCC__)
#define BCP_WIDTHS_HD __host__ __device__
#else
#define BCP_WIDTHS_HD
#endif

namespace bcp {

enum MppiAdaptRefusal {
    kMppiAdaptOk = 0, kMppiAdaptNull = 1, kMppiAdaptRate = 2, kMppiAdaptMin = 3, kMppiAdaptMax = 4, kMppiAdaptOrder = 5
};

// finite and not negative, written with comparisons alone (a NaN fails the first one)
BCP_WIDTHS_HD inline bool mppi_width_bound_ok(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }

// The first rule the arguments break: ad or ad->sigma NULL; rate NaN or outside [0, 1]; then per component d = 0, 1 a
// negative or non-finite sigma_min[d], the same of sigma_max[d], sigma_min[d] > sigma_max[d].  *component is the d of a
// refusal that has one (else untouched).
BCP_WIDTHS_HD inline int mppi_adapt_check_args(bool have_ad, bool have_sigma, double rate, const double* sigma_min,
                                               const double* sigma_max, int* component)
{
    if (!have_ad || !have_sigma) return kMppiAdaptNull;
    if (!(rate >= 0.0 && rate <= 1.0)) return kMppiAdaptRate;
    for (int d = 0; d < 2; ++d) {
        int bad = kMppiAdaptOk;
        if (!mppi_width_bound_ok(sigma_min[d])) bad = kMppiAdaptMin;
        else if (!mppi_width_bound_ok(sigma_max[d])) bad = kMppiAdaptMax;
        else if (sigma_min[d] > sigma_max[d]) bad = kMppiAdaptOrder;
        if (bad != kMppiAdaptOk) {
            if (component) *component = d;
            return bad;
        }
    }
    return kMppiAdaptOk;
}

// clampd of the header: a NaN goes to the minimum
BCP_WIDTHS_HD inline double mppi_clamp_width(double s, double lo, double hi) { return !(s >= lo) ? lo : (s > hi ? hi : s); }

// sigma_{j+1} from sigma_j and the weighted spread sd: the difference, the product and the sum rounded on their own
BCP_WIDTHS_HD inline double mppi_next_width(double sigma, double sd, double rate, double lo, double hi)
{
    const double step = rate * (sd - sigma);
    return mppi_clamp_width(sigma + step, lo, hi);
}

}  // namespace bcp

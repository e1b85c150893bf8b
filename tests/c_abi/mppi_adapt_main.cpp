// The host side of bcp_mppi_adapt's widths (csrc/bcp_mppi_widths.h) on its own: the very functions bcp_mppi_adapt and
// mppi_kernel<.., ADAPT> call -- the checks of the struct, the clamp and the move of a width.  The header has no HIP in it;
// this program includes nothing else of the library and is built with -ffp-contract=off -fsanitize=address,undefined.
// It drives mppi_adapt_check_args through every refusal and their order, with NaN and +-inf in every field, and the clamp
// and the move through their branches; prints one line per failed expectation and "mppi adapt ok" when there is none.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "bcp_mppi_widths.h"

using namespace bcp;

static int failures = 0;

static void expect(bool ok, const char* what, int line)
{
    if (ok) return;
    printf("line %d: %s\n", line, what);
    ++failures;
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

struct Case {
    bool have_ad, have_sigma;
    double rate, lo[2], hi[2];
};

static int check(const Case& c, int* d)
{
    // heap copies of exactly two doubles: a read of element 2 is an AddressSanitizer report
    std::vector<double> lo(c.lo, c.lo + 2), hi(c.hi, c.hi + 2);
    return mppi_adapt_check_args(c.have_ad, c.have_sigma, c.rate, lo.data(), hi.data(), d);
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double big = std::numeric_limits<double>::max(), tiny = std::numeric_limits<double>::denorm_min();
    const Case good = {true, true, 0.5, {0.025, 0.1}, {0.4, 1.6}};
    int d = -1;

    // ---- what passes
    EXPECT(check(good, &d) == kMppiAdaptOk && d == -1);
    EXPECT(mppi_adapt_check_args(true, true, 0.5, good.lo, good.hi, nullptr) == kMppiAdaptOk);
    for (double rate : {0.0, -0.0, tiny, 1.0, 0.25}) {
        Case c = good;
        c.rate = rate;
        EXPECT(check(c, &d) == kMppiAdaptOk);
    }
    {
        Case c = good;
        c.lo[0] = c.hi[0] = 0.0;   // a width pinned at zero
        c.lo[1] = c.hi[1] = big;   // and one at the largest finite number
        EXPECT(check(c, &d) == kMppiAdaptOk);
        c.lo[0] = -0.0;
        EXPECT(check(c, &d) == kMppiAdaptOk);
    }

    // ---- null arguments come first, whatever else is wrong
    {
        Case c = good;
        c.rate = nan;
        c.lo[0] = -1.0;
        c.have_ad = false;
        EXPECT(check(c, &d) == kMppiAdaptNull);
        c.have_ad = true;
        c.have_sigma = false;
        EXPECT(check(c, &d) == kMppiAdaptNull);
        // (without a struct there are no arrays to read)
        EXPECT(mppi_adapt_check_args(false, false, nan, nullptr, nullptr, &d) == kMppiAdaptNull && d == -1);
    }

    // ---- the rate, before any bound
    for (double rate : {nan, inf, -inf, -tiny, -1.0, 1.0000000000000002, 2.0, big}) {
        Case c = good;
        c.rate = rate;
        c.lo[0] = nan;
        c.hi[1] = -1.0;
        d = -1;
        EXPECT(check(c, &d) == kMppiAdaptRate && d == -1);
    }

    // ---- the bounds: per component sigma_min, then sigma_max, then their order; component 0 before component 1
    for (int comp = 0; comp < 2; ++comp) {
        for (double bad : {nan, inf, -inf, -tiny, -1.0}) {
            Case c = good;
            c.lo[comp] = bad;
            d = -1;
            EXPECT(check(c, &d) == kMppiAdaptMin && d == comp);
            c.hi[comp] = nan;   // sigma_min is reported before sigma_max of the same component
            EXPECT(check(c, &d) == kMppiAdaptMin && d == comp);
            c = good;
            c.hi[comp] = bad;
            d = -1;
            EXPECT(check(c, &d) == kMppiAdaptMax && d == comp);
        }
        Case c = good;
        c.lo[comp] = 2.0;
        c.hi[comp] = 1.0;
        d = -1;
        EXPECT(check(c, &d) == kMppiAdaptOrder && d == comp);
        c.hi[comp] = std::nextafter(2.0, 0.0);
        EXPECT(check(c, &d) == kMppiAdaptOrder && d == comp);
        c.hi[comp] = 2.0;
        EXPECT(check(c, &d) == kMppiAdaptOk);
    }
    {
        Case c = good;   // component 0's order before component 1's sigma_min; component 0's sigma_max before both
        c.lo[0] = 1.0;
        c.hi[0] = 0.5;
        c.lo[1] = nan;
        EXPECT(check(c, &d) == kMppiAdaptOrder && d == 0);
        c.hi[0] = inf;
        EXPECT(check(c, &d) == kMppiAdaptMax && d == 0);
        c = good;
        c.hi[0] = -1.0;
        c.lo[1] = -1.0;
        EXPECT(check(c, &d) == kMppiAdaptMax && d == 0);
        c.hi[0] = good.hi[0];
        EXPECT(check(c, &d) == kMppiAdaptMin && d == 1);
    }

    // ---- the clamp: a NaN goes to the minimum, the infinities to their sides, the bounds are kept bit for bit
    EXPECT(mppi_clamp_width(nan, 0.1, 0.8) == 0.1);
    EXPECT(mppi_clamp_width(-nan, 0.1, 0.8) == 0.1);
    EXPECT(mppi_clamp_width(-1.0, 0.1, 0.8) == 0.1);
    EXPECT(mppi_clamp_width(-inf, 0.1, 0.8) == 0.1);
    EXPECT(mppi_clamp_width(inf, 0.1, 0.8) == 0.8);
    EXPECT(mppi_clamp_width(1e300, 0.1, 0.8) == 0.8);
    EXPECT(mppi_clamp_width(0.1, 0.1, 0.8) == 0.1 && mppi_clamp_width(0.8, 0.1, 0.8) == 0.8);
    EXPECT(mppi_clamp_width(0.3, 0.1, 0.8) == 0.3);
    EXPECT(mppi_clamp_width(0.3, 0.5, 0.5) == 0.5 && mppi_clamp_width(0.7, 0.5, 0.5) == 0.5);
    EXPECT(std::signbit(mppi_clamp_width(-0.0, 0.0, 1.0)));   // -0 >= 0: kept as it is

    // ---- the move: rate 0 keeps a width, rate 1 takes the spread, in between the three roundings of the header
    EXPECT(mppi_next_width(0.3, 0.05, 0.0, 0.0, 1.0) == 0.3);
    EXPECT(mppi_next_width(0.3, 0.05, 1.0, 0.0, 1.0) == 0.3 + (0.05 - 0.3));
    EXPECT(mppi_next_width(0.3, 0.0, 0.5, 0.0, 1.0) == 0.3 + 0.5 * (0.0 - 0.3));
    EXPECT(mppi_next_width(0.3, 0.0, 1.0, 0.1, 1.0) == 0.1);     // the spread of a one-hot weight, on the lower clamp
    EXPECT(mppi_next_width(0.3, 5.0, 1.0, 0.1, 0.6) == 0.6);
    EXPECT(mppi_next_width(0.3, nan, 0.5, 0.1, 0.6) == 0.1);     // (no spread is ever a NaN; if one were, the width would not be)
    {
        const double s = 0.2, sd = 0.07, rate = 0.3;
        const double diff = sd - s, step = rate * diff, sum = s + step;
        EXPECT(mppi_next_width(s, sd, rate, 0.0, 1.0) == sum);
    }

    if (failures) {
        printf("%d expectations failed\n", failures);
        return 1;
    }
    printf("mppi adapt ok\n");
    return 0;
}

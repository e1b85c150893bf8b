// goal_field_kernel's phases on the host, one map, in sequence: the lethal mask, the closed mask by goal_half_width /
// goal_widen_word, the plane and the seeds, then in-place sweeps of goal_relax_cell -- or, with a table,
// goal_relax_cell_cost with the extra of the relaxed cell's own byte, looked up for open cells only -- until one changes
// nothing or max_passes sweeps were made.  The functions are csrc/bcp_goal_cell.h's, the very ones the kernel calls; the
// loops of phases 2 and 3 around them are the kernel's (csrc/bcp_goal.h) restated here, once.  Every word, cell, byte and
// table entry is read and written through a bounds-checked accessor.  goal_field_main.cpp and goal_cost_main.cpp run it.
#pragma once

#include <cstdint>
#include <vector>

#include "bcp_goal_cell.h"
#include "host_io.h"

struct HostSweep {
    std::vector<uint16_t> plane;   // [rows][cols]
    int32_t sweeps, gave_up;
    long long reached, lookups;    // cells that hold a value; table lookups made
};

// data [rows][cols], seeds [n_seeds][2] (row, col), table: nullptr (the plain field) or [256].  false: a relaxation
// raised a value or left the uint16 range (values only fall).
inline bool host_goal_sweep(int32_t rows, int32_t cols, int32_t vr, int32_t vc, const std::vector<uint8_t>& data,
                            const std::vector<int32_t>& seeds, int32_t n_seeds, int32_t clearance_d2, int32_t max_passes,
                            const std::vector<uint16_t>* table, HostSweep& out)
{
    using namespace bcp;
    const int32_t wpr = (cols + 31) / 32, reach = goal_isqrt(clearance_d2);
    std::vector<uint32_t> lethal((size_t)rows * wpr, 0u), closed((size_t)rows * wpr, 0u);
    for (int32_t r = 0; r < vr; ++r)
        for (int32_t c = 0; c < vc; ++c)
            if (data.at((size_t)r * cols + c) == 254) lethal.at((size_t)r * wpr + (c >> 5)) |= 1u << (c & 31);
    for (int32_t r = 0; r < rows; ++r) {
        for (int32_t w = 0; w < wpr; ++w) {
            const int32_t first = 32 * w;
            const uint32_t inside = r < vr && vc > first ? (vc - first >= 32 ? ~0u : (1u << (vc - first)) - 1u) : 0u;
            uint32_t acc = 0u;
            if (inside) {
                const int32_t lo = r - reach > 0 ? r - reach : 0, hi = r + reach < vr - 1 ? r + reach : vr - 1;
                for (int32_t rr = lo; rr <= hi; ++rr) {
                    const int32_t hw = goal_half_width(clearance_d2, rr > r ? rr - r : r - rr), kw = (hw + 31) >> 5;
                    const int32_t k0 = w - kw > 0 ? w - kw : 0, k1 = w + kw < wpr - 1 ? w + kw : wpr - 1;
                    for (int32_t k = k0; k <= k1; ++k) acc |= goal_widen_word(lethal.at((size_t)rr * wpr + k), 32 * (k - w), hw);
                }
            }
            closed.at((size_t)r * wpr + w) = (acc & inside) | ~inside;
        }
    }
    std::vector<uint16_t>& plane = out.plane;
    plane.assign((size_t)rows * cols, (uint16_t)kGoalNone);
    for (int32_t s = 0; s < n_seeds; ++s) {
        const int32_t sr = seeds.at((size_t)2 * s), sc = seeds.at((size_t)2 * s + 1);
        if (sr >= 0 && sr < vr && sc >= 0 && sc < vc) {
            plane.at((size_t)sr * cols + sc) = 0;
            closed.at((size_t)sr * wpr + (sc >> 5)) &= ~(1u << (sc & 31));
        }
    }
    const HostPlane get = {&plane, cols, rows, cols};
    out.sweeps = out.gave_up = 0;
    out.lookups = 0;
    for (;;) {
        if (out.sweeps == max_passes) {
            out.gave_up = 1;
            break;
        }
        ++out.sweeps;
        bool lowered = false;
        for (int32_t r = 0; r < vr; ++r) {
            for (int32_t c = 0; c < vc; ++c) {
                if ((closed.at((size_t)r * wpr + (c >> 5)) >> (c & 31)) & 1u) continue;
                const int32_t own = plane.at((size_t)r * cols + c);
                if (own == 0) continue;
                int32_t now;
                if (table) {
                    const int32_t extra = table->at(data.at((size_t)r * cols + c));
                    ++out.lookups;
                    now = goal_relax_cell_cost(get, vr, vc, r, c, own, extra);
                } else {
                    now = goal_relax_cell(get, vr, vc, r, c, own);
                }
                if (now > own || now < 0 || now > kGoalNone) return false;   // (values only fall)
                if (now != own) {
                    plane.at((size_t)r * cols + c) = (uint16_t)now;
                    lowered = true;
                }
            }
        }
        if (!lowered) break;
    }
    out.reached = 0;
    for (uint16_t v : plane) out.reached += v != (uint16_t)kGoalNone;
    return true;
}

// bcp_inflate_host.h -- bcp_inflate_costmaps: checks, the choice of where the 16-bit plane lives, the launch.
// Included by bcplan.hip after bcp_host.h; the kernel is in bcp_inflate.h.
#pragma once

// Global-plane route: a slice of scratch per workgroup, so the grid is what sizes the scratch.  512 workgroups of 1024
// threads fill the chip twice over; 512 MiB caps what a handle keeps for the largest maps (2048 x 2048: 64 workgroups).
constexpr int64_t kInflateGlobalGrid = 512;
constexpr int64_t kInflateScratchBytes = 512ll << 20;

extern "C" int bcp_inflate_costmaps(bcp_handle* h, const uint8_t* data, int64_t n_maps, int32_t rows, int32_t cols,
                                    const int32_t* valid_rows, const int32_t* valid_cols, double resolution,
                                    double inscribed_radius, double cost_scaling_factor, uint8_t* out, float* distance_out,
                                    void* stream)
{
    if (!h) return fail(BCP_E_INVALID, "bcp_inflate_costmaps: null handle");
    if (n_maps < 0) return fail(BCP_E_INVALID, "bcp_inflate_costmaps: n_maps %lld is negative", (long long)n_maps);
    if (rows < 1 || rows > 2048 || cols < 1 || cols > 2048)
        return fail(BCP_E_INVALID, "bcp_inflate_costmaps: shape %d x %d outside [1, 2048] x [1, 2048]", rows, cols);
    if (!std::isfinite(resolution) || !(resolution > 0))
        return fail(BCP_E_INVALID, "bcp_inflate_costmaps: resolution must be finite and > 0");
    if (!std::isfinite(inscribed_radius) || !(inscribed_radius > 0))
        return fail(BCP_E_INVALID, "bcp_inflate_costmaps: inscribed_radius must be finite and > 0");
    if (!std::isfinite(cost_scaling_factor) || !(cost_scaling_factor > 0))
        return fail(BCP_E_INVALID, "bcp_inflate_costmaps: cost_scaling_factor must be finite and > 0");
    if ((valid_rows == nullptr) != (valid_cols == nullptr))
        return fail(BCP_E_INVALID, "bcp_inflate_costmaps: valid_rows and valid_cols go together, both or neither");
    if (n_maps == 0) return BCP_OK;
    if (!data || !out) return fail(BCP_E_INVALID, "bcp_inflate_costmaps: null data / out");
    const int64_t cells = (int64_t)rows * cols, bytes = n_maps * cells;
    if (out != data && (uintptr_t)out < (uintptr_t)data + (uint64_t)bytes && (uintptr_t)data < (uintptr_t)out + (uint64_t)bytes)
        return fail(BCP_E_INVALID, "bcp_inflate_costmaps: out overlaps data without being data itself");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;

    InflateArgs a = {};
    a.data = data;
    a.out = out;
    a.dist = distance_out;
    a.valid_rows = valid_rows;
    a.valid_cols = valid_cols;
    a.n_maps = n_maps;
    a.rows = rows;
    a.cols = cols;
    a.wpr = (cols + 31) / 32;
    a.pir = inscribed_radius / resolution;         // :56
    a.psf = cost_scaling_factor * resolution;      // :57
    a.lethal_below = a.pir / 1000.;                // :59
    const size_t fixed = (size_t)inflate_fixed_words(rows, a.wpr) * sizeof(uint32_t);
    const size_t with_plane = fixed + (((size_t)cells * sizeof(uint16_t) + 3) & ~(size_t)3);
    const bool in_lds = with_plane <= kMaxDynamicLds && h->tune.inflate_route != 2;
    if (!in_lds && fixed > kMaxDynamicLds)   // (2048 x 2048: 64 KiB of mask + 8 KiB of lists -- cannot happen within the limits above)
        return fail(BCP_E_INVALID, "bcp_inflate_costmaps: the map's bit mask does not fit the LDS");
    // a workgroup's threads: enough cells each to be worth their barriers
    const unsigned threads = cells >= 128 * 128 ? 1024u : 256u;
    if (in_lds) {
        const unsigned grid = (unsigned)std::min<int64_t>(n_maps, 16384);
        return launch_variant(h, reinterpret_cast<const void*>(inflate_kernel<true>), dim3(grid), dim3(threads), with_plane, s, a);
    }
    const int64_t fit = std::max<int64_t>(1, kInflateScratchBytes / (cells * (int64_t)sizeof(uint16_t)));
    const int64_t grid = std::min(std::min(n_maps, kInflateGlobalGrid), fit);
    if (h->inflate_scratch.reserve((size_t)(grid * cells)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(BCP_E_HIP, "bcp_inflate_costmaps: cannot allocate %lld bytes of scratch", (long long)(grid * cells * 2));
    }
    a.scratch = h->inflate_scratch.get();
    return launch_variant(h, reinterpret_cast<const void*>(inflate_kernel<false>), dim3((unsigned)grid), dim3(threads), fixed, s, a);
}

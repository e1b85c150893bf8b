// bcp_philox.h -- Philox4x32-10, the one counter-based generator of the library: the step's noise stream and the planners'
// perturbations (bcp_device.h, bcp_mppi.h) and the box sampler's draws (bcp_boxes_cell.h).  Plain C++ with no HIP in it, so
// that a host program draws the very words a kernel draws.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BCP_HD_INLINE __host__ __device__ __forceinline__
#else
#define BCP_HD_INLINE inline
#endif

namespace bcp {

// Philox4x32-10 (Salmon et al., SC'11), counter = (env_lo, env_hi, step_lo, step_hi), key = seed.
BCP_HD_INLINE void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

}  // namespace bcp

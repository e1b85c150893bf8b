// bcp_diag.h -- what only a -DBCP_DIAG build (tools/libbcplan_diag.so) carries: the ablation switches of the step flags and
// the time stamps the step kernels leave in g_diag.  The shipping build sees `false` and empty statements.
#pragma once

#include "bcp_step_args.h"

// Ablation switches in the upper half of the step flags (tools/ablate*.py time the step with stages removed; results
// are then WRONG by construction).  Not part of the ABI: bcplan.h only defines bits 0-1.
enum : uint32_t {
    kAblateNoCollision = 1u << 16,   // skip pose_collides altogether
    kAblateNoReward = 1u << 17,      // skip the reward scan
    kAblateNoCoop = 1u << 19,        // kernel 2: skip the cooperative rasteriser
    kAblateNoPark = 1u << 21,        // kernel 1: do not park undecided envs
    kAblateNoClassify = 1u << 22     // kernel 1: skip the distance-field lookups
};
// The ablation switches exist in -DBCP_DIAG builds only (tools/libbcplan_diag.so): the shipping kernels neither fetch nor test them.
#ifdef BCP_DIAG
#define ABLATED(a, bits) (((a).flags & (bits)) != 0)
#else
#define ABLATED(a, bits) false
#endif

#ifdef BCP_DIAG
constexpr int kDiagBlocks = 4096;   // stamps of the first kDiagBlocks workgroups of a step kernel, 16 slots each
__device__ unsigned long long g_diag[kDiagBlocks * 16];
#define DIAG_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 512) g_diag[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)   /* (rows 512 .. 2047 hold the per-wave tables) */
// lane 0 of wave `w` of the workgroup
#define DIAG_STAMP_W(w, k) do { if (threadIdx.x == (w) * 64 && blockIdx.x < kDiagBlocks) g_diag[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
// maxima over the waves of a workgroup live in the upper half of the array (slot k of workgroup b: (2048 + b) * 16 + k)
#define DIAG_MAX(k, v) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 2048) atomicMax(&g_diag[(2048 + blockIdx.x) * 16 + (k)], (unsigned long long)(v)); } while (0)
#define DIAG_NOW() __builtin_amdgcn_s_memtime()
// wall-clock stamps (s_memrealtime: 100 MHz, the same counter chip-wide -- s_memtime is not comparable between compute units):
// rows 3072 + workgroup (grids of up to 1024 workgroups), slot 0 = earliest entry of a wave, slot 1 = latest exit
#define DIAG_REAL_ENTRY() do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 1024) atomicMax(&g_diag[(3072 + blockIdx.x) * 16 + 0], ~(unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)   /* (the complement: bcp_diag_clear zeroes) */
#define DIAG_REAL_EXIT() do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 1024) atomicMax(&g_diag[(3072 + blockIdx.x) * 16 + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)
// further stamps of lane 0 of wave `w`, in the upper half next to the maxima: slot k = 1 .. 15 of workgroup b at (2048 + b) * 16 + k
#define DIAG_STAMP_U(w, k) do { if (threadIdx.x == (w) * 64 && blockIdx.x < 2048) g_diag[(2048 + blockIdx.x) * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define DIAG_WAIT_VMEM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
// lane 0 of EVERY wave: row (base + workgroup), slot = wave number (base = 1024, 1536: arrival at barrier 0 / 1)
#define DIAG_STAMP_WAVES(base) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 256) g_diag[((base) + blockIdx.x) * 16 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime(); } while (0)
// maximum over ALL lanes of the workgroup (not only lane 0 of each wave)
/* the finishing pass (finalize_env_from) of wave 0, lane 0: rows 1792 .. 2047, slots 0 .. 3 -- arguments in hand, outputs stored, reset values in hand, state stored */
#define DIAG_STAMP_FIN(k) do { if (threadIdx.x == 0 && blockIdx.x < 256) g_diag[(1792 + blockIdx.x) * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define DIAG_WAIT_LGKM() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define DIAG_MAX_ALL(k, v) do { if (blockIdx.x < 2048) atomicMax(&g_diag[(2048 + blockIdx.x) * 16 + (k)], (unsigned long long)(v)); } while (0)
extern "C" int bcp_diag_read(unsigned long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag), sizeof(g_diag));
}
extern "C" int bcp_diag_clear()
{
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_diag)) != hipSuccess) return -1;
    return (int)hipMemset(p, 0, sizeof(g_diag));
}

#else
#define DIAG_STAMP(k) do { } while (0)
#define DIAG_STAMP_W(w, k) do { } while (0)
#define DIAG_MAX(k, v) do { } while (0)
#define DIAG_NOW() 0ull
#define DIAG_REAL_ENTRY() do { } while (0)
#define DIAG_REAL_EXIT() do { } while (0)
#define DIAG_STAMP_U(w, k) do { } while (0)
#define DIAG_WAIT_VMEM() do { } while (0)
#define DIAG_STAMP_WAVES(base) do { } while (0)
#define DIAG_STAMP_FIN(k) do { } while (0)
#define DIAG_WAIT_LGKM() do { } while (0)
#define DIAG_MAX_ALL(k, v) do { } while (0)
#endif

// kf_scan.h -- LDS and wave prefix-sum helpers shared by the device sources (also
// by kf_sparse.hip, which does not use the count front end, kf_front.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kf {

// Atomic add to the LDS word at byte address `a`.  The histogram is the whole
// dynamic LDS allocation and the kernel declares no static LDS, so it starts at
// LDS address 0 (checked once per kernel): a raw address-space-3 pointer avoids a
// base add per k-mer.
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ void lds_add(uint32_t a, uint32_t v) {
    __hip_atomic_fetch_add((lds_u32*)(uintptr_t)a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t lds_add_rtn(uint32_t a, uint32_t v) {
    return __hip_atomic_fetch_add((lds_u32*)(uintptr_t)a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Workgroup barrier ordering LDS only: waits for this wave's LDS operations, not
// for its vector-memory ones (__syncthreads waits for vmcnt(0) too, i.e. for
// prefetches and row stores in flight).  Not for global memory that another wave
// of the workgroup wrote.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Inclusive prefix sum over a whole (fully active) wave on the VALU (DPP row
// shifts and row broadcasts; no LDS traffic, unlike __shfl_up's ds_bpermute).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);   // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return v;
}

}  // namespace kf

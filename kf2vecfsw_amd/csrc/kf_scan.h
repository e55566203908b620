// kf_scan.h -- LDS and wave prefix-sum helpers shared by the device sources (also
// by kf_sparse.hip, which does not use the count front end, kf_front.h): the wave
// and workgroup scans, the one-workgroup scan with carry of the device pre-passes,
// the three-level scan of longer tables and the per-thread search of a sorted
// table (kf_compact.h builds the pre-passes' count -> scan -> scatter compaction
// on them).
//
// Every workgroup helper (block_excl_scan, block_sum, scan_with_carry, and
// kf_compact.h's compact_count and compact_first_slot) must be reached by EVERY
// thread of a workgroup of whole waves: the DPP wave scan reads its neighbours'
// lanes and the barriers wait for every wave.  A thread with nothing to add brings
// 0 (the pre-passes' predicates return 0 past the end of the input); it does not
// leave the kernel first.
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
// 64-bit values: __shfl_up steps on the whole value (ds_bpermute; the FASTQ
// index's scan levels only, which are not hot).
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Exclusive prefix of one value per thread over an NW-wave workgroup; *total
// (optional) gets the sum.  wsum: NW words of LDS.  Contains two barriers
// (LDS-only ones if LDSB), the second after the last read of wsum.
template <int NW, bool LDSB = false, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* wsum, T* total = nullptr) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    if (lane == 63) wsum[w] = inc;
    if (LDSB) lds_barrier();
    else __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int x = 0; x < NW; ++x) {
        const T s = wsum[x];
        before += x < w ? s : T(0);
        all += s;
    }
    if (total) *total = all;
    if (LDSB) lds_barrier();
    else __syncthreads();
    return before + inc - v;
}

// Sum of one value per thread over an NW-wave workgroup, to every thread.  red:
// NW words of LDS.  One barrier, after the writes of red.
template <int NW>
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* red) {
    const uint32_t inc = wave_incl_scan(v);
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t all = 0;
#pragma unroll
    for (int x = 0; x < NW; ++x) all += red[x];
    return all;
}

// Exclusive scan of load(0) .. load(n - 1) by ONE workgroup of 1,024 threads,
// 1,024 entries per round with the rounds' carry in a register: store(i, prefix)
// for every i < n, in place if load and store name the same table (entry i is read
// and written by one thread).  Returns the total to every thread.
template <typename Load, typename Store>
__device__ __forceinline__ uint32_t scan_with_carry(uint32_t n, Load load, Store store) {
    __shared__ uint32_t wsum[16];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<16>(i < n ? (uint32_t)load(i) : 0u, wsum, &tot);
        if (i < n) store(i, carry + ex);
        carry += tot;
    }
    return carry;
}

// A table too long for one workgroup is scanned in levels of kScanLevel entries
// per workgroup (the FASTQ index's tables, the sorted merge's tile counts): level
// 1 turns the entries of each workgroup into exclusive prefixes in place and
// leaves a sum per workgroup, level 2 does the same to those sums, level 3 (one
// workgroup) to level 2's; entry i of the scanned table is scanned(v, s1, s2, i).
constexpr uint32_t kScanLevel = 1024;
constexpr uint64_t kScanMaxEntries = (uint64_t)kScanLevel * kScanLevel * kScanLevel;   // level 3 is one workgroup

// One scan level: workgroup i replaces v[i * 1024 + t] (entries below n) by their
// exclusive prefix sums and writes their total to sums[i].
namespace {
template <typename T>
__global__ void __launch_bounds__(kScanLevel) scan_level_kernel(T* v, uint64_t n, T* sums) {
    __shared__ T wsum[kScanLevel / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kScanLevel + threadIdx.x;
    T all;
    const T ex = block_excl_scan<kScanLevel / 64>(i < n ? v[i] : T(0), wsum, &all);
    if (i < n) v[i] = ex;
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}
}  // namespace

// entry i of a scanned table: its three levels added up
__device__ __forceinline__ uint64_t scanned(const uint64_t* v, const uint64_t* s1, const uint64_t* s2, uint64_t i) {
    return v[i] + s1[i >> 10] + s2[i >> 20];
}

// The last g in [0, n) with key(g) <= x, or 0 if there is none (key ascending).
template <typename X, typename Key>
__device__ __forceinline__ int last_at_or_before(int n, X x, Key key) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (key(m) <= x) lo = m;
        else hi = m;
    }
    return lo;
}

}  // namespace kf

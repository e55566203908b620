// kf_compact.h -- the count -> scan -> scatter compaction of a byte stream that
// the FASTA index, the FASTQ index's newline table and get_chunks share: a
// workgroup of kCompactBlock threads covers kCompactSpan bytes, kCompactPer per
// thread.  Each pre-pass brings its predicate (which of a thread's bytes produce
// an output) and its writes:
//   count    c = the thread's number of outputs; compact_count(c, blk)
//   scan     blk[0, nb) in place (compact_scan_kernel <<<1, 1024>>>, or levels)
//   scatter  the same c again; the thread's outputs go to the slots from
//            compact_first_slot(scanned blk[blockIdx.x], c)
// kf_scan.h's rule holds: every thread of the workgroup reaches both calls.
#pragma once
#include "kf_scan.h"

namespace kf {
namespace {

constexpr int kCompactBlock = 256;
constexpr int kCompactPer = 16;
constexpr uint32_t kCompactSpan = kCompactBlock * kCompactPer;   // 4 KiB per workgroup

// first byte of the calling thread
__device__ __forceinline__ uint64_t compact_p0() {
    return (uint64_t)blockIdx.x * kCompactSpan + (uint64_t)threadIdx.x * kCompactPer;
}

template <typename T>
__device__ __forceinline__ void compact_count(uint32_t c, T* blk) {
    __shared__ uint32_t red[kCompactBlock / 64];
    const uint32_t all = block_sum<kCompactBlock / 64>(c, red);
    if (threadIdx.x == 0) blk[blockIdx.x] = all;
}

__device__ __forceinline__ uint64_t compact_first_slot(uint64_t base, uint32_t c) {
    __shared__ uint32_t wsum[kCompactBlock / 64];
    return base + block_excl_scan<kCompactBlock / 64>(c, wsum);
}

// Exclusive scan of nb block counts in place (one workgroup); blk[nb] = total,
// also written to *total64 unless that is null.
__global__ void __launch_bounds__(1024) compact_scan_kernel(uint32_t* blk, uint32_t nb, uint64_t* total64) {
    const uint32_t all = scan_with_carry(
        nb, [&](uint32_t i) { return blk[i]; }, [&](uint32_t i, uint32_t p) { blk[i] = p; });
    if (threadIdx.x == 0) {
        blk[nb] = all;
        if (total64) *total64 = all;
    }
}

}  // namespace
}  // namespace kf

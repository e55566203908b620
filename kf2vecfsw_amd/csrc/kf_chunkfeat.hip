// kf_chunkfeat.hip -- kf_chunk_features: the chunk trainer's samples built on the device.
//
// get_chunks leaves one row of window counts per 10 kbp window.  The chunk
// trainer's dataset (kf2vec/datasets.py:27-101, Dataset_chunks_2rows) draws, for
// every item of every epoch, two contiguous runs of a genome's window rows, sums
// each run column-wise, divides by the grand total and scales.  This kernel does
// that for a table of (first row, row count) samples over a count matrix that
// stays in HBM: c_j = sum over the sample's rows of min(count, cap), T = sum of
// c_j over all columns, out[s][j] = (double)c_j / (double)T * scaler, rounded to
// float32 last when the output is float32.  Sums are exact u64; conversion,
// division and product round to nearest even (the library is built without
// fast-math), so the result equals numpy's float64 statement bit for bit.
//
// A streaming kernel: threads run along the columns, 16 bytes (8 u16 or 4 u32
// columns) per load where the rows allow it; a thread holds 32 columns of a TILE
// of kCTile = 8192 columns, walks its sample's rows (read once, non-temporal,
// several rows in flight) and keeps the 32 sums in registers.  A workgroup takes
// (sample, tile) items grid-stride.  T is a reduction over all columns:
//   nbins <= kCTile (every k <= 7): a sample is one tile, so the workgroup that
//     summed it reduces its threads' sums to T (shuffles + LDS) and divides: one
//     launch, the rows read once;
//   larger nbins: chunk_total_kernel folds each wave's sums and adds them to the
//     sample's u64 in d_work (one vector atomic per wave and item: integer adds,
//     so the result does not depend on their order); chunk_write_kernel then
//     sums the rows again (a second read) and divides by the finished total.
// The sample table is checked by every workgroup of every launch before it reads
// a row or writes anything (the table is small and stays in L2; no workgroup
// waits for another): a sample that leaves [0, n_rows] gives *d_status = 2 and
// leaves d_out alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <type_traits>

#include "kf_internal.h"

namespace kf {
namespace {

constexpr int kCBlock = 256;                 // threads per workgroup
constexpr int kCWaves = kCBlock / 64;
constexpr int kCCols = 32;                   // columns (u64 sums) per thread
constexpr int kCTile = kCBlock * kCCols;     // columns per tile: 8192, every k <= 7 in one
constexpr int kCMaxGrid = 256 * 8;           // workgroups: the rest of the items grid-stride

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// How a thread reads a row: one LOAD is L columns, a thread makes NV of them per
// row (kCBlock loads apart, so consecutive lanes read consecutive addresses) and
// keeps R rows in flight.
template <int CB, bool VEC>
struct Shape {
    using Load = std::conditional_t<VEC, v4u, std::conditional_t<CB == 2, uint16_t, uint32_t>>;
    static constexpr int L = VEC ? 16 / CB : 1;
    static constexpr int NV = kCCols / L;
    static constexpr int R = !VEC ? 1 : CB == 2 ? 4 : 2;   // 16 loads in flight per thread (32 on the scalar path)
};

__device__ __forceinline__ uint64_t capped(uint32_t v, uint32_t cap) { return v < cap ? v : cap; }

template <int CB>
__device__ __forceinline__ void add_load(uint64_t* acc, v4u a, uint32_t cap) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (CB == 2) {
            acc[2 * j] += capped(a[j] & 0xFFFFu, cap);
            acc[2 * j + 1] += capped(a[j] >> 16, cap);
        } else {
            acc[j] += capped(a[j], cap);
        }
    }
}
template <int CB>
__device__ __forceinline__ void add_load(uint64_t* acc, uint16_t a, uint32_t cap) { acc[0] += capped(a, cap); }
template <int CB>
__device__ __forceinline__ void add_load(uint64_t* acc, uint32_t a, uint32_t cap) { acc[0] += capped(a, cap); }

// the table: lo[s] + n[s] neither wraps nor passes n_rows, for every s (the same answer in every thread)
__device__ __forceinline__ int bad_table(const uint64_t* __restrict__ lo, const uint64_t* __restrict__ n,
                                         int32_t n_samples, uint64_t n_rows) {
    int bad = 0;
    for (int64_t s = threadIdx.x; s < n_samples; s += kCBlock) {
        const uint64_t m = n[s];
        bad |= m > n_rows || lo[s] > n_rows - m;
    }
    return __syncthreads_or(bad);
}

// acc[v * L + j] = the capped sum of column (u0 + v * kCBlock) * L + j over the rows [lo, lo + n);
// `cols` is the number of loads per row, loads at and past it count as zero columns
template <int CB, bool VEC>
__device__ __forceinline__ void tile_sums(const typename Shape<CB, VEC>::Load* __restrict__ src, uint64_t cols,
                                          uint64_t lo, uint64_t n, uint64_t u0, uint32_t cap, uint64_t* acc) {
    using S = Shape<CB, VEC>;
    using Load = typename S::Load;
#pragma unroll
    for (int i = 0; i < kCCols; ++i) acc[i] = 0;
    bool ok[S::NV];
#pragma unroll
    for (int v = 0; v < S::NV; ++v) ok[v] = u0 + (uint64_t)v * kCBlock < cols;
    const Load* p = src + lo * cols + u0;
    uint64_t r = 0;
    for (; r + S::R <= n; r += S::R, p += S::R * cols) {
        Load a[S::R][S::NV];
#pragma unroll
        for (int i = 0; i < S::R; ++i)
#pragma unroll
            for (int v = 0; v < S::NV; ++v)
                a[i][v] = ok[v] ? __builtin_nontemporal_load(p + i * cols + v * kCBlock) : Load{};
#pragma unroll
        for (int i = 0; i < S::R; ++i)
#pragma unroll
            for (int v = 0; v < S::NV; ++v) add_load<CB>(acc + v * S::L, a[i][v], cap);
    }
    for (; r < n; ++r, p += cols) {
        Load a[S::NV];
#pragma unroll
        for (int v = 0; v < S::NV; ++v) a[v] = ok[v] ? __builtin_nontemporal_load(p + v * kCBlock) : Load{};
#pragma unroll
        for (int v = 0; v < S::NV; ++v) add_load<CB>(acc + v * S::L, a[v], cap);
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t t) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_down((unsigned long long)t, d, 64);
    return t;   // in lane 0
}

// Launch 1 of 2 (nbins > kCTile): totals[s] += the sums of the sample's tile, per wave.
template <int CB, bool VEC>
__global__ void __launch_bounds__(kCBlock) chunk_total_kernel(const typename Shape<CB, VEC>::Load* __restrict__ src,
                                                              uint64_t n_rows, uint64_t cols,
                                                              const uint64_t* __restrict__ lo,
                                                              const uint64_t* __restrict__ n, int32_t n_samples,
                                                              uint32_t cap, uint64_t* totals) {
    using S = Shape<CB, VEC>;
    if (bad_table(lo, n, n_samples, n_rows)) return;
    const uint64_t tiles = (cols * S::L + kCTile - 1) / kCTile;
    const uint64_t items = tiles * (uint64_t)n_samples;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint64_t s = it / tiles;
        const uint64_t u0 = (it - s * tiles) * (uint64_t)(kCBlock * S::NV) + threadIdx.x;
        uint64_t acc[kCCols];
        tile_sums<CB, VEC>(src, cols, lo[s], n[s], u0, cap, acc);
        uint64_t t = 0;
#pragma unroll
        for (int i = 0; i < kCCols; ++i) t += acc[i];
        t = wave_sum(t);
        if ((threadIdx.x & 63) == 0 && t != 0) atomicAdd((unsigned long long*)(totals + s), (unsigned long long)t);
    }
}

template <typename OUT>
__device__ __forceinline__ OUT quotient(uint64_t c, uint64_t T, double dT, double scaler) {
    return T ? (OUT)((double)c / dT * scaler) : (OUT)0.0;
}

// The launch that writes.  totals == nullptr: nbins <= kCTile, a sample is one
// item and its total is reduced here; else totals[s] is the finished total.
template <int CB, bool VEC, typename OUT>
__global__ void __launch_bounds__(kCBlock) chunk_write_kernel(const typename Shape<CB, VEC>::Load* __restrict__ src,
                                                              uint64_t n_rows, uint64_t cols,
                                                              const uint64_t* __restrict__ lo,
                                                              const uint64_t* __restrict__ n, int32_t n_samples,
                                                              uint32_t cap, double scaler,
                                                              const uint64_t* __restrict__ totals,
                                                              OUT* __restrict__ out, uint32_t* status) {
    using S = Shape<CB, VEC>;
    __shared__ uint64_t s_part[kCWaves];
    const int bad = bad_table(lo, n, n_samples, n_rows);
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = bad ? 2u : 0u;
    if (bad) return;
    const uint64_t nbins = cols * S::L;
    const uint64_t tiles = (nbins + kCTile - 1) / kCTile;
    const uint64_t items = tiles * (uint64_t)n_samples;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint64_t s = it / tiles;
        const uint64_t u0 = (it - s * tiles) * (uint64_t)(kCBlock * S::NV) + threadIdx.x;
        uint64_t acc[kCCols];
        tile_sums<CB, VEC>(src, cols, lo[s], n[s], u0, cap, acc);
        uint64_t T;
        if (totals) {
            T = totals[s];
        } else {
            uint64_t t = 0;
#pragma unroll
            for (int i = 0; i < kCCols; ++i) t += acc[i];
            t = wave_sum(t);
            if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = t;
            __syncthreads();
            T = 0;
#pragma unroll
            for (int w = 0; w < kCWaves; ++w) T += s_part[w];
            __syncthreads();   // s_part is written again in the next item
        }
        const double dT = (double)T;
        OUT* const o = out + s * nbins;
#pragma unroll
        for (int v = 0; v < S::NV; ++v) {
            const uint64_t u = u0 + (uint64_t)v * kCBlock;
            if (u >= cols) continue;
            const uint64_t* a = acc + v * S::L;
            if constexpr (!VEC) {
                o[u] = quotient<OUT>(a[0], T, dT, scaler);
            } else if constexpr (sizeof(OUT) == 4) {
#pragma unroll
                for (int j = 0; j < S::L; j += 4) {
                    v4f q;
                    q.x = quotient<float>(a[j], T, dT, scaler);
                    q.y = quotient<float>(a[j + 1], T, dT, scaler);
                    q.z = quotient<float>(a[j + 2], T, dT, scaler);
                    q.w = quotient<float>(a[j + 3], T, dT, scaler);
                    *(v4f*)(o + u * S::L + j) = q;
                }
            } else {
#pragma unroll
                for (int j = 0; j < S::L; j += 2) {
                    v2d q;
                    q.x = quotient<double>(a[j], T, dT, scaler);
                    q.y = quotient<double>(a[j + 1], T, dT, scaler);
                    *(v2d*)(o + u * S::L + j) = q;
                }
            }
        }
    }
}

template <int CB, bool VEC>
int launch(const void* d_counts, uint64_t n_rows, uint64_t nbins, const uint64_t* d_lo, const uint64_t* d_n,
           int32_t n_samples, uint32_t cap, double scaler, void* d_out, int out_bytes, uint32_t* d_status,
           uint64_t* totals, hipStream_t s) {
    using S = Shape<CB, VEC>;
    using Load = typename S::Load;
    const uint64_t cols = nbins / S::L;
    const uint64_t items = (nbins + kCTile - 1) / kCTile * (uint64_t)n_samples;
    const uint32_t grid = (uint32_t)(items < (uint64_t)kCMaxGrid ? items : (uint64_t)kCMaxGrid);
    const bool two = nbins > (uint64_t)kCTile;
    if (two) {
        if (hipMemsetAsync(totals, 0, 8 * (size_t)n_samples, s) != hipSuccess)
            return kf_fail(KF_EHIP, "kf_chunk_features: memset failed");
        hipLaunchKernelGGL((chunk_total_kernel<CB, VEC>), dim3(grid), dim3(kCBlock), 0, s, (const Load*)d_counts, n_rows,
                           cols, d_lo, d_n, n_samples, cap, totals);
    }
    if (out_bytes == 4)
        hipLaunchKernelGGL((chunk_write_kernel<CB, VEC, float>), dim3(grid), dim3(kCBlock), 0, s, (const Load*)d_counts,
                           n_rows, cols, d_lo, d_n, n_samples, cap, scaler, two ? totals : nullptr, (float*)d_out,
                           d_status);
    else
        hipLaunchKernelGGL((chunk_write_kernel<CB, VEC, double>), dim3(grid), dim3(kCBlock), 0, s, (const Load*)d_counts,
                           n_rows, cols, d_lo, d_n, n_samples, cap, scaler, two ? totals : nullptr, (double*)d_out,
                           d_status);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_chunk_features: launch failed");
    return KF_OK;
}

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" uint64_t kf_chunk_features_scratch_bytes(int32_t n_samples) {
    return 8 * (uint64_t)(n_samples > 0 ? n_samples : 1);   // a u64 total per sample
}

extern "C" int kf_chunk_features(const void* d_counts, int count_bytes, uint64_t n_rows, uint64_t nbins,
                                 const uint64_t* d_lo, const uint64_t* d_n, int32_t n_samples, uint32_t cap,
                                 double scaler, void* d_out, int out_bytes, uint32_t* d_status, void* d_work,
                                 uint64_t work_bytes, void* stream) {
    if (count_bytes != 2 && count_bytes != 4)
        return kf_fail(KF_EINVAL, "kf_chunk_features: count_bytes=%d is neither 2 nor 4", count_bytes);
    if (out_bytes != 4 && out_bytes != 8)
        return kf_fail(KF_EINVAL, "kf_chunk_features: out_bytes=%d is neither 4 nor 8", out_bytes);
    if (nbins == 0) return kf_fail(KF_EINVAL, "kf_chunk_features: nbins == 0");
    if (n_samples < 0) return kf_fail(KF_EINVAL, "kf_chunk_features: negative sample count");
    if (!std::isfinite(scaler)) return kf_fail(KF_EINVAL, "kf_chunk_features: scaler is not finite");
    if (!d_counts && n_rows) return kf_fail(KF_EINVAL, "kf_chunk_features: null d_counts with n_rows > 0");
    if (!d_lo || !d_n) return kf_fail(KF_EINVAL, "kf_chunk_features: null sample table (d_lo, d_n)");
    if (!d_out) return kf_fail(KF_EINVAL, "kf_chunk_features: null d_out");
    if (!d_status) return kf_fail(KF_EINVAL, "kf_chunk_features: null d_status");
    if (!d_work) return kf_fail(KF_EINVAL, "kf_chunk_features: null d_work");
    if ((uintptr_t)d_counts & (uintptr_t)(count_bytes - 1))
        return kf_fail(KF_EINVAL, "kf_chunk_features: misaligned d_counts (needs %d bytes)", count_bytes);
    if (((uintptr_t)d_lo & 7) || ((uintptr_t)d_n & 7))
        return kf_fail(KF_EINVAL, "kf_chunk_features: misaligned sample table (d_lo, d_n need 8 bytes)");
    if ((uintptr_t)d_work & 7) return kf_fail(KF_EINVAL, "kf_chunk_features: misaligned d_work (needs 8 bytes)");
    if ((uintptr_t)d_out & (uintptr_t)(out_bytes - 1))
        return kf_fail(KF_EINVAL, "kf_chunk_features: misaligned d_out (needs %d bytes)", out_bytes);
    if ((uintptr_t)d_status & 3) return kf_fail(KF_EINVAL, "kf_chunk_features: misaligned d_status (needs 4 bytes)");
    const uint64_t need = kf_chunk_features_scratch_bytes(n_samples);
    if (work_bytes < need)
        return kf_fail(KF_ERANGE, "kf_chunk_features: scratch needs %llu bytes, %llu given", (unsigned long long)need,
                       (unsigned long long)work_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (n_samples == 0) {   // no table to check and nothing to write
        if (hipMemsetAsync(d_status, 0, 4, s) != hipSuccess)
            return kf_fail(KF_EHIP, "kf_chunk_features: memset failed");
        return KF_OK;
    }
    uint64_t* const totals = (uint64_t*)d_work;
    // 16 bytes per load where the row pitch and both base pointers allow it
    const bool vec = nbins % (uint64_t)(16 / count_bytes) == 0 && !((uintptr_t)d_counts & 15) && !((uintptr_t)d_out & 15);
#define KF_CF_LAUNCH(CB, VEC) \
    launch<CB, VEC>(d_counts, n_rows, nbins, d_lo, d_n, n_samples, cap, scaler, d_out, out_bytes, d_status, totals, s)
    if (count_bytes == 2) return vec ? KF_CF_LAUNCH(2, true) : KF_CF_LAUNCH(2, false);
    return vec ? KF_CF_LAUNCH(4, true) : KF_CF_LAUNCH(4, false);
#undef KF_CF_LAUNCH
}

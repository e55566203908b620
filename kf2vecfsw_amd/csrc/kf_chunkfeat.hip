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
//
// kf_chunk_features8 is the same templates over rows of one byte per count (the
// store that -cap keeps: every count already min(count, 255)), Shape<1, VEC>: 16
// columns per load, two loads per row and thread, eight rows in flight.  Its
// vector path adds the bytes of a load two to a 32-bit word (the even and the odd
// bytes of every word, masked, so four adds take in 16 columns) and folds these
// 16-bit partial sums into the u64 sums every kCFold8 = 256 rows, before one can
// pass 255 * 257 = 65535; the sums stay exact for any d_n.  kf_rows_cap8 makes
// such rows from u16 rows.
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
    using Load = std::conditional_t<VEC, v4u, std::conditional_t<CB == 1, uint8_t, std::conditional_t<CB == 2, uint16_t, uint32_t>>>;
    static constexpr int L = VEC ? 16 / CB : 1;
    static constexpr int NV = kCCols / L;
    static constexpr int R = !VEC ? 1 : CB == 1 ? 8 : CB == 2 ? 4 : 2;   // 16 loads in flight per thread (32 on the scalar path)
};
constexpr int kCFold8 = 256;   // rows of u8 counts between two folds of the 16-bit partial sums: 256 * 255 < 2^16
static_assert(kCFold8 % Shape<1, true>::R == 0 && (uint64_t)kCFold8 * 255 <= 0xFFFFu, "a partial sum may not wrap");

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
template <int CB>
__device__ __forceinline__ void add_load(uint64_t* acc, uint8_t a, uint32_t) { acc[0] += a; }   // u8 rows are capped rows

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

// tile_sums for u8 rows on the vector path.  part[v * 8 + 2 * j] holds the partial sums of the columns
// 4 j and 4 j + 2 of load v (bytes 0 and 2 of word j) in its halves, part[v * 8 + 2 * j + 1] those of the
// columns 4 j + 1 and 4 j + 3; they are folded into acc after at most kCFold8 rows.
__device__ __forceinline__ void fold8(uint64_t* acc, uint32_t* part) {
#pragma unroll
    for (int v = 0; v < Shape<1, true>::NV; ++v)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t* const q = part + v * 8 + 2 * j;
            uint64_t* const a = acc + v * 16 + 4 * j;
            a[0] += q[0] & 0xFFFFu;
            a[1] += q[1] & 0xFFFFu;
            a[2] += q[0] >> 16;
            a[3] += q[1] >> 16;
            q[0] = q[1] = 0;
        }
}
__device__ __forceinline__ void add_load8(uint32_t* part, v4u a) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        part[2 * j] += a[j] & 0x00FF00FFu;
        part[2 * j + 1] += (a[j] >> 8) & 0x00FF00FFu;
    }
}
__device__ __forceinline__ void tile_sums8(const v4u* __restrict__ src, uint64_t cols, uint64_t lo, uint64_t n,
                                           uint64_t u0, uint64_t* acc) {
    using S = Shape<1, true>;
#pragma unroll
    for (int i = 0; i < kCCols; ++i) acc[i] = 0;
    uint32_t part[kCCols / 2];
#pragma unroll
    for (int i = 0; i < kCCols / 2; ++i) part[i] = 0;
    bool ok[S::NV];
#pragma unroll
    for (int v = 0; v < S::NV; ++v) ok[v] = u0 + (uint64_t)v * kCBlock < cols;
    const v4u* p = src + lo * cols + u0;
    uint64_t r = 0;
    while (r + S::R <= n) {
        const uint64_t left = (n - r) / S::R, most = kCFold8 / S::R;
        const uint64_t end = r + (left < most ? left : most) * S::R;   // whole rounds of R rows, kCFold8 rows at most
        for (; r < end; r += S::R, p += S::R * cols) {
            v4u a[S::R][S::NV];
#pragma unroll
            for (int i = 0; i < S::R; ++i)
#pragma unroll
                for (int v = 0; v < S::NV; ++v)
                    a[i][v] = ok[v] ? __builtin_nontemporal_load(p + i * cols + v * kCBlock) : v4u{};
#pragma unroll
            for (int i = 0; i < S::R; ++i)
#pragma unroll
                for (int v = 0; v < S::NV; ++v) add_load8(part + v * 8, a[i][v]);
        }
        fold8(acc, part);
    }
    for (; r < n; ++r, p += cols) {   // fewer than R rows: their partial sums start at zero
        v4u a[S::NV];
#pragma unroll
        for (int v = 0; v < S::NV; ++v) a[v] = ok[v] ? __builtin_nontemporal_load(p + v * kCBlock) : v4u{};
#pragma unroll
        for (int v = 0; v < S::NV; ++v) add_load8(part + v * 8, a[v]);
    }
    fold8(acc, part);
}

template <int CB, bool VEC>
__device__ __forceinline__ void sample_sums(const typename Shape<CB, VEC>::Load* __restrict__ src, uint64_t cols,
                                            uint64_t lo, uint64_t n, uint64_t u0, uint32_t cap, uint64_t* acc) {
    if constexpr (CB == 1 && VEC)
        tile_sums8(src, cols, lo, n, u0, acc);
    else
        tile_sums<CB, VEC>(src, cols, lo, n, u0, cap, acc);
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
        sample_sums<CB, VEC>(src, cols, lo[s], n[s], u0, cap, acc);
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
        sample_sums<CB, VEC>(src, cols, lo[s], n[s], u0, cap, acc);
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
           uint64_t* totals, hipStream_t s, const char* who) {
    using S = Shape<CB, VEC>;
    using Load = typename S::Load;
    const uint64_t cols = nbins / S::L;
    const uint64_t items = (nbins + kCTile - 1) / kCTile * (uint64_t)n_samples;
    const uint32_t grid = (uint32_t)(items < (uint64_t)kCMaxGrid ? items : (uint64_t)kCMaxGrid);
    const bool two = nbins > (uint64_t)kCTile;
    if (two) {
        if (hipMemsetAsync(totals, 0, 8 * (size_t)n_samples, s) != hipSuccess)
            return kf_fail(KF_EHIP, "%s: memset failed", who);
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
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "%s: launch failed", who);
    return KF_OK;
}

// kf_rows_cap8: dst[i] = min(src[i], 255).  A streaming kernel: thread t < groups takes the 16 elements from
// head + 16 t on (two 16-byte loads, one 16-byte store; the host chose `head` so that both are aligned), every
// later thread one of the elements in front of `head` or behind the last group.
constexpr int kCapMaxGrid = 256 * 8;

__device__ __forceinline__ uint32_t cap2(uint32_t w) {   // two u16 to two bytes
    const uint32_t a = w & 0xFFFFu, b = w >> 16;
    return (a < 255u ? a : 255u) | (b < 255u ? b : 255u) << 8;
}

__global__ void __launch_bounds__(kCBlock) rows_cap8_kernel(const uint16_t* __restrict__ src, uint64_t n,
                                                            uint8_t* __restrict__ dst, uint64_t head, uint64_t groups) {
    const uint64_t threads = groups + (n - 16 * groups);
    for (uint64_t t = (uint64_t)blockIdx.x * kCBlock + threadIdx.x; t < threads; t += (uint64_t)gridDim.x * kCBlock) {
        if (t < groups) {
            const v4u* const p = (const v4u*)(src + head + 16 * t);
            const v4u x = __builtin_nontemporal_load(p), y = __builtin_nontemporal_load(p + 1);
            v4u o;
            o.x = cap2(x.x) | cap2(x.y) << 16;
            o.y = cap2(x.z) | cap2(x.w) << 16;
            o.z = cap2(y.x) | cap2(y.y) << 16;
            o.w = cap2(y.z) | cap2(y.w) << 16;
            *(v4u*)(dst + head + 16 * t) = o;
        } else {
            const uint64_t e = t - groups, i = e < head ? e : 16 * groups + e;
            const uint16_t v = src[i];
            dst[i] = (uint8_t)(v < 255 ? v : 255);
        }
    }
}

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" uint64_t kf_chunk_features_scratch_bytes(int32_t n_samples) {
    return 8 * (uint64_t)(n_samples > 0 ? n_samples : 1);   // a u64 total per sample
}

// Both entries behind their own check of count_bytes (1, 2 or 4 here); `who` names the entry in the messages.
static int chunk_features(const char* who, const void* d_counts, int count_bytes, uint64_t n_rows, uint64_t nbins,
                          const uint64_t* d_lo, const uint64_t* d_n, int32_t n_samples, uint32_t cap, double scaler,
                          void* d_out, int out_bytes, uint32_t* d_status, void* d_work, uint64_t work_bytes,
                          void* stream) {
    if (out_bytes != 4 && out_bytes != 8)
        return kf_fail(KF_EINVAL, "%s: out_bytes=%d is neither 4 nor 8", who, out_bytes);
    if (nbins == 0) return kf_fail(KF_EINVAL, "%s: nbins == 0", who);
    if (n_samples < 0) return kf_fail(KF_EINVAL, "%s: negative sample count", who);
    if (!std::isfinite(scaler)) return kf_fail(KF_EINVAL, "%s: scaler is not finite", who);
    if (!d_counts && n_rows) return kf_fail(KF_EINVAL, "%s: null d_counts with n_rows > 0", who);
    if (!d_lo || !d_n) return kf_fail(KF_EINVAL, "%s: null sample table (d_lo, d_n)", who);
    if (!d_out) return kf_fail(KF_EINVAL, "%s: null d_out", who);
    if (!d_status) return kf_fail(KF_EINVAL, "%s: null d_status", who);
    if (!d_work) return kf_fail(KF_EINVAL, "%s: null d_work", who);
    if ((uintptr_t)d_counts & (uintptr_t)(count_bytes - 1))
        return kf_fail(KF_EINVAL, "%s: misaligned d_counts (needs %d bytes)", who, count_bytes);
    if (((uintptr_t)d_lo & 7) || ((uintptr_t)d_n & 7))
        return kf_fail(KF_EINVAL, "%s: misaligned sample table (d_lo, d_n need 8 bytes)", who);
    if ((uintptr_t)d_work & 7) return kf_fail(KF_EINVAL, "%s: misaligned d_work (needs 8 bytes)", who);
    if ((uintptr_t)d_out & (uintptr_t)(out_bytes - 1))
        return kf_fail(KF_EINVAL, "%s: misaligned d_out (needs %d bytes)", who, out_bytes);
    if ((uintptr_t)d_status & 3) return kf_fail(KF_EINVAL, "%s: misaligned d_status (needs 4 bytes)", who);
    const uint64_t need = kf_chunk_features_scratch_bytes(n_samples);
    if (work_bytes < need)
        return kf_fail(KF_ERANGE, "%s: scratch needs %llu bytes, %llu given", who, (unsigned long long)need,
                       (unsigned long long)work_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (n_samples == 0) {   // no table to check and nothing to write
        if (hipMemsetAsync(d_status, 0, 4, s) != hipSuccess)
            return kf_fail(KF_EHIP, "%s: memset failed", who);
        return KF_OK;
    }
    uint64_t* const totals = (uint64_t*)d_work;
    // 16 bytes per load where the row pitch and both base pointers allow it
    const bool vec = nbins % (uint64_t)(16 / count_bytes) == 0 && !((uintptr_t)d_counts & 15) && !((uintptr_t)d_out & 15);
#define KF_CF_LAUNCH(CB, VEC) \
    launch<CB, VEC>(d_counts, n_rows, nbins, d_lo, d_n, n_samples, cap, scaler, d_out, out_bytes, d_status, totals, s, who)
    if (count_bytes == 1) return vec ? KF_CF_LAUNCH(1, true) : KF_CF_LAUNCH(1, false);
    if (count_bytes == 2) return vec ? KF_CF_LAUNCH(2, true) : KF_CF_LAUNCH(2, false);
    return vec ? KF_CF_LAUNCH(4, true) : KF_CF_LAUNCH(4, false);
#undef KF_CF_LAUNCH
}

extern "C" int kf_chunk_features(const void* d_counts, int count_bytes, uint64_t n_rows, uint64_t nbins,
                                 const uint64_t* d_lo, const uint64_t* d_n, int32_t n_samples, uint32_t cap,
                                 double scaler, void* d_out, int out_bytes, uint32_t* d_status, void* d_work,
                                 uint64_t work_bytes, void* stream) {
    if (count_bytes != 2 && count_bytes != 4)
        return kf_fail(KF_EINVAL, "kf_chunk_features: count_bytes=%d is neither 2 nor 4", count_bytes);
    return chunk_features("kf_chunk_features", d_counts, count_bytes, n_rows, nbins, d_lo, d_n, n_samples, cap, scaler,
                          d_out, out_bytes, d_status, d_work, work_bytes, stream);
}

extern "C" int kf_chunk_features8(const uint8_t* d_counts, uint64_t n_rows, uint64_t nbins, const uint64_t* d_lo,
                                  const uint64_t* d_n, int32_t n_samples, double scaler, void* d_out, int out_bytes,
                                  uint32_t* d_status, void* d_work, uint64_t work_bytes, void* stream) {
    return chunk_features("kf_chunk_features8", d_counts, 1, n_rows, nbins, d_lo, d_n, n_samples, UINT32_MAX, scaler,
                          d_out, out_bytes, d_status, d_work, work_bytes, stream);
}

extern "C" int kf_rows_cap8(const uint16_t* d_src, uint64_t n, uint8_t* d_dst, void* stream) {
    if (n == 0) return KF_OK;
    if (!d_src) return kf_fail(KF_EINVAL, "kf_rows_cap8: null d_src");
    if (!d_dst) return kf_fail(KF_EINVAL, "kf_rows_cap8: null d_dst");
    if ((uintptr_t)d_src & 1) return kf_fail(KF_EINVAL, "kf_rows_cap8: misaligned d_src (needs 2 bytes)");
    // the head up to d_dst's next 16-byte line goes element by element, so that the body's stores are aligned;
    // its loads are 16 bytes too where d_src is then aligned as well
    uint64_t head = (16 - ((uintptr_t)d_dst & 15)) & 15;
    if (head > n) head = n;
    const bool vec = !((uintptr_t)(d_src + head) & 15);
    const uint64_t groups = vec ? (n - head) / 16 : 0;
    const uint64_t threads = groups + (n - 16 * groups);   // a thread per 16-element group, and one per other element
    const uint64_t blocks = (threads + kCBlock - 1) / kCBlock;
    const uint32_t grid = (uint32_t)(blocks < (uint64_t)kCapMaxGrid ? blocks : (uint64_t)kCapMaxGrid);
    hipLaunchKernelGGL(rows_cap8_kernel, dim3(grid), dim3(kCBlock), 0, (hipStream_t)stream, d_src, n, d_dst, head,
                       groups);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_rows_cap8: launch failed");
    return KF_OK;
}

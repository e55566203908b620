// kf_kmers.hip -- kf_kmers_rows: the get_kmers matrix built on the device.
//
// get_kmers (kf2vec/main.py:147-172) writes, per genome, a float32 matrix with one
// row per present canonical k-mer: its k bases as digits (A0 T1 C2 G3,
// main.py:118) and its count divided by the genome's total.  The counters leave
// (key, count) pairs in HBM; this kernel expands them into rows there: 12 bytes
// in (16 with u64 counts), 4 (k + 1) bytes out, every row independent.
//
// A streaming store kernel.  The output of a call is the slab of rows
// [row_lo, row_hi) of a matrix that several segments (genomes) tile; a workgroup
// takes tiles of kKTileRows slab rows grid-stride.  Per tile it finds the first
// row's segment by a binary search of the segments' first rows and every thread
// walks on from there for its rows; it loads its rows' keys and counts once
// (consecutive lanes on consecutive rows), divides, and stages key and quotient
// in LDS (12 KiB).  Then the tile leaves as one flat stream of 16-byte
// non-temporal stores, consecutive lanes on consecutive 16 bytes: an element's
// (row, column) is a division by the compile-time row width k + 1, its value a
// shift of the staged key or the staged quotient.  kKTileRows is a multiple of 4,
// so every tile starts 16-byte aligned in the slab; only the slab's last tile can
// end in up to three 4-byte stores.  A row that belongs to no key (the gap behind
// a segment's rows, the padding of a [B, Nmax, k + 1] batch) is staged as key 0,
// quotient 0: all zeros.  The tables are checked by every workgroup before it
// writes (they are small and stay in L2; no workspace, and no workgroup waits
// for another).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "kf_internal.h"

namespace kf {
namespace {

constexpr int kKBlock = 256;         // threads per workgroup
constexpr int kKTileRows = 1024;     // slab rows per tile (a multiple of 4: tiles start 16-byte aligned)
constexpr int kKMaxGrid = 256 * 8;   // workgroups (8 of them fill a CU's wave slots): the rest of the tiles grid-stride

static_assert(kKTileRows % 4 == 0, "a tile must start on a 16-byte boundary of the slab");

typedef float v4f __attribute__((ext_vector_type(4)));

template <int K>
__global__ void __launch_bounds__(kKBlock) kmers_rows_kernel(const uint64_t* __restrict__ keys,
                                                             const void* __restrict__ counts, int count_bytes,
                                                             const uint64_t* __restrict__ src0,
                                                             const uint64_t* __restrict__ n,
                                                             const uint64_t* __restrict__ dst0,
                                                             const float* __restrict__ denom, int32_t n_seg,
                                                             uint64_t row_lo, uint64_t row_hi, float* __restrict__ out,
                                                             uint32_t* status) {
    constexpr uint32_t W = K + 1;   // floats per row
    __shared__ uint64_t s_key[kKTileRows];
    __shared__ float s_q[kKTileRows];

    // the tables: dst0[0] <= ... <= dst0[n_seg], n[s] <= dst0[s+1] - dst0[s], row_hi <= dst0[n_seg]
    int bad = 0;
    for (int64_t s = threadIdx.x; s < n_seg; s += kKBlock) {
        const uint64_t a = dst0[s], b = dst0[s + 1];
        bad |= b < a || n[s] > b - a;
    }
    if (threadIdx.x == 0) bad |= row_hi > dst0[n_seg];
    bad = __syncthreads_or(bad);
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = bad ? 2u : 0u;
    if (bad) return;

    // element (row, col) of the staged tile: a digit of the key, first base first
    // (standard code A0 C1 G2 T3 -> get_kmers digit A0 T1 C2 G3: [0, 2, 3, 1]), or the quotient
    auto value = [&](uint32_t row, uint32_t col) -> float {
        if (col == (uint32_t)K) return s_q[row];
        const uint32_t d = (uint32_t)(s_key[row] >> (2 * ((uint32_t)K - 1 - col))) & 3u;
        return (float)((0x78u >> (2 * d)) & 3u);
    };

    const uint64_t tiles = (row_hi - row_lo + kKTileRows - 1) / kKTileRows;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = row_lo + t * kKTileRows;
        const uint32_t nr = (uint32_t)(row_hi - r0 < (uint64_t)kKTileRows ? row_hi - r0 : (uint64_t)kKTileRows);
        // the number of segments that start at or before the tile's first row
        int64_t lo = 0, hi = n_seg;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (dst0[mid] <= r0) lo = mid + 1; else hi = mid;
        }
        int64_t s = lo - 1;   // the last of them (-1: the row lies before every segment); a thread's rows ascend
        for (uint32_t i = threadIdx.x; i < nr; i += kKBlock) {
            const uint64_t r = r0 + i;
            while (s + 1 < n_seg && dst0[s + 1] <= r) ++s;
            uint64_t key = 0;
            float q = 0.0f;
            if (s >= 0) {
                const uint64_t j = r - dst0[s];
                if (j < n[s]) {
                    const uint64_t x = src0[s] + j;
                    key = __builtin_nontemporal_load(keys + x);
                    const float c = count_bytes == 8 ? (float)__builtin_nontemporal_load((const uint64_t*)counts + x)
                                                     : (float)__builtin_nontemporal_load((const uint32_t*)counts + x);
                    q = __fdiv_rn(c, denom[s]);
                }
            }
            s_key[i] = key;
            s_q[i] = q;
        }
        __syncthreads();
        float* const o = out + t * (uint64_t)kKTileRows * W;
        const uint32_t elems = nr * W, chunks = elems >> 2;
        for (uint32_t c = threadIdx.x; c < chunks; c += kKBlock) {
            uint32_t row = (4 * c) / W, col = 4 * c - row * W;
            v4f v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = value(row, col);
                if (++col == W) {
                    col = 0;
                    ++row;
                }
            }
            __builtin_nontemporal_store(v, (v4f*)o + c);
        }
        for (uint32_t e = 4 * chunks + threadIdx.x; e < elems; e += kKBlock) o[e] = value(e / W, e % W);   // slab tail
        __syncthreads();
    }
}

using KmersKernel = decltype(&kmers_rows_kernel<KF_MIN_K>);

// the instantiation for k, out of kmers_rows_kernel<KF_MIN_K + I> for every I of the sequence
template <int... I>
constexpr KmersKernel kernel_for(int k, std::integer_sequence<int, I...>) {
    KmersKernel f = nullptr;
    ((k == KF_MIN_K + I ? (void)(f = kmers_rows_kernel<KF_MIN_K + I>) : (void)0), ...);
    return f;
}

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_kmers_tile_rows(void) { return kKTileRows; }

extern "C" int kf_kmers_rows(const uint64_t* d_keys, const void* d_counts, int count_bytes, const uint64_t* d_src0,
                             const uint64_t* d_n, const uint64_t* d_dst0, const float* d_denom, int32_t n_seg, int k,
                             uint64_t row_lo, uint64_t row_hi, float* d_out, uint32_t* d_status, void* stream) {
    if (k < KF_MIN_K || k > KF_SPARSE_MAX_K)
        return kf_fail(KF_EINVAL, "kf_kmers_rows: k=%d out of range [%d, %d]", k, KF_MIN_K, KF_SPARSE_MAX_K);
    if (count_bytes != 4 && count_bytes != 8)
        return kf_fail(KF_EINVAL, "kf_kmers_rows: count_bytes=%d is neither 4 nor 8", count_bytes);
    if (n_seg < 0) return kf_fail(KF_EINVAL, "kf_kmers_rows: negative segment count");
    if (row_lo > row_hi) return kf_fail(KF_EINVAL, "kf_kmers_rows: row_lo > row_hi");
    if (!d_keys || !d_counts || !d_src0 || !d_n || !d_dst0 || !d_denom || !d_out || !d_status)
        return kf_fail(KF_EINVAL, "kf_kmers_rows: null device pointer");
    if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_counts & (uintptr_t)(count_bytes - 1)) || ((uintptr_t)d_src0 & 7) ||
        ((uintptr_t)d_n & 7) || ((uintptr_t)d_dst0 & 7) || ((uintptr_t)d_denom & 3) || ((uintptr_t)d_out & 15) ||
        ((uintptr_t)d_status & 3))
        return kf_fail(KF_EINVAL, "kf_kmers_rows: misaligned device pointer (d_out needs 16 bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (n_seg == 0) {   // no table to check and no row to write
        if (hipMemsetAsync(d_status, 0, 4, s) != hipSuccess) return kf_fail(KF_EHIP, "kf_kmers_rows: memset failed");
        return KF_OK;
    }
    // an empty slab still runs one workgroup: the tables are checked, nothing is written
    const uint64_t tiles = (row_hi - row_lo + kKTileRows - 1) / kKTileRows;
    const uint32_t grid = (uint32_t)(tiles < 1 ? 1 : tiles < (uint64_t)kKMaxGrid ? tiles : (uint64_t)kKMaxGrid);
    const KmersKernel f = kernel_for(k, std::make_integer_sequence<int, KF_SPARSE_MAX_K - KF_MIN_K + 1>{});
    hipLaunchKernelGGL(f, dim3(grid), dim3(kKBlock), 0, s, d_keys, d_counts, count_bytes, d_src0, d_n, d_dst0, d_denom,
                       n_seg, row_lo, row_hi, d_out, d_status);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_kmers_rows: launch failed");
    return KF_OK;
}

// kf_rows.hip -- kf_rows_accumulate: column-wise sums of count rows on the device.
//
// get_frequencies counts a file above its split limit in pieces, each piece one
// "genome" of a batch (one row of kf_count_batch's matrix); this kernel adds the
// piece rows up into one row per file: destination row r receives the sum of the
// source rows [seg[r], seg[r+1]) (the seg_row0 idiom of kf_write_kf_segments),
// added to what it holds under KF_ACCUMULATE, so a file's pieces may span several
// batches.  The reference counts a file of any size in one Jellyfish hash
// (kf2vec/main.py:309-311); a sum of u32 piece counts can pass 2^32 - 1 where
// that hash would not, so the add detects its carry: the column saturates at
// UINT32_MAX and bit 0 of the row's status word is set.
//
// A streaming kernel: threads run along the columns, four columns (16 bytes) per
// thread where the rows allow it, each thread walks its segment's source rows
// (read once, non-temporal, four rows in flight) and writes its destination
// columns once.  A workgroup takes (row, column tile) items grid-stride; every
// wave of it works on one destination row, folds its lanes' carry flags and
// issues at most one atomic OR on the row's status word.  The segment table is
// checked by every workgroup before it writes (the table is small and stays in
// L2; no workspace, and no workgroup waits for another): a table that is not
// non-decreasing inside [0, n_src] leaves d_dst and d_dst_totals alone and sets
// every status word to 2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_internal.h"

namespace kf {
namespace {

constexpr int kRBlock = 256;         // threads per workgroup
constexpr int kRMaxGrid = 256 * 16;  // workgroups: the rest of the items grid-stride

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// a + b, saturating at UINT32_MAX; ovf collects the carries
__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b, uint32_t& ovf) {
    const uint32_t s = a + b;
    const uint32_t c = s < a ? 0xFFFFFFFFu : 0u;
    ovf |= c;
    return s | c;
}

__device__ __forceinline__ void sat_add(uint32_t& a, uint32_t b, uint32_t& ovf, int) { a = sat_add(a, b, ovf); }

__device__ __forceinline__ void sat_add(v4u& a, v4u b, uint32_t& ovf, int) {
    a.x = sat_add(a.x, b.x, ovf);
    a.y = sat_add(a.y, b.y, ovf);
    a.z = sat_add(a.z, b.z, ovf);
    a.w = sat_add(a.w, b.w, ovf);
}

// T = v4u: rows of nbins % 4 == 0 columns, 16-byte aligned; T = uint32_t: any rows.
// `cols` is the number of T per row.
template <typename T>
__global__ void __launch_bounds__(kRBlock) rows_accumulate_kernel(const T* __restrict__ src,
                                                                  const uint64_t* __restrict__ src_totals, int32_t n_src,
                                                                  const int32_t* __restrict__ seg, int32_t n_dst,
                                                                  uint64_t cols, T* __restrict__ dst,
                                                                  uint64_t* __restrict__ dst_totals, uint32_t* status,
                                                                  uint32_t accumulate) {
    // the segment table: 0 <= seg[0] <= ... <= seg[n_dst] <= n_src
    int bad = 0;
    for (int64_t i = threadIdx.x; i <= n_dst; i += kRBlock) {
        const int32_t v = seg[i];
        bad |= v < 0 || v > n_src || (i > 0 && seg[i - 1] > v);
    }
    if (__syncthreads_or(bad)) {
        for (int64_t r = (int64_t)blockIdx.x * kRBlock + threadIdx.x; r < n_dst; r += (int64_t)gridDim.x * kRBlock)
            status[r] = 2u;
        return;
    }
    const uint64_t tiles = (cols + kRBlock - 1) / kRBlock;
    const uint64_t items = tiles * (uint64_t)n_dst;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int32_t r = (int32_t)(it / tiles);
        const uint64_t c = (it - (uint64_t)r * tiles) * kRBlock + threadIdx.x;
        const int32_t s0 = seg[r], s1 = seg[r + 1];
        if (accumulate && s0 == s1) continue;   // an empty segment leaves the row, its total and status alone
        if (c == 0) {
            uint64_t t = accumulate ? dst_totals[r] : 0;
            for (int32_t s = s0; s < s1; ++s) t += src_totals[s];
            dst_totals[r] = t;
        }
        uint32_t ovf = 0;
        if (c < cols) {
            T* const d = dst + (uint64_t)r * cols + c;
            T acc = accumulate ? *d : T{};
            const T* p = src + (uint64_t)s0 * cols + c;
            int32_t s = s0;
            for (; s + 4 <= s1; s += 4, p += 4 * cols) {   // four rows in flight
                const T a0 = __builtin_nontemporal_load(p);
                const T a1 = __builtin_nontemporal_load(p + cols);
                const T a2 = __builtin_nontemporal_load(p + 2 * cols);
                const T a3 = __builtin_nontemporal_load(p + 3 * cols);
                sat_add(acc, a0, ovf, 0);
                sat_add(acc, a1, ovf, 0);
                sat_add(acc, a2, ovf, 0);
                sat_add(acc, a3, ovf, 0);
            }
            for (; s < s1; ++s, p += cols) sat_add(acc, __builtin_nontemporal_load(p), ovf, 0);
            *d = acc;
        }
        // one OR per wave and row, and only from a wave that saw a carry
        if (__builtin_amdgcn_ballot_w64(ovf != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(status + r, 1u);
    }
}

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_rows_accumulate(const uint32_t* d_src, const uint64_t* d_src_totals, int32_t n_src,
                                  const int32_t* d_seg, int32_t n_dst, uint64_t nbins, uint32_t* d_dst,
                                  uint64_t* d_dst_totals, uint32_t* d_status, uint32_t flags, void* stream) {
    if (n_src < 0 || n_dst < 0) return kf_fail(KF_EINVAL, "kf_rows_accumulate: negative row count");
    if (nbins == 0) return kf_fail(KF_EINVAL, "kf_rows_accumulate: nbins == 0");
    if (!d_src || !d_src_totals || !d_seg || !d_dst || !d_dst_totals || !d_status)
        return kf_fail(KF_EINVAL, "kf_rows_accumulate: null device pointer");
    if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3) || ((uintptr_t)d_src_totals & 7) ||
        ((uintptr_t)d_dst_totals & 7) || ((uintptr_t)d_seg & 3) || ((uintptr_t)d_status & 3))
        return kf_fail(KF_EINVAL, "kf_rows_accumulate: misaligned device pointer");
    if (n_dst == 0) return KF_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t acc = flags & KF_ACCUMULATE;
    if (!acc && hipMemsetAsync(d_status, 0, 4 * (size_t)n_dst, s) != hipSuccess)
        return kf_fail(KF_EHIP, "kf_rows_accumulate: memset failed");
    const bool vec = nbins % 4 == 0 && !((uintptr_t)d_src & 15) && !((uintptr_t)d_dst & 15);
    const uint64_t cols = vec ? nbins / 4 : nbins;
    const uint64_t items = (cols + kRBlock - 1) / kRBlock * (uint64_t)n_dst;
    const uint32_t grid = (uint32_t)(items < (uint64_t)kRMaxGrid ? items : (uint64_t)kRMaxGrid);
    if (vec)
        hipLaunchKernelGGL(rows_accumulate_kernel<v4u>, dim3(grid), dim3(kRBlock), 0, s, (const v4u*)d_src, d_src_totals,
                           n_src, d_seg, n_dst, cols, (v4u*)d_dst, d_dst_totals, d_status, acc);
    else
        hipLaunchKernelGGL(rows_accumulate_kernel<uint32_t>, dim3(grid), dim3(kRBlock), 0, s, d_src, d_src_totals,
                           n_src, d_seg, n_dst, cols, d_dst, d_dst_totals, d_status, acc);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_rows_accumulate: launch failed");
    return KF_OK;
}

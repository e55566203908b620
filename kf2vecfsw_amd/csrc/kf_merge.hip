// kf_merge.hip -- kf_sparse_merge: the union of two sorted (key, count) lists.
//
// get_kmers counts a FASTA file above 1 GiB in pieces (main.py, fasta_pieces);
// kf_sparse_count leaves every piece's distinct k-mers strictly ascending with
// their counts.  This merges a piece into its file's running result: the
// ascending union of the keys, a key of both lists once with the sum of its two
// counts (u64).  Two inputs in, one output out; no sort and no copy of the inputs.
//
// Merge path in tiles of kMTile merged positions.  On a tie A goes first, so an
// equal pair is always (A's entry, then B's) and, the inputs being strictly
// ascending, the output is: every entry of A, with its count plus that of the
// equal entry of B if there is one (then the next entry in merged order), and
// every entry of B whose key is not the entry of A before it.  Launches:
//   check    both lists strictly ascending?  *status = 1 if not.  It runs FIRST:
//            merge-path splits are not monotone for unsorted input, so nothing
//            that depends on the order runs on such input -- the count and
//            scatter kernels return at once when the check failed (the other
//            option of the contract, clamping every tile's ranges, is not used).
//   count    one workgroup per tile: its split by a binary search along its
//            diagonal (kept in scratch), its ranges of A and B into LDS, the
//            merge (each thread kMPer consecutive positions after a search of
//            its own in LDS), the tile's number of output entries to scratch
//            (0 for every tile if the check failed, so *n_out becomes 0)
//   scan     those numbers, by the three levels of kf_scan.h; the total is *n_out
//   scatter  the tile's merge again from the stored split; its output entries,
//            compacted in LDS, leave as consecutive 8-byte stores from its slot
// The inputs are read twice (12 or 16 B per entry each time) and their keys once
// more by the check, the output is written once (16 B per entry).
//
// LDS per workgroup: (kMTile + 2) keys and as many u64 counts, 32 KiB, so four
// workgroups fit a CU's 160 KiB (the count kernel holds the keys only).  A tile's
// entries of A carry A's entry before them (does the tile's first entry of B
// repeat it?) and its entries of B the one after them (does it repeat the tile's
// last entry of A?), where those exist.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_internal.h"
#include "kf_scan.h"

namespace kf {
namespace {

constexpr int kMBlock = 256;                 // threads per workgroup
constexpr int kMPer = 8;                     // merged positions per thread
constexpr int kMTile = kMBlock * kMPer;      // merged positions per tile
constexpr int kMCheckGrid = 256 * 8;         // workgroups of the order check (grid-stride)
// 2^23 tiles: one workgroup per tile stays below 2^32 threads per launch, and the
// three scan levels cover 2^30 tiles
constexpr uint64_t kMMaxEntries = 1ull << 34;

static_assert(kMMaxEntries / kMTile <= kScanMaxEntries, "the tile counts must fit the three scan levels");
static_assert(kMMaxEntries / kMTile * kMBlock < (1ull << 32), "a launch stays below 2^32 threads");

inline uint64_t div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Scratch layout in 64-bit words: every tile's split (its first index in A) and
// its number of output entries with the two levels of their sums.
struct MergeLayout {
    uint64_t tiles, nb1, nb2;
    uint64_t split, heads, heads1, heads2, words;
};

inline MergeLayout merge_layout(uint64_t n) {
    MergeLayout L;
    L.tiles = div_up(n, kMTile);
    L.nb1 = div_up(L.tiles, kScanLevel);
    L.nb2 = div_up(L.nb1, kScanLevel);
    uint64_t w = 0;
    L.split = w, w += L.tiles;
    L.heads = w, w += L.tiles;
    L.heads1 = w, w += L.nb1;
    L.heads2 = w, w += L.nb2 + 1;   // (never empty)
    L.words = w;
    return L;
}

// Adjacent pairs of the two lists, grid-stride: position i < n_a is the pair
// (A[i], A[i+1]), position n_a + j the pair (B[j], B[j+1]).  *status was zeroed.
__global__ void __launch_bounds__(kMBlock) merge_check_kernel(const uint64_t* __restrict__ ka, uint64_t n_a,
                                                              const uint64_t* __restrict__ kb, uint64_t n_b,
                                                              uint32_t* status) {
    int bad = 0;
    const uint64_t n = n_a + n_b;
    for (uint64_t i = (uint64_t)blockIdx.x * kMBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kMBlock) {
        if (i < n_a) {
            if (i + 1 < n_a) bad |= ka[i] >= ka[i + 1];
        } else {
            const uint64_t j = i - n_a;
            if (j + 1 < n_b) bad |= kb[j] >= kb[j + 1];
        }
    }
    bad = __syncthreads_or(bad);
    if (bad && threadIdx.x == 0) atomicOr(status, 1u);
}

// The number of entries of A among the first d of the merged order (ties: A first).
__device__ __forceinline__ uint64_t merge_split(const uint64_t* __restrict__ ka, uint64_t n_a,
                                                const uint64_t* __restrict__ kb, uint64_t n_b, uint64_t d) {
    uint64_t lo = d > n_b ? d - n_b : 0, hi = d < n_a ? d : n_a;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);   // mid < n_a, 0 <= d - 1 - mid < n_b
        if (ka[mid] <= kb[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t load_count(const void* c, int count_bytes, uint64_t i) {
    return count_bytes == 8 ? ((const uint64_t*)c)[i] : (uint64_t)((const uint32_t*)c)[i];
}

// One tile.  SCATTER = false: its number of output entries to heads[tile] and its
// split to split[tile].  SCATTER = true: its output entries to keys_out /
// counts_out from the scanned heads[tile].
template <bool SCATTER>
__global__ void __launch_bounds__(kMBlock) merge_tile_kernel(const uint64_t* __restrict__ ka,
                                                             const void* __restrict__ ca, int cb_a, uint64_t n_a,
                                                             const uint64_t* __restrict__ kb,
                                                             const void* __restrict__ cb, int cb_b, uint64_t n_b,
                                                             uint64_t* split, uint64_t* heads, const uint64_t* heads1,
                                                             const uint64_t* heads2, uint64_t* __restrict__ keys_out,
                                                             uint64_t* __restrict__ counts_out,
                                                             const uint32_t* status) {
    __shared__ uint64_t s_key[kMTile + 2];
    __shared__ uint64_t s_cnt[SCATTER ? kMTile + 2 : 1];
    __shared__ uint64_t s_split[2];
    __shared__ uint32_t s_red[kMBlock / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x, n = n_a + n_b;
    if (*status != 0) {   // not in order (the same for the whole grid): nothing depends on the inputs
        if (!SCATTER && tid == 0) heads[tile] = 0;
        return;
    }
    const uint64_t d0 = tile * kMTile, d1 = d0 + kMTile < n ? d0 + kMTile : n;
    if (SCATTER) {
        if (tid == 0) s_split[0] = split[tile];
        if (tid == 64) s_split[1] = d1 == n ? n_a : split[tile + 1];
    } else {
        if (tid == 0) s_split[0] = split[tile] = merge_split(ka, n_a, kb, n_b, d0);
        if (tid == 64) s_split[1] = merge_split(ka, n_a, kb, n_b, d1);
    }
    __syncthreads();
    const uint64_t a0 = s_split[0], a1 = s_split[1], b0 = d0 - a0, b1 = d1 - a1;
    // in order: a0 <= a1 and b0 <= b1, and an + bn = tn <= kMTile
    const uint32_t tn = (uint32_t)(d1 - d0), an = (uint32_t)(a1 - a0), bn = tn - an;
    const uint32_t pre = a0 > 0, post = b1 < n_b;
    if (a1 < a0 || a1 > n_a || b1 < b0 || b1 > n_b || an > tn) {   // cannot happen after the check
        if (!SCATTER && tid == 0) heads[tile] = 0;
        return;
    }
    // LDS: [A[a0 - 1]] A[a0, a1) B[b0, b1) [B[b1]]
    const uint32_t na = pre + an, all = na + bn + post;
    for (uint32_t i = tid; i < all; i += kMBlock) {
        const bool from_a = i < na;
        const uint64_t x = from_a ? a0 - pre + i : b0 + (i - na);
        s_key[i] = from_a ? ka[x] : kb[x];
        if (SCATTER) s_cnt[i] = from_a ? load_count(ca, cb_a, x) : load_count(cb, cb_b, x);
    }
    __syncthreads();
    const uint64_t* const pa = s_key + pre;        // pa[-1] is A[a0 - 1] if pre
    const uint64_t* const pb = s_key + na;         // pb[bn] is B[b1] if post
    const uint64_t* const qa = s_cnt + (SCATTER ? pre : 0);
    const uint64_t* const qb = s_cnt + (SCATTER ? na : 0);
    // the thread's positions [dd, dd + kMPer) of the tile: its own split
    const uint32_t dd = tid * kMPer < tn ? tid * kMPer : tn;
    uint32_t lo = dd > bn ? dd - bn : 0, hi = dd < an ? dd : an;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pa[mid] <= pb[dd - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    uint32_t a = lo, b = dd - lo, h = 0;
    uint64_t okey[kMPer], ocnt[kMPer];
    uint32_t omask = 0;
#pragma unroll
    for (int i = 0; i < kMPer; ++i) {
        okey[i] = 0;
        ocnt[i] = 0;
        if (a + b < tn) {
            const bool have_a = a < an, have_b = b < bn;
            const uint64_t x = have_a ? pa[a] : 0, y = (have_b || (b == bn && post)) ? pb[b] : 0;
            if (!have_b || (have_a && x <= y)) {   // an entry of A: with the equal entry of B, which comes next
                const bool pair = (have_b || post) && x == y;
                okey[i] = x;
                if (SCATTER) ocnt[i] = qa[a] + (pair ? qb[b] : 0);
                omask |= 1u << i;
                ++a;
            } else {                               // an entry of B: already out if the entry of A before it is equal
                const bool dup = (a > 0 || pre) && pa[(int)a - 1] == y;
                if (!dup) {
                    okey[i] = y;
                    if (SCATTER) ocnt[i] = qb[b];
                    omask |= 1u << i;
                }
                ++b;
            }
        }
    }
    h = (uint32_t)__builtin_popcount(omask);
    if (!SCATTER) {
        const uint32_t sum = block_sum<kMBlock / 64>(h, s_red);
        if (tid == 0) heads[tile] = sum;
        return;
    }
    // every thread has read its entries (the scan's barriers): the tile's output, compacted, takes their place
    uint32_t tot;
    uint32_t u = block_excl_scan<kMBlock / 64, true>(h, s_red, &tot);
#pragma unroll
    for (int i = 0; i < kMPer; ++i) {
        if (omask >> i & 1) {
            s_key[u] = okey[i];
            s_cnt[u] = ocnt[i];
            ++u;
        }
    }
    lds_barrier();
    const uint64_t base = scanned(heads, heads1, heads2, tile);
    for (uint32_t i = tid; i < tot; i += kMBlock) {
        if (base + i < n) {   // (always: a prefix of the output has no more entries than the merged order)
            keys_out[base + i] = s_key[i];
            counts_out[base + i] = s_cnt[i];
        }
    }
}

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_sparse_merge_tile(void) { return kMTile; }

extern "C" uint64_t kf_sparse_merge_scratch_bytes(uint64_t n_a, uint64_t n_b) {
    if (n_a > kMMaxEntries || n_b > kMMaxEntries || n_a + n_b > kMMaxEntries) return 0;
    return 8 * merge_layout(n_a + n_b).words;
}

extern "C" int kf_sparse_merge(const uint64_t* d_keys_a, const void* d_counts_a, int count_bytes_a, uint64_t n_a,
                               const uint64_t* d_keys_b, const void* d_counts_b, int count_bytes_b, uint64_t n_b,
                               uint64_t* d_keys_out, uint64_t* d_counts_out, uint64_t* d_n_out, uint32_t* d_status,
                               void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if ((count_bytes_a != 4 && count_bytes_a != 8) || (count_bytes_b != 4 && count_bytes_b != 8))
        return kf_fail(KF_EINVAL, "kf_sparse_merge: count_bytes=%d, %d: each must be 4 or 8", count_bytes_a,
                       count_bytes_b);
    if (n_a > kMMaxEntries || n_b > kMMaxEntries || n_a + n_b > kMMaxEntries)
        return kf_fail(KF_EINVAL, "kf_sparse_merge: n_a + n_b above the limit of %llu entries",
                       (unsigned long long)kMMaxEntries);
    if ((n_a && (!d_keys_a || !d_counts_a)) || (n_b && (!d_keys_b || !d_counts_b)) || !d_keys_out || !d_counts_out ||
        !d_n_out || !d_status || !d_scratch)
        return kf_fail(KF_EINVAL, "kf_sparse_merge: null device pointer");
    if (((uintptr_t)d_keys_a & 7) || ((uintptr_t)d_keys_b & 7) || ((uintptr_t)d_counts_a & (uintptr_t)(count_bytes_a - 1)) ||
        ((uintptr_t)d_counts_b & (uintptr_t)(count_bytes_b - 1)) || ((uintptr_t)d_keys_out & 7) ||
        ((uintptr_t)d_counts_out & 7) || ((uintptr_t)d_n_out & 7) || ((uintptr_t)d_scratch & 7) ||
        ((uintptr_t)d_status & 3))
        return kf_fail(KF_EINVAL, "kf_sparse_merge: misaligned device pointer (8 bytes for the u64 arrays and the "
                                  "scratch, count_bytes for the counts, 4 for d_status)");
    const uint64_t n = n_a + n_b;
    const MergeLayout L = merge_layout(n);
    if (scratch_bytes < 8 * L.words)
        return kf_fail(KF_ERANGE, "kf_sparse_merge: scratch needs %llu bytes", (unsigned long long)(8 * L.words));
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_status, 0, 4, s) != hipSuccess) return kf_fail(KF_EHIP, "kf_sparse_merge: memset failed");
    if (n == 0) {
        if (hipMemsetAsync(d_n_out, 0, 8, s) != hipSuccess) return kf_fail(KF_EHIP, "kf_sparse_merge: memset failed");
        return KF_OK;
    }
    uint64_t* const w = (uint64_t*)d_scratch;
    const uint32_t tiles = (uint32_t)L.tiles;
    hipLaunchKernelGGL(merge_check_kernel, dim3(tiles < (uint32_t)kMCheckGrid ? tiles : (uint32_t)kMCheckGrid),
                       dim3(kMBlock), 0, s, d_keys_a, n_a, d_keys_b, n_b, d_status);
    hipLaunchKernelGGL(merge_tile_kernel<false>, dim3(tiles), dim3(kMBlock), 0, s, d_keys_a, d_counts_a, count_bytes_a,
                       n_a, d_keys_b, d_counts_b, count_bytes_b, n_b, w + L.split, w + L.heads, w + L.heads1,
                       w + L.heads2, d_keys_out, d_counts_out, d_status);
    hipLaunchKernelGGL(scan_level_kernel<uint64_t>, dim3((uint32_t)L.nb1), dim3(kScanLevel), 0, s, w + L.heads,
                       L.tiles, w + L.heads1);
    hipLaunchKernelGGL(scan_level_kernel<uint64_t>, dim3((uint32_t)L.nb2), dim3(kScanLevel), 0, s, w + L.heads1, L.nb1,
                       w + L.heads2);
    hipLaunchKernelGGL(scan_level_kernel<uint64_t>, dim3(1), dim3(kScanLevel), 0, s, w + L.heads2, L.nb2, d_n_out);
    hipLaunchKernelGGL(merge_tile_kernel<true>, dim3(tiles), dim3(kMBlock), 0, s, d_keys_a, d_counts_a, count_bytes_a,
                       n_a, d_keys_b, d_counts_b, count_bytes_b, n_b, w + L.split, w + L.heads, w + L.heads1,
                       w + L.heads2, d_keys_out, d_counts_out, d_status);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_sparse_merge: launch failed");
    return KF_OK;
}

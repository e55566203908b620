// kf_index.hip -- the FASTA record index of a batch on the device (what the host
// finds per file with kf_index_records, reference path kf2vec/main.py:309-311:
// Jellyfish's record parsing), so that the CLI's readers only copy bytes.
//
// A header is a line that starts with '>' (at a genome start or after '\n'); it
// is excluded up to its '\n' (or the genome end).  Unlike the host index, header
// lines that follow each other stay separate pairs (the count kernels treat
// adjacent ranges like one).  Three launches, the compaction of kf_compact.h:
// per-block header counts, their scan by one workgroup (with carry over rounds of
// 1,024 blocks), and a scatter of the pairs in order; the number of pairs stays on
// the device (kf_count_batch_dev reads it there).
//
// The FASTQ index (kf_index_fastq, second half of this file) covers genomes in
// the regular four-line form, where a line's role is its number mod 4 and the
// number is a prefix count of '\n': a table of the newline positions in order
// (count, a three-level scan of the block counts, scatter), then one thread per
// genome (its first newline, its lines, its pairs), a scan of the pairs per
// genome, and one thread per pair that writes it and checks its record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_compact.h"
#include "kf_internal.h"

namespace kf {
namespace {

constexpr int kIBlock = kCompactBlock;     // threads per workgroup (also of the per-genome and per-pair kernels)
constexpr int kIPer = kCompactPer;         // bytes per thread
constexpr uint32_t kISpan = kCompactSpan;  // 4 KiB per workgroup

// header starts among the thread's 16 bytes (bit q: byte p0 + q)
__device__ __forceinline__ uint32_t thread_heads(const uint8_t* bytes, uint64_t end, const uint64_t* goff, int n,
                                                 uint64_t p0) {
    uint32_t m = 0;
    if (p0 >= end) return 0;
    uint8_t prev = p0 > 0 ? bytes[p0 - 1] : (uint8_t)'\n';
    for (int q = 0; q < kIPer; ++q) {
        const uint64_t i = p0 + q;
        if (i >= end) break;
        const uint8_t c = bytes[i];
        if (c == '>') {
            bool start = prev == '\n' || i == 0;
            if (!start) {   // a genome start (genomes need not end with '\n')
                start = goff[last_at_or_before(n, i, [&](int g) { return goff[g]; })] == i;
            }
            if (start) m |= 1u << q;
        }
        prev = c;
    }
    return m;
}

__global__ void __launch_bounds__(kIBlock) idx_count_kernel(const uint8_t* bytes, uint64_t end, const uint64_t* goff,
                                                            int n, uint32_t* blk) {
    compact_count((uint32_t)__builtin_popcount(thread_heads(bytes, end, goff, n, compact_p0())), blk);
}

__global__ void __launch_bounds__(kIBlock) idx_scatter_kernel(const uint8_t* bytes, uint64_t end, const uint64_t* goff,
                                                              int n, const uint32_t* blk, uint64_t* excl,
                                                              uint64_t cap) {
    const uint64_t p0 = compact_p0();
    uint32_t m = thread_heads(bytes, end, goff, n, p0);
    uint64_t u = compact_first_slot(blk[blockIdx.x], (uint32_t)__builtin_popcount(m));
    while (m) {
        const int q = __builtin_ctz(m);
        m &= m - 1;
        const uint64_t j = p0 + (uint64_t)q;
        if (u < cap) {
            const uint64_t ge = goff[last_at_or_before(n, j, [&](int g) { return goff[g]; }) + 1];   // its genome's end
            uint64_t e = j;
            while (e < ge && bytes[e] != '\n') ++e;   // the header line (short)
            excl[2 * u] = j;
            excl[2 * u + 1] = e;
        }
        ++u;
    }
}

// ------------------------------------------------------------------ FASTQ
// Scratch layout of kf_index_fastq, in 64-bit words (kf_index_fastq_scratch_bytes
// is its size).  The two scans share one shape: the three levels of kf_scan.h.
constexpr uint32_t kQLevel = kScanLevel;   // entries per workgroup of a scan level
constexpr uint64_t kQMaxEntries = kScanMaxEntries;
constexpr auto fq_scan_level_kernel = scan_level_kernel<uint64_t>;

struct FqLayout {
    uint64_t nb, nb1, nb2;   // newline counts per block and their two levels of sums
    uint64_t ng1, ng2;       // the same for the pairs per genome
    uint64_t blk, blk1, blk2, g_nl, g_lines, g_end, g_pairs, g_pairs1, g_pairs2, nlpos, words;
};

inline uint64_t div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

inline FqLayout fq_layout(uint64_t batch_bytes, uint64_t n_genomes, uint64_t cap_lines) {
    FqLayout L;
    L.nb = div_up(batch_bytes, kISpan);
    L.nb1 = div_up(L.nb, kQLevel);
    L.nb2 = div_up(L.nb1, kQLevel);
    L.ng1 = div_up(n_genomes, kQLevel);
    L.ng2 = div_up(L.ng1, kQLevel);
    uint64_t w = 0;
    L.blk = w, w += L.nb;
    L.blk1 = w, w += L.nb1;
    L.blk2 = w, w += L.nb2;
    L.g_nl = w, w += n_genomes;      // newlines before the genome's first byte
    L.g_lines = w, w += n_genomes;   // lines up to the last non-empty one
    L.g_end = w, w += n_genomes;     // end of the last non-empty line
    L.g_pairs = w, w += n_genomes;
    L.g_pairs1 = w, w += L.ng1;
    L.g_pairs2 = w, w += L.ng2;
    L.nlpos = w, w += cap_lines;     // position of every '\n', in order
    L.words = w;
    return L;
}

// bits 0..3: which bytes of w are '\n'
__device__ __forceinline__ uint32_t nl_bits(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 where the byte is 0
    return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// newlines among the thread's 16 bytes (bit q: byte p0 + q), one 16-byte load
__device__ __forceinline__ uint32_t thread_newlines(const uint8_t* bytes, uint64_t end, uint64_t p0) {
    if (p0 >= end) return 0;
    const uint4 v = *reinterpret_cast<const uint4*>(bytes + p0);
    uint32_t m = nl_bits(v.x) | nl_bits(v.y) << 4 | nl_bits(v.z) << 8 | nl_bits(v.w) << 12;
    if (end - p0 < kIPer) m &= (1u << (uint32_t)(end - p0)) - 1u;
    return m;
}

__global__ void __launch_bounds__(kIBlock) fq_count_kernel(const uint8_t* bytes, uint64_t end, uint64_t* blk) {
    compact_count((uint32_t)__builtin_popcount(thread_newlines(bytes, end, compact_p0())), blk);
}

__global__ void __launch_bounds__(kIBlock) fq_scatter_kernel(const uint8_t* bytes, uint64_t end, const uint64_t* blk,
                                                             const uint64_t* blk1, const uint64_t* blk2,
                                                             uint64_t* nlpos, uint64_t cap_lines) {
    const uint64_t p0 = compact_p0();
    uint32_t m = thread_newlines(bytes, end, p0);
    uint64_t u = compact_first_slot(scanned(blk, blk1, blk2, blockIdx.x), (uint32_t)__builtin_popcount(m));
    while (m) {
        const int q = __builtin_ctz(m);
        m &= m - 1;
        if (u < cap_lines) nlpos[u] = p0 + (uint64_t)q;
        ++u;
    }
}

// first u in [0, n) with pos[u] >= x (n if none)
__device__ __forceinline__ uint64_t first_at_or_after(const uint64_t* pos, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (pos[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One thread per genome: where its newlines start in the table, how many lines
// it has up to its last non-empty one, where that line ends, and its pairs.
__global__ void __launch_bounds__(kIBlock) fq_genome_kernel(const uint64_t* goff, int n, uint64_t end,
                                                            const uint64_t* nlpos, const uint64_t* n_lines,
                                                            uint64_t cap_lines, uint64_t* g_nl, uint64_t* g_lines,
                                                            uint64_t* g_end, uint64_t* g_pairs, uint32_t* status) {
    const uint64_t g = (uint64_t)blockIdx.x * kIBlock + threadIdx.x;
    if (g >= (uint64_t)n) return;
    const uint64_t tot = *n_lines, a = goff[g], b = goff[g + 1];
    uint64_t first = 0, lines = 0, cend = a;
    if (tot <= cap_lines) {   // else the table is incomplete: no pairs, the caller runs again
        if (b < a || b > end) {
            status[g] = 2;   // offsets that decrease or pass the batch end: nothing of this genome is read
        } else {
            first = first_at_or_after(nlpos, tot, a);
            const uint64_t last = first_at_or_after(nlpos, tot, b);
            // the newlines that end the genome (padding, empty lines): the first u
            // from which every byte up to b is a '\n'
            uint64_t lo = first, hi = last;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (nlpos[mid] + (last - mid) == b) hi = mid;
                else lo = mid + 1;
            }
            cend = b - (last - lo);
            if (cend > a) lines = (lo - first) + 1;
        }
    }
    g_nl[g] = first;
    g_lines[g] = lines;
    g_end[g] = cend;
    g_pairs[g] = lines ? 1 + (lines + 1) / 4 : 0;
}

// One thread per pair: pair 0 of a genome is its first header line, pair r >= 1
// runs from the '+' line of record r - 1 to the end of record r's header line (or
// of the genome's last non-empty line).  The thread also checks record r (lines
// 4r .. 4r + 3) against the four-line form.
__global__ void __launch_bounds__(kIBlock) fq_pair_kernel(const uint8_t* bytes, const uint64_t* goff, int n,
                                                          const uint64_t* nlpos, const uint64_t* n_lines,
                                                          uint64_t cap_lines, const uint64_t* g_nl,
                                                          const uint64_t* g_lines, const uint64_t* g_end,
                                                          const uint64_t* g_pairs, const uint64_t* g_pairs1,
                                                          const uint64_t* g_pairs2, const uint64_t* n_pairs,
                                                          uint64_t* excl, uint64_t cap_pairs, uint32_t* status) {
    const uint64_t q = (uint64_t)blockIdx.x * kIBlock + threadIdx.x;
    if (q >= cap_pairs || q >= *n_pairs || *n_lines > cap_lines) return;
    // the last genome whose first pair is at or before q
    const uint64_t g = (uint64_t)last_at_or_before(
        n, q, [&](int m) { return scanned(g_pairs, g_pairs1, g_pairs2, (uint64_t)m); });
    const uint64_t r = q - scanned(g_pairs, g_pairs1, g_pairs2, g);
    const uint64_t lines = g_lines[g], a = goff[g], cend = g_end[g];
    const uint64_t* nl = nlpos + g_nl[g];   // nl[j]: the '\n' that ends line j (j < lines - 1)
    if (lines == 0 || r >= 1 + (lines + 1) / 4) return;   // cannot happen: q is one of this genome's pairs
    auto start_of = [&](uint64_t j) { return j == 0 ? a : nl[j - 1] + 1; };
    auto end_of = [&](uint64_t j) { return j + 1 < lines ? nl[j] : cend; };
    uint64_t s, e;
    if (r == 0) {
        s = a;
        e = end_of(0);
    } else {
        const uint64_t plus = 4 * r - 2, to = plus + 2 < lines ? plus + 2 : lines - 1;
        s = start_of(plus);
        e = end_of(to);
    }
    excl[2 * q] = s;
    excl[2 * q + 1] = e;
    const uint64_t j0 = 4 * r;
    if (j0 >= lines) return;
    bool bad;
    uint64_t len_seq = 0;
    {
        const uint64_t s0 = start_of(j0), e0 = end_of(j0);
        bad = !(e0 > s0 && bytes[s0] == '@');
    }
    if (j0 + 1 < lines) {
        const uint64_t s1 = start_of(j0 + 1);
        len_seq = end_of(j0 + 1) - s1;
        bad |= len_seq > 0 && bytes[s1] == '+';
    }
    if (j0 + 2 < lines) {
        const uint64_t s2 = start_of(j0 + 2);
        bad |= !(end_of(j0 + 2) > s2 && bytes[s2] == '+');
    }
    if (j0 + 3 < lines) {
        const uint64_t len_qual = end_of(j0 + 3) - start_of(j0 + 3);
        bad |= len_seq == 0 ? len_qual != 0 : len_qual < len_seq;
    }
    if (bad) status[g] = 1;
}

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_index_fasta(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_genomes, uint64_t batch_bytes,
                              uint64_t* d_excl, uint64_t cap_pairs, uint64_t* d_n_pairs, uint32_t* d_scratch,
                              uint64_t scratch_words, void* stream) {
    if (n_genomes < 0) return kf_fail(KF_EINVAL, "n_genomes < 0");
    if (!d_n_pairs) return kf_fail(KF_EINVAL, "null device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_genomes == 0 || batch_bytes == 0) {
        if (hipMemsetAsync(d_n_pairs, 0, 8, s) != hipSuccess) return kf_fail(KF_EHIP, "memset failed");
        return KF_OK;
    }
    if (!d_bytes || !d_goff || !d_scratch || (cap_pairs && !d_excl)) return kf_fail(KF_EINVAL, "null device pointer");
    const uint64_t nb = (batch_bytes + kISpan - 1) / kISpan;
    if (nb >= (1ull << 31)) return kf_fail(KF_EINVAL, "batch too large");
    if (scratch_words < nb + 1)
        return kf_fail(KF_ERANGE, "scratch needs %llu words", (unsigned long long)(nb + 1));
    hipLaunchKernelGGL(idx_count_kernel, dim3((uint32_t)nb), dim3(kIBlock), 0, s, d_bytes, batch_bytes, d_goff,
                       n_genomes, d_scratch);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, d_scratch, (uint32_t)nb, d_n_pairs);
    hipLaunchKernelGGL(idx_scatter_kernel, dim3((uint32_t)nb), dim3(kIBlock), 0, s, d_bytes, batch_bytes, d_goff,
                       n_genomes, d_scratch, d_excl, cap_pairs);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "record index launch failed");
    return KF_OK;
}

extern "C" uint64_t kf_index_fastq_scratch_bytes(uint64_t batch_bytes, int32_t n_genomes, uint64_t cap_lines) {
    if (n_genomes < 0) return 0;
    return 8 * fq_layout(batch_bytes, (uint64_t)n_genomes, cap_lines).words;
}

extern "C" int kf_index_fastq(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_genomes, uint64_t batch_bytes,
                              uint64_t* d_excl, uint64_t cap_pairs, uint64_t cap_lines, uint64_t* d_n,
                              uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (n_genomes < 0) return kf_fail(KF_EINVAL, "n_genomes < 0");
    if (!d_n) return kf_fail(KF_EINVAL, "null device pointer (d_n)");
    if (n_genomes > 0 && !d_status) return kf_fail(KF_EINVAL, "null device pointer (d_status)");
    hipStream_t s = (hipStream_t)stream;
    if (n_genomes == 0 || batch_bytes == 0) {
        if (hipMemsetAsync(d_n, 0, 16, s) != hipSuccess ||
            (n_genomes && hipMemsetAsync(d_status, 0, 4 * (size_t)n_genomes, s) != hipSuccess))
            return kf_fail(KF_EHIP, "memset failed");
        return KF_OK;
    }
    if (!d_bytes || !d_goff || !d_scratch || (cap_pairs && !d_excl)) return kf_fail(KF_EINVAL, "null device pointer");
    if (((uintptr_t)d_bytes & 15) || ((uintptr_t)d_scratch & 7))
        return kf_fail(KF_EINVAL, "d_bytes must be 16-byte and d_scratch 8-byte aligned");
    const FqLayout L = fq_layout(batch_bytes, (uint64_t)n_genomes, cap_lines);
    if (L.nb > kQMaxEntries) return kf_fail(KF_EINVAL, "batch too large");
    if ((uint64_t)n_genomes > kQMaxEntries) return kf_fail(KF_EINVAL, "too many genomes");
    if (cap_pairs >= (1ull << 31) * kIBlock) return kf_fail(KF_EINVAL, "cap_pairs too large");
    if (scratch_bytes < 8 * L.words)
        return kf_fail(KF_ERANGE, "scratch needs %llu bytes", (unsigned long long)(8 * L.words));
    uint64_t* w = (uint64_t*)d_scratch;
    if (hipMemsetAsync(d_status, 0, 4 * (size_t)n_genomes, s) != hipSuccess) return kf_fail(KF_EHIP, "memset failed");
    // the newline table: counts per block, their scan, the positions in order
    hipLaunchKernelGGL(fq_count_kernel, dim3((uint32_t)L.nb), dim3(kIBlock), 0, s, d_bytes, batch_bytes, w + L.blk);
    hipLaunchKernelGGL(fq_scan_level_kernel, dim3((uint32_t)L.nb1), dim3(kQLevel), 0, s, w + L.blk, L.nb, w + L.blk1);
    hipLaunchKernelGGL(fq_scan_level_kernel, dim3((uint32_t)L.nb2), dim3(kQLevel), 0, s, w + L.blk1, L.nb1,
                       w + L.blk2);
    hipLaunchKernelGGL(fq_scan_level_kernel, dim3(1), dim3(kQLevel), 0, s, w + L.blk2, L.nb2, d_n + 1);
    hipLaunchKernelGGL(fq_scatter_kernel, dim3((uint32_t)L.nb), dim3(kIBlock), 0, s, d_bytes, batch_bytes, w + L.blk,
                       w + L.blk1, w + L.blk2, w + L.nlpos, cap_lines);
    // lines and pairs per genome, the pairs' scan, the pairs
    const uint32_t gb = (uint32_t)div_up((uint64_t)n_genomes, kIBlock);
    hipLaunchKernelGGL(fq_genome_kernel, dim3(gb), dim3(kIBlock), 0, s, d_goff, n_genomes, batch_bytes, w + L.nlpos,
                       d_n + 1, cap_lines, w + L.g_nl, w + L.g_lines, w + L.g_end, w + L.g_pairs, d_status);
    hipLaunchKernelGGL(fq_scan_level_kernel, dim3((uint32_t)L.ng1), dim3(kQLevel), 0, s, w + L.g_pairs,
                       (uint64_t)n_genomes, w + L.g_pairs1);
    hipLaunchKernelGGL(fq_scan_level_kernel, dim3((uint32_t)L.ng2), dim3(kQLevel), 0, s, w + L.g_pairs1, L.ng1,
                       w + L.g_pairs2);
    hipLaunchKernelGGL(fq_scan_level_kernel, dim3(1), dim3(kQLevel), 0, s, w + L.g_pairs2, L.ng2, d_n);
    if (cap_pairs)
        hipLaunchKernelGGL(fq_pair_kernel, dim3((uint32_t)div_up(cap_pairs, kIBlock)), dim3(kIBlock), 0, s, d_bytes,
                           d_goff, n_genomes, w + L.nlpos, d_n + 1, cap_lines, w + L.g_nl, w + L.g_lines, w + L.g_end,
                           w + L.g_pairs, w + L.g_pairs1, w + L.g_pairs2, d_n, d_excl, cap_pairs, d_status);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "FASTQ index launch failed");
    return KF_OK;
}

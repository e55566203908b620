// kf_kfrows.h -- the passes that the readers of rows of text share (kf_kfparse.hip:
// get_chunks rows of whole numbers into uint16; kf_kffloat.hip: get_frequencies
// rows of decimal floats into float64 / float32; kf_tsvfloat.hip: tab-separated
// tables of signed decimal floats, the columns placed by a map).  All read many
// units of text back to back, unit u being d_bytes[goff[u], goff[u+1]), find the
// rows, walk each row's fields and report the error at the lowest byte offset;
// they differ in the separator, in what a field is and in where its value goes,
// which a Sink states (below, "','" stands for the Sink's separator):
//
//   struct Sink {
//       static constexpr uint32_t kSep;   // the byte between the name and the fields: ',' or '\t'
//       typedef ... Field;            // one field's state, with
//                                     //   int feed(uint32_t c): 0 go on, 1 the field
//                                     //   ended well (c is kSep or '\n'), else the code
//       Field fresh() const;          // the state before a field's first byte
//       // field `col` of row r ended well: store its value if `store`, or note
//       // (into err) the code that the value itself earns
//       void done(uint64_t r, uint64_t nbins, uint64_t col, const Field& f, bool store, uint64_t& err) const;
//       // row r's name is the `len` bytes at `at` (called by the thread that holds the row's first ',')
//       void name(uint64_t r, uint32_t at, uint32_t len, bool store) const;
//   };
//
// Two passes over the text:
//   1. line starts: the compaction of kf_compact.h (count per 4 KiB block, scan
//      by one workgroup, scatter) over the predicate "a non-empty line starts
//      here": the byte is inside a unit, is not '\n', and is the unit's first
//      byte or follows a '\n'.  Unit edges come from the offsets alone, so two
//      units without padding between them do not fuse.  The table holds the
//      starts of the first cap_rows + 1 rows (row cap_rows, if there is one, is
//      where "more rows than cap_rows" is reported).
//   2. rows: workgroups take rows grid-stride.  A row is walked in 4 KiB tiles
//      (aligned in the batch), 16 bytes per thread by one aligned vector load,
//      the bytes before the row start and from the unit end on masked.  A thread
//      counts the commas of its bytes that lie before the row's first '\n'; one
//      block_excl_scan of (commas | newline seen << 16) plus the carry of the
//      tiles before gives the column of the first field that starts in its
//      bytes and tells the threads behind the row end to stand by.  A thread
//      parses every field that starts in its bytes -- from its registers, then
//      byte by byte past its 16 bytes (the neighbour's bytes, already in cache),
//      never past the row's unit -- and hands each to the Sink.  The thread that
//      holds the row's end checks the field count.
// Errors: a thread keeps the least (column << 3 | code) of what it saw; the
// row's least goes through one LDS atomic per erring thread, and the least
// erring row through one global atomicMin per erring row.  The last launch (one
// workgroup) parses that row once more to name code and column, which keeps the
// hot loop free of any packing limit on row and column numbers.
// No workgroup waits for another; nothing is allocated; the host never waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_compact.h"
#include "kf_internal.h"

namespace kf {
namespace {

constexpr int kPBlock = kCompactBlock;       // threads per workgroup (both passes)
constexpr int kPWaves = kPBlock / 64;
constexpr uint32_t kPTile = kCompactSpan;    // bytes per tile: 4 KiB, 16 per thread
constexpr uint32_t kPMaxGrid = 256 * 8;      // row workgroups: the rest of the rows grid-stride
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
constexpr uint64_t kNoErr = ~0ull;

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// the codes of d_status[0] (include/kf2vec_gpu.h): 4 is kf_parse_kf_rows' alone, 6 and 7 kf_parse_kf_floats'
enum { kErrFew = 1, kErrMany = 2, kErrForm = 3, kErrValue = 4, kErrRows = 5, kErrDigits = 6, kErrRange = 7 };

// scratch: [0] the row count, [1] the least erring row (low word), then the
// block counts (nb + 1 words, padded to 8 bytes), then the line-start table
struct Scratch {
    uint64_t* total;
    uint32_t* bad_row;
    uint32_t* blk;
    uint32_t* table;
};
__host__ __device__ inline uint64_t blk_words(uint64_t nb) { return (nb + 1 + 1) / 2 * 2; }
__host__ __device__ inline Scratch carve(void* scratch, uint64_t nb) {
    Scratch s;
    s.total = (uint64_t*)scratch;
    s.bad_row = (uint32_t*)((uint64_t*)scratch + 1);
    s.blk = (uint32_t*)((uint64_t*)scratch + 2);
    s.table = s.blk + blk_words(nb);
    return s;
}

// a row is at least one byte, so a batch never has more rows than bytes: a larger cap asks for no larger table
inline uint64_t cap_of(uint64_t batch_bytes, uint64_t cap_rows) { return cap_rows < batch_bytes ? cap_rows : batch_bytes; }

// bytes of scratch that carve() lays out: 16 + a word per 4 KiB of text + a word per row allowed for
inline uint64_t rows_scratch_bytes(uint64_t batch_bytes, uint64_t cap_rows) {
    const uint64_t nb = (batch_bytes + kPTile - 1) / kPTile;
    const uint64_t table = (cap_of(batch_bytes, cap_rows) + 1 + 1) / 2 * 2;   // u32 entries, padded to 8 bytes
    return 16 + 4 * blk_words(nb) + 4 * table;
}

// The unit of byte p: the last u in [0, n_units) with goff[u] <= p (of empty
// units at one offset the last, so the one that holds p), n_units >= 1.
__device__ __forceinline__ int unit_of(const uint64_t* __restrict__ goff, int n_units, uint64_t p) {
    return last_at_or_before(n_units, p, [&](int m) { return goff[m]; });
}

// byte q (0..15) of a 16-byte load
__device__ __forceinline__ uint32_t byte_of(const v4u& w, int q) { return (w[q >> 2] >> (8 * (q & 3))) & 0xFFu; }

// The 16 bytes at p (16-aligned): one vector load where all 16 are inside the
// batch, byte loads of the bytes below `len` else (zeros past it).
__device__ __forceinline__ v4u load16(const uint8_t* __restrict__ bytes, uint64_t p, uint64_t len) {
    v4u w = {0u, 0u, 0u, 0u};
    if (p + 16 <= len) {
        w = *(const v4u*)(bytes + p);
    } else {
        for (int q = 0; q < 16; ++q)
            if (p + q < len) w[q >> 2] |= (uint32_t)bytes[p + q] << (8 * (q & 3));
    }
    return w;
}

// Which of the 16 bytes equal c, as a bit mask, four bytes at a time: x = w ^ cccc
// has a zero byte where they are equal; ~(((x & 0x7F..) + 0x7F..) | x | 0x7F..) keeps
// bit 7 of exactly the zero bytes, and the multiply gathers the four bits.
__host__ __device__ inline uint32_t eq_mask4(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return ((t >> 7) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t eq_mask(const v4u& w, uint32_t c) {
    return eq_mask4(w[0], c) | eq_mask4(w[1], c) << 4 | eq_mask4(w[2], c) << 8 | eq_mask4(w[3], c) << 12;
}

// ---------------------------------------------------------------- pass 1
// Non-empty line starts among the calling thread's 16 bytes, as a bit mask.
__device__ __forceinline__ uint32_t line_starts(const uint8_t* __restrict__ bytes, uint64_t len,
                                                const uint64_t* __restrict__ goff, int n_units, uint64_t p0) {
    if (n_units <= 0 || p0 >= len) return 0;
    const v4u w = load16(bytes, p0, len);
    uint32_t prev = p0 ? bytes[p0 - 1] : (uint32_t)'\n';
    // the unit of the workgroup's first byte (the same for all its threads) holds nearly every thread's bytes
    const uint64_t blk0 = (uint64_t)blockIdx.x * kCompactSpan;
    const int ub = unit_of(goff, n_units, blk0);
    if (goff[ub] <= p0 && p0 + 16 <= min(goff[ub + 1], len)) {
        const uint32_t nm = eq_mask(w, '\n');
        const uint32_t after = (nm << 1 | (p0 == goff[ub] || prev == '\n' ? 1u : 0u)) & 0xFFFFu;
        return after & ~nm;
    }
    int u = unit_of(goff, n_units, p0);   // a unit edge among these bytes, or bytes outside every unit
    uint64_t a = goff[u], b = min(goff[u + 1], len);
    uint32_t mask = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint64_t p = p0 + q;
        const uint32_t c = byte_of(w, q);
        if (p >= b && u + 1 < n_units && goff[u + 1] <= p) {   // a unit edge among these bytes
            u = unit_of(goff, n_units, p);
            a = goff[u];
            b = min(goff[u + 1], len);
        }
        if (p >= a && p < b && c != '\n' && (p == a || prev == '\n')) mask |= 1u << q;
        prev = c;
    }
    return mask;
}

__global__ void __launch_bounds__(kPBlock) kfp_count_kernel(const uint8_t* __restrict__ bytes, uint64_t len,
                                                            const uint64_t* __restrict__ goff, int n_units,
                                                            uint32_t* blk, uint32_t* bad_row) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad_row = kNoRow;
    compact_count((uint32_t)__popc(line_starts(bytes, len, goff, n_units, compact_p0())), blk);
}

__global__ void __launch_bounds__(kPBlock) kfp_scatter_kernel(const uint8_t* __restrict__ bytes, uint64_t len,
                                                              const uint64_t* __restrict__ goff, int n_units,
                                                              const uint32_t* __restrict__ blk, uint32_t* table,
                                                              uint64_t cap) {
    const uint64_t p0 = compact_p0();
    uint32_t mask = line_starts(bytes, len, goff, n_units, p0);
    uint64_t slot = compact_first_slot(blk[blockIdx.x], (uint32_t)__popc(mask));
    for (; mask && slot <= cap; mask &= mask - 1, ++slot) table[slot] = (uint32_t)(p0 + (uint32_t)__ffs(mask) - 1);
}

// ---------------------------------------------------------------- pass 2
__device__ __forceinline__ void note(uint64_t& err, uint64_t col, int code) {
    const uint64_t key = (col << 3) | (uint64_t)code;
    err = key < err ? key : err;
}

// Parse row r, which starts at s in the unit that ends at lim (<= len), handing
// its fields to the sink (which stores nothing unless `store`).  Every thread of
// the workgroup calls it; returns the row's least (column << 3 | code), or
// kNoErr, to every thread.
template <class Sink>
__device__ __forceinline__ uint64_t parse_row(const uint8_t* __restrict__ bytes, uint64_t len, uint64_t s, uint64_t lim,
                                              uint64_t nbins, const Sink& sink, uint64_t r, bool store,
                                              uint64_t* s_err, uint32_t* wsum) {
    typedef typename Sink::Field Field;
    if (threadIdx.x == 0) *s_err = kNoErr;   // ordered before the first atomic by the scan's barriers
    uint64_t err = kNoErr;
    uint64_t carry = 0;                      // the row's commas in the tiles before
    for (uint64_t base = s & ~(uint64_t)(kPTile - 1);; base += kPTile) {
        const uint64_t p = base + (uint64_t)threadIdx.x * 16;
        v4u w = {0u, 0u, 0u, 0u};
        uint32_t valid = 0, cm = 0, nm = 0;
        if (p < lim && p + 16 > s) {
            w = load16(bytes, p, len);
            // (byte by byte: the word-wise eq_mask of pass 1 measured slower here)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint64_t x = p + q;
                if (x < s || x >= lim) continue;
                const uint32_t c = byte_of(w, q);
                valid |= 1u << q;
                cm |= (c == Sink::kSep ? 1u : 0u) << q;
                nm |= (c == '\n' ? 1u : 0u) << q;
            }
        }
        const int fn = nm ? __ffs(nm) - 1 : 16;                       // the row's end, if it is among these bytes
        const uint32_t mine = (uint32_t)__popc(cm & ((1u << fn) - 1u));   // commas before it
        uint32_t tot;
        const uint32_t ex = block_excl_scan<kPWaves>(mine | (nm ? 1u << 16 : 0u), wsum, &tot);
        if ((ex >> 16) == 0 && valid) {      // the row has not ended before these bytes
            uint64_t j = carry + (ex & 0xFFFFu);   // the field that the next comma starts
            bool active = false;
            uint64_t col = 0;
            Field f = sink.fresh();
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (!((valid >> q) & 1u) || q > fn) continue;
                const uint32_t c = byte_of(w, q);
                if (active) {
                    const int e = f.feed(c);
                    if (e) {
                        active = false;
                        if (e == 1) sink.done(r, nbins, col, f, store, err);
                        else note(err, col, e);
                    }
                }
                if (c == Sink::kSep) {
                    if (j == 0) sink.name(r, (uint32_t)s, (uint32_t)(p + q - s), store);
                    if (j >= nbins) {
                        note(err, nbins, kErrMany);
                    } else {
                        active = true;
                        col = j;
                        f = sink.fresh();
                    }
                    ++j;
                }
            }
            if (active) {                    // the field runs on past these 16 bytes
                for (uint64_t x = p + 16;; ++x) {
                    const int e = f.feed(x < lim ? (uint32_t)bytes[x] : (uint32_t)'\n');
                    if (e == 0) continue;
                    if (e == 1) sink.done(r, nbins, col, f, store, err);
                    else note(err, col, e);
                    break;
                }
            }
            if (nm && j < nbins) note(err, j, kErrFew);   // this thread holds the row's end
        }
        if (tot >> 16) break;                // a '\n' ended the row in this tile
        carry += tot & 0xFFFFu;
        if (base + kPTile >= lim) {          // the unit's end ended it
            if (threadIdx.x == 0 && carry < nbins) note(err, carry, kErrFew);
            break;
        }
    }
    if (err != kNoErr) atomicMin((unsigned long long*)s_err, (unsigned long long)err);
    __syncthreads();
    const uint64_t all = *s_err;
    __syncthreads();                         // s_err is written again for the next row
    return all;
}

// where row r starts and its unit ends
__device__ __forceinline__ void row_span(const uint32_t* __restrict__ table, const uint64_t* __restrict__ goff,
                                         int n_units, uint64_t len, uint64_t r, uint64_t* s, uint64_t* lim, int* unit) {
    *s = table[r];
    *unit = unit_of(goff, n_units, *s);
    *lim = min(goff[*unit + 1], len);
}

template <class Sink>
__global__ void __launch_bounds__(kPBlock) kfp_rows_kernel(const uint8_t* __restrict__ bytes, uint64_t len,
                                                           const uint64_t* __restrict__ goff, int n_units,
                                                           uint64_t nbins, uint64_t cap, Sink sink,
                                                           const uint64_t* __restrict__ total,
                                                           const uint32_t* __restrict__ table, uint32_t* bad_row) {
    __shared__ uint64_t s_err;
    __shared__ uint32_t wsum[kPWaves];
    const uint64_t n = min(*total, cap);
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        uint64_t s, lim;
        int u;
        row_span(table, goff, n_units, len, r, &s, &lim, &u);
        const uint64_t e = parse_row(bytes, len, s, lim, nbins, sink, r, true, &s_err, wsum);
        if (e != kNoErr && threadIdx.x == 0) atomicMin(bad_row, (uint32_t)r);
    }
}

// rows that start before x: the table holds the first nt row starts, ascending
__device__ __forceinline__ uint64_t rows_before(const uint32_t* __restrict__ table, uint64_t nt, uint64_t x) {
    uint64_t lo = 0, hi = nt;
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (table[m] < x) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// One workgroup: every unit's first row, and the status.
template <class Sink>
__global__ void __launch_bounds__(kPBlock) kfp_finish_kernel(const uint8_t* __restrict__ bytes, uint64_t len,
                                                             const uint64_t* __restrict__ goff, int n_units,
                                                             uint64_t nbins, uint64_t cap, Sink sink,
                                                             const uint64_t* __restrict__ total,
                                                             const uint32_t* __restrict__ table,
                                                             const uint32_t* __restrict__ bad_row,
                                                             uint64_t* unit_row0, uint64_t* status) {
    __shared__ uint64_t s_err;
    __shared__ uint32_t wsum[kPWaves];
    const uint64_t n_rows = *total;
    const uint64_t nt = min(n_rows, cap + 1);   // table entries
    for (int u = threadIdx.x; u <= n_units; u += kPBlock)
        unit_row0[u] = u < n_units ? rows_before(table, nt, goff[u]) : nt;
    uint64_t code = 0, row = 0, col = 0;
    const uint32_t bad = *bad_row;
    if (bad != kNoRow) {
        row = bad;
    } else if (n_rows > cap) {
        row = cap;
        code = kErrRows;
    }
    if (bad == kNoRow && code == 0) {
        if (threadIdx.x < 4) status[threadIdx.x] = 0;
        return;
    }
    uint64_t s, lim;
    int u;
    row_span(table, goff, n_units, len, row, &s, &lim, &u);
    if (bad != kNoRow) {                        // the same parse, for the row's code and column
        const uint64_t e = parse_row(bytes, len, s, lim, nbins, sink, row, false, &s_err, wsum);
        code = e & 7;
        col = e >> 3;
    }
    if (threadIdx.x == 0) {
        status[0] = code;
        status[1] = (uint64_t)u;
        status[2] = row - rows_before(table, nt, goff[u]);
        status[3] = col;
    }
}

__global__ void kfp_empty_kernel(int n_units, uint64_t* unit_row0, uint64_t* status) {
    for (int u = threadIdx.x; u <= n_units; u += blockDim.x) unit_row0[u] = 0;
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

// The launches of a call whose arguments were checked (scratch: rows_scratch_bytes
// of it, 8-byte aligned): one for a call without text, five else.
template <class Sink>
inline int parse_launch(const char* who, const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_units,
                        uint64_t batch_bytes, uint64_t nbins, uint64_t cap_rows, const Sink& sink,
                        uint64_t* d_unit_row0, uint64_t* d_status, void* d_scratch, hipStream_t s) {
    if (n_units == 0 || batch_bytes == 0) {   // no text: no rows
        hipLaunchKernelGGL(kfp_empty_kernel, dim3(1), dim3(256), 0, s, n_units, d_unit_row0, d_status);
        if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "%s: launch failed", who);
        return KF_OK;
    }
    const uint64_t nb = (batch_bytes + kPTile - 1) / kPTile;
    const uint64_t cap = cap_of(batch_bytes, cap_rows);
    const Scratch sc = carve(d_scratch, nb);
    const int n = n_units;
    hipLaunchKernelGGL(kfp_count_kernel, dim3((uint32_t)nb), dim3(kPBlock), 0, s, d_bytes, batch_bytes, d_goff, n, sc.blk,
                       sc.bad_row);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, sc.blk, (uint32_t)nb, sc.total);
    hipLaunchKernelGGL(kfp_scatter_kernel, dim3((uint32_t)nb), dim3(kPBlock), 0, s, d_bytes, batch_bytes, d_goff, n,
                       sc.blk, sc.table, cap);
    if (cap) {
        const uint32_t grid = (uint32_t)(cap < kPMaxGrid ? cap : kPMaxGrid);
        hipLaunchKernelGGL(kfp_rows_kernel<Sink>, dim3(grid), dim3(kPBlock), 0, s, d_bytes, batch_bytes, d_goff, n, nbins,
                           cap, sink, sc.total, sc.table, sc.bad_row);
    }
    hipLaunchKernelGGL(kfp_finish_kernel<Sink>, dim3(1), dim3(kPBlock), 0, s, d_bytes, batch_bytes, d_goff, n, nbins, cap,
                       sink, sc.total, sc.table, sc.bad_row, d_unit_row0, d_status);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "%s: launch failed", who);
    return KF_OK;
}

}  // namespace
}  // namespace kf

// kf_kfformat.hip -- kf_format_kf_rows16: get_chunks `.kf` text written in HBM.
//
// The inverse of kf_kfparse.hip: uint16 window rows become the lines that
// kf_write_kf_segments16 writes for raw counts (format_line in kf_host.cpp),
// back to back in d_text, with every line's offset.  The contract (the line,
// the three column forms, status codes, errors) is in include/kf2vec_gpu.h;
// chunks.format_rows_host states it on the host.
//
// The flat cell array (n_rows * nbins counts) is cut into tiles of kFTile cells,
// 8 consecutive cells per thread, whatever nbins is: thousands of 32-column rows
// and a few rows of millions of columns fill the device alike.  Row edges fall
// inside tiles; the thread that holds a row's first cell also owns its name.
//   0. one workgroup: the flags of the call, and d_prefix_off checked
//   1. rows: a thread per row checks the row's prefix, stores the name's length
//      and zeroes the row's count of zero columns
//   2. zeros (without pseudocount only): a row's form -- "c.0", or "c" if it has
//      no zero column or only zero columns -- is known before any length in it is
//   3. count: a tile's text length (thread_len, the one function that both this
//      pass and the scatter take a thread's length from)
//   4. one workgroup: the tile lengths scanned in place, d_row_off[n_rows] and
//      the status
//   5. scatter: the same lengths again, a workgroup scan for every thread's first
//      byte, the row offsets, and the text.  A tile's text is staged in LDS at
//      the same offset modulo 16 as its place in d_text has, so its interior
//      leaves as aligned 16-byte stores and its ragged head and tail (and
//      anything cut by cap_bytes) as byte stores: no dword is shared between
//      workgroups.  Text longer than the LDS stage (long names) goes window by
//      window.
// No workgroup waits for another; nothing is allocated; the host never waits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_internal.h"
#include "kf_scan.h"

namespace kf {
namespace {

constexpr int kFBlock = 256;                  // threads per workgroup
constexpr int kFWaves = kFBlock / 64;
constexpr int kFPer = 8;                      // cells per thread: one 16-byte load
constexpr uint32_t kFTile = kFBlock * kFPer;  // cells per tile
constexpr uint32_t kFStage = 20u << 10;       // bytes of LDS stage: 8 B x kFTile cells + 4 KiB of names
constexpr uint64_t kNoRow = ~0ull;
constexpr uint64_t kBadName = ~0ull;

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// scratch: [0] the first bad row, [1] d_prefix_off is decreasing somewhere, then
// a name length and a zero count per row, then the tile lengths (nt + 1)
struct Scratch {
    unsigned long long* bad_row;
    uint64_t* table_bad;
    uint64_t* name_len;
    unsigned long long* zeros;
    uint64_t* tile;
};
__host__ __device__ inline Scratch carve(void* scratch, uint64_t n_rows) {
    Scratch s;
    uint64_t* w = (uint64_t*)scratch;
    s.bad_row = (unsigned long long*)w;
    s.table_bad = w + 1;
    s.name_len = w + 2;
    s.zeros = (unsigned long long*)(w + 2 + n_rows);
    s.tile = w + 2 + 2 * n_rows;
    return s;
}

struct Shape {
    uint64_t n_rows, nbins, n_cells;
    int shift;   // log2(nbins) if it is a power of two, else -1
};
__device__ __forceinline__ void row_col(const Shape& S, uint64_t i, uint64_t* r, uint64_t* c) {
    if (S.shift >= 0) {
        *r = i >> S.shift;
        *c = i & (S.nbins - 1);
    } else {
        *r = i / S.nbins;
        *c = i - *r * S.nbins;
    }
}

// decimal digits of x
__device__ __forceinline__ uint32_t ndig64(uint64_t x) {
    uint32_t n = 1;
    while (x >= 10) {
        x /= 10;
        ++n;
    }
    return n;
}
__device__ __forceinline__ uint32_t ndig16(uint32_t c) {
    return 1u + (c >= 10u) + (c >= 100u) + (c >= 1000u) + (c >= 10000u);
}

// THE length of a cell's text with its ',' or '\n': count and scatter both use it.
__device__ __forceinline__ uint32_t cell_len(uint32_t c, bool flt) { return ndig16(c) + (flt ? 3u : 1u); }

// A cell's text, first byte lowest (at most 8 bytes: "65535.0,"); cell_len bytes of it count.
__device__ __forceinline__ uint64_t cell_text(uint32_t c, bool flt, uint32_t frac, uint32_t term) {
    uint64_t v = term;
    if (flt) v = v << 16 | (uint64_t)(frac << 8 | '.');
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        if (d == 0 || c) {
            const uint32_t q = (c * 52429u) >> 19;   // c / 10 for c < 81920
            v = v << 8 | (uint64_t)('0' + (c - q * 10u));
            c = q;
        }
    }
    return v;
}

// A thread's 8 cells, packed (two words, so a loop that is not unrolled can take
// cell q without an indexed register array).
struct Cells {
    uint64_t lo, hi;
    __device__ __forceinline__ uint32_t operator[](int q) const {
        return (uint32_t)((q < 4 ? lo : hi) >> (16 * (q & 3))) & 0xFFFFu;
    }
};
// the 8 cells from i0, zero from n_cells on
__device__ __forceinline__ Cells load_cells(const uint16_t* __restrict__ counts, uint64_t i0, uint64_t n_cells) {
    Cells c{0, 0};
    if (i0 + kFPer <= n_cells && (((uintptr_t)(counts + i0)) & 15) == 0) {
        const v4u w = *(const v4u*)(counts + i0);
        c.lo = (uint64_t)w[1] << 32 | w[0];
        c.hi = (uint64_t)w[3] << 32 | w[2];
    } else {
#pragma unroll
        for (int q = 0; q < kFPer; ++q) {
            const uint64_t x = i0 + q < n_cells ? (uint64_t)counts[i0 + q] : 0ull;
            if (q < 4) c.lo |= x << (16 * q);
            else c.hi |= x << (16 * (q - 4));
        }
    }
    return c;
}

// whether row r is written as float text
__device__ __forceinline__ bool row_is_float(const Scratch& sc, const Shape& S, int pseudo, uint64_t r) {
    if (pseudo) return true;
    const uint64_t z = sc.zeros[r];
    return !(z == 0 || z == S.nbins);
}

// a row's name length with its ',' (0 for a bad row: nothing is formatted then)
__device__ __forceinline__ uint64_t name_len_of(const Scratch& sc, uint64_t r) {
    const uint64_t n = sc.name_len[r];
    return n == kBadName ? 0 : n;
}

// Text bytes of the calling thread's cells (with the names of the rows that
// start among them): the count pass adds these up, the scatter pass places the
// thread's text by them.
__device__ __forceinline__ uint64_t thread_len(const Scratch& sc, const Shape& S, int pseudo, uint64_t i0,
                                               const Cells& c) {
    if (i0 >= S.n_cells) return 0;
    uint64_t r, col;
    row_col(S, i0, &r, &col);
    bool flt = row_is_float(sc, S, pseudo, r);
    uint64_t len = 0;
#pragma unroll
    for (int q = 0; q < kFPer; ++q) {
        if (i0 + q >= S.n_cells) break;
        if (col == 0) {
            if (q) flt = row_is_float(sc, S, pseudo, r);
            len += name_len_of(sc, r);
        }
        len += cell_len(c[q], flt);
        if (++col == S.nbins) {
            col = 0;
            ++r;
        }
    }
    return len;
}

// ---------------------------------------------------------------- 0, 1: tables
__global__ void __launch_bounds__(1024) kff_init_kernel(const uint64_t* __restrict__ prefix_off, int32_t n_prefixes,
                                                        Scratch sc) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int32_t p = threadIdx.x; p < n_prefixes; p += 1024)
        if (prefix_off[p] > prefix_off[p + 1]) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        *sc.bad_row = kNoRow;
        *sc.table_bad = (uint64_t)bad;
    }
}

__global__ void __launch_bounds__(kFBlock) kff_rows_kernel(uint64_t n_rows, const uint64_t* __restrict__ prefix_off,
                                                           int32_t n_prefixes, const uint32_t* __restrict__ row_prefix,
                                                           const uint64_t* __restrict__ row_start, uint32_t win_len,
                                                           Scratch sc) {
    const uint64_t r = (uint64_t)blockIdx.x * kFBlock + threadIdx.x;
    if (r >= n_rows) return;
    sc.zeros[r] = 0;
    const uint32_t p = row_prefix[r];
    uint64_t len = kBadName;
    if (p < (uint32_t)n_prefixes) {
        const uint64_t a = prefix_off[p], b = prefix_off[p + 1];
        if (a <= b) {
            len = b - a + 1;
            if (win_len) {
                const uint64_t s = row_start[r];
                len += ndig64(s + 1) + 1 + ndig64(s + win_len);
            }
        }
    }
    sc.name_len[r] = len;
    if (len == kBadName) atomicMin(sc.bad_row, (unsigned long long)r);
}

// ---------------------------------------------------------------- 2: zero columns per row
__global__ void __launch_bounds__(kFBlock) kff_zeros_kernel(const uint16_t* __restrict__ counts, Shape S, Scratch sc) {
    __shared__ uint32_t red[kFWaves];
    const uint64_t t0 = (uint64_t)blockIdx.x * kFTile;
    const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kFPer;
    const Cells c = load_cells(counts, i0, S.n_cells);
    uint64_t ra, rb, ca, cb;
    row_col(S, t0, &ra, &ca);
    row_col(S, min(t0 + kFTile, S.n_cells) - 1, &rb, &cb);
    if (ra == rb) {   // the whole tile inside one row (the same answer in every thread): one atomic
        uint32_t z = 0;
#pragma unroll
        for (int q = 0; q < kFPer; ++q) z += i0 + q < S.n_cells && c[q] == 0 ? 1u : 0u;
        const uint32_t all = block_sum<kFWaves>(z, red);
        if (threadIdx.x == 0 && all) atomicAdd(sc.zeros + ra, (unsigned long long)all);
        return;
    }
    if (i0 >= S.n_cells) return;
    uint64_t r, col;
    row_col(S, i0, &r, &col);
    uint32_t z = 0;
#pragma unroll
    for (int q = 0; q < kFPer; ++q) {
        if (i0 + q >= S.n_cells) break;
        z += c[q] == 0 ? 1u : 0u;
        if (++col == S.nbins) {
            if (z) atomicAdd(sc.zeros + r, (unsigned long long)z);
            z = 0;
            col = 0;
            ++r;
        }
    }
    if (z) atomicAdd(sc.zeros + r, (unsigned long long)z);
}

// ---------------------------------------------------------------- 3, 4: lengths and their scan
__global__ void __launch_bounds__(kFBlock) kff_count_kernel(const uint16_t* __restrict__ counts, Shape S, int pseudo,
                                                            Scratch sc) {
    __shared__ uint64_t wsum[kFWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * kFTile + (uint64_t)threadIdx.x * kFPer;
    const Cells c = load_cells(counts, i0, S.n_cells);
    uint64_t tot;
    block_excl_scan<kFWaves>(thread_len(sc, S, pseudo, i0, c), wsum, &tot);
    if (threadIdx.x == 0) sc.tile[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) kff_scan_kernel(uint64_t nt, uint64_t n_rows, uint64_t cap, Scratch sc,
                                                        uint64_t* row_off, uint64_t* status) {
    __shared__ uint64_t wsum[16];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nt; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        uint64_t tot;
        const uint64_t ex = block_excl_scan<16>(i < nt ? sc.tile[i] : (uint64_t)0, wsum, &tot);
        if (i < nt) sc.tile[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        const uint64_t bad = *sc.bad_row;
        const bool refused = bad != kNoRow || *sc.table_bad;
        sc.tile[nt] = carry;
        row_off[n_rows] = refused ? 0 : carry;
        status[0] = refused ? 2 : carry > cap ? 1 : 0;
        status[1] = refused ? 0 : carry;
        status[2] = refused ? (bad != kNoRow ? bad : n_rows) : 0;
        status[3] = 0;
    }
}

// ---------------------------------------------------------------- 5: the text
// The LDS stage holds the bytes [w0, w0 + kFStage) of the tile's text, counted
// from the 16-byte line of d_text that the tile's first byte lies in.
struct Stage {
    uint8_t* lds;
    uint64_t w0;
    __device__ __forceinline__ void put(uint64_t v, uint32_t b) const {
        const uint64_t x = v - w0;
        if (x < kFStage) lds[x] = (uint8_t)b;
    }
    // `len` low bytes of `text` at v
    __device__ __forceinline__ void put_cell(uint64_t v, uint64_t text, uint32_t len) const {
        const uint64_t x = v - w0;   // wraps far above kFStage if v < w0
        if (x <= kFStage - 8) {      // 8 bytes from x lie inside the stage
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b)
                if (b < len) lds[x + b] = (uint8_t)(text >> (8 * b));
        } else {
            for (uint32_t b = 0; b < len; ++b) put(v + b, (uint32_t)(text >> (8 * b)) & 0xFFu);
        }
    }
    // decimal text of x (nd digits) at v
    __device__ __forceinline__ void put_dec(uint64_t v, uint64_t x, uint32_t nd) const {
        for (uint32_t k = nd; k-- > 0;) {
            put(v + k, '0' + (uint32_t)(x % 10));
            x /= 10;
        }
    }
};

__global__ void __launch_bounds__(kFBlock) kff_scatter_kernel(
    const uint16_t* __restrict__ counts, Shape S, const uint8_t* __restrict__ prefix_bytes,
    const uint64_t* __restrict__ prefix_off, const uint32_t* __restrict__ row_prefix,
    const uint64_t* __restrict__ row_start, uint32_t win_len, int pseudo, uint8_t* __restrict__ text, uint64_t cap,
    uint64_t* __restrict__ row_off, Scratch sc) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kFStage];
    __shared__ uint64_t wsum[kFWaves];
    if (*sc.bad_row != kNoRow || *sc.table_bad) return;   // the same in every thread: nothing is formatted
    const uint64_t i0 = (uint64_t)blockIdx.x * kFTile + (uint64_t)threadIdx.x * kFPer;
    const Cells c = load_cells(counts, i0, S.n_cells);
    uint64_t tot;
    const uint64_t ex = block_excl_scan<kFWaves>(thread_len(sc, S, pseudo, i0, c), wsum, &tot);
    const uint64_t g0 = sc.tile[blockIdx.x];                     // the tile's first byte in the text
    const uint32_t a = (uint32_t)((uintptr_t)(text + g0) & 15);  // and in its 16-byte line
    uint8_t* const line0 = text + g0 - a;                        // that line (never dereferenced below text + g0)
    const uint64_t vend = (uint64_t)a + tot;
    const uint32_t frac = pseudo ? '5' : '0';
    for (uint64_t w0 = 0; w0 < vend; w0 += kFStage) {
        const Stage st{lds, w0};
        if (i0 < S.n_cells) {
            uint64_t r, col;
            row_col(S, i0, &r, &col);
            bool flt = row_is_float(sc, S, pseudo, r);
            uint64_t v = (uint64_t)a + ex;
#pragma unroll 1
            for (int q = 0; q < kFPer; ++q) {
                if (i0 + q >= S.n_cells) break;
                if (col == 0) {   // the row starts here: its offset and its name
                    if (q) flt = row_is_float(sc, S, pseudo, r);
                    if (w0 == 0) row_off[r] = g0 + (v - a);
                    const uint64_t nl = sc.name_len[r];
                    if (v + nl > w0 && v < w0 + kFStage) {
                        const uint64_t b0 = prefix_off[row_prefix[r]];
                        const uint64_t pl = prefix_off[row_prefix[r] + 1] - b0;
                        const uint64_t j0 = v < w0 ? w0 - v : 0;
                        const uint64_t j1 = min(pl, w0 + kFStage - v);
                        for (uint64_t j = j0; j < j1; ++j) st.put(v + j, prefix_bytes[b0 + j]);
                        uint64_t x = v + pl;
                        if (win_len) {
                            const uint64_t s1 = row_start[r] + 1, s2 = row_start[r] + win_len;
                            const uint32_t n1 = ndig64(s1), n2 = ndig64(s2);
                            st.put_dec(x, s1, n1);
                            st.put(x + n1, '-');
                            st.put_dec(x + n1 + 1, s2, n2);
                            x += n1 + 1 + n2;
                        }
                        st.put(x, ',');
                    }
                    v += nl;
                }
                const bool last = col + 1 == S.nbins;
                const uint32_t len = cell_len(c[q], flt);
                st.put_cell(v, cell_text(c[q], flt, frac, last ? '\n' : ','), len);
                v += len;
                if (last) {
                    col = 0;
                    ++r;
                } else {
                    ++col;
                }
            }
        }
        __syncthreads();
        // the stage to d_text: whole 16-byte lines that this tile alone owns as one
        // store, the tile's first and last line and whatever cap cuts byte by byte
        const uint64_t wn = min((uint64_t)kFStage, vend - w0);
        for (uint32_t x = threadIdx.x * 16; x < wn; x += kFBlock * 16) {
            const uint64_t v = w0 + x;                       // first byte of the line
            const uint64_t lo = max(v, (uint64_t)a), hi = min(v + 16, vend);   // the tile's bytes in it
            if (lo == v && hi == v + 16 && g0 + (v - a) + 16 <= cap) {   // (lo == v: v >= a)
                *(v4u*)(line0 + v) = *(const v4u*)(lds + x);
            } else {
                for (uint64_t y = lo; y < hi; ++y)
                    if (g0 + (y - a) < cap) line0[y] = lds[y - w0];
            }
        }
        __syncthreads();
    }
}

__global__ void kff_empty_kernel(uint64_t* row_off, uint64_t* status) {
    if (threadIdx.x == 0) row_off[0] = 0;
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

inline bool mul_overflows(uint64_t a, uint64_t b) { return b && a > ~0ull / b; }
constexpr uint64_t kMaxTiles = 1ull << 31;   // grid size

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" uint64_t kf_format_kf_scratch_bytes(uint64_t n_rows, uint64_t nbins) {
    if (mul_overflows(n_rows, nbins)) return ~0ull;
    const uint64_t nt = (n_rows * nbins + kFTile - 1) / kFTile;
    return 16 + 16 * n_rows + 8 * (nt + 1);
}

extern "C" int kf_format_kf_rows16(const uint16_t* d_counts, uint64_t n_rows, uint64_t nbins,
                                   const uint8_t* d_prefix_bytes, const uint64_t* d_prefix_off, int32_t n_prefixes,
                                   const uint32_t* d_row_prefix, const uint64_t* d_row_start, uint32_t win_len,
                                   int pseudocount, uint8_t* d_text, uint64_t cap_bytes, uint64_t* d_row_off,
                                   uint64_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (nbins == 0) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: nbins == 0");
    if (n_rows >= (1ull << 31))
        return kf_fail(KF_EINVAL, "kf_format_kf_rows16: %llu rows: fewer than 2^31 per call", (unsigned long long)n_rows);
    if (cap_bytes >= (1ull << 32))
        return kf_fail(KF_EINVAL, "kf_format_kf_rows16: cap_bytes %llu: at most 4 GiB - 1 per call",
                       (unsigned long long)cap_bytes);
    if (n_prefixes < 0) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: negative prefix count");
    if (mul_overflows(n_rows, nbins) || (n_rows * nbins + kFTile - 1) / kFTile >= kMaxTiles)
        return kf_fail(KF_EINVAL, "kf_format_kf_rows16: %llu x %llu cells: fewer than 2^42 per call",
                       (unsigned long long)n_rows, (unsigned long long)nbins);
    if (!d_row_off) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_row_off");
    if (!d_status) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_status");
    if (n_rows) {
        if (!d_counts) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_counts");
        if (!d_prefix_bytes) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_prefix_bytes");
        if (!d_prefix_off) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_prefix_off");
        if (!d_row_prefix) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_row_prefix");
        if (!d_row_start) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_row_start");
        if (!d_text) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_text");
        if (!d_scratch) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: null d_scratch");
    }
    if ((uintptr_t)d_counts & 1) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: misaligned d_counts (needs 2 bytes)");
    if ((uintptr_t)d_row_prefix & 3)
        return kf_fail(KF_EINVAL, "kf_format_kf_rows16: misaligned d_row_prefix (needs 4 bytes)");
    if ((uintptr_t)d_prefix_off & 7)
        return kf_fail(KF_EINVAL, "kf_format_kf_rows16: misaligned d_prefix_off (needs 8 bytes)");
    if ((uintptr_t)d_row_start & 7)
        return kf_fail(KF_EINVAL, "kf_format_kf_rows16: misaligned d_row_start (needs 8 bytes)");
    if ((uintptr_t)d_row_off & 7) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: misaligned d_row_off (needs 8 bytes)");
    if ((uintptr_t)d_status & 7) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: misaligned d_status (needs 8 bytes)");
    if ((uintptr_t)d_scratch & 7) return kf_fail(KF_EINVAL, "kf_format_kf_rows16: misaligned d_scratch (needs 8 bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        hipLaunchKernelGGL(kff_empty_kernel, dim3(1), dim3(64), 0, s, d_row_off, d_status);
        if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_format_kf_rows16: launch failed");
        return KF_OK;
    }
    const uint64_t need = kf_format_kf_scratch_bytes(n_rows, nbins);
    if (scratch_bytes < need)
        return kf_fail(KF_ERANGE, "kf_format_kf_rows16: scratch needs %llu bytes, %llu given", (unsigned long long)need,
                       (unsigned long long)scratch_bytes);
    Shape S;
    S.n_rows = n_rows;
    S.nbins = nbins;
    S.n_cells = n_rows * nbins;
    S.shift = -1;
    if ((nbins & (nbins - 1)) == 0)
        for (int b = 0; b < 64; ++b)
            if (nbins >> b == 1) S.shift = b;
    const uint64_t nt = (S.n_cells + kFTile - 1) / kFTile;
    const Scratch sc = carve(d_scratch, n_rows);
    const uint32_t row_grid = (uint32_t)((n_rows + kFBlock - 1) / kFBlock);
    hipLaunchKernelGGL(kff_init_kernel, dim3(1), dim3(1024), 0, s, d_prefix_off, n_prefixes, sc);
    hipLaunchKernelGGL(kff_rows_kernel, dim3(row_grid), dim3(kFBlock), 0, s, n_rows, d_prefix_off, n_prefixes,
                       d_row_prefix, d_row_start, win_len, sc);
    if (!pseudocount) hipLaunchKernelGGL(kff_zeros_kernel, dim3((uint32_t)nt), dim3(kFBlock), 0, s, d_counts, S, sc);
    hipLaunchKernelGGL(kff_count_kernel, dim3((uint32_t)nt), dim3(kFBlock), 0, s, d_counts, S, pseudocount ? 1 : 0, sc);
    hipLaunchKernelGGL(kff_scan_kernel, dim3(1), dim3(1024), 0, s, nt, n_rows, cap_bytes, sc, d_row_off, d_status);
    hipLaunchKernelGGL(kff_scatter_kernel, dim3((uint32_t)nt), dim3(kFBlock), 0, s, d_counts, S, d_prefix_bytes,
                       d_prefix_off, d_row_prefix, d_row_start, win_len, pseudocount ? 1 : 0, d_text, cap_bytes,
                       d_row_off, sc);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_format_kf_rows16: launch failed");
    return KF_OK;
}

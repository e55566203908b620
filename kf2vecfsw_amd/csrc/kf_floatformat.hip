// kf_floatformat.hip -- kf_format_float_rows: tables of floats as text in HBM.
//
// The inverse of kf_kffloat.hip and kf_tsvfloat.hip: row r of d_vals becomes the
// line  prefix_r sep f_0 sep ... sep f_{ncols-1} eol,  every f the shortest
// decimal that reads back as the value (kf_shortest.h), the lines back to back in
// d_text with every line's offset.  The contract (the three forms, the NaN flag,
// status codes, errors) is in include/kf2vec_gpu.h; tables.format_float_rows_host
// states it on the host, and kf_format_float_host runs the same inline code there.
//
// The skeleton is kf_kfformat.hip's: the flat cell array (n_rows * ncols values)
// is cut into tiles of kTTile cells, kTPer consecutive cells per thread, whatever
// ncols is; row edges fall inside tiles; the thread that holds a row's first cell
// also owns its prefix.
//   0. one workgroup: the flags of the call, and d_prefix_off checked
//   1. rows: a thread per row checks the row's prefix and stores its length
//   2. count: every cell's decimal (w, q, digits, sign, class, notation), kept
//      in the scratch, and a tile's text length
//   3. one workgroup: the tile lengths scanned in place, d_row_off[n_rows] and
//      the status
//   4. scatter: the decimals read back, a workgroup scan for every thread's first
//      byte, the row offsets, and the text, staged in LDS at the same offset
//      modulo 16 as its place in d_text has: the interior leaves as aligned
//      16-byte stores, the ragged head and tail (and anything cut by cap_bytes)
//      as byte stores.
// A cell's digits cost three 64 x 128-bit products and a few 64-bit divisions;
// the count pass keeps them, 16 bytes a cell, and the scatter pass reads them
// back instead of computing them again.  Measured against computing them in
// both passes (profiles/r20/float_format_ab.json, the two taking turns twice):
// 2.48 against 2.99 ms for 4,000 x 10,000 float32 widened, 1.86 against 2.18 ms
// in the float32 form, 1.02 against 1.20 ms for 4,000 x 4,000 float64.  The
// kernels are bound by their integer work, so 32 bytes of traffic per cell cost
// less than the second computation.  The price is scratch: 16 bytes per cell.
// No workgroup waits for another; nothing is allocated; the host never waits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "kf_internal.h"
#include "kf_scan.h"
#include "kf_shortest.h"

namespace kf {
namespace {

constexpr int kTBlock = 256;                  // threads per workgroup
constexpr int kTWaves = kTBlock / 64;
constexpr int kTPer = 4;                      // cells per thread: 16 bytes of float32, 32 of float64
constexpr uint32_t kTTile = kTBlock * kTPer;  // cells per tile
constexpr uint32_t kTStage = 32u << 10;       // bytes of LDS stage: 26 B x kTTile cells + 5.9 KiB of prefixes
constexpr uint64_t kNoRow = ~0ull;
constexpr uint64_t kBadName = ~0ull;

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// scratch: the powers of ten, then [0] the first bad row, [1] d_prefix_off is
// decreasing somewhere, then a prefix length per row, the tile lengths (nt + 1),
// and two words per cell: w, and q | digits << 32 | sign << 40 | class << 48 | fixed << 56
struct Scratch {
    const uint64_t* pow10;
    unsigned long long* bad_row;
    uint64_t* table_bad;
    uint64_t* name_len;
    uint64_t* tile;
    uint64_t* cell_w;
    uint64_t* cell_m;
};
__host__ __device__ inline Scratch carve(void* scratch, uint64_t n_rows, uint64_t nt, uint64_t n_cells) {
    Scratch s;
    uint64_t* w = (uint64_t*)scratch;
    s.pow10 = w;
    w += kShTableWords;
    s.bad_row = (unsigned long long*)w;
    s.table_bad = w + 1;
    s.name_len = w + 2;
    s.tile = w + 2 + n_rows;
    s.cell_w = s.tile + nt + 1;
    s.cell_m = s.cell_w + n_cells;
    return s;
}

struct Shape {
    uint64_t n_rows, ncols, n_cells;
    int shift;       // log2(ncols) if it is a power of two, else -1
    int form;        // kFormF64, kFormF32, kFormF32Wide
    int nan_empty;
    uint32_t sep, eol0, eol1, eol_len;
};
__device__ __forceinline__ void row_col(const Shape& S, uint64_t i, uint64_t* r, uint64_t* c) {
    if (S.shift >= 0) {
        *r = i >> S.shift;
        *c = i & (S.ncols - 1);
    } else {
        *r = i / S.ncols;
        *c = i - *r * S.ncols;
    }
}

// A thread's kTPer cells as bit patterns (a float32 in the low word), zero from n_cells on
struct Cells {
    uint64_t b[kTPer];
};
__device__ __forceinline__ Cells load_cells(const void* __restrict__ vals, int form, uint64_t i0, uint64_t n_cells) {
    Cells c;
#pragma unroll
    for (int q = 0; q < kTPer; ++q) c.b[q] = 0;
    if (form == kFormF64) {
        const uint64_t* p = (const uint64_t*)vals + i0;
        if (i0 + kTPer <= n_cells && ((uintptr_t)p & 15) == 0) {
            const v4u a = *(const v4u*)p, b = *(const v4u*)(p + 2);
            c.b[0] = (uint64_t)a[1] << 32 | a[0];
            c.b[1] = (uint64_t)a[3] << 32 | a[2];
            c.b[2] = (uint64_t)b[1] << 32 | b[0];
            c.b[3] = (uint64_t)b[3] << 32 | b[2];
        } else {
#pragma unroll
            for (int q = 0; q < kTPer; ++q)
                if (i0 + q < n_cells) c.b[q] = p[q];
        }
    } else {
        const uint32_t* p = (const uint32_t*)vals + i0;
        if (i0 + kTPer <= n_cells && ((uintptr_t)p & 15) == 0) {
            const v4u a = *(const v4u*)p;
#pragma unroll
            for (int q = 0; q < kTPer; ++q) c.b[q] = a[q];
        } else {
#pragma unroll
            for (int q = 0; q < kTPer; ++q)
                if (i0 + q < n_cells) c.b[q] = p[q];
        }
    }
    return c;
}

// a row's prefix length with its separator (0 for an empty prefix, and for a bad row: nothing is formatted then)
__device__ __forceinline__ uint64_t name_len_of(const Scratch& sc, uint64_t r) {
    const uint64_t n = sc.name_len[r];
    return n == kBadName ? 0 : n;
}

// A thread's cells as decimals: the count pass computes them and keeps them in
// the scratch, the scatter pass reads them back.
struct Decs {
    Dec d[kTPer];
};
__device__ __forceinline__ uint64_t pack_meta(const Dec& d) {
    return (uint64_t)(uint32_t)d.q | (uint64_t)d.nd << 32 | (uint64_t)d.neg << 40 | (uint64_t)d.cls << 48 |
           (uint64_t)d.fixed << 56;
}
__device__ __forceinline__ Dec unpack(uint64_t w, uint64_t m) {
    Dec d;
    d.w = w;
    d.q = (int32_t)(uint32_t)m;
    d.nd = (uint8_t)(m >> 32);
    d.neg = (uint8_t)(m >> 40);
    d.cls = (uint8_t)(m >> 48);
    d.fixed = (uint8_t)(m >> 56);
    return d;
}

// The text bytes of the thread (with the prefixes of the rows that start among
// its cells): the count pass adds these up, the scatter pass places the thread's
// text by them.
__device__ __forceinline__ uint64_t thread_len(const Scratch& sc, const Shape& S, uint64_t i0, const Decs& ds) {
    if (i0 >= S.n_cells) return 0;
    uint64_t r, col;
    row_col(S, i0, &r, &col);
    uint64_t len = 0;
#pragma unroll
    for (int q = 0; q < kTPer; ++q) {
        if (i0 + q < S.n_cells) {
            if (col == 0) len += name_len_of(sc, r);
            len += dec_len(ds.d[q], S.nan_empty != 0);
            if (++col == S.ncols) {
                len += S.eol_len;
                col = 0;
                ++r;
            } else {
                len += 1;
            }
        }
    }
    return len;
}

// ---------------------------------------------------------------- 0, 1: tables
__global__ void __launch_bounds__(1024) kft_init_kernel(const uint64_t* __restrict__ prefix_off, int32_t n_prefixes,
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

__global__ void __launch_bounds__(kTBlock) kft_rows_kernel(uint64_t n_rows, const uint64_t* __restrict__ prefix_off,
                                                           int32_t n_prefixes, const uint32_t* __restrict__ row_prefix,
                                                           Scratch sc) {
    const uint64_t r = (uint64_t)blockIdx.x * kTBlock + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t p = row_prefix[r];
    uint64_t len = kBadName;
    if (p < (uint32_t)n_prefixes) {
        const uint64_t a = prefix_off[p], b = prefix_off[p + 1];
        if (a <= b) len = b > a ? b - a + 1 : 0;
    }
    sc.name_len[r] = len;
    if (len == kBadName) atomicMin(sc.bad_row, (unsigned long long)r);
}

// ---------------------------------------------------------------- 2, 3: lengths and their scan
__global__ void __launch_bounds__(kTBlock) kft_count_kernel(const void* __restrict__ vals, Shape S, Scratch sc) {
    __shared__ uint64_t wsum[kTWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTTile + (uint64_t)threadIdx.x * kTPer;
    const Cells c = load_cells(vals, S.form, i0, S.n_cells);
    Decs ds;
#pragma unroll
    for (int q = 0; q < kTPer; ++q) {
        if (i0 + q < S.n_cells) {
            ds.d[q] = dec_of(c.b[q], S.form, sc.pow10);
            sc.cell_w[i0 + q] = ds.d[q].w;
            sc.cell_m[i0 + q] = pack_meta(ds.d[q]);
        }
    }
    uint64_t tot;
    block_excl_scan<kTWaves>(thread_len(sc, S, i0, ds), wsum, &tot);
    if (threadIdx.x == 0) sc.tile[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) kft_scan_kernel(uint64_t nt, uint64_t n_rows, uint64_t cap, Scratch sc,
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

// ---------------------------------------------------------------- 4: the text
// The LDS stage holds the bytes [w0, w0 + kTStage) of the tile's text, counted
// from the 16-byte line of d_text that the tile's first byte lies in.
struct Stage {
    uint8_t* lds;
    uint64_t w0;
    __device__ __forceinline__ void put(uint64_t v, uint32_t b) const {
        const uint64_t x = v - w0;           // wraps far above kTStage if v < w0
        if (x < kTStage) lds[x] = (uint8_t)b;
    }
};
// dec_put's sink: a cell's text from byte v of the tile on
struct CellSink {
    const Stage& st;
    uint64_t v;
    __device__ __forceinline__ void put(uint32_t i, uint32_t b) const { st.put(v + i, b); }
};

__global__ void __launch_bounds__(kTBlock) kft_scatter_kernel(
    Shape S, const uint8_t* __restrict__ prefix_bytes,
    const uint64_t* __restrict__ prefix_off, const uint32_t* __restrict__ row_prefix, uint8_t* __restrict__ text,
    uint64_t cap, uint64_t* __restrict__ row_off, Scratch sc) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kTStage];
    __shared__ uint64_t wsum[kTWaves];
    if (*sc.bad_row != kNoRow || *sc.table_bad) return;   // the same in every thread: nothing is formatted
    const uint64_t i0 = (uint64_t)blockIdx.x * kTTile + (uint64_t)threadIdx.x * kTPer;
    Decs ds;
#pragma unroll
    for (int q = 0; q < kTPer; ++q)
        if (i0 + q < S.n_cells) ds.d[q] = unpack(sc.cell_w[i0 + q], sc.cell_m[i0 + q]);
    uint64_t tot;
    const uint64_t ex = block_excl_scan<kTWaves>(thread_len(sc, S, i0, ds), wsum, &tot);
    const uint64_t g0 = sc.tile[blockIdx.x];                     // the tile's first byte in the text
    const uint32_t a = (uint32_t)((uintptr_t)(text + g0) & 15);  // and in its 16-byte line
    uint8_t* const line0 = text + g0 - a;                        // that line (never dereferenced below text + g0)
    const uint64_t vend = (uint64_t)a + tot;
    const bool nan_empty = S.nan_empty != 0;
    for (uint64_t w0 = 0; w0 < vend; w0 += kTStage) {
        const Stage st{lds, w0};
        if (i0 < S.n_cells) {
            uint64_t r, col;
            row_col(S, i0, &r, &col);
            uint64_t v = (uint64_t)a + ex;
#pragma unroll
            for (int q = 0; q < kTPer; ++q) {
                if (i0 + q < S.n_cells) {
                    if (col == 0) {          // the row starts here: its offset and its prefix
                        if (w0 == 0) row_off[r] = g0 + (v - a);
                        const uint64_t nl = sc.name_len[r];
                        if (nl && v + nl > w0 && v < w0 + kTStage) {
                            const uint64_t b0 = prefix_off[row_prefix[r]];
                            const uint64_t pl = nl - 1;
                            const uint64_t j0 = v < w0 ? w0 - v : 0;
                            const uint64_t j1 = min(pl, w0 + kTStage - v);
                            for (uint64_t j = j0; j < j1; ++j) st.put(v + j, prefix_bytes[b0 + j]);
                            st.put(v + pl, S.sep);
                        }
                        v += nl;
                    }
                    const uint32_t len = dec_len(ds.d[q], nan_empty);
                    if (v + len + 2 > w0 && v < w0 + kTStage) {
                        const CellSink sink{st, v};
                        dec_put(ds.d[q], nan_empty, sink);
                    }
                    v += len;
                    if (col + 1 == S.ncols) {
                        st.put(v, S.eol0);
                        if (S.eol_len == 2) st.put(v + 1, S.eol1);
                        v += S.eol_len;
                        col = 0;
                        ++r;
                    } else {
                        st.put(v, S.sep);
                        v += 1;
                        ++col;
                    }
                }
            }
        }
        __syncthreads();
        // the stage to d_text: whole 16-byte lines that this tile alone owns as one
        // store, the tile's first and last line and whatever cap cuts byte by byte
        const uint64_t wn = min((uint64_t)kTStage, vend - w0);
        for (uint32_t x = threadIdx.x * 16; x < wn; x += kTBlock * 16) {
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

__global__ void kft_empty_kernel(uint64_t* row_off, uint64_t* status) {
    if (threadIdx.x == 0) row_off[0] = 0;
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

inline bool mul_overflows(uint64_t a, uint64_t b) { return b && a > ~0ull / b; }
constexpr uint64_t kMaxTiles = 1ull << 24;   // a launch has fewer than 2^32 threads

// the form of a call, or -1
inline int form_of(int val_bytes, int mode) {
    if (val_bytes == 8 && mode == KF_FLOAT_SHORTEST) return kFormF64;
    if (val_bytes == 4 && mode == KF_FLOAT_SHORTEST) return kFormF32;
    if (val_bytes == 4 && mode == KF_FLOAT_WIDENED) return kFormF32Wide;
    return -1;
}

struct HostSink {
    uint8_t* p;
    void put(uint32_t i, uint32_t b) const { p[i] = (uint8_t)b; }
};

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_format_float_tile(void) { return (int)kTTile; }

extern "C" int kf_format_float_host(const void* vals, int val_bytes, int mode, int nan_empty, uint64_t n, uint8_t* out,
                                    uint8_t* len) {
    const int form = form_of(val_bytes, mode);
    if (form < 0)
        return kf_fail(KF_EINVAL, "kf_format_float_host: val_bytes %d with mode %d: 8 or 4 bytes shortest, 4 bytes widened",
                       val_bytes, mode);
    if (n && (!vals || !out || !len)) return kf_fail(KF_EINVAL, "kf_format_float_host: null pointer");
    const uint64_t* table = kf_pow10_ceil_table();
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t bits = 0;
        memcpy(&bits, (const uint8_t*)vals + i * (uint64_t)val_bytes, (size_t)val_bytes);   // little-endian: the low word
        const Dec d = dec_of(bits, form, table);
        uint8_t* slot = out + kFloatTextMax * i;
        memset(slot, 0, kFloatTextMax);
        len[i] = (uint8_t)dec_len(d, nan_empty != 0);
        const HostSink sink{slot};
        dec_put(d, nan_empty != 0, sink);
    }
    return KF_OK;
}

extern "C" int kf_shortest_decimal_host(const void* vals, int val_bytes, int mode, uint64_t n, uint64_t* w, int32_t* q,
                                        uint8_t* cls) {
    const int form = form_of(val_bytes, mode);
    if (form < 0) return kf_fail(KF_EINVAL, "kf_shortest_decimal_host: val_bytes %d with mode %d", val_bytes, mode);
    if (n && (!vals || !w || !q || !cls)) return kf_fail(KF_EINVAL, "kf_shortest_decimal_host: null pointer");
    const uint64_t* table = kf_pow10_ceil_table();
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t bits = 0;
        memcpy(&bits, (const uint8_t*)vals + i * (uint64_t)val_bytes, (size_t)val_bytes);
        const Dec d = dec_of(bits, form, table);
        w[i] = d.w;
        q[i] = d.q;
        cls[i] = (uint8_t)(d.cls | d.neg << 7);
    }
    return KF_OK;
}

extern "C" uint64_t kf_format_float_scratch_bytes(uint64_t n_rows, uint64_t ncols) {
    if (mul_overflows(n_rows, ncols)) return ~0ull;
    const uint64_t nt = (n_rows * ncols + kTTile - 1) / kTTile;
    return kShTableBytes + 16 + 8 * n_rows + 8 * (nt + 1) + 16 * n_rows * ncols;
}

extern "C" int kf_format_float_rows(const void* d_vals, int val_bytes, uint64_t n_rows, uint64_t ncols, int mode,
                                    uint32_t sep, uint32_t eol, int eol_len, int nan_empty,
                                    const uint8_t* d_prefix_bytes, const uint64_t* d_prefix_off, int32_t n_prefixes,
                                    const uint32_t* d_row_prefix, uint8_t* d_text, uint64_t cap_bytes,
                                    uint64_t* d_row_off, uint64_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                                    void* stream) {
    const int form = form_of(val_bytes, mode);
    if (val_bytes != 4 && val_bytes != 8)
        return kf_fail(KF_EINVAL, "kf_format_float_rows: val_bytes %d: 8 (float64) or 4 (float32)", val_bytes);
    if (form < 0)
        return kf_fail(KF_EINVAL, "kf_format_float_rows: mode %d with %d-byte values: KF_FLOAT_SHORTEST, or "
                       "KF_FLOAT_WIDENED for float32", mode, val_bytes);
    if (ncols == 0) return kf_fail(KF_EINVAL, "kf_format_float_rows: ncols == 0");
    if (sep == 0 || sep > 255) return kf_fail(KF_EINVAL, "kf_format_float_rows: separator %u: one byte, not NUL", sep);
    if (eol_len != 1 && eol_len != 2) return kf_fail(KF_EINVAL, "kf_format_float_rows: eol_len %d: 1 or 2", eol_len);
    if (n_rows >= (1ull << 31))
        return kf_fail(KF_EINVAL, "kf_format_float_rows: %llu rows: fewer than 2^31 per call", (unsigned long long)n_rows);
    if (cap_bytes >= (1ull << 32))
        return kf_fail(KF_EINVAL, "kf_format_float_rows: cap_bytes %llu: at most 4 GiB - 1 per call",
                       (unsigned long long)cap_bytes);
    if (n_prefixes < 0) return kf_fail(KF_EINVAL, "kf_format_float_rows: negative prefix count");
    if (mul_overflows(n_rows, ncols) || (n_rows * ncols + kTTile - 1) / kTTile >= kMaxTiles)
        return kf_fail(KF_EINVAL, "kf_format_float_rows: %llu x %llu cells: fewer than 2^34 per call",
                       (unsigned long long)n_rows, (unsigned long long)ncols);
    if (!d_row_off) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_row_off");
    if (!d_status) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_status");
    if (n_rows) {
        if (!d_vals) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_vals");
        if (!d_prefix_bytes) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_prefix_bytes");
        if (!d_prefix_off) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_prefix_off");
        if (!d_row_prefix) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_row_prefix");
        if (!d_text) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_text");
        if (!d_scratch) return kf_fail(KF_EINVAL, "kf_format_float_rows: null d_scratch");
    }
    if ((uintptr_t)d_vals & (uintptr_t)(val_bytes - 1))
        return kf_fail(KF_EINVAL, "kf_format_float_rows: misaligned d_vals (needs %d bytes)", val_bytes);
    if ((uintptr_t)d_row_prefix & 3)
        return kf_fail(KF_EINVAL, "kf_format_float_rows: misaligned d_row_prefix (needs 4 bytes)");
    if ((uintptr_t)d_prefix_off & 7)
        return kf_fail(KF_EINVAL, "kf_format_float_rows: misaligned d_prefix_off (needs 8 bytes)");
    if ((uintptr_t)d_row_off & 7) return kf_fail(KF_EINVAL, "kf_format_float_rows: misaligned d_row_off (needs 8 bytes)");
    if ((uintptr_t)d_status & 7) return kf_fail(KF_EINVAL, "kf_format_float_rows: misaligned d_status (needs 8 bytes)");
    if ((uintptr_t)d_scratch & 7) return kf_fail(KF_EINVAL, "kf_format_float_rows: misaligned d_scratch (needs 8 bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        hipLaunchKernelGGL(kft_empty_kernel, dim3(1), dim3(64), 0, s, d_row_off, d_status);
        if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_format_float_rows: launch failed");
        return KF_OK;
    }
    const uint64_t need = kf_format_float_scratch_bytes(n_rows, ncols);
    if (scratch_bytes < need)
        return kf_fail(KF_ERANGE, "kf_format_float_rows: scratch needs %llu bytes, %llu given", (unsigned long long)need,
                       (unsigned long long)scratch_bytes);
    if (hipMemcpyAsync(d_scratch, kf_pow10_ceil_table(), kShTableBytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return kf_fail(KF_EHIP, "kf_format_float_rows: the copy of the powers of ten failed");
    Shape S;
    S.n_rows = n_rows;
    S.ncols = ncols;
    S.n_cells = n_rows * ncols;
    S.shift = -1;
    if ((ncols & (ncols - 1)) == 0)
        for (int b = 0; b < 64; ++b)
            if (ncols >> b == 1) S.shift = b;
    S.form = form;
    S.nan_empty = nan_empty ? 1 : 0;
    S.sep = sep;
    S.eol0 = eol & 0xFFu;
    S.eol1 = eol_len == 2 ? (eol >> 8) & 0xFFu : 0;
    S.eol_len = (uint32_t)eol_len;
    const uint64_t nt = (S.n_cells + kTTile - 1) / kTTile;
    const Scratch sc = carve(d_scratch, n_rows, nt, S.n_cells);
    const uint32_t row_grid = (uint32_t)((n_rows + kTBlock - 1) / kTBlock);
    hipLaunchKernelGGL(kft_init_kernel, dim3(1), dim3(1024), 0, s, d_prefix_off, n_prefixes, sc);
    hipLaunchKernelGGL(kft_rows_kernel, dim3(row_grid), dim3(kTBlock), 0, s, n_rows, d_prefix_off, n_prefixes,
                       d_row_prefix, sc);
    hipLaunchKernelGGL(kft_count_kernel, dim3((uint32_t)nt), dim3(kTBlock), 0, s, d_vals, S, sc);
    hipLaunchKernelGGL(kft_scan_kernel, dim3(1), dim3(1024), 0, s, nt, n_rows, cap_bytes, sc, d_row_off, d_status);
    hipLaunchKernelGGL(kft_scatter_kernel, dim3((uint32_t)nt), dim3(kTBlock), 0, s, S, d_prefix_bytes, d_prefix_off,
                       d_row_prefix, d_text, cap_bytes, d_row_off, sc);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_format_float_rows: launch failed");
    return KF_OK;
}

// kf_tsvfloat.hip -- kf_parse_tsv_floats: tab-separated tables of decimal floats
// parsed in HBM.
//
// The distance trainers of the reference read the true distance matrix of a
// clade (`<tree>_subtree_<c>.di_mtrx`, N x N repr(float64) fields under a header
// line) with pandas and reindex it into the feature matrix's order
// (kf2vec/utils.py:141-192); query reads the backbone embeddings
// (`embeddings_subtree_<c>.csv`, signed floats, no header) the same way
// (kf2vec/query.py:129-134).  Both are a name and `ncols` fields per row with
// '\t' between them: a get_frequencies `.kf` row with another separator, a sign,
// and a consumer that wants the columns in its own order.  Here the text of many
// pieces of such a file lies back to back on the device, as for
// kf_parse_kf_floats, and comes out as float64 (or float32) rows whose columns
// a map has placed, with every row's name span and every unit's row range.  The
// contract is in include/kf2vec_gpu.h; tables.parse_tsv_floats_host states it on
// the host.
//
// The passes, the scratch layout and the error reporting are kf_kfrows.h's; the
// unsigned field and the table of powers of five are kf_floatfield.h's, shared
// with kf_kffloat.hip.  This file states the sign, the map lookup and the
// strided store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_decimal.h"
#include "kf_floatfield.h"
#include "kf_kfrows.h"

namespace kf {
namespace {

// One field's state: an optional '-' as the first byte, then kf_floatfield.h's field ("-nan" is refused at its 'n').
struct TsvField {
    FloatFieldT<'\t'> f;
    uint32_t sgn;    // a '-' opened the field
    __device__ __forceinline__ int feed(uint32_t c) {
        if (f.st == 0) {
            if (c == '-' && !sgn) {
                sgn = 1;
                return 0;
            }
            if (c == 'n' && sgn) return kErrForm;
        }
        return f.feed(c);                    // a '-' anywhere else is the exponent's, or malformed
    }
};

// kf_kfrows.h's Sink: field j of row r, converted, goes to vals[r * out_cols + col_map[j]] if the map places it
struct TsvSink {
    typedef TsvField Field;
    static constexpr uint32_t kSep = '\t';
    void* __restrict__ vals;
    uint32_t* __restrict__ row_name;
    const uint64_t* __restrict__ pow5;
    const int32_t* __restrict__ col_map;     // ncols entries, or null: the identity
    uint64_t out_cols;
    int val_bytes;
    __device__ __forceinline__ Field fresh() const { return Field{{0, 0, 0, 0, 0, 0}, 0}; }
    __device__ __forceinline__ void done(uint64_t r, uint64_t ncols, uint64_t col, const Field& f, bool store,
                                         uint64_t& err) const {
        (void)ncols;
        // a negative entry widens to above any out_cols; col < ncols: the row walk hands over no other field
        const uint64_t dst = col_map ? (uint64_t)(int64_t)col_map[col] : col;
        if (dst >= out_cols) return;         // a skipped column: its form and digit count were checked, no more
        uint64_t bits = kQuietNan;
        if (f.f.st != 8) {
            if (!decimal_to_double(f.f.w, f.f.q(), pow5, &bits)) {
                note(err, col, kErrRange);
                return;
            }
            bits |= (uint64_t)f.sgn << 63;
        }
        if (!store) return;
        const double v = __longlong_as_double((long long)bits);
        if (val_bytes == 8) ((double*)vals)[r * out_cols + dst] = v;
        else ((float*)vals)[r * out_cols + dst] = (float)v;
    }
    __device__ __forceinline__ void name(uint64_t r, uint32_t at, uint32_t len, bool store) const {
        if (store) {
            row_name[2 * r] = at;
            row_name[2 * r + 1] = len;
        }
    }
};

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" uint64_t kf_parse_tsv_floats_scratch_bytes(uint64_t batch_bytes, int32_t n_units, uint64_t cap_rows) {
    (void)n_units;
    return kTableBytes + rows_scratch_bytes(batch_bytes, cap_rows);
}

extern "C" int kf_parse_tsv_floats(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_units, uint64_t batch_bytes,
                                   uint64_t ncols, const int32_t* d_col_map, uint64_t out_cols, uint64_t cap_rows,
                                   void* d_vals, int val_bytes, uint32_t* d_row_name, uint64_t* d_unit_row0,
                                   uint64_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (ncols == 0) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: ncols == 0");
    if (out_cols == 0) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: out_cols == 0");
    if (!d_col_map && out_cols != ncols)
        return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: no d_col_map (the identity) but out_cols %llu != ncols %llu",
                       (unsigned long long)out_cols, (unsigned long long)ncols);
    if (n_units < 0) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: negative unit count");
    if (val_bytes != 4 && val_bytes != 8)
        return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: val_bytes %d: 8 (float64) or 4 (float32)", val_bytes);
    if (batch_bytes >= (1ull << 32))
        return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: batch of %llu bytes: at most 4 GiB - 1 per call",
                       (unsigned long long)batch_bytes);
    if (!d_bytes) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: null d_bytes");
    if (!d_goff) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: null d_goff");
    if (!d_vals) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: null d_vals");
    if (!d_row_name) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: null d_row_name");
    if (!d_unit_row0) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: null d_unit_row0");
    if (!d_status) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: null d_status");
    if (!d_scratch) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: null d_scratch");
    if ((uintptr_t)d_bytes & 15) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_bytes (needs 16 bytes)");
    if ((uintptr_t)d_col_map & 3) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_col_map (needs 4 bytes)");
    if ((uintptr_t)d_vals & (uintptr_t)(val_bytes - 1))
        return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_vals (needs %d bytes)", val_bytes);
    if ((uintptr_t)d_row_name & 3)
        return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_row_name (needs 4 bytes)");
    if ((uintptr_t)d_goff & 7) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_goff (needs 8 bytes)");
    if ((uintptr_t)d_unit_row0 & 7)
        return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_unit_row0 (needs 8 bytes)");
    if ((uintptr_t)d_status & 7) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_status (needs 8 bytes)");
    if ((uintptr_t)d_scratch & 7) return kf_fail(KF_EINVAL, "kf_parse_tsv_floats: misaligned d_scratch (needs 8 bytes)");
    const uint64_t need = kf_parse_tsv_floats_scratch_bytes(batch_bytes, n_units, cap_rows);
    if (scratch_bytes < need)
        return kf_fail(KF_ERANGE, "kf_parse_tsv_floats: scratch needs %llu bytes, %llu given", (unsigned long long)need,
                       (unsigned long long)scratch_bytes);
    hipStream_t s = (hipStream_t)stream;
    uint64_t* d_pow5 = (uint64_t*)d_scratch;
    if (n_units != 0 && batch_bytes != 0 &&
        hipMemcpyAsync(d_pow5, kf_pow5_table(), kTableBytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return kf_fail(KF_EHIP, "kf_parse_tsv_floats: the copy of the powers of five failed");
    const TsvSink sink{d_vals, d_row_name, d_pow5, d_col_map, out_cols, val_bytes};
    return parse_launch("kf_parse_tsv_floats", d_bytes, d_goff, n_units, batch_bytes, ncols, cap_rows, sink, d_unit_row0,
                        d_status, (uint8_t*)d_scratch + kTableBytes, s);
}

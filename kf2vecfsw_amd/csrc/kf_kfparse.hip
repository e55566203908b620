// kf_kfparse.hip -- kf_parse_kf_rows: get_chunks `.kf` text parsed in HBM.
//
// The chunk trainers of the reference read a directory of get_chunks `.kf` files
// with pandas (my_read_csv_chunk, kf2vec/utils.py:402-405: read_csv with
// dtype=uint16).  Here the text of many files (or pieces of files cut at line
// starts) lies back to back on the device, unit u being d_bytes[goff[u],
// goff[u+1]), and comes out as the uint16 count rows the trainer holds, in byte
// order, with every unit's row range.  The contract (lines, fields, the field
// form, errors) is in include/kf2vec_gpu.h; chunks.parse_kf_rows_host states it
// on the host.
//
// The passes (line starts, then a workgroup per row), the scratch layout and the
// error reporting are kf_kfrows.h's, shared with kf_kffloat.hip; this file states
// the field of a get_chunks row and the uint16 store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_kfrows.h"

namespace kf {
namespace {

// One field's state: digits, then maybe '.' and zeros.
struct CountField {
    uint32_t v;
    int st;          // 0 no digit yet, 1 in the digits, 2 after the '.'
    // Feed the next byte: 0 go on, 1 the field ended well (value v), else the error code.
    __device__ __forceinline__ int feed(uint32_t c) {
        const uint32_t d = c - '0';
        if (d < 10u) {
            if (st == 2) return d == 0 ? 0 : kErrForm;
            v = v * 10 + d;      // v <= 65535 before: no wrap
            st = 1;
            return v > 65535u ? kErrValue : 0;
        }
        if (c == '.') {
            if (st != 1) return kErrForm;
            st = 2;
            return 0;
        }
        if (c == ',' || c == '\n') return st == 0 ? kErrForm : 1;
        return kErrForm;
    }
};

// kf_kfrows.h's Sink: field j of row r goes to rows[r * nbins + j]; the name is not kept
struct U16Sink {
    typedef CountField Field;
    static constexpr uint32_t kSep = ',';
    uint16_t* __restrict__ rows;
    __device__ __forceinline__ Field fresh() const { return Field{0, 0}; }
    __device__ __forceinline__ void done(uint64_t r, uint64_t nbins, uint64_t col, const Field& f, bool store,
                                         uint64_t&) const {
        if (store) rows[r * nbins + col] = (uint16_t)f.v;
    }
    __device__ __forceinline__ void name(uint64_t, uint32_t, uint32_t, bool) const {}
};

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" uint64_t kf_parse_kf_scratch_bytes(uint64_t batch_bytes, int32_t n_units, uint64_t cap_rows) {
    (void)n_units;
    return rows_scratch_bytes(batch_bytes, cap_rows);
}

extern "C" int kf_parse_kf_rows(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_units, uint64_t batch_bytes,
                                uint64_t nbins, uint64_t cap_rows, uint16_t* d_rows, uint64_t* d_unit_row0,
                                uint64_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (nbins == 0) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: nbins == 0");
    if (n_units < 0) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: negative unit count");
    if (batch_bytes >= (1ull << 32))
        return kf_fail(KF_EINVAL, "kf_parse_kf_rows: batch of %llu bytes: at most 4 GiB - 1 per call",
                       (unsigned long long)batch_bytes);
    if (!d_bytes) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: null d_bytes");
    if (!d_goff) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: null d_goff");
    if (!d_rows) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: null d_rows");
    if (!d_unit_row0) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: null d_unit_row0");
    if (!d_status) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: null d_status");
    if (!d_scratch) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: null d_scratch");
    if ((uintptr_t)d_bytes & 15) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: misaligned d_bytes (needs 16 bytes)");
    if ((uintptr_t)d_rows & 1) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: misaligned d_rows (needs 2 bytes)");
    if ((uintptr_t)d_goff & 7) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: misaligned d_goff (needs 8 bytes)");
    if ((uintptr_t)d_unit_row0 & 7)
        return kf_fail(KF_EINVAL, "kf_parse_kf_rows: misaligned d_unit_row0 (needs 8 bytes)");
    if ((uintptr_t)d_status & 7) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: misaligned d_status (needs 8 bytes)");
    if ((uintptr_t)d_scratch & 7) return kf_fail(KF_EINVAL, "kf_parse_kf_rows: misaligned d_scratch (needs 8 bytes)");
    const uint64_t need = kf_parse_kf_scratch_bytes(batch_bytes, n_units, cap_rows);
    if (scratch_bytes < need)
        return kf_fail(KF_ERANGE, "kf_parse_kf_rows: scratch needs %llu bytes, %llu given", (unsigned long long)need,
                       (unsigned long long)scratch_bytes);
    return parse_launch("kf_parse_kf_rows", d_bytes, d_goff, n_units, batch_bytes, nbins, cap_rows, U16Sink{d_rows},
                        d_unit_row0, d_status, d_scratch, (hipStream_t)stream);
}

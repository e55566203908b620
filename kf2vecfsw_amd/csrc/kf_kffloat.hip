// kf_kffloat.hip -- kf_parse_kf_floats: get_frequencies `.kf` text parsed in HBM.
//
// The trainers of the reference read a directory of get_frequencies `.kf` files
// (one long row of repr(float64) fields per genome) with pandas (my_read_csv,
// kf2vec/utils.py:436-437) and multiply by features_scaler.  Here the text of
// many files lies back to back on the device, as for kf_parse_kf_rows, and comes
// out as the float64 (or float32) feature rows, every value the correctly
// rounded binary64 of its decimal (kf_decimal.h) times the scaler, with every
// row's name span and every unit's row range.  The contract is in
// include/kf2vec_gpu.h; features.parse_kf_floats_host states it on the host.
//
// The passes (line starts, then a workgroup per row), the scratch layout and the
// error reporting are kf_kfrows.h's, shared with kf_kfparse.hip; this file states
// the field of a get_frequencies row and what becomes of its value.  The table
// of powers of five (10.2 KiB, kf_pow5_table) is copied to the head of the
// scratch on the call's stream before the launches, so the call keeps no state
// on any device (the source is pageable: the runtime stages the copy, and a
// stream under graph capture cannot take it; include/kf2vec_gpu.h says so).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_decimal.h"
#include "kf_floatfield.h"
#include "kf_kfrows.h"

namespace kf {
namespace {

typedef FloatFieldT<','> FloatField;       // kf_floatfield.h: ',' or '\n' ends a field

// kf_kfrows.h's Sink: field j of row r, converted and scaled, goes to vals[r * nbins + j]; the name's span is kept
struct FloatSink {
    typedef FloatField Field;
    static constexpr uint32_t kSep = ',';
    void* __restrict__ vals;
    uint32_t* __restrict__ row_name;
    const uint64_t* __restrict__ pow5;
    double scaler;
    int val_bytes;
    __device__ __forceinline__ Field fresh() const { return Field{0, 0, 0, 0, 0, 0}; }
    __device__ __forceinline__ void done(uint64_t r, uint64_t nbins, uint64_t col, const Field& f, bool store,
                                         uint64_t& err) const {
        uint64_t bits = kQuietNan;
        if (f.st != 8 && !decimal_to_double(f.w, (f.neg ? -f.ex : f.ex) - f.frac, pow5, &bits)) {
            note(err, col, kErrRange);
            return;
        }
        if (!store) return;
        const double v = __longlong_as_double((long long)bits) * scaler;
        if (val_bytes == 8) ((double*)vals)[r * nbins + col] = v;
        else ((float*)vals)[r * nbins + col] = (float)v;
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

extern "C" int kf_decimal_to_double(const uint64_t* w, const int32_t* q, uint64_t n, double* out, uint8_t* in_range) {
    if (n && (!w || !q || !out || !in_range)) return kf_fail(KF_EINVAL, "kf_decimal_to_double: null pointer");
    const uint64_t* table = kf_pow5_table();
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t bits = 0;
        in_range[i] = decimal_to_double(w[i], q[i], table, &bits) ? 1 : 0;
        memcpy(&out[i], &bits, 8);           // 0.0 where the product is out of range
    }
    return KF_OK;
}

extern "C" uint64_t kf_parse_kf_floats_scratch_bytes(uint64_t batch_bytes, int32_t n_units, uint64_t cap_rows) {
    (void)n_units;
    return kTableBytes + rows_scratch_bytes(batch_bytes, cap_rows);
}

extern "C" int kf_parse_kf_floats(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_units, uint64_t batch_bytes,
                                  uint64_t nbins, uint64_t cap_rows, double scaler, void* d_vals, int val_bytes,
                                  uint32_t* d_row_name, uint64_t* d_unit_row0, uint64_t* d_status, void* d_scratch,
                                  uint64_t scratch_bytes, void* stream) {
    if (nbins == 0) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: nbins == 0");
    if (n_units < 0) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: negative unit count");
    if (val_bytes != 4 && val_bytes != 8)
        return kf_fail(KF_EINVAL, "kf_parse_kf_floats: val_bytes %d: 8 (float64) or 4 (float32)", val_bytes);
    if (batch_bytes >= (1ull << 32))
        return kf_fail(KF_EINVAL, "kf_parse_kf_floats: batch of %llu bytes: at most 4 GiB - 1 per call",
                       (unsigned long long)batch_bytes);
    if (!d_bytes) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: null d_bytes");
    if (!d_goff) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: null d_goff");
    if (!d_vals) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: null d_vals");
    if (!d_row_name) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: null d_row_name");
    if (!d_unit_row0) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: null d_unit_row0");
    if (!d_status) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: null d_status");
    if (!d_scratch) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: null d_scratch");
    if ((uintptr_t)d_bytes & 15) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: misaligned d_bytes (needs 16 bytes)");
    if ((uintptr_t)d_vals & (uintptr_t)(val_bytes - 1))
        return kf_fail(KF_EINVAL, "kf_parse_kf_floats: misaligned d_vals (needs %d bytes)", val_bytes);
    if ((uintptr_t)d_row_name & 3)
        return kf_fail(KF_EINVAL, "kf_parse_kf_floats: misaligned d_row_name (needs 4 bytes)");
    if ((uintptr_t)d_goff & 7) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: misaligned d_goff (needs 8 bytes)");
    if ((uintptr_t)d_unit_row0 & 7)
        return kf_fail(KF_EINVAL, "kf_parse_kf_floats: misaligned d_unit_row0 (needs 8 bytes)");
    if ((uintptr_t)d_status & 7) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: misaligned d_status (needs 8 bytes)");
    if ((uintptr_t)d_scratch & 7) return kf_fail(KF_EINVAL, "kf_parse_kf_floats: misaligned d_scratch (needs 8 bytes)");
    const uint64_t need = kf_parse_kf_floats_scratch_bytes(batch_bytes, n_units, cap_rows);
    if (scratch_bytes < need)
        return kf_fail(KF_ERANGE, "kf_parse_kf_floats: scratch needs %llu bytes, %llu given", (unsigned long long)need,
                       (unsigned long long)scratch_bytes);
    hipStream_t s = (hipStream_t)stream;
    uint64_t* d_pow5 = (uint64_t*)d_scratch;
    if (n_units != 0 && batch_bytes != 0 &&
        hipMemcpyAsync(d_pow5, kf_pow5_table(), kTableBytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return kf_fail(KF_EHIP, "kf_parse_kf_floats: the copy of the powers of five failed");
    const FloatSink sink{d_vals, d_row_name, d_pow5, scaler, val_bytes};
    return parse_launch("kf_parse_kf_floats", d_bytes, d_goff, n_units, batch_bytes, nbins, cap_rows, sink, d_unit_row0,
                        d_status, (uint8_t*)d_scratch + kTableBytes, s);
}

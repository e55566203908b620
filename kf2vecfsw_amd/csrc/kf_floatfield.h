// kf_floatfield.h -- what the readers of decimal float text share (kf_kffloat.hip:
// get_frequencies `.kf` rows, ',' between fields; kf_tsvfloat.hip: distance
// matrices and embedding tables, '\t' between fields): the state of one field as
// kf_kfrows.h's row walk feeds it, byte by byte, and the table of powers of five
// that kf_decimal.h's conversion reads.
#pragma once
#include <stdint.h>

#include <mutex>

#include "kf_decimal.h"
#include "kf_kfrows.h"

namespace kf {

constexpr int32_t kMaxExp = 99999;           // the explicit exponent saturates here
constexpr int32_t kMaxFrac = 1 << 20;        // and the count of fraction digits here: either is out of range unless w == 0
constexpr int kMaxDigits = 19;               // 10^19 - 1 < 2^64: w is exact
constexpr uint64_t kQuietNan = 0x7FF8000000000000ull;
constexpr uint64_t kTableBytes = 8ull * kDecTableWords;

namespace {

// One field's state: digits [ '.' digits* ] [ e|E [+|-] digits ], or "nan"; Sep or '\n' ends it.
template <uint32_t Sep>
struct FloatFieldT {
    uint64_t w;      // the significant digits so far
    int32_t frac;    // digits after the '.', significant or not
    int32_t ex;      // the explicit exponent's magnitude
    int16_t nd;      // significant digits: those from the first that is not '0' on, trailing zeros included
    int8_t st;       // 0 nothing yet, 1 integer digits, 2 after '.', 3 after 'e', 4 after its sign, 5 exponent digits,
                     // 6 after "n", 7 after "na", 8 after "nan"
    int8_t neg;      // the exponent's sign
    // Feed the next byte: 0 go on, 1 the field ended well, else the error code.
    __device__ __forceinline__ int feed(uint32_t c) {
        const uint32_t d = c - '0';
        if (d < 10u) {
            if (st >= 3) {
                if (st > 5) return kErrForm;
                st = 5;
                ex = ex * 10 + (int32_t)d;
                ex = ex > kMaxExp ? kMaxExp : ex;
                return 0;
            }
            if (st == 0) st = 1;
            if (st == 2) frac = frac < kMaxFrac ? frac + 1 : kMaxFrac;
            if (w == 0 && d == 0) return 0;  // a leading zero
            if (nd == kMaxDigits) return kErrDigits;
            w = w * 10 + d;
            ++nd;
            return 0;
        }
        if (c == Sep || c == '\n') return st == 1 || st == 2 || st == 5 || st == 8 ? 1 : kErrForm;
        if (c == '.') {
            if (st != 1) return kErrForm;
            st = 2;
            return 0;
        }
        if ((c | 0x20u) == 'e') {
            if (st != 1 && st != 2) return kErrForm;
            st = 3;
            return 0;
        }
        if (c == '+' || c == '-') {
            if (st != 3) return kErrForm;
            st = 4;
            neg = c == '-';
            return 0;
        }
        if (c == 'n') {
            if (st != 0 && st != 7) return kErrForm;
            st = st == 0 ? 6 : 8;
            return 0;
        }
        if (c == 'a' && st == 6) {
            st = 7;
            return 0;
        }
        return kErrForm;
    }
    // the decimal exponent of w once the field has ended well
    __device__ __forceinline__ int32_t q() const { return (neg ? -ex : ex) - frac; }
};

}  // namespace

// The powers of five of kf_decimal.h, computed on first use, once per process.
inline const uint64_t* kf_pow5_table() {
    static uint64_t table[kDecTableWords];
    static std::once_flag once;
    std::call_once(once, [] { pow5_table_build(table); });
    return table;
}

}  // namespace kf

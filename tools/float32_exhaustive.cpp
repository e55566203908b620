// float32_exhaustive.cpp -- every one of the 2^32 float32 patterns through
// csrc/kf_shortest.h, in both float32 forms (the float32's own shortest digits,
// and the digits of the value widened to double), on the host.
//
//   hipcc -O2 -std=c++17 -pthread -I kf2vecfsw_amd/csrc tools/float32_exhaustive.cpp -o float32_exhaustive
//   ./float32_exhaustive [threads]        (one JSON line; exit status 1 if a pattern fails)
//
// For every finite pattern other than zero, with (w, q) the decimal behind the
// text (dec_of):
//   back     w * 10^q parses back to the same bits: by the project's own
//            conversion (decimal_to_double) for the widened form; for the
//            float32 form as the nearest float32 of the decimal, rounded once
//            (parses_to below)
//   shorter  no decimal of one digit less does: the multiples of 10^(q+1) from
//            two below w * 10^q to two above it are tried, which covers every
//            such decimal inside the value's rounding interval (w has no
//            trailing zero, so a shorter decimal is never w itself rescaled)
//   digits   at most 9 for the float32 form, at most 17 widened
// Zeros, infinities and NaNs are checked for their class and sign.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "kf_shortest.h"

using namespace kf;

static uint64_t* g_pow5;
static const uint64_t* g_pow10;

// the sign of w * 10^q - m * 2^e (m * 2^e: a double), exactly, by big integers
static int cmp_decimal_double(uint64_t w, int32_t q, uint64_t m, int32_t e) {
    using namespace dec_detail;
    Big l, r;
    big_set(&l, (uint32_t)w);
    l.v[1] = (uint32_t)(w >> 32);
    l.n = l.v[1] ? 2 : l.n;
    big_set(&r, (uint32_t)m);
    r.v[1] = (uint32_t)(m >> 32);
    r.n = r.v[1] ? 2 : r.n;
    for (int i = 0; i < q; ++i) big_mul_small(&l, 5);
    for (int i = 0; i < -q; ++i) big_mul_small(&r, 5);
    const int32_t low = q < e ? q : e;       // the powers of two, made non-negative on both sides
    for (int i = 0; i < q - low; ++i) big_mul_small(&l, 2);
    for (int i = 0; i < e - low; ++i) big_mul_small(&r, 2);
    if (big_ge(&l, &r, 64)) return big_ge(&r, &l, 64) ? 0 : 1;
    return -1;
}

// Whether w * 10^q, rounded once to the nearest float32 (a tie to even), is |bits|.
// The project's conversion gives the nearest double; rounding that once more is
// the same unless the double is exactly half way between two float32 (bits 0..28
// are 1 << 28), where the decimal's side of it decides: that case is settled
// exactly.  (The parsers round twice, as strtod followed by a cast does: of
// all float32 one pattern and its negative, 0x15ae43fd = 7.038531e-26, read back
// one unit off that way, and numpy's own text for it does the same.)
static bool parses_to(uint64_t w, int32_t q, int form, uint32_t bits) {
    uint64_t d = 0;
    if (!decimal_to_double(w, q, g_pow5, &d)) return false;
    double x;
    memcpy(&x, &d, 8);
    float want;
    const uint32_t a = bits & 0x7FFFFFFFu;
    memcpy(&want, &a, 4);
    if (form != kFormF32) return x == (double)want;
    const int32_t ex = (int32_t)(d >> 52);                         // x > 0 and normal
    if ((d & 0x1FFFFFFFull) == 0x10000000ull && ex > 896 && ex < 1151) {   // half way, in the float32 normal range
        const int c = cmp_decimal_double(w, q, (d & 0xFFFFFFFFFFFFFull) | 1ull << 52, ex - 1075);
        if (c != 0) {
            const uint64_t lo = d & ~0x1FFFFFFFull, hi = lo + 0x20000000ull;     // the two float32 around it
            const uint64_t pick = c < 0 ? lo : hi;
            double y;
            memcpy(&y, &pick, 8);
            return y == (double)want;
        }
    }
    const float f = (float)x;
    return memcmp(&f, &want, 4) == 0;
}

struct Tally {
    uint64_t finite = 0, back = 0, shorter = 0, digits = 0, special = 0;
    uint32_t first_bad = 0;
    bool any_bad = false;
};

static void run(uint64_t lo, uint64_t hi, Tally* t) {
    for (uint64_t b = lo; b < hi; ++b) {
        const uint32_t bits = (uint32_t)b;
        const uint32_t ex = (bits >> 23) & 0xFFu, m = bits & 0x7FFFFFu;
        for (int form = kFormF32; form <= kFormF32Wide; ++form) {
            const Dec d = dec_of(bits, form, g_pow10);
            bool bad = false;
            if (d.neg != (bits >> 31)) bad = true, ++t->special;
            if (ex == 0xFF || (ex == 0 && m == 0)) {
                const uint8_t cls = ex == 0xFF ? (m ? kClsNan : kClsInf) : kClsZero;
                if (d.cls != cls) bad = true, ++t->special;
            } else {
                ++t->finite;
                if (d.cls != kClsFinite) bad = true, ++t->special;
                if (d.w == 0 || d.w % 10 == 0 || d.nd != sh_ndigits(d.w) || d.nd > (form == kFormF32 ? 9 : 17))
                    bad = true, ++t->digits;
                if (!parses_to(d.w, d.q, form, bits)) bad = true, ++t->back;
                if (d.nd > 1) {
                    const uint64_t s = d.w / 10;
                    for (int k = -2; k <= 2; ++k) {
                        const uint64_t c = s + (uint64_t)(int64_t)k;
                        if ((int64_t)s + k <= 0) continue;
                        if (sh_ndigits(c) >= d.nd) continue;            // one digit less only
                        if (parses_to(c, d.q + 1, form, bits)) {
                            bad = true;
                            ++t->shorter;
                        }
                    }
                }
            }
            if (bad && !t->any_bad) {
                t->any_bad = true;
                t->first_bad = bits;
            }
        }
    }
}

int main(int argc, char** argv) {
    const int nt = argc > 1 ? atoi(argv[1]) : 16;
    static uint64_t pow5[kDecTableWords];
    pow5_table_build(pow5);
    g_pow5 = pow5;
    g_pow10 = kf_pow10_ceil_table();
    std::vector<Tally> tally((size_t)nt);
    std::vector<std::thread> th;
    const uint64_t total = 1ull << 32;
    for (int i = 0; i < nt; ++i)
        th.emplace_back(run, total * (uint64_t)i / (uint64_t)nt, total * (uint64_t)(i + 1) / (uint64_t)nt, &tally[(size_t)i]);
    for (auto& x : th) x.join();
    Tally s;
    for (const Tally& t : tally) {
        s.finite += t.finite;
        s.back += t.back;
        s.shorter += t.shorter;
        s.digits += t.digits;
        s.special += t.special;
        if (t.any_bad && !s.any_bad) {
            s.any_bad = true;
            s.first_bad = t.first_bad;
        }
    }
    printf("{\"patterns\": %llu, \"forms\": 2, \"finite_checks\": %llu, \"not_parsed_back\": %llu, "
           "\"shorter_also_parses_back\": %llu, \"bad_digits\": %llu, \"bad_class_or_sign\": %llu, \"first_bad_bits\": \"%s%08x\"}\n",
           (unsigned long long)total, (unsigned long long)s.finite, (unsigned long long)s.back,
           (unsigned long long)s.shorter, (unsigned long long)s.digits, (unsigned long long)s.special,
           s.any_bad ? "0x" : "none:", s.first_bad);
    return s.any_bad ? 1 : 0;
}

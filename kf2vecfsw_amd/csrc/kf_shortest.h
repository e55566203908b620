// kf_shortest.h -- binary32 / binary64 to the shortest decimal that reads back
// as the same value, and that decimal as text: the inverse of kf_decimal.h.
//
// dec_of(bits, form, table): sign, class and -- for finite values other than
// zero -- the significand w and exponent q of the shortest decimal w * 10^q that
// rounds to the value in its own format (at most 17 digits for binary64, 9 for
// binary32); of the shortest candidates the one closest to the value, a tie to
// the even digit.  These are the digits of Python's repr(float) and of numpy's
// str(np.float32).  The algorithm is Schubfach (Giulietti): the value
// and the two ends of its rounding interval are multiplied by one 128-bit power
// of ten, rounded up, from a table, and truncated with a sticky bit; the answer
// is found among the multiples of 10^k and of 10^(k+1) in the interval.  Every
// binary32 and every binary64, subnormals included, goes through the same code:
// a binary32 is the same product with a 24-bit significand.
//
// The three forms (kf2vec_gpu.h: KF_FLOAT_SHORTEST for either width,
// KF_FLOAT_WIDENED) differ in the digits and in where the notation switches:
//   kFormF64       the digits of the binary64; fixed notation iff the decimal
//                  point falls in -3 .. 16 (repr: 0.0001 .. 9999999999999998.0)
//   kFormF32       the digits of the binary32; fixed iff 1e-4 <= |v| < 1e16 as
//                  real numbers (numpy compares the value: float32(1e-4) lies
//                  below 1e-4 and prints "1e-04", repr of its double 9.999...e-05)
//   kFormF32Wide   the binary32 converted to binary64 (exact), then kFormF64
//
// dec_len / dec_put: the text, at most kFloatTextMax = 24 bytes --
//   fixed       ddd.ddd, 0.000ddd, ddd000.0; integral values end in ".0"
//   otherwise   d[.ddd]e+XX / e-XX, at least two exponent digits
//   -0.0, inf, -inf; NaN "nan" (never signed) or nothing at all (nan_empty)
// dec_put writes through a sink (put(i, byte)), so the device writes straight
// into its LDS stage and the host into a slot.
//
// The table: entry e (kShMinK <= e <= kShMaxK) is ceil(10^e / 2^(floor(log2 10^e) - 127)),
// two uint64, high word first -- the 128-bit power of ten ROUNDED UP, which is
// what Schubfach's proof asks for; kf_pow5_table's entries are truncated (and
// stop at 308), so this is a second table, built the same way: schoolbook
// big-integer arithmetic of kf_decimal.h on the host, once per process
// (kf_pow10_ceil_table); nothing is generated or stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "kf_decimal.h"

namespace kf {

constexpr int kShMinK = -292;                // binary64: q in [-1074, 971], so -k in [-292, 324]
constexpr int kShMaxK = 324;
constexpr int kShTableWords = 2 * (kShMaxK - kShMinK + 1);   // 1,234 uint64: 9.6 KiB
constexpr uint64_t kShTableBytes = 8ull * kShTableWords;
constexpr uint32_t kFloatTextMax = 24;       // "-1.2345678901234567e-308"

constexpr int kFormF64 = 0, kFormF32 = 1, kFormF32Wide = 2;
constexpr uint8_t kClsFinite = 0, kClsZero = 1, kClsInf = 2, kClsNan = 3;

struct Dec {
    uint64_t w;      // significand without trailing zeros (finite, non-zero values)
    int32_t q;       // its decimal exponent
    uint8_t nd;      // decimal digits of w
    uint8_t neg;     // the sign bit (of a NaN too; its text never shows it)
    uint8_t cls;
    uint8_t fixed;   // fixed notation
};

// ---- Schubfach
// floor(g * cp / 2^128) with every bit below gathered into the last one
__host__ __device__ inline uint64_t sh_round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
    uint64_t xhi, xlo, yhi, ylo;
    mul_64x64(cp, glo, &xhi, &xlo);
    mul_64x64(cp, ghi, &yhi, &ylo);
    ylo += xhi;
    yhi += ylo < xhi ? 1u : 0u;
    return yhi | (ylo > 1 ? 1u : 0u);
}

__host__ __device__ inline uint32_t sh_ndigits(uint64_t w) {
    uint32_t n = 1;
    while (w >= 10) {
        w /= 10;
        ++n;
    }
    return n;
}

// The shortest decimal of c * 2^q; lower_closer: c is a power of two with a
// smaller binade below it, whose spacing is half as wide.
__host__ __device__ inline void sh_shortest(uint64_t c, int32_t q, bool lower_closer, const uint64_t* table,
                                            uint64_t* w_out, int32_t* q_out) {
    const bool even = (c & 1) == 0;
    const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1 : 0);
    const uint64_t cb = 4 * c;
    const uint64_t cbr = 4 * c + 2;
    // k = floor(log10(2^q)), or floor(log10(3/4 * 2^q)); h = q + floor(log2(10^-k)) + 1 in 1..4
    const int32_t k = lower_closer ? (q * 1262611 - 524031) >> 22 : (q * 1262611) >> 22;
    const int32_t h = q + ((-k * 1741647) >> 19) + 1;
    const uint64_t* g = table + 2 * (-k - kShMinK);
    const uint64_t vbl = sh_round_to_odd(g[0], g[1], cbl << h);
    const uint64_t vb = sh_round_to_odd(g[0], g[1], cb << h);
    const uint64_t vbr = sh_round_to_odd(g[0], g[1], cbr << h);
    const uint64_t lower = vbl + (even ? 0 : 1);
    const uint64_t upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb / 4;
    uint64_t w = 0;
    int32_t e = k;
    bool done = false;
    if (s >= 10) {                           // a multiple of 10^(k+1) inside the interval is shorter
        const uint64_t sp = s / 10;
        const bool up_in = lower <= 40 * sp;
        const bool wp_in = 40 * sp + 40 <= upper;
        if (up_in != wp_in) {
            w = sp + (wp_in ? 1 : 0);
            e = k + 1;
            done = true;
        }
    }
    if (!done) {
        const bool u_in = lower <= 4 * s;
        const bool w_in = 4 * s + 4 <= upper;
        if (u_in != w_in) {
            w = s + (w_in ? 1 : 0);
        } else {                             // both or neither: the closer one, a tie to the even one
            const uint64_t mid = 4 * s + 2;
            const bool up = vb > mid || (vb == mid && (s & 1));
            w = s + (up ? 1 : 0);
        }
    }
    while (w % 10 == 0) {                    // w != 0
        w /= 10;
        ++e;
    }
    *w_out = w;
    *q_out = e;
}

// bits: a binary64, or a binary32 in the low word (kFormF32, kFormF32Wide)
__host__ __device__ inline Dec dec_of(uint64_t bits, int form, const uint64_t* table) {
    Dec d;
    d.w = 0;
    d.q = 0;
    d.nd = 1;
    d.fixed = 1;
    bool by_value = false;
    if (form == kFormF32Wide) {              // to binary64, exactly
        const uint32_t b = (uint32_t)bits;
        const uint32_t ex = (b >> 23) & 0xFFu, m = b & 0x7FFFFFu;
        uint64_t o = (uint64_t)(b >> 31) << 63;
        if (ex == 0xFF) {
            o |= 0x7FF0000000000000ull | (uint64_t)m << 29;
        } else if (ex) {
            o |= (uint64_t)(ex + 896) << 52 | (uint64_t)m << 29;
        } else if (m) {                      // a binary32 subnormal is a normal binary64
            const int lz = __builtin_clz(m) - 8;          // shifts that bring bit 23 up
            o |= (uint64_t)(897 - lz) << 52 | ((uint64_t)(m << lz) & 0x7FFFFFull) << 29;
        }
        bits = o;
        form = kFormF64;
    }
    uint64_t c;
    int32_t q;
    bool lower_closer;
    if (form == kFormF64) {
        const uint32_t ex = (uint32_t)(bits >> 52) & 0x7FFu;
        const uint64_t m = bits & 0xFFFFFFFFFFFFFull;
        d.neg = (uint8_t)(bits >> 63);
        if (ex == 0x7FF) {
            d.cls = m ? kClsNan : kClsInf;
            return d;
        }
        if (ex == 0 && m == 0) {
            d.cls = kClsZero;
            return d;
        }
        c = ex ? m | 1ull << 52 : m;
        q = (ex ? (int32_t)ex : 1) - 1075;
        lower_closer = m == 0 && ex > 1;
    } else {
        const uint32_t b = (uint32_t)bits;
        const uint32_t ex = (b >> 23) & 0xFFu, m = b & 0x7FFFFFu;
        d.neg = (uint8_t)(b >> 31);
        if (ex == 0xFF) {
            d.cls = m ? kClsNan : kClsInf;
            return d;
        }
        if (ex == 0 && m == 0) {
            d.cls = kClsZero;
            return d;
        }
        c = ex ? m | 1u << 23 : m;
        q = (ex ? (int32_t)ex : 1) - 150;
        lower_closer = m == 0 && ex > 1;
        // 0x38D1B718 is the least binary32 >= 1e-4, 0x5A0E1BCA the least >= 1e16
        const uint32_t a = b & 0x7FFFFFFFu;
        d.fixed = a >= 0x38D1B718u && a < 0x5A0E1BCAu;
        by_value = true;
    }
    d.cls = kClsFinite;
    sh_shortest(c, q, lower_closer, table, &d.w, &d.q);
    d.nd = (uint8_t)sh_ndigits(d.w);
    if (!by_value) {
        const int32_t pt = (int32_t)d.nd + d.q;          // digits in front of the decimal point
        d.fixed = pt >= -3 && pt <= 16;
    }
    return d;
}

// ---- the text
__host__ __device__ inline uint32_t dec_len(const Dec& d, bool nan_empty) {
    if (d.cls == kClsNan) return nan_empty ? 0u : 3u;
    if (d.cls == kClsInf) return 3u + d.neg;
    if (d.cls == kClsZero) return 3u + d.neg;
    const int32_t nd = d.nd, pt = nd + d.q;
    if (d.fixed) {
        if (pt <= 0) return (uint32_t)(d.neg + 2 - pt + nd);           // 0.000ddd
        if (pt >= nd) return (uint32_t)(d.neg + pt + 2);               // ddd000.0
        return (uint32_t)(d.neg + nd + 1);                             // dd.ddd
    }
    const int32_t e = pt - 1, ae = e < 0 ? -e : e;
    return (uint32_t)(d.neg + nd + (nd > 1 ? 1 : 0) + 2 + (ae >= 100 ? 3 : 2));
}

// dec_len(d) bytes through sink.put(i, byte), i from 0
template <class Sink>
__host__ __device__ inline void dec_put(const Dec& d, bool nan_empty, Sink& sink) {
    uint32_t at = 0;
    if (d.cls == kClsNan) {
        if (!nan_empty) {
            sink.put(0, 'n');
            sink.put(1, 'a');
            sink.put(2, 'n');
        }
        return;
    }
    if (d.neg) sink.put(at++, '-');
    if (d.cls == kClsInf) {
        sink.put(at, 'i');
        sink.put(at + 1, 'n');
        sink.put(at + 2, 'f');
        return;
    }
    if (d.cls == kClsZero) {
        sink.put(at, '0');
        sink.put(at + 1, '.');
        sink.put(at + 2, '0');
        return;
    }
    const int32_t nd = d.nd, pt = nd + d.q;
    uint64_t w = d.w;
    if (d.fixed) {
        if (pt <= 0) {
            sink.put(at, '0');
            sink.put(at + 1, '.');
            for (int32_t i = 0; i < -pt; ++i) sink.put(at + 2 + i, '0');
            at += 2 - pt;
            for (int32_t i = nd - 1; i >= 0; --i) {
                sink.put(at + i, '0' + (uint32_t)(w % 10));
                w /= 10;
            }
        } else if (pt >= nd) {
            for (int32_t i = nd - 1; i >= 0; --i) {
                sink.put(at + i, '0' + (uint32_t)(w % 10));
                w /= 10;
            }
            for (int32_t i = nd; i < pt; ++i) sink.put(at + i, '0');
            sink.put(at + pt, '.');
            sink.put(at + pt + 1, '0');
        } else {
            for (int32_t i = nd - 1; i >= 0; --i) {
                sink.put(at + i + (i >= pt ? 1 : 0), '0' + (uint32_t)(w % 10));
                w /= 10;
            }
            sink.put(at + pt, '.');
        }
        return;
    }
    for (int32_t i = nd - 1; i >= 1; --i) {
        sink.put(at + 1 + i, '0' + (uint32_t)(w % 10));
        w /= 10;
    }
    sink.put(at, '0' + (uint32_t)w);
    if (nd > 1) sink.put(at + 1, '.');
    at += nd + (nd > 1 ? 1 : 0);
    const int32_t e = pt - 1;
    uint32_t ae = (uint32_t)(e < 0 ? -e : e);
    sink.put(at, 'e');
    sink.put(at + 1, e < 0 ? '-' : '+');
    at += 2;
    if (ae >= 100) {
        sink.put(at++, '0' + ae / 100);
        ae %= 100;
    }
    sink.put(at, '0' + ae / 10);
    sink.put(at + 1, '0' + ae % 10);
}

// ---- the table, on the host
// table[2 * (e - kShMinK)], [+ 1]: ceil(10^e * 2^-(floor(log2 10^e) - 127)), high word first
inline void pow10_ceil_table_build(uint64_t* table) {
    using namespace dec_detail;
    Big p;
    big_set(&p, 1);
    for (int e = 0; e <= kShMaxK; ++e) {     // 5^e: its top 128 bits, plus one if a bit below them is set
        uint64_t* t = table + 2 * (e - kShMinK);
        Big x = p;
        int top = big_bits(&p);
        for (; top < 128; ++top) big_shl1(&x, 4, 0);
        big_window(&x, top, &t[0], &t[1]);
        bool below = false;
        for (int i = 0; i < top - 128; ++i) below |= big_bit(&x, i) != 0;
        if (below && ++t[1] == 0) ++t[0];
        big_mul_small(&p, 5);
    }
    big_set(&p, 1);
    for (int n = 1; n <= -kShMinK; ++n) {    // e = -n: floor(2^b / 5^n) + 1 (never exact), 128 bits
        big_mul_small(&p, 5);
        const int z = big_bits(&p);          // 2^(z-1) < 5^n < 2^z
        const int b = z + 127;
        const int nl = p.n + 1;              // the remainder stays below 2 * 5^n
        Big r, quo;
        big_set(&r, 0);
        big_set(&quo, 0);
        for (int i = b; i >= 0; --i) {
            big_shl1(&r, nl, i == b ? 1u : 0u);
            if (big_ge(&r, &p, nl)) {
                big_sub(&r, &p, nl);
                quo.v[i >> 5] |= 1u << (i & 31);
            }
        }
        uint64_t* t = table + 2 * (-n - kShMinK);
        t[0] = (uint64_t)quo.v[3] << 32 | quo.v[2];
        t[1] = (uint64_t)quo.v[1] << 32 | quo.v[0];
        if (++t[1] == 0) ++t[0];
    }
}

// The rounded-up powers of ten, computed on first use, once per process.
inline const uint64_t* kf_pow10_ceil_table() {
    static uint64_t table[kShTableWords];
    static std::once_flag once;
    std::call_once(once, [] { pow10_ceil_table_build(table); });
    return table;
}

}  // namespace kf

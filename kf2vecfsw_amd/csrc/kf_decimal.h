// kf_decimal.h -- decimal to binary64, correctly rounded: the value of a `.kf`
// float field once its digits are a significand w and an exponent q.
//
// decimal_to_double(w, q, table, &bits): the bit pattern of the binary64 nearest
// to w * 10^q under round-half-to-even (what Python's float() and strtod return)
// for ANY uint64 w, by the Eisel-Lemire scheme: w is shifted until
// its top bit is set and multiplied by a 128-bit truncated power of five from a
// table; the top bits of the product are the significand, the bits below them
// the rounding decision.  Mushtak & Lemire (2023) prove that the second word of
// the power is needed only when the low 9 bits of the first product's high word
// are all ones and that no case is left undecided after it, so there is no
// fallback to a slower algorithm.  The same inline code is compiled for the
// device (the kernels of kf_kffloat.hip and kf_tsvfloat.hip) and for the host (kf_decimal_to_double
// in the same file, which the CPU tests call).
//
// Contract:
//   w == 0                       0.0, in range, whatever q is
//   q outside [kDecMinQ, kDecMaxQ] = [-342, 308]   not in range (with w != 0 such
//                                a product is below 2^-1022 or above DBL_MAX)
//   w * 10^q < 2^-1022           not in range: subnormals are not produced, and a
//                                decimal just below 2^-1022 is not rounded up to it
//   the rounded result > DBL_MAX not in range: a decimal that rounds to DBL_MAX is
//                                in range, one that would round to infinity is not
//   else                         in range, *bits is the correctly rounded value
// "Not in range" is reported (the function returns false and leaves *bits); no
// writer of `.kf` files produces such a number.
//
// The table: entry q is two uint64 (high word first).  q >= 0: the top 128 bits
// of 5^q, truncated.  q < 0: a 128-bit reciprocal of 5^-q, 2^b / 5^-q with b
// such that the top bit is set -- plus one in the last place for q >= -27 (where
// 5^-q fits 64 bits and an exact quotient must be seen as exact), truncated
// below that.  pow5_table_build computes it with schoolbook big-integer
// arithmetic on the host, 13 ms once per process (kf_pow5_table in kf_floatfield.h);
// nothing is generated or stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace kf {

constexpr int kDecMinQ = -342;
constexpr int kDecMaxQ = 308;
constexpr int kDecTableWords = 2 * (kDecMaxQ - kDecMinQ + 1);   // 1,302 uint64: 10.2 KiB

// a * b as two words (on gfx950 the 128-bit product lowers to v_mad_u64_u32 on the 32-bit halves)
__host__ __device__ inline void mul_64x64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
    const unsigned __int128 p = (unsigned __int128)a * b;
    *lo = (uint64_t)p;
    *hi = (uint64_t)(p >> 64);
}

__host__ __device__ inline bool decimal_to_double(uint64_t w, int32_t q, const uint64_t* table, uint64_t* bits) {
    if (w == 0) {
        *bits = 0;
        return true;
    }
    if (q < kDecMinQ || q > kDecMaxQ) return false;
    const int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t* t = table + 2 * (q - kDecMinQ);
    uint64_t hi, lo;
    mul_64x64(w, t[0], &hi, &lo);
    if ((hi & 0x1FFu) == 0x1FFu) {           // the 55 bits that decide are not settled by the first word
        uint64_t hi2, lo2;
        mul_64x64(w, t[1], &hi2, &lo2);
        lo += hi2;
        if (hi2 > lo) ++hi;
    }
    const int upper = (int)(hi >> 63);
    const int shift = upper + 64 - 52 - 3;   // 53 bits and a round bit stay
    uint64_t m = hi >> shift;
    // floor(q * log2(10)) + 63: the binary exponent of 10^q's 64-bit normalised form
    int32_t p2 = (int32_t)(((152170 + 65536) * q) >> 16) + 63 + upper - lz + 1023;
    if (p2 <= 0) return false;               // below 2^-1022
    // an exact tie (possible only where 5^q or 5^-q divides out: -4 <= q <= 23) goes to the even neighbour
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) m &= ~1ull;
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) {                 // rounded up to the next power of two
        m = 1ull << 52;
        ++p2;
    }
    if (p2 >= 0x7FF) return false;           // above DBL_MAX
    *bits = (m & ~(1ull << 52)) | (uint64_t)p2 << 52;
    return true;
}

// ---- the table, on the host
namespace dec_detail {

// unsigned big integers of up to 64 x 32 bits, least significant limb first
struct Big {
    uint32_t v[64];
    int n;                                   // limbs in use (v[n - 1] != 0, or n == 0)
};
inline void big_set(Big* a, uint32_t x) {
    memset(a->v, 0, sizeof a->v);
    a->v[0] = x;
    a->n = x ? 1 : 0;
}
inline void big_mul_small(Big* a, uint32_t m) {
    uint64_t c = 0;
    for (int i = 0; i < a->n; ++i) {
        c += (uint64_t)a->v[i] * m;
        a->v[i] = (uint32_t)c;
        c >>= 32;
    }
    if (c) a->v[a->n++] = (uint32_t)c;
}
inline int big_bits(const Big* a) { return a->n ? 32 * a->n - __builtin_clz(a->v[a->n - 1]) : 0; }
inline int big_bit(const Big* a, int i) { return i < 0 || i >= 32 * 64 ? 0 : (a->v[i >> 5] >> (i & 31)) & 1; }
// bits [top - 128, top) of a (zeros below bit 0), as two words
inline void big_window(const Big* a, int top, uint64_t* hi, uint64_t* lo) {
    uint64_t w[2] = {0, 0};
    for (int i = 0; i < 128; ++i) w[i >> 6] = w[i >> 6] << 1 | (uint64_t)big_bit(a, top - 1 - i);
    *hi = w[0];
    *lo = w[1];
}
// a = 2a + bit over nl limbs
inline void big_shl1(Big* a, int nl, uint32_t bit) {
    for (int i = 0; i < nl; ++i) {
        const uint32_t out = a->v[i] >> 31;
        a->v[i] = a->v[i] << 1 | bit;
        bit = out;
    }
}
inline bool big_ge(const Big* a, const Big* b, int nl) {
    for (int i = nl - 1; i >= 0; --i)
        if (a->v[i] != b->v[i]) return a->v[i] > b->v[i];
    return true;
}
inline void big_sub(Big* a, const Big* b, int nl) {
    uint64_t borrow = 0;
    for (int i = 0; i < nl; ++i) {
        const uint64_t d = (uint64_t)a->v[i] - b->v[i] - borrow;
        a->v[i] = (uint32_t)d;
        borrow = (d >> 32) & 1;
    }
}

}  // namespace dec_detail

// table[2 * (q - kDecMinQ)], [+ 1]: the 128-bit power of five of q, high word first
inline void pow5_table_build(uint64_t* table) {
    using namespace dec_detail;
    Big p;
    big_set(&p, 1);
    for (int q = 0; q <= kDecMaxQ; ++q) {    // 5^q, its top 128 bits (shifted up if it has fewer)
        uint64_t* t = table + 2 * (q - kDecMinQ);
        Big x = p;
        int top = big_bits(&p);
        for (; top < 128; ++top) big_shl1(&x, 4, 0);
        big_window(&x, top, &t[0], &t[1]);
        big_mul_small(&p, 5);
    }
    big_set(&p, 1);
    for (int n = 1; n <= -kDecMinQ; ++n) {   // q = -n: floor(2^b / 5^n) by binary long division
        big_mul_small(&p, 5);
        const int z = big_bits(&p);          // 2^(z-1) < 5^n < 2^z
        const int b = n <= 27 ? z + 127 : 2 * z + 128;
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
        for (int i = 0; i < 64; ++i)         // + 1
            if (++quo.v[i]) break;
        quo.n = 64;
        while (quo.n && !quo.v[quo.n - 1]) --quo.n;
        uint64_t* t = table + 2 * (-n - kDecMinQ);
        big_window(&quo, big_bits(&quo), &t[0], &t[1]);   // truncated to 128 bits (n <= 27: it has 128)
    }
}
}  // namespace kf

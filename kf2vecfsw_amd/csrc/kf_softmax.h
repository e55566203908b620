// kf_softmax.h -- the row softmax that kf_class_probs (kf_classprobs.hip) and kf_class_loss
// (kf_classloss.hip) share, so that both give a probability the same bits.
//
// For a row x[0..C) of logits (float32), every operation rounded to float32:
//   m = max_j x_j;  t_j = x_j - m;  e_j = expf(t_j);  s = sum_j e_j;  p_j = e_j / s
// with a correctly rounded division.  A wave owns a row.  Lane l takes the columns l,
// l + 64, l + 128, ...; with NT > 0 the row stays in NT registers per lane (C <= 64 * NT),
// with NT == 0 it is read three times (max; sum; divide).  The sum is a fixed function of C
// alone: a lane adds its own columns in ascending order, then the 64 partial sums meet in
// an xor butterfly (32, 16, 8, 4, 2, 1), in which both lanes of a pair add the same two
// numbers, so every lane ends with the same bits.
//
// A row that holds a NaN or +inf, or is all -inf, is refused: the maximum is taken with
// fmaxf, which drops NaN, so the test is made on the values themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// as in kf_sqdist.hip: no product and sum of the including file may become an fma
#pragma clang fp contract(off)

namespace kf {
namespace softmax {

constexpr int kWave = 64;
constexpr int kRegTiles = 16;                   // values per lane at most while the row stays in registers
constexpr int kRegCols = kWave * kRegTiles;     // 1024

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ int wave_any(int v) { return __any(v); }

// the largest value and, among equals, the lowest index
__device__ __forceinline__ void wave_best(float& v, uint32_t& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, kWave);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, o, kWave);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ __forceinline__ bool refused(float x) { return x != x || x == INFINITY; }

// The row x[0..C) of the calling wave: m and s to every lane, and each(j, p_j) for this
// lane's columns in ascending order.  Returns false, with nothing handed to `each`, for a
// refused row; the answer is the same in every lane.
template <int NT, class Each>
__device__ __forceinline__ bool row(const float* __restrict__ x, uint32_t C, uint32_t lane, float& m, float& s,
                                    Each&& each) {
    m = -INFINITY;
    s = 0.0f;
    int bad = 0;
    if constexpr (NT > 0) {
        float v[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const uint32_t j = lane + (uint32_t)i * kWave;
            v[i] = j < C ? x[j] : -INFINITY;
            bad |= refused(v[i]);
            m = fmaxf(m, v[i]);
        }
        m = wave_max(m);
        if (wave_any(bad) || m == -INFINITY) return false;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const uint32_t j = lane + (uint32_t)i * kWave;
            if (j < C) {
                const float t = v[i] - m;
                v[i] = expf(t);
                s = s + v[i];
            }
        }
        s = wave_sum(s);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const uint32_t j = lane + (uint32_t)i * kWave;
            if (j < C) each(j, __fdiv_rn(v[i], s));
        }
    } else {
        for (uint32_t j = lane; j < C; j += kWave) {
            const float xv = x[j];
            bad |= refused(xv);
            m = fmaxf(m, xv);
        }
        m = wave_max(m);
        if (wave_any(bad) || m == -INFINITY) return false;
        for (uint32_t j = lane; j < C; j += kWave) {
            const float t = x[j] - m;
            s = s + expf(t);
        }
        s = wave_sum(s);
        for (uint32_t j = lane; j < C; j += kWave) {
            const float t = x[j] - m;
            each(j, __fdiv_rn(expf(t), s));
        }
    }
    return true;
}

}  // namespace softmax
}  // namespace kf

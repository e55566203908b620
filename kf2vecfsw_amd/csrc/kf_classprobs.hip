// kf_classprobs.hip -- kf_class_probs: the classifier head's softmax, its first-index
// argmax and the row that classes.out prints, in one launch.
//
// For a row x[0..C) of logits (float32), every operation rounded to float32:
//   m = max_j x_j;  t_j = x_j - m;  e_j = expf(t_j);  s = sum_j e_j;  p_j = e_j / s
// with a correctly rounded division.  This is the reference's
// torch.exp(F.log_softmax(fc3(...), dim=1)) (kf2vec/models.py:126-132,
// classify.py:117) in the direct form: it never passes through
// exp(x - m - log s), which loses |t| units of float32 in small probabilities.
// out[r, 1 + j] = p_j; top[r] = the lowest j whose rounded p_j is the row's
// largest (what topk(1) gives for tied values on the CPU); out[r, 0] = p[top[r]].
// classify.class_probs_host states it in numpy.
//
// A wave owns a row.  Lane l takes the columns l, l + 64, l + 128, ...; up to
// kRegCols columns the row stays in registers (1, 4 or 16 values per lane, the
// smallest that holds C), above that it is read three times (max; sum; divide).
// The sum is a fixed function of C alone: a lane adds its own columns in
// ascending order, then the 64 partial sums meet in an xor butterfly (32, 16, 8,
// 4, 2, 1), in which both lanes of a pair add the same two numbers, so every
// lane ends with the same bits.  Nothing in it depends on Q, on the row's place
// or on the workgroup, so a caller may cut Q into calls as it likes.
//
// A row that holds a NaN or +inf, or is all -inf, is NaN in all C + 1 outputs
// with top = 0: IEEE evaluation of the lines above (inf - inf, NaN sums), said
// here because the maximum is taken with fmaxf, which drops NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kf_internal.h"
#include "kf_softmax.h"                          // the row softmax, shared with kf_classloss.hip

// as in kf_sqdist.hip: no product and sum of this file may become an fma
#pragma clang fp contract(off)

namespace kf {
namespace {

using softmax::wave_best;

constexpr int kPWave = softmax::kWave;
constexpr int kPRows = 4;                       // rows (waves) per workgroup
constexpr int kPBlock = kPWave * kPRows;
constexpr int kPRegTiles = softmax::kRegTiles;  // values per lane at most while the row stays in registers
constexpr int kRegCols = softmax::kRegCols;     // 1024

__device__ __forceinline__ void nan_row(float* __restrict__ o, int32_t* __restrict__ top, uint64_t r, uint32_t C,
                                        uint32_t lane) {
    const float qnan = __int_as_float(0x7fc00000);
    for (uint64_t j = lane; j < (uint64_t)C + 1; j += kPWave) o[j] = qnan;
    if (lane == 0) top[r] = 0;
}

// NT > 0: the row in NT registers per lane (C <= 64 * NT).  NT == 0: the row read three times.
template <int NT>
__global__ void __launch_bounds__(kPBlock) class_probs_kernel(const float* __restrict__ logits, uint64_t Q, uint32_t C,
                                                              float* __restrict__ out, int32_t* __restrict__ top) {
    const uint32_t lane = threadIdx.x % kPWave;
    const uint64_t r = (uint64_t)blockIdx.x * kPRows + threadIdx.x / kPWave;
    if (r >= Q) return;                          // a whole wave leaves: nothing below waits for another wave
    const float* __restrict__ x = logits + r * C;
    float* __restrict__ o = out + r * ((uint64_t)C + 1);
    float m, s;
    float best = -1.0f;                          // below every probability
    uint32_t besti = 0xffffffffu;
    const bool ok = softmax::row<NT>(x, C, lane, m, s, [&](uint32_t j, float p) {
        o[1 + (uint64_t)j] = p;
        if (p > best) {                          // ascending j: the first of equals stays
            best = p;
            besti = j;
        }
    });
    if (!ok) {
        nan_row(o, top, r, C, lane);
        return;
    }
    wave_best(best, besti);
    if (lane == 0) {
        o[0] = best;
        top[r] = (int32_t)besti;
    }
}

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_class_probs_reg_cols(void) { return kRegCols; }

extern "C" int kf_class_probs_rows(void) { return kPRows; }

extern "C" int kf_class_probs(const float* d_logits, uint64_t Q, uint64_t C, float* d_out, int32_t* d_top,
                              void* stream) {
    if (C == 0) return kf_fail(KF_EINVAL, "kf_class_probs: C == 0");
    if (C >= (1ull << 31))
        return kf_fail(KF_EINVAL, "kf_class_probs: C = %llu: 2^31 columns or more", (unsigned long long)C);
    const uint64_t blocks = Q / kPRows + (Q % kPRows != 0);
    if (blocks >= (1ull << 24))                  // a launch has fewer than 2^32 threads
        return kf_fail(KF_EINVAL, "kf_class_probs: Q = %llu: fewer than 2^24 workgroups of %d rows per call",
                       (unsigned long long)Q, kPRows);
    if (Q && !d_logits) return kf_fail(KF_EINVAL, "kf_class_probs: null d_logits");
    if (Q && !d_out) return kf_fail(KF_EINVAL, "kf_class_probs: null d_out");
    if (Q && !d_top) return kf_fail(KF_EINVAL, "kf_class_probs: null d_top");
    if ((uintptr_t)d_logits & 3) return kf_fail(KF_EINVAL, "kf_class_probs: misaligned d_logits (needs 4 bytes)");
    if ((uintptr_t)d_out & 3) return kf_fail(KF_EINVAL, "kf_class_probs: misaligned d_out (needs 4 bytes)");
    if ((uintptr_t)d_top & 3) return kf_fail(KF_EINVAL, "kf_class_probs: misaligned d_top (needs 4 bytes)");
    if (Q == 0) return KF_OK;
    const dim3 grid((uint32_t)blocks), block(kPBlock);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t c = (uint32_t)C;
    if (C <= 1 * kPWave)
        hipLaunchKernelGGL(class_probs_kernel<1>, grid, block, 0, s, d_logits, Q, c, d_out, d_top);
    else if (C <= 4 * kPWave)
        hipLaunchKernelGGL(class_probs_kernel<4>, grid, block, 0, s, d_logits, Q, c, d_out, d_top);
    else if (C <= (uint64_t)kRegCols)
        hipLaunchKernelGGL(class_probs_kernel<kPRegTiles>, grid, block, 0, s, d_logits, Q, c, d_out, d_top);
    else
        hipLaunchKernelGGL(class_probs_kernel<0>, grid, block, 0, s, d_logits, Q, c, d_out, d_top);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_class_probs: launch failed");
    return KF_OK;
}

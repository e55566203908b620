// kf_classloss.hip -- kf_class_loss: the classifier trainer's loss of a batch, its gradient
// with respect to the logits, the batch's count of right classes and the epoch's running
// totals, in one call.
//
// For a row x[0..C) of logits (float32) with the true class c, every operation rounded to
// float32 and none contracted into an fma (kf_softmax.h has the first line, which is
// kf_class_probs' to the bit):
//   m = max_j x_j;  t_j = x_j - m;  e_j = expf(t_j);  s = sum_j e_j;  p_j = e_j / s
//   nll = logf(s) - t_c
//   hit = (the first index of the largest p_j) == c
//   g_j = (p_j - (j == c ? 1 : 0)) * invB,   invB = 1.0f / (float)B
// and per call, in float64,
//   loss = (sum_i (double)nll_i) * (1.0 / (double)B)     the sum from 0.0, i ascending, by one thread
//   hits = sum_i hit_i;  status = 1 if a class is outside [0, C)
// This is F.log_softmax, nn.NLLLoss() (mean), autograd's backward of both down to the logits,
// and exp / topk(1) / accuracy_score of the reference's step
// (kf2vec/train_classifier_model.py:323-342) in the direct form;
// train_classifier.class_loss_host states it in numpy.
//
// A wave owns a row, in the register tiers of kf_class_probs.  Up to kCSmallB rows one
// workgroup does it all: its 16 waves walk the rows, nll and hit meet in LDS, thread 0
// finishes.  Above, the row kernel (4 rows per workgroup) leaves nll and hit in the caller's
// scratch and a second launch of one workgroup finishes.  No atomics, no counters, no memset.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kf_internal.h"
#include "kf_softmax.h"

// no product and sum of this file may become an fma, in float32 or float64
#pragma clang fp contract(off)

namespace kf {
namespace {

constexpr int kCWave = softmax::kWave;
constexpr int kCSmallB = 64;                   // rows up to which one workgroup does it all
constexpr int kCSmallWaves = 16;
constexpr int kCSmallBlock = kCWave * kCSmallWaves;
constexpr int kCRows = 4;                      // rows (waves) per workgroup of the row kernel
constexpr int kCBlock = kCWave * kCRows;
constexpr uint64_t kCMaxB = 1ull << 16;        // rows at most: one thread adds them in order
constexpr int kCSumChunk = 1024;               // rows per LDS load of the finishing kernel
constexpr int kCFinishBlock = 256;

// a row's flags, as the row kernel leaves them for the finish
constexpr int32_t kHit = 1, kBadClass = 2;

// One row by the calling wave: nll and the flags to every lane; g (if not null) is the row
// of the gradient.  A class outside [0, C) or a refused row: nll and the gradient row NaN.
template <int NT>
__device__ __forceinline__ void loss_row(const float* __restrict__ x, uint32_t C, int64_t c, float invB, uint32_t lane,
                                         float* __restrict__ g, float& nll, int32_t& flags) {
    const float qnan = __int_as_float(0x7fc00000);
    const bool in_range = c >= 0 && c < (int64_t)C;
    const uint32_t cj = in_range ? (uint32_t)c : 0xffffffffu;
    float m, s;
    float best = -1.0f;                          // below every probability
    uint32_t besti = 0xffffffffu;
    bool ok = false;
    if (in_range)                                // the same in every lane of the wave
        ok = softmax::row<NT>(x, C, lane, m, s, [&](uint32_t j, float p) {
            if (g != nullptr) {
                const float d = p - (j == cj ? 1.0f : 0.0f);
                g[j] = d * invB;
            }
            if (p > best) {                      // ascending j: the first of equals stays
                best = p;
                besti = j;
            }
        });
    if (!ok) {
        if (g != nullptr)
            for (uint32_t j = lane; j < C; j += kCWave) g[j] = qnan;
        nll = qnan;
        flags = in_range ? 0 : kBadClass;
        return;
    }
    softmax::wave_best(best, besti);
    const float tc = x[cj] - m;                  // every lane reads the one element
    nll = logf(s) - tc;
    flags = besti == cj ? kHit : 0;
}

template <int NT>
__device__ __forceinline__ void one_row(const float* __restrict__ logits, uint32_t C, const int64_t* __restrict__ cls,
                                        uint64_t r, float invB, uint32_t lane, float* __restrict__ grad, float& nll,
                                        int32_t& flags) {
    loss_row<NT>(logits + r * C, C, cls[r], invB, lane, grad != nullptr ? grad + r * C : nullptr, nll, flags);
}

// what the finishing thread writes, from the sum of the rows' nll and their flags
__device__ __forceinline__ void finish(double sum, int32_t hits, int32_t bad, uint64_t B, double* __restrict__ loss,
                                       int32_t* __restrict__ hits_out, int32_t* __restrict__ status,
                                       double* __restrict__ totals) {
    const double l = sum * (1.0 / (double)B);
    *loss = l;
    *hits_out = hits;
    *status = bad;
    if (totals != nullptr) {                     // plain loads and stores: calls on one buffer share a stream
        totals[0] = totals[0] + l * (double)B;
        totals[1] = totals[1] + (double)hits;
        totals[2] = totals[2] + (double)bad;
    }
}

// ---------------------------------------------------------------------------
// B <= kCSmallB: one workgroup
// ---------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(kCSmallBlock) class_loss_small_kernel(
    const float* __restrict__ logits, uint32_t B, uint32_t C, const int64_t* __restrict__ cls, float invB,
    double* __restrict__ loss, float* __restrict__ grad, float* __restrict__ row_loss, int32_t* __restrict__ hits,
    int32_t* __restrict__ status, double* __restrict__ totals) {
    __shared__ float nll_s[kCSmallB];
    __shared__ int32_t flag_s[kCSmallB];
    const uint32_t lane = threadIdx.x % kCWave, wave = threadIdx.x / kCWave;
    for (uint32_t r = wave; r < B; r += kCSmallWaves) {          // the same trip count in a wave's 64 lanes
        float nll;
        int32_t flags;
        one_row<NT>(logits, C, cls, r, invB, lane, grad, nll, flags);
        if (lane == 0) {
            nll_s[r] = nll;
            flag_s[r] = flags;
            if (row_loss != nullptr) row_loss[r] = nll;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        int32_t h = 0, bad = 0;
        for (uint32_t i = 0; i < B; ++i) {
            a = a + (double)nll_s[i];
            h += flag_s[i] & kHit;
            bad |= (flag_s[i] & kBadClass) != 0;
        }
        finish(a, h, bad, B, loss, hits, status, totals);
    }
}

// ---------------------------------------------------------------------------
// B > kCSmallB: the rows, then the finish
// ---------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(kCBlock) class_loss_rows_kernel(const float* __restrict__ logits, uint64_t B,
                                                                  uint32_t C, const int64_t* __restrict__ cls,
                                                                  float invB, float* __restrict__ grad,
                                                                  float* __restrict__ row_loss,
                                                                  float* __restrict__ nll_out,
                                                                  int32_t* __restrict__ flag_out) {
    const uint32_t lane = threadIdx.x % kCWave;
    const uint64_t r = (uint64_t)blockIdx.x * kCRows + threadIdx.x / kCWave;
    if (r >= B) return;                          // a whole wave leaves: nothing below waits for another wave
    float nll;
    int32_t flags;
    one_row<NT>(logits, C, cls, r, invB, lane, grad, nll, flags);
    if (lane == 0) {
        nll_out[r] = nll;
        flag_out[r] = flags;
        if (row_loss != nullptr) row_loss[r] = nll;
    }
}

// one workgroup: the rows' nll added in order by thread 0, kCSumChunk of them per LDS load
__global__ void __launch_bounds__(kCFinishBlock) class_loss_finish_kernel(
    const float* __restrict__ nll_in, const int32_t* __restrict__ flag_in, uint64_t B, double* __restrict__ loss,
    int32_t* __restrict__ hits, int32_t* __restrict__ status, double* __restrict__ totals) {
    __shared__ float part[kCSumChunk];
    __shared__ int32_t fpart[kCSumChunk];
    double a = 0.0;
    int32_t h = 0, bad = 0;
    for (uint64_t i0 = 0; i0 < B; i0 += kCSumChunk) {
        const uint32_t n = (uint32_t)(B - i0 < (uint64_t)kCSumChunk ? B - i0 : (uint64_t)kCSumChunk);
        for (uint32_t q = threadIdx.x; q < n; q += kCFinishBlock) {
            part[q] = nll_in[i0 + q];
            fpart[q] = flag_in[i0 + q];
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t q = 0; q < n; ++q) {
                a = a + (double)part[q];
                h += fpart[q] & kHit;
                bad |= (fpart[q] & kBadClass) != 0;
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) finish(a, h, bad, B, loss, hits, status, totals);
}

// bytes of scratch for B rows: nll [B] float32, then the flags [B] int32
inline uint64_t scratch_need(uint64_t B) { return B <= (uint64_t)kCSmallB ? 0 : 8 * B; }

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_class_loss_small_b(void) { return kCSmallB; }

extern "C" uint64_t kf_class_loss_max_b(void) { return kCMaxB; }

extern "C" int kf_class_loss_scratch_bytes(uint64_t B, uint64_t* bytes) {
    if (!bytes) return kf_fail(KF_EINVAL, "kf_class_loss_scratch_bytes: null bytes");
    if (B == 0) return kf_fail(KF_EINVAL, "kf_class_loss_scratch_bytes: B == 0");
    if (B > kCMaxB)
        return kf_fail(KF_EINVAL, "kf_class_loss_scratch_bytes: B = %llu: %llu rows at most per call",
                       (unsigned long long)B, (unsigned long long)kCMaxB);
    *bytes = scratch_need(B);
    return KF_OK;
}

extern "C" int kf_class_loss(const float* d_logits, uint64_t B, uint64_t C, const int64_t* d_true, double* d_loss,
                             float* d_grad, float* d_row_loss, int32_t* d_hits, int32_t* d_status, double* d_totals,
                             void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (B == 0) return kf_fail(KF_EINVAL, "kf_class_loss: B == 0");
    if (C == 0) return kf_fail(KF_EINVAL, "kf_class_loss: C == 0");
    if (C >= (1ull << 31))
        return kf_fail(KF_EINVAL, "kf_class_loss: C = %llu: 2^31 columns or more", (unsigned long long)C);
    if (B > kCMaxB)
        return kf_fail(KF_EINVAL, "kf_class_loss: B = %llu: %llu rows at most per call", (unsigned long long)B,
                       (unsigned long long)kCMaxB);
    if (!d_logits) return kf_fail(KF_EINVAL, "kf_class_loss: null d_logits");
    if (!d_true) return kf_fail(KF_EINVAL, "kf_class_loss: null d_true");
    if (!d_loss) return kf_fail(KF_EINVAL, "kf_class_loss: null d_loss");
    if (!d_hits) return kf_fail(KF_EINVAL, "kf_class_loss: null d_hits");
    if (!d_status) return kf_fail(KF_EINVAL, "kf_class_loss: null d_status");
    if ((uintptr_t)d_logits & 3) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_logits (needs 4 bytes)");
    if ((uintptr_t)d_true & 7) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_true (needs 8 bytes)");
    if ((uintptr_t)d_loss & 7) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_loss (needs 8 bytes)");
    if ((uintptr_t)d_grad & 3) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_grad (needs 4 bytes)");
    if ((uintptr_t)d_row_loss & 3) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_row_loss (needs 4 bytes)");
    if ((uintptr_t)d_hits & 3) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_hits (needs 4 bytes)");
    if ((uintptr_t)d_status & 3) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_status (needs 4 bytes)");
    if ((uintptr_t)d_totals & 7) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_totals (needs 8 bytes)");
    if ((uintptr_t)d_scratch & 7) return kf_fail(KF_EINVAL, "kf_class_loss: misaligned d_scratch (needs 8 bytes)");
    const uint64_t need = scratch_need(B);
    if (need && !d_scratch) return kf_fail(KF_EINVAL, "kf_class_loss: null d_scratch");
    if (scratch_bytes < need)
        return kf_fail(KF_EINVAL, "kf_class_loss: scratch of %llu bytes, %llu needed", (unsigned long long)scratch_bytes,
                       (unsigned long long)need);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t c = (uint32_t)C;
    const float invB = 1.0f / (float)B;
    if (B <= (uint64_t)kCSmallB) {
        const dim3 grid(1), block(kCSmallBlock);
        const uint32_t b = (uint32_t)B;
        if (C <= 1 * kCWave)
            hipLaunchKernelGGL(class_loss_small_kernel<1>, grid, block, 0, s, d_logits, b, c, d_true, invB, d_loss, d_grad,
                               d_row_loss, d_hits, d_status, d_totals);
        else if (C <= 4 * kCWave)
            hipLaunchKernelGGL(class_loss_small_kernel<4>, grid, block, 0, s, d_logits, b, c, d_true, invB, d_loss, d_grad,
                               d_row_loss, d_hits, d_status, d_totals);
        else if (C <= (uint64_t)softmax::kRegCols)
            hipLaunchKernelGGL(class_loss_small_kernel<softmax::kRegTiles>, grid, block, 0, s, d_logits, b, c, d_true,
                               invB, d_loss, d_grad, d_row_loss, d_hits, d_status, d_totals);
        else
            hipLaunchKernelGGL(class_loss_small_kernel<0>, grid, block, 0, s, d_logits, b, c, d_true, invB, d_loss, d_grad,
                               d_row_loss, d_hits, d_status, d_totals);
        if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_class_loss: launch failed");
        return KF_OK;
    }
    float* nll = (float*)d_scratch;
    int32_t* flags = (int32_t*)(nll + B);
    const dim3 grid((uint32_t)((B + kCRows - 1) / kCRows)), block(kCBlock);
    if (C <= 1 * kCWave)
        hipLaunchKernelGGL(class_loss_rows_kernel<1>, grid, block, 0, s, d_logits, B, c, d_true, invB, d_grad, d_row_loss,
                           nll, flags);
    else if (C <= 4 * kCWave)
        hipLaunchKernelGGL(class_loss_rows_kernel<4>, grid, block, 0, s, d_logits, B, c, d_true, invB, d_grad, d_row_loss,
                           nll, flags);
    else if (C <= (uint64_t)softmax::kRegCols)
        hipLaunchKernelGGL(class_loss_rows_kernel<softmax::kRegTiles>, grid, block, 0, s, d_logits, B, c, d_true, invB,
                           d_grad, d_row_loss, nll, flags);
    else
        hipLaunchKernelGGL(class_loss_rows_kernel<0>, grid, block, 0, s, d_logits, B, c, d_true, invB, d_grad, d_row_loss,
                           nll, flags);
    hipLaunchKernelGGL(class_loss_finish_kernel, dim3(1), dim3(kCFinishBlock), 0, s, nll, flags, B, d_loss, d_hits,
                       d_status, d_totals);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_class_loss: launch failed");
    return KF_OK;
}

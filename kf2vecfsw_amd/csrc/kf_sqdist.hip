// kf_sqdist.hip -- kf_sq_distances: squared Euclidean distances in the direct form.
//
// out[i, j] for x[Q x D] and y[B x D], float32, exactly as query holds them after
// torch.cdist(..., compute_mode='donot_use_mm_for_euclid_dist') squared and cut
// (kf2vec/query.py:169-176), with the order of the sum fixed:
//   s = 0;  for d ascending: t = x_d - y_d, s = s + t * t   (every operation
//   rounded to float32, none contracted into an fma);  r = sqrt(s);  v = r * r;
//   out = v < 1e-6f ? 0 : v
// The differences are formed before anything is squared, so small distances keep
// their digits: the matmul form |x|^2 + |y|^2 - 2 x.y cancels there, which is
// why the reference asks cdist for this one.  query.sq_distances_host states the
// same operations in numpy.
//
// A workgroup owns a kSTile x kSTile tile of out.  It walks D in slices of kSDepth:
// the slice of its kSTile rows of x and of y goes through LDS (transposed, so a
// thread reads its four rows and four columns as one 16-byte load each), read
// from HBM once per tile pair; a thread keeps 4 x 4 sums in registers.  Rows past
// Q or B and columns past D are zeros in LDS: t = 0, s + 0 = s, so a ragged edge
// adds nothing, and since the order over d within a pair is fixed the result
// does not depend on how the tiles are cut.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_internal.h"

// No product and sum below may become an fma.  __fmul_rn and __fadd_rn do not
// keep them apart: they are plain operators in a header compiled with
// contraction allowed, and inlined here the pair becomes v_pk_fma_f32.  So the
// operators are written out under this pragma, which covers the whole file (the
// ISA of sqdist_kernel then has v_pk_mul_f32 and v_pk_add_f32 and no fma but
// the ones inside the square root's refinement).  __fsqrt_rn is kept: in this
// toolchain it is the library's native square root, which the compiler lowers
// to v_sqrt_f32 and an fma refinement that rounds correctly; nothing in the
// language promises that lowering, so the bit-for-bit comparison with numpy's
// sqrt in tests/test_gpu_float_format.py is what guards it.
#pragma clang fp contract(off)

namespace kf {
namespace {

constexpr int kSTile = 64;                    // rows of x, and of y, per workgroup
constexpr int kSDepth = 32;                   // columns per slice
constexpr int kSBlock = 256;                  // threads: 16 x 16, each 4 x 4 outputs
constexpr int kSPitch = kSTile + 4;           // floats per LDS row: 16-byte rows, banks staggered

typedef float v4f __attribute__((ext_vector_type(4)));

// rows [r0, r0 + kSTile) x columns [d0, d0 + kSDepth) of m[n x D] into lds[dd][row], zeros outside
__device__ __forceinline__ void load_slice(const float* __restrict__ m, uint64_t n, uint64_t D, uint64_t r0,
                                           uint64_t d0, float (*lds)[kSPitch]) {
    const uint32_t dd = threadIdx.x % kSDepth;
#pragma unroll
    for (uint32_t i = 0; i < kSTile * kSDepth / kSBlock; ++i) {
        const uint32_t row = threadIdx.x / kSDepth + i * (kSBlock / kSDepth);
        const uint64_t r = r0 + row, d = d0 + dd;
        lds[dd][row] = r < n && d < D ? m[r * D + d] : 0.0f;
    }
}

__global__ void __launch_bounds__(kSBlock) sqdist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         uint64_t Q, uint64_t B, uint64_t D, uint64_t tiles_b,
                                                         float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float xs[kSDepth][kSPitch];
    __shared__ __attribute__((aligned(16))) float ys[kSDepth][kSPitch];
    const uint64_t tq = blockIdx.x / tiles_b, tb = blockIdx.x - tq * tiles_b;
    const uint64_t q0 = tq * kSTile, b0 = tb * kSTile;
    const uint32_t tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    float s[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[i][j] = 0.0f;
    for (uint64_t d0 = 0; d0 < D; d0 += kSDepth) {
        load_slice(x, Q, D, q0, d0, xs);
        load_slice(y, B, D, b0, d0, ys);
        __syncthreads();
#pragma unroll 8
        for (int dd = 0; dd < kSDepth; ++dd) {
            const v4f xv = *(const v4f*)&xs[dd][4 * ty];
            const v4f yv = *(const v4f*)&ys[dd][4 * tx];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float t = xv[i] - yv[j];
                    const float p = t * t;
                    s[i][j] = s[i][j] + p;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t q = q0 + 4 * ty + i;
        if (q >= Q) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t b = b0 + 4 * tx + j;
            if (b >= B) continue;
            const float r = __fsqrt_rn(s[i][j]);
            const float v = r * r;
            out[q * B + b] = v < 1e-6f ? 0.0f : v;
        }
    }
}

inline bool mul_overflows(uint64_t a, uint64_t b) { return b && a > ~0ull / b; }

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_sq_distances_tile(void) { return kSTile; }

extern "C" int kf_sq_distances(const float* d_x, uint64_t Q, const float* d_y, uint64_t B, uint64_t D, float* d_out,
                               void* stream) {
    if (D == 0) return kf_fail(KF_EINVAL, "kf_sq_distances: D == 0");
    if (mul_overflows(Q, D) || mul_overflows(B, D) || mul_overflows(Q, B) || Q * D >= (1ull << 61) ||
        B * D >= (1ull << 61) || Q * B >= (1ull << 61))
        return kf_fail(KF_EINVAL, "kf_sq_distances: %llu x %llu x %llu: a matrix of 2^61 elements or more",
                       (unsigned long long)Q, (unsigned long long)B, (unsigned long long)D);
    const uint64_t tiles_q = (Q + kSTile - 1) / kSTile, tiles_b = (B + kSTile - 1) / kSTile;
    if (mul_overflows(tiles_q, tiles_b) || tiles_q * tiles_b >= (1ull << 24))   // a launch has fewer than 2^32 threads
        return kf_fail(KF_EINVAL, "kf_sq_distances: %llu x %llu outputs: fewer than 2^24 tiles of %d x %d per call",
                       (unsigned long long)Q, (unsigned long long)B, kSTile, kSTile);
    if (Q && !d_x) return kf_fail(KF_EINVAL, "kf_sq_distances: null d_x");
    if (B && !d_y) return kf_fail(KF_EINVAL, "kf_sq_distances: null d_y");
    if (Q && B && !d_out) return kf_fail(KF_EINVAL, "kf_sq_distances: null d_out");
    if ((uintptr_t)d_x & 3) return kf_fail(KF_EINVAL, "kf_sq_distances: misaligned d_x (needs 4 bytes)");
    if ((uintptr_t)d_y & 3) return kf_fail(KF_EINVAL, "kf_sq_distances: misaligned d_y (needs 4 bytes)");
    if ((uintptr_t)d_out & 3) return kf_fail(KF_EINVAL, "kf_sq_distances: misaligned d_out (needs 4 bytes)");
    if (Q == 0 || B == 0) return KF_OK;
    hipLaunchKernelGGL(sqdist_kernel, dim3((uint32_t)(tiles_q * tiles_b)), dim3(kSBlock), 0, (hipStream_t)stream, d_x,
                       d_y, Q, B, D, tiles_b, d_out);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "kf_sq_distances: launch failed");
    return KF_OK;
}

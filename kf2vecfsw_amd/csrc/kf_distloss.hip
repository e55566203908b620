// kf_distloss.hip -- kf_dist_loss and kf_dist_loss_views: the distance trainers' weighted loss
// of a batch and its gradient with respect to the embeddings, with the order of every sum fixed.
//
// For embeddings y[B x E] (float32), the clade's true distances P[N x N] (float64) and the
// batch's labels l[B] (rows and columns of P), over i, j in [0, B)
// (kf2vec/train_model_set.py:448-467, losses.py:13-49, utils.py:240-256):
//   s_ij = 0;  for e ascending: t = y_i[e] - y_j[e], s = s + t * t        (float32)
//   d_ij = sqrtf(s_ij)                                                     (correctly rounded)
//   T = P[l_i, l_j];  w = 1 / (T + eps);  r = sqrt(T);  u = (double)d_ij - r
//   v_ij = (u * u) * w;  inv = 1 / (double)(B * B)                         (float64)
//   loss = (sum_i (sum_j v_ij)) * inv       (float64, both sums from 0.0, j and i ascending)
//   g_ij = (float)(((2 * u) * w) * inv)
//   c_ij = d_ij == 0 ? 0 : (g_ij + g_ji) / d_ij                            (float32, g_ji at P[l_j, l_i])
//   grad_i[e] = 0;  for j ascending: grad = grad + c_ij * (y_i[e] - y_j[e])   (float32)
// Every operation is rounded on its own and none is contracted into an fma.  This is
// torch.cdist(..., 'donot_use_mm_for_euclid_dist'), the reference's Loss and autograd's
// backward of both in the direct form; train.dist_loss_host states it in numpy, and the
// kernels equal it bit for bit whatever path they take, because every output's chain of
// additions is walked by one thread in the stated order.
//
// kf_dist_loss has a label per row and eps = 1e-6.  kf_dist_loss_views is the chunk trainer's
// (kf2vec/train_model_set_chunks.py:392-418, losses.py:58-117): `views` rows that follow each
// other share a label, l_i = labels[i / views] (torch.repeat_interleave), and eps is the
// caller's (Loss_chunks has 1000).  Both are one code: the labels' load, pair_terms and the
// labels' check are the three places that know of either.
//
// s_ij and s_ji are the same bits (t and -t have the same square), so d is symmetric and
// the element at [j, i] serves as d_ij: the pair kernel reads, and the gradient kernel's
// coefficients are stored, with i as the fast index, which keeps every access coalesced.
//
// B <= kLSmallB: one workgroup does it all (the default batch of 16 rows pays for one
// launch of one workgroup, and needs no scratch).  Above: five launches --
//   dist   d[i, j] by 32 x 32 tiles, E walked in slices through LDS (as sqdist_kernel)
//   pair   one thread per pair: v to vT[j, i] (float64), c over d in place at [j, i]
//   rows   thread i adds vT[0..B, i] in order
//   total  one workgroup: the labels' check, the B row sums added in order, loss and status
//   grad   32 x 32 tiles of grad, j walked in slices of c and y through LDS
// A thread of dist and grad keeps 2 x 2 sums, not sqdist_kernel's 4 x 4: every sum is a chain of
// dependent additions whose length the contract fixes, so a workgroup's time is the chains a
// thread interleaves times their length, and at a clade's sizes (64 to 850 rows) tiles of 64
// left most of the device idle behind a few long-running workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kf_internal.h"

// as in kf_sqdist.hip: no product and sum of this file may become an fma, in float32 or float64
#pragma clang fp contract(off)
// The float32 square root is sqrtf, not __fsqrt_rn: the latter is the library's native square
// root, and in dist_loss_small_kernel the compiler lowered it to a bare v_sqrt_f32 (one unit
// off in some d, seen in the loss at B = 16 and 32), while sqrtf, under hipcc's default of
// correctly rounded float32 division and square root, gets the fma fix-up in both kernels.

namespace kf {
namespace {

constexpr int kLSmallB = 32;                  // rows up to which one workgroup does it all
constexpr int kLSmallBlock = 1024;            // its threads: a pair each
constexpr uint64_t kLMaxB = 8192;             // rows at most: 12 * B * B bytes of scratch
constexpr uint64_t kLMaxE = 1ull << 24;
constexpr int kLPer = 2;                      // outputs per thread and dimension: short chains per thread, many workgroups
constexpr int kLTile = 16 * kLPer;            // rows and columns of a tile of d, rows and columns of a tile of grad
constexpr int kLDepth = 32;                   // columns of y per slice (dist), rows j per slice (grad)
constexpr int kLSmallDepth = kLDepth;         // columns of y per slice of the small path: an element per thread
static_assert(kLSmallB * kLSmallDepth == kLSmallBlock, "a thread carries one element of a slice");
constexpr int kLBlock = 256;                  // threads: 16 x 16, each kLPer x kLPer outputs
constexpr int kLPitch = kLTile + kLPer;       // floats per LDS row: rows aligned to a thread's read, banks staggered
constexpr int kLSumChunk = 1024;              // row sums per LDS load of the total kernel

typedef float vLf __attribute__((ext_vector_type(kLPer)));

// v_ij, and c_ij if want_c, of one pair: d = d_ij (= d_ji), tij = P[l_i, l_j], tji = P[l_j, l_i]
__device__ __forceinline__ void pair_terms(float d, double tij, double tji, double eps, double inv, bool want_c,
                                           double& v, float& c) {
    const double w = 1.0 / (tij + eps);
    const double r = sqrt(tij);
    const double u = (double)d - r;
    const double uu = u * u;
    v = uu * w;
    c = 0.0f;
    if (want_c) {
        const double a = 2.0 * u;
        const double aw = a * w;
        const float gij = (float)(aw * inv);
        const double w2 = 1.0 / (tji + eps);
        const double r2 = sqrt(tji);
        const double u2 = (double)d - r2;
        const double a2 = 2.0 * u2;
        const double aw2 = a2 * w2;
        const float gji = (float)(aw2 * inv);
        const float gs = gij + gji;
        c = d == 0.0f ? 0.0f : __fdiv_rn(gs, d);
    }
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the place of row i's label: `views` rows that follow each other share one (i < 2^13)
__device__ __forceinline__ uint32_t label_of(uint32_t i, uint32_t views) { return views == 1 ? i : i / views; }

// ---------------------------------------------------------------------------
// B <= kLSmallB: one workgroup
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kLSmallBlock) dist_loss_small_kernel(
    const float* __restrict__ y, uint32_t B, uint64_t E, const double* __restrict__ P, uint64_t N,
    const int64_t* __restrict__ labels, uint32_t views, double eps, double* __restrict__ loss,
    float* __restrict__ grad, int32_t* __restrict__ status) {
    __shared__ float ys[kLSmallB][kLSmallDepth + 1];
    __shared__ double vs[kLSmallB][kLSmallB + 1];
    __shared__ float cs[kLSmallB][kLSmallB + 1];
    __shared__ double rsum[kLSmallB];
    __shared__ int64_t lab[kLSmallB];
    const uint32_t tid = threadIdx.x;
    int mine_bad = 0;
    if (tid < B) {
        const int64_t l = labels[label_of(tid, views)];
        lab[tid] = l;
        mine_bad = l < 0 || (uint64_t)l >= N;
    }
    const int bad = __syncthreads_or(mine_bad);          // lab[] is visible behind it
    const uint32_t pairs = B * B;
    const uint32_t i = tid / B, j = tid - i * B;         // the pair of this thread, if tid < pairs
    // the element of a slice that this thread carries from y to LDS, fetched a slice ahead of its use
    const uint32_t lr = tid / kLSmallDepth, ld = tid % kLSmallDepth;
    auto fetch = [&](uint64_t e0) -> float {
        const uint64_t e = e0 + ld;
        return lr < B && e < E ? y[(uint64_t)lr * E + e] : 0.0f;    // a column past E: t = 0, s + 0 = s
    };
    float s = 0.0f;
    float nxt = fetch(0);
    for (uint64_t e0 = 0; e0 < E; e0 += kLSmallDepth) {
        ys[lr][ld] = nxt;
        __syncthreads();
        if (e0 + kLSmallDepth < E) nxt = fetch(e0 + kLSmallDepth);
        if (tid < pairs) {
#pragma unroll                                           // a slice's 64 LDS reads in flight at once: one wait, not four
            for (int dd = 0; dd < kLSmallDepth; ++dd) {
                const float t = ys[i][dd] - ys[j][dd];
                const float p = t * t;
                s = s + p;
            }
        }
        __syncthreads();
    }
    const double inv = 1.0 / (double)((uint64_t)B * B);
    if (tid < pairs) {
        const float d = sqrtf(s);
        double tij = quiet_nan(), tji = quiet_nan();
        if (!bad) {
            tij = P[(uint64_t)lab[i] * N + (uint64_t)lab[j]];
            tji = P[(uint64_t)lab[j] * N + (uint64_t)lab[i]];
        }
        double v;
        float c;
        pair_terms(d, tij, tji, eps, inv, grad != nullptr, v, c);
        vs[i][j] = v;
        cs[i][j] = c;
    }
    __syncthreads();
    if (tid < B) {
        double a = 0.0;
        for (uint32_t q = 0; q < B; ++q) a = a + vs[tid][q];
        rsum[tid] = a;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (uint32_t q = 0; q < B; ++q) a = a + rsum[q];
        *loss = bad ? quiet_nan() : a * inv;
        *status = bad ? 1 : 0;
    }
    if (grad != nullptr) {                               // cs[][] is visible since the barrier behind it
        nxt = fetch(0);
        for (uint64_t e0 = 0; e0 < E; e0 += kLSmallDepth) {
            ys[lr][ld] = nxt;
            __syncthreads();
            if (e0 + kLSmallDepth < E) nxt = fetch(e0 + kLSmallDepth);
            const uint64_t e = e0 + ld;
            if (lr < B && e < E) {                       // grad[lr, e]: this thread's own element of the slice
                const float yi = ys[lr][ld];
                float g = 0.0f;
#pragma unroll 4
                for (uint32_t q = 0; q < B; ++q) {
                    const float t = yi - ys[q][ld];
                    const float p = cs[lr][q] * t;
                    g = g + p;
                }
                grad[(uint64_t)lr * E + e] = g;
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------
// B > kLSmallB
// ---------------------------------------------------------------------------
// rows [r0, r0 + kLTile) x columns [e0, e0 + kLDepth) of y[B x E] into lds[dd][row], zeros outside
__device__ __forceinline__ void load_y_slice(const float* __restrict__ y, uint64_t B, uint64_t E, uint64_t r0,
                                             uint64_t e0, float (*lds)[kLPitch]) {
    const uint32_t dd = threadIdx.x % kLDepth;
#pragma unroll
    for (uint32_t k = 0; k < kLTile * kLDepth / kLBlock; ++k) {
        const uint32_t row = threadIdx.x / kLDepth + k * (kLBlock / kLDepth);
        const uint64_t r = r0 + row, e = e0 + dd;
        lds[dd][row] = r < B && e < E ? y[r * E + e] : 0.0f;
    }
}

// d[i, j] = sqrtf(s_ij): sqdist_kernel's tiling with both operands y
__global__ void __launch_bounds__(kLBlock) dist_kernel(const float* __restrict__ y, uint64_t B, uint64_t E,
                                                       uint64_t tiles, float* __restrict__ d) {
    __shared__ __attribute__((aligned(4 * kLPer))) float as[kLDepth][kLPitch];
    __shared__ __attribute__((aligned(4 * kLPer))) float bs[kLDepth][kLPitch];
    const uint64_t ta = blockIdx.x / tiles, tb = blockIdx.x - ta * tiles;
    const uint64_t a0 = ta * kLTile, b0 = tb * kLTile;
    const uint32_t tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    float s[kLPer][kLPer];
#pragma unroll
    for (int a = 0; a < kLPer; ++a)
#pragma unroll
        for (int b = 0; b < kLPer; ++b) s[a][b] = 0.0f;
    for (uint64_t e0 = 0; e0 < E; e0 += kLDepth) {
        load_y_slice(y, B, E, a0, e0, as);
        load_y_slice(y, B, E, b0, e0, bs);
        __syncthreads();
#pragma unroll 8
        for (int dd = 0; dd < kLDepth; ++dd) {
            const vLf av = *(const vLf*)&as[dd][kLPer * ty];
            const vLf bv = *(const vLf*)&bs[dd][kLPer * tx];
#pragma unroll
            for (int a = 0; a < kLPer; ++a)
#pragma unroll
                for (int b = 0; b < kLPer; ++b) {
                    const float t = av[a] - bv[b];
                    const float p = t * t;
                    s[a][b] = s[a][b] + p;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < kLPer; ++a) {
        const uint64_t r = a0 + kLPer * ty + a;
        if (r >= B) continue;
#pragma unroll
        for (int b = 0; b < kLPer; ++b) {
            const uint64_t q = b0 + kLPer * tx + b;
            if (q >= B) continue;
            d[r * B + q] = sqrtf(s[a][b]);
        }
    }
}

// one thread per pair, i the fast index: reads d at [j, i] (the bits of d_ij), writes v_ij to
// vT[j, i] and, if want_c, c_ij over d at [j, i]
__global__ void __launch_bounds__(kLBlock) pair_kernel(float* __restrict__ dc, double* __restrict__ vT, uint64_t B,
                                                       const double* __restrict__ P, uint64_t N,
                                                       const int64_t* __restrict__ labels, uint32_t views, double eps,
                                                       int want_c) {
    const uint64_t x = (uint64_t)blockIdx.x * kLBlock + threadIdx.x;
    if (x >= B * B) return;
    const uint64_t j = x / B, i = x - j * B;
    const int64_t li = labels[label_of((uint32_t)i, views)], lj = labels[label_of((uint32_t)j, views)];
    double tij = quiet_nan(), tji = quiet_nan();
    if (li >= 0 && (uint64_t)li < N && lj >= 0 && (uint64_t)lj < N) {
        tij = P[(uint64_t)li * N + (uint64_t)lj];
        tji = P[(uint64_t)lj * N + (uint64_t)li];
    }
    const double inv = 1.0 / (double)(B * B);
    double v;
    float c;
    pair_terms(dc[x], tij, tji, eps, inv, want_c != 0, v, c);
    vT[x] = v;
    if (want_c) dc[x] = c;
}

// rsum[i] = sum over j ascending of vT[j, i]
__global__ void __launch_bounds__(64) rows_kernel(const double* __restrict__ vT, uint64_t B,
                                                  double* __restrict__ rsum) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    double a = 0.0;
#pragma unroll 8
    for (uint64_t j = 0; j < B; ++j) a = a + vT[j * B + i];
    rsum[i] = a;
}

// one workgroup: the labels' check, the row sums added in order, loss and status
__global__ void __launch_bounds__(kLBlock) total_kernel(const double* __restrict__ rsum, uint64_t B,
                                                        const int64_t* __restrict__ labels, uint64_t n_labels,
                                                        uint64_t N, double* __restrict__ loss,
                                                        int32_t* __restrict__ status) {
    __shared__ double part[kLSumChunk];
    int mine_bad = 0;
    for (uint64_t i = threadIdx.x; i < n_labels; i += kLBlock) {
        const int64_t l = labels[i];
        mine_bad |= l < 0 || (uint64_t)l >= N;
    }
    const int bad = __syncthreads_or(mine_bad);
    double a = 0.0;
    for (uint64_t i0 = 0; i0 < B; i0 += kLSumChunk) {
        const uint32_t n = (uint32_t)(B - i0 < (uint64_t)kLSumChunk ? B - i0 : (uint64_t)kLSumChunk);
        for (uint32_t q = threadIdx.x; q < n; q += kLBlock) part[q] = rsum[i0 + q];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t q = 0; q < n; ++q) a = a + part[q];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double inv = 1.0 / (double)(B * B);
        *loss = bad ? quiet_nan() : a * inv;
        *status = bad ? 1 : 0;
    }
}

// grad[i, e] for a kLTile x kLTile tile: j walked in slices of kLDepth, c[j, i] (stored with i
// fast) and y[j, e] through LDS; a thread keeps 2 x 2 sums and its own y_i[e] in registers
__global__ void __launch_bounds__(kLBlock) grad_kernel(const float* __restrict__ y, const float* __restrict__ cT,
                                                       uint64_t B, uint64_t E, uint64_t tiles_e,
                                                       float* __restrict__ grad) {
    __shared__ __attribute__((aligned(4 * kLPer))) float cs[kLDepth][kLPitch];
    __shared__ __attribute__((aligned(4 * kLPer))) float ys[kLDepth][kLPitch];
    const uint64_t ti = blockIdx.x / tiles_e, te = blockIdx.x - ti * tiles_e;
    const uint64_t i0 = ti * kLTile, e0 = te * kLTile;
    const uint32_t tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    float yi[kLPer][kLPer], g[kLPer][kLPer];
#pragma unroll
    for (int a = 0; a < kLPer; ++a)
#pragma unroll
        for (int b = 0; b < kLPer; ++b) {
            const uint64_t r = i0 + kLPer * ty + a, e = e0 + kLPer * tx + b;
            yi[a][b] = r < B && e < E ? y[r * E + e] : 0.0f;
            g[a][b] = 0.0f;
        }
    const uint32_t col = threadIdx.x % kLTile;
    for (uint64_t j0 = 0; j0 < B; j0 += kLDepth) {
        const int nj = (int)(B - j0 < (uint64_t)kLDepth ? B - j0 : (uint64_t)kLDepth);   // the same in every thread
#pragma unroll
        for (uint32_t k = 0; k < kLTile * kLDepth / kLBlock; ++k) {
            const uint32_t jj = threadIdx.x / kLTile + k * (kLBlock / kLTile);
            const uint64_t j = j0 + jj;
            cs[jj][col] = j < B && i0 + col < B ? cT[j * B + i0 + col] : 0.0f;
            ys[jj][col] = j < B && e0 + col < E ? y[j * E + e0 + col] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < nj; ++jj) {                // rows j past B are not walked: nothing is added for them
            const vLf cv = *(const vLf*)&cs[jj][kLPer * ty];
            const vLf yv = *(const vLf*)&ys[jj][kLPer * tx];
#pragma unroll
            for (int a = 0; a < kLPer; ++a)
#pragma unroll
                for (int b = 0; b < kLPer; ++b) {
                    const float t = yi[a][b] - yv[b];
                    const float p = cv[a] * t;
                    g[a][b] = g[a][b] + p;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < kLPer; ++a) {
        const uint64_t r = i0 + kLPer * ty + a;
        if (r >= B) continue;
#pragma unroll
        for (int b = 0; b < kLPer; ++b) {
            const uint64_t e = e0 + kLPer * tx + b;
            if (e >= E) continue;
            grad[r * E + e] = g[a][b];
        }
    }
}

// bytes of scratch for B rows: vT [B x B] float64, the row sums [B] float64, d and then c [B x B] float32
inline uint64_t scratch_need(uint64_t B) { return B <= (uint64_t)kLSmallB ? 0 : 8 * B * B + 8 * B + 4 * B * B; }

}  // namespace
}  // namespace kf

using namespace kf;

extern "C" int kf_dist_loss_small_b(void) { return kLSmallB; }

extern "C" int kf_dist_loss_tile(void) { return kLTile; }

extern "C" int kf_dist_loss_depth(void) { return kLDepth; }

extern "C" uint64_t kf_dist_loss_max_b(void) { return kLMaxB; }

extern "C" int kf_dist_loss_scratch_bytes(uint64_t B, uint64_t* bytes) {
    if (!bytes) return kf_fail(KF_EINVAL, "kf_dist_loss_scratch_bytes: null bytes");
    if (B == 0) return kf_fail(KF_EINVAL, "kf_dist_loss_scratch_bytes: B == 0");
    if (B > kLMaxB)
        return kf_fail(KF_EINVAL, "kf_dist_loss_scratch_bytes: B = %llu: %llu rows at most per call",
                       (unsigned long long)B, (unsigned long long)kLMaxB);
    *bytes = scratch_need(B);
    return KF_OK;
}

namespace kf {
namespace {

// both entries: `what` names the one called in its refusals
int dist_loss_run(const char* what, const float* d_y, uint64_t B, uint64_t E, const double* d_true, uint64_t N,
                  const int64_t* d_labels, uint64_t views, double eps, double* d_loss, float* d_grad,
                  int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (B == 0) return kf_fail(KF_EINVAL, "%s: B == 0", what);
    if (E == 0) return kf_fail(KF_EINVAL, "%s: E == 0", what);
    if (views == 0) return kf_fail(KF_EINVAL, "%s: views == 0", what);
    if (B % views != 0)
        return kf_fail(KF_EINVAL, "%s: B = %llu rows are no multiple of views = %llu", what, (unsigned long long)B,
                       (unsigned long long)views);
    if (!(eps >= 0.0) || isinf(eps)) return kf_fail(KF_EINVAL, "%s: eps = %g: a finite value, not negative", what, eps);
    if (B > kLMaxB)
        return kf_fail(KF_EINVAL, "%s: B = %llu: %llu rows at most per call", what, (unsigned long long)B,
                       (unsigned long long)kLMaxB);
    if (E > kLMaxE)
        return kf_fail(KF_EINVAL, "%s: E = %llu: 2^24 columns at most", what, (unsigned long long)E);
    if (N == 0 || N >= (1ull << 30))
        return kf_fail(KF_EINVAL, "%s: N = %llu: a matrix of 1 to 2^30 - 1 rows", what, (unsigned long long)N);
    if (!d_y) return kf_fail(KF_EINVAL, "%s: null d_y", what);
    if (!d_true) return kf_fail(KF_EINVAL, "%s: null d_true", what);
    if (!d_labels) return kf_fail(KF_EINVAL, "%s: null d_labels", what);
    if (!d_loss) return kf_fail(KF_EINVAL, "%s: null d_loss", what);
    if (!d_status) return kf_fail(KF_EINVAL, "%s: null d_status", what);
    if ((uintptr_t)d_y & 3) return kf_fail(KF_EINVAL, "%s: misaligned d_y (needs 4 bytes)", what);
    if ((uintptr_t)d_true & 7) return kf_fail(KF_EINVAL, "%s: misaligned d_true (needs 8 bytes)", what);
    if ((uintptr_t)d_labels & 7) return kf_fail(KF_EINVAL, "%s: misaligned d_labels (needs 8 bytes)", what);
    if ((uintptr_t)d_loss & 7) return kf_fail(KF_EINVAL, "%s: misaligned d_loss (needs 8 bytes)", what);
    if ((uintptr_t)d_grad & 3) return kf_fail(KF_EINVAL, "%s: misaligned d_grad (needs 4 bytes)", what);
    if ((uintptr_t)d_status & 3) return kf_fail(KF_EINVAL, "%s: misaligned d_status (needs 4 bytes)", what);
    if ((uintptr_t)d_scratch & 7) return kf_fail(KF_EINVAL, "%s: misaligned d_scratch (needs 8 bytes)", what);
    const uint64_t need = scratch_need(B);
    if (need && !d_scratch) return kf_fail(KF_EINVAL, "%s: null d_scratch", what);
    if (scratch_bytes < need)
        return kf_fail(KF_EINVAL, "%s: scratch of %llu bytes, %llu needed", what, (unsigned long long)scratch_bytes,
                       (unsigned long long)need);
    const hipStream_t s = (hipStream_t)stream;
    if (B <= (uint64_t)kLSmallB) {
        hipLaunchKernelGGL(dist_loss_small_kernel, dim3(1), dim3(kLSmallBlock), 0, s, d_y, (uint32_t)B, E, d_true, N,
                           d_labels, (uint32_t)views, eps, d_loss, d_grad, d_status);
        if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "%s: launch failed", what);
        return KF_OK;
    }
    double* vT = (double*)d_scratch;
    double* rsum = vT + B * B;
    float* dc = (float*)(rsum + B);
    const uint64_t tiles = (B + kLTile - 1) / kLTile, tiles_e = (E + kLTile - 1) / kLTile;
    hipLaunchKernelGGL(dist_kernel, dim3((uint32_t)(tiles * tiles)), dim3(kLBlock), 0, s, d_y, B, E, tiles, dc);
    hipLaunchKernelGGL(pair_kernel, dim3((uint32_t)((B * B + kLBlock - 1) / kLBlock)), dim3(kLBlock), 0, s, dc, vT, B,
                       d_true, N, d_labels, (uint32_t)views, eps, d_grad != nullptr ? 1 : 0);
    hipLaunchKernelGGL(rows_kernel, dim3((uint32_t)((B + 63) / 64)), dim3(64), 0, s, vT, B, rsum);
    hipLaunchKernelGGL(total_kernel, dim3(1), dim3(kLBlock), 0, s, rsum, B, d_labels, B / views, N, d_loss,
                       d_status);
    if (d_grad != nullptr)
        hipLaunchKernelGGL(grad_kernel, dim3((uint32_t)(tiles * tiles_e)), dim3(kLBlock), 0, s, d_y, dc, B, E, tiles_e,
                           d_grad);
    if (hipGetLastError() != hipSuccess) return kf_fail(KF_EHIP, "%s: launch failed", what);
    return KF_OK;
}

}  // namespace
}  // namespace kf

extern "C" int kf_dist_loss(const float* d_y, uint64_t B, uint64_t E, const double* d_true, uint64_t N,
                            const int64_t* d_labels, double* d_loss, float* d_grad, int32_t* d_status,
                            void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return dist_loss_run("kf_dist_loss", d_y, B, E, d_true, N, d_labels, 1, 1e-6, d_loss, d_grad, d_status, d_scratch,
                         scratch_bytes, stream);
}

extern "C" int kf_dist_loss_views(const float* d_y, uint64_t B, uint64_t E, const double* d_true, uint64_t N,
                                  const int64_t* d_labels, uint64_t views, double eps, double* d_loss, float* d_grad,
                                  int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return dist_loss_run("kf_dist_loss_views", d_y, B, E, d_true, N, d_labels, views, eps, d_loss, d_grad, d_status,
                         d_scratch, scratch_bytes, stream);
}

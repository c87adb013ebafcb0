// Training of the classifier head on the device (reference train.py restricted to net._fc, model.py:50-61):
//   Dropout(p0) -> Linear 1280x512 -> BatchNorm1d -> ReLU -> Dropout(p1) -> Linear 512x256 -> BatchNorm1d -> ReLU ->
//   Dropout(p2) -> Linear 256x1, FocalLoss (train.py:360-392) with mixup_criterion's two label vectors (:352-354),
//   gradient accumulation, clip_grad_norm_, torch.optim.AdamW, EMAModel (:398-416).  fp32 throughout; the backbone is
//   frozen, so nothing flows back past the pooled features.
//
// A batch has at most 256 rows, so one workgroup owns ALL rows of a 16-column slab of a layer: the BatchNorm column
// statistics (mean / variance forward, sum dz and sum dz.xhat backward) are in-block reductions and GEMM + BN + ReLU +
// dropout is one launch per layer in each direction.  The backward GEMMs run on the exact fp32 MFMA (16x16x4), the
// forward ones on the fp64 MFMA of the same shape (slab_gemm_xwt says why).  Lane (r, q) of a wave loads 4 consecutive
// k of its operand row as one 16-byte load and issues 4 MFMAs on them, both operands with the same k per lane, so the
// fragment needs no LDS; each output is summed in 4 independent chains.  Rows past n are masked to zero at the load,
// never read.
//
// Launches of one accumulate: dropout0, layer 1 fwd, layer 2 fwd, loss (logits + focal loss + fc3 gradients), layer 2
// bwd (BN), layer 1 bwd (dY2.W2 + BN), weight gradients of fc2 and fc1.  One apply: sum of squares, then one
// elementwise launch over the flat parameter arena (clip, AdamW, EMA, zeroing).  Every reduction has a fixed order (no
// atomics): a step is reproducible from (seed, counter).
//
// The gradient of b1 / b2 is identically zero (a bias in front of batch-statistics BatchNorm cancels in y - mean(y));
// autograd produces rounding noise of order 1e-10 there, this file adds nothing to those slots.
//
// Built with -ffp-contract=off (Makefile): outside the MFMA chains every operation is rounded on its own.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "b0_kernels.h"
#include "dfd_common.h"
#include "head_train_state.h"
#include "kernel_util.h"

using namespace dfd;

namespace {

// sizes and the layout of the parameter arena: head_train_state.h
static_assert(HT_THREADS == HT_H2, "ht_loss_kernel: one thread per column of w3");

typedef float f4 __attribute__((ext_vector_type(4)));

// fmix32 / mask_key / mask_keep: head_train_state.h

// ---------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(HT_THREADS) void ht_dropout0_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 uint8_t* __restrict__ mask, int count, uint32_t key,
                                                                 uint32_t thr, float scale) {
    const int i = blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= count) return;
    const bool k = mask_keep(key, (uint32_t)i, thr);
    mask[i] = k ? 1 : 0;
    y[i] = k ? x[i] * scale : 0.f;
}

// Y slab [n][16] = X [n][K] . W[col0 .. col0 + 16][K]^T + bias into LDS (rows of tiles past n stay unwritten).  4 waves,
// wave w owns the 16-row tiles w, w + 4, w + 8, w + 12.  The forward products go through the fp64 MFMA
// (v_mfma_f64_16x16x4_f64: A / B one value per lane as the f32 16x16x4 form, C / D col = lane & 15, row = (lane >> 4) +
// 4 reg): the product of two floats is exact in double and the sums carry 53 bits, so y is the dot product rounded
// ONCE to fp32 - the logit, the loss and the fc3 gradients sit behind two BatchNorms that amplify whatever error y
// carries.  4 independent chains per tile (k mod 4) keep the MFMA pipe from waiting on its own result.
typedef double d4 __attribute__((ext_vector_type(4)));
template <int K>
__device__ __forceinline__ void slab_gemm_xwt(const float* __restrict__ X, const float* __restrict__ W,
                                              const float* __restrict__ bias, int n, int col0, float (*ys)[HT_SLAB + 1]) {
    static_assert(K % 16 == 0, "16-wide k steps");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int ntiles = (n + 15) >> 4;
    d4 acc[4][4];
    const float* xrow[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = (d4){0.0, 0.0, 0.0, 0.0};
        const int row = (wv + 4 * i) * 16 + r16;
        ok[i] = row < n;
        xrow[i] = X + (size_t)(ok[i] ? row : 0) * K + 4 * q;
    }
    const float* wrow = W + (size_t)(col0 + r16) * K + 4 * q;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const f4 b = *reinterpret_cast<const f4*>(wrow + k0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (wv + 4 * i >= ntiles) continue;                 // wave-uniform
            f4 a = *reinterpret_cast<const f4*>(xrow[i] + k0);
            if (!ok[i]) a = (f4){0.f, 0.f, 0.f, 0.f};
            acc[i][0] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.x, (double)b.x, acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.y, (double)b.y, acc[i][1], 0, 0, 0);
            acc[i][2] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.z, (double)b.z, acc[i][2], 0, 0, 0);
            acc[i][3] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.w, (double)b.w, acc[i][3], 0, 0, 0);
        }
    }
    const double bc = (double)bias[col0 + r16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (wv + 4 * i >= ntiles) continue;
        const d4 s = (acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) ys[(wv + 4 * i) * 16 + q + 4 * e][r16] = (float)(s[e] + bc);
    }
}

// sum over the rows < n of f(row, col) for the block's 16 columns, in double, fixed order: 16 row groups, then their sum.
// Result for column c in out[c] (valid after the call for every thread).
template <typename F>
__device__ __forceinline__ void column_sums(F f, int n, double (*red)[HT_SLAB], double* out) {
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    double s = 0.0;
    for (int r = g; r < n; r += 16) s += f(r, c);
    red[g][c] = s;
    __syncthreads();
    if (threadIdx.x < HT_SLAB) {
        double t = red[0][threadIdx.x];
        for (int i = 1; i < 16; ++i) t += red[i][threadIdx.x];
        out[threadIdx.x] = t;
    }
    __syncthreads();
}

// One layer forward for a 16-column slab: y = X W^T + b, BatchNorm (TRAIN: batch statistics + running update; else the
// running statistics), ReLU, and - TRAIN - dropout.  grid = N / 16.
template <int K, int N, bool TRAIN>
__global__ __launch_bounds__(HT_THREADS) void ht_layer_fwd_kernel(
    const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar, float* __restrict__ Z,
    float* __restrict__ XH, float* __restrict__ istd_out, float* __restrict__ A, uint8_t* __restrict__ M, int n, uint32_t key,
    uint32_t thr, float dscale, float momentum, float eps) {
    __shared__ float ys[HT_MAX_N][HT_SLAB + 1];
    __shared__ double red[16][HT_SLAB];
    __shared__ double csum[HT_SLAB];
    __shared__ double cmean[HT_SLAB], cistd[HT_SLAB];
    const int t = threadIdx.x, col0 = blockIdx.x * HT_SLAB;
    slab_gemm_xwt<K>(X, W, bias, n, col0, ys);
    __syncthreads();
    if constexpr (TRAIN) {
        column_sums([&](int r, int c) { return (double)ys[r][c]; }, n, red, csum);
        if (t < HT_SLAB) cmean[t] = csum[t] / n;
        __syncthreads();
        column_sums([&](int r, int c) { const double d = (double)ys[r][c] - cmean[c]; return d * d; }, n, red, csum);
        if (t < HT_SLAB) {
            const double var = csum[t] / n;                      // biased: what normalises
            cistd[t] = 1.0 / sqrt(var + (double)eps);
            istd_out[col0 + t] = (float)cistd[t];
            const float unb = (float)(var * ((double)n / (double)(n - 1)));
            rmean[col0 + t] = (1.f - momentum) * rmean[col0 + t] + momentum * (float)cmean[t];
            rvar[col0 + t] = (1.f - momentum) * rvar[col0 + t] + momentum * unb;
        }
    } else {
        if (t < HT_SLAB) {
            cmean[t] = (double)rmean[col0 + t];
            cistd[t] = 1.0 / sqrt((double)rvar[col0 + t] + (double)eps);
        }
    }
    __syncthreads();
    // the epilogue of an element in double from its fp32 y, each stored value rounded once
    for (int e = t; e < n * HT_SLAB; e += HT_THREADS) {
        const int r = e >> 4, c = e & 15;
        const size_t o = (size_t)r * N + col0 + c;
        const double xh = ((double)ys[r][c] - cmean[c]) * cistd[c];
        const float z = (float)(xh * (double)gamma[col0 + c] + (double)beta[col0 + c]);
        float a = z > 0.f ? z : 0.f;
        if constexpr (TRAIN) {
            Z[o] = z;
            XH[o] = (float)xh;
            const bool k = mask_keep(key, (uint32_t)o, thr);
            M[o] = k ? 1 : 0;
            a = k ? a * dscale : 0.f;
        }
        A[o] = a;
    }
}

// ---------------------------------------------------------------------------------------------- loss
// FocalLoss.forward on one logit, in double: value and d/dz.  bce = max(z, 0) - z t + log1p(exp(-|z|)) (the form
// binary_cross_entropy_with_logits uses), p and 1 - p from the overflow-safe sigmoid, 1 - p_t = p (1 - t) + (1 - p) t.
__device__ __forceinline__ void focal_term(double z, double y, double gamma, double alpha, double ls, double* loss, double* dz) {
    const double t = ls > 0.0 ? y * (1.0 - ls) + 0.5 * ls : y;
    const double e = exp(-fabs(z));
    const double bce = fmax(z, 0.0) - z * t + log1p(e);
    const double p = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e), q = z >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
    const double u = p * (1.0 - t) + q * t;                     // 1 - p_t
    const double at = alpha * t + (1.0 - alpha) * (1.0 - t);
    double w = 1.0, dw = 0.0;                                    // u^gamma and d(u^gamma)/dz, du/dz = p q (1 - 2t)
    if (gamma != 0.0) {
        w = pow(u, gamma);
        dw = u > 0.0 ? gamma * pow(u, gamma - 1.0) * (p * q * (1.0 - 2.0 * t)) : 0.0;
    }
    *loss = at * w * bce;
    *dz = at * (dw * bce + w * (p - t));
}

// One block.  logits [n] = A2 . w3 + b3; train: the loss (unscaled, *loss_out), dlogit [n] = d(loss * loss_scale)/dz and
// the gradients of w3 / b3 added to gw3 / gb3.
__global__ __launch_bounds__(HT_THREADS) void ht_loss_kernel(const float* __restrict__ A2, const float* __restrict__ w3,
                                                             const float* __restrict__ b3, const float* __restrict__ ya,
                                                             const float* __restrict__ yb, float lam, float loss_scale,
                                                             float fgamma, float falpha, float fls, float* __restrict__ logits,
                                                             float* __restrict__ dlogit, float* __restrict__ loss_out,
                                                             float* __restrict__ gw3, float* __restrict__ gb3, int n, int train) {
    __shared__ float zl[HT_MAX_N];
    __shared__ double dl[HT_MAX_N], lv[HT_MAX_N];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const f4 w = *reinterpret_cast<const f4*>(w3 + 4 * lane);
    for (int r = wv; r < n; r += HT_THREADS / 64) {
        const f4 a = *reinterpret_cast<const f4*>(A2 + (size_t)r * HT_H2 + 4 * lane);
        // 256 exact products summed in double in a fixed order, rounded once (as the column reductions are)
        double s = ((double)a.x * (double)w.x + (double)a.y * (double)w.y) + ((double)a.z * (double)w.z + (double)a.w * (double)w.w);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) {
            const float z = (float)(s + (double)b3[0]);
            zl[r] = z;
            logits[r] = z;
        }
    }
    if (!train) return;
    __syncthreads();
    if (t < n) {
        double la, da, lb = 0.0, db = 0.0;
        focal_term((double)zl[t], (double)ya[t], (double)fgamma, (double)falpha, (double)fls, &la, &da);
        if (yb) {
            focal_term((double)zl[t], (double)yb[t], (double)fgamma, (double)falpha, (double)fls, &lb, &db);
            la = (double)lam * la + (1.0 - (double)lam) * lb;
            da = (double)lam * da + (1.0 - (double)lam) * db;
        }
        lv[t] = la;
        dl[t] = da * (double)loss_scale / n;
        dlogit[t] = (float)dl[t];
    }
    __syncthreads();
    {   // t = column of w3
        double s = 0.0;
        for (int r = 0; r < n; ++r) s += dl[r] * (double)A2[(size_t)r * HT_H2 + t];
        gw3[t] += (float)s;
    }
    if (t == 0) {
        double s = 0.0, g = 0.0;
        for (int r = 0; r < n; ++r) { s += lv[r]; g += dl[r]; }
        loss_out[0] = (float)(s / n);
        gb3[0] += (float)g;
    }
}

// ---------------------------------------------------------------------------------------------- backward
// Y slab [n][16] = dYn [n][NOUT] . Wn [NOUT][N] columns col0 .. col0 + 16 into LDS, on the exact fp32 MFMA: the backward's
// dY . W form (ht_layer_bwd_kernel, ht_dfeat_kernel).
template <int NOUT, int N>
__device__ __forceinline__ void slab_gemm_dyw(const float* __restrict__ dYn, const float* __restrict__ Wn, int n, int col0,
                                              float (*ys)[HT_SLAB + 1]) {
    const int t = threadIdx.x;
    const int lane = t & 63, wv = t >> 6, r16 = lane & 15, q = lane >> 4;
    const int ntiles = (n + 15) >> 4;
    f4 acc[4][4];                                            // 4 independent chains per tile (k mod 4), as the forward
    const float* arow[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = (f4){0.f, 0.f, 0.f, 0.f};
        const int row = (wv + 4 * i) * 16 + r16;
        ok[i] = row < n;
        arow[i] = dYn + (size_t)(ok[i] ? row : 0) * NOUT + 4 * q;
    }
    const float* wcol = Wn + (size_t)(4 * q) * N + col0 + r16;      // B[k][j] = Wn[k][col0 + j]
    for (int k0 = 0; k0 < NOUT; k0 += 16) {
        const float* wp = wcol + (size_t)k0 * N;
        const float b0 = wp[0], b1 = wp[N], b2 = wp[2 * N], b3 = wp[3 * N];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (wv + 4 * i >= ntiles) continue;
            f4 a = *reinterpret_cast<const f4*>(arow[i] + k0);
            if (!ok[i]) a = (f4){0.f, 0.f, 0.f, 0.f};
            acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc[i][1], 0, 0, 0);
            acc[i][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc[i][2], 0, 0, 0);
            acc[i][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc[i][3], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (wv + 4 * i >= ntiles) continue;
        const f4 s = (acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) ys[(wv + 4 * i) * 16 + q * 4 + e][r16] = s[e];
    }
}

// One layer backward for a 16-column slab.  Upstream gradient of the layer's output a = dropout(relu(z)):
//   LAST: da[r][c] = dlogit[r] w3[c]                       (Wn = w3, dYn = dlogit)
//   else: da = dYn [n][NOUT] . Wn [NOUT][N]                 (MFMA, reduction over NOUT)
// then dz = da * mask * dscale * [z > 0], the BatchNorm backward with the column sums in-block:
//   dgamma = sum dz xhat, dbeta = sum dz, dy = gamma istd (dz - dbeta / n - xhat dgamma / n)
// dY [n][N] out; dgamma / dbeta added to ggamma / gbeta.  grid = N / 16.
template <int NOUT, int N, bool LAST>
__global__ __launch_bounds__(HT_THREADS) void ht_layer_bwd_kernel(
    const float* __restrict__ dYn, const float* __restrict__ Wn, const float* __restrict__ Z, const float* __restrict__ XH,
    const float* __restrict__ istd, const float* __restrict__ gamma, const uint8_t* __restrict__ M, float dscale,
    float* __restrict__ dY, float* __restrict__ ggamma, float* __restrict__ gbeta, int n) {
    __shared__ float ys[HT_MAX_N][HT_SLAB + 1];
    __shared__ double red[16][HT_SLAB];
    __shared__ double sdz[HT_SLAB], sdx[HT_SLAB];
    const int t = threadIdx.x, col0 = blockIdx.x * HT_SLAB;
    if constexpr (LAST) {
        for (int e = t; e < n * HT_SLAB; e += HT_THREADS) ys[e >> 4][e & 15] = dYn[e >> 4] * Wn[col0 + (e & 15)];
    } else {
        slab_gemm_dyw<NOUT, N>(dYn, Wn, n, col0, ys);
    }
    __syncthreads();
    for (int e = t; e < n * HT_SLAB; e += HT_THREADS) {
        const int r = e >> 4, c = e & 15;
        const size_t o = (size_t)r * N + col0 + c;
        ys[r][c] = (M[o] && Z[o] > 0.f) ? ys[r][c] * dscale : 0.f;
    }
    __syncthreads();
    column_sums([&](int r, int c) { return (double)ys[r][c]; }, n, red, sdz);
    column_sums([&](int r, int c) { return (double)ys[r][c] * (double)XH[(size_t)r * N + col0 + c]; }, n, red, sdx);
    for (int e = t; e < n * HT_SLAB; e += HT_THREADS) {
        const int r = e >> 4, c = e & 15;
        const size_t o = (size_t)r * N + col0 + c;
        const float mdz = (float)(sdz[c] / n), mdx = (float)(sdx[c] / n);
        dY[o] = gamma[col0 + c] * istd[col0 + c] * ((ys[r][c] - mdz) - XH[o] * mdx);
    }
    if (t < HT_SLAB) {
        ggamma[col0 + t] += (float)sdx[t];
        gbeta[col0 + t] += (float)sdz[t];
    }
}

// The gradient with respect to the pooled features, for the conv stage (head_train_conv.hip): dfeat [n][1280] =
// (dY1 [n][512] . W1 [512][1280]) * mask0 * dscale0 - layer 0's dropout has no BatchNorm or ReLU behind it.  grid = 1280 / 16.
__global__ __launch_bounds__(HT_THREADS) void ht_dfeat_kernel(const float* __restrict__ dY1, const float* __restrict__ W1,
                                                              const uint8_t* __restrict__ M0, float dscale,
                                                              float* __restrict__ dfeat, int n) {
    __shared__ float ys[HT_MAX_N][HT_SLAB + 1];
    const int t = threadIdx.x, col0 = blockIdx.x * HT_SLAB;
    slab_gemm_dyw<HT_H1, HT_IN>(dY1, W1, n, col0, ys);
    __syncthreads();
    for (int e = t; e < n * HT_SLAB; e += HT_THREADS) {
        const int r = e >> 4, c = e & 15;
        const size_t o = (size_t)r * HT_IN + col0 + c;
        dfeat[o] = M0[o] ? ys[r][c] * dscale : 0.f;
    }
}

// G [NO][NI] += dY [n][NO]^T . X [n][NI] (reduction over the n rows, masked past n).  A wave owns a 16 x 64 strip:
// grid (ceil(NI / 256), NO / 16), NI % 16 == 0.
__global__ __launch_bounds__(HT_THREADS) void ht_wgrad_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                              float* __restrict__ G, int n, int NO, int NI) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int o0 = blockIdx.y * 16, i0 = (blockIdx.x * 4 + wv) * 64;
    if (i0 >= NI) return;                                       // wave-uniform
    const int nj = min(4, (NI - i0) / 16);
    f4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < n; k0 += 4) {
        const int row = k0 + q;
        const bool ok = row < n;
        const size_t rr = ok ? (size_t)row : 0;
        float a = dY[rr * NO + o0 + r16];                       // A[m = o][k = row]
        if (!ok) a = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nj) continue;
            float b = X[rr * NI + i0 + j * 16 + r16];           // B[k = row][j = i]
            if (!ok) b = 0.f;
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= nj) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) G[(size_t)(o0 + q * 4 + e) * NI + i0 + j * 16 + r16] += acc[j][e];
    }
}

// ---------------------------------------------------------------------------------------------- apply
__device__ __forceinline__ double block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = HT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(HT_THREADS) void ht_sumsq_kernel(const float* __restrict__ g, int count, double* __restrict__ partial) {
    __shared__ double sh[HT_THREADS];
    double s = 0.0;
    for (int i = blockIdx.x * HT_THREADS + threadIdx.x; i < count; i += gridDim.x * HT_THREADS) s += (double)g[i] * (double)g[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// clip_grad_norm_ + torch.optim.AdamW (single-tensor path, in its order) + EMAModel.update + zero_grad, one element per thread.
// decay_mul = 1 - lr wd, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t): computed on the host in double.
// The squared norm is the sum of the arenas' partials, added entry by entry in the table's order (head, conv, block 15, 14,
// 13, 12, 11; null entries left out): one norm over every group.
__global__ __launch_bounds__(HT_THREADS) void ht_adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, float* __restrict__ ema, int count,
                                                              NormParts parts, float clip_norm,
                                                              float decay_mul, float w1, float beta2, float w2, float step_size,
                                                              float bc2_sqrt, float eps, float ema_decay, float ema_w,
                                                              float* __restrict__ norm_out) {
    __shared__ double sh[HT_THREADS];
    static_assert(NORM_BLOCKS == HT_THREADS, "one partial per thread");
    double mine = parts.p[0][threadIdx.x];
#pragma unroll
    for (int a = 1; a < HT_ARENAS; ++a)
        if (parts.p[a]) mine += parts.p[a][threadIdx.x];
    const float norm = (float)sqrt(block_sum(mine, sh));
    const float coef = fminf(clip_norm / (norm + 1e-6f), 1.f);
    const int i = blockIdx.x * HT_THREADS + threadIdx.x;
    if (i == 0) norm_out[0] = norm;
    if (i >= count) return;
    const float gi = g[i] * coef;
    float pi = p[i] * decay_mul;
    const float mi = m[i] + (gi - m[i]) * w1;                   // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = v[i] * beta2 + (w2 * gi) * gi;             // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi - step_size * (mi / denom);                         // param.addcdiv_(exp_avg, denom, value = -step_size)
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    ema[i] = ema[i] * ema_decay + ema_w * pi;
    g[i] = 0.f;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- host
namespace dfd {

// HeadTrainState: head_train_state.h
void head_train_destroy(dfd_handle* h) {
    HeadTrainState* S = h->head_train;
    if (!S) return;
    headblock_destroy(S);
    headconv_destroy(S);
    if (S->pool) hipFree(S->pool);
    delete S;
    h->head_train = nullptr;
}

void head_train_launch_sumsq(hipStream_t s, const float* g, int count, double* partial) {
    hipLaunchKernelGGL(ht_sumsq_kernel, dim3(NORM_BLOCKS), dim3(HT_THREADS), 0, s, g, count, partial);
}

NormParts head_train_norm_parts(HeadTrainState* S) {
    NormParts parts{};
    parts.p[0] = S->partial;
    parts.p[1] = S->conv ? headconv_partial(S) : nullptr;
    for (int k = 0; k < HT_STAGES; ++k) parts.p[2 + k] = headblock_partial(S, k);
    return parts;
}

void head_train_launch_adamw(hipStream_t s, float* p, float* g, float* m, float* v, float* ema, int count, const NormParts& parts,
                             const dfd_head_config& c, double lr, double t, float* norm_out) {
    const double bc1 = 1.0 - std::pow((double)c.beta1, t), bc2 = 1.0 - std::pow((double)c.beta2, t);
    hipLaunchKernelGGL(ht_adamw_kernel, dim3((count + HT_THREADS - 1) / HT_THREADS), dim3(HT_THREADS), 0, s, p, g, m, v, ema, count,
                       parts, c.clip_norm, (float)(1.0 - lr * (double)c.weight_decay), (float)(1.0 - (double)c.beta1),
                       c.beta2, (float)(1.0 - (double)c.beta2), (float)(lr / bc1), (float)std::sqrt(bc2), c.eps, c.ema_decay,
                       (float)(1.0 - (double)c.ema_decay), norm_out);
}

}  // namespace dfd

namespace {

struct Field { float* dfd_head_params::*ptr; int off, count; };
const Field kTrainable[] = {
    {&dfd_head_params::w1, O_W1, HT_H1 * HT_IN}, {&dfd_head_params::b1, O_B1, HT_H1}, {&dfd_head_params::g1, O_G1, HT_H1},
    {&dfd_head_params::be1, O_BE1, HT_H1},       {&dfd_head_params::w2, O_W2, HT_H2 * HT_H1}, {&dfd_head_params::b2, O_B2, HT_H2},
    {&dfd_head_params::g2, O_G2, HT_H2},         {&dfd_head_params::be2, O_BE2, HT_H2},  {&dfd_head_params::w3, O_W3, HT_H2},
    {&dfd_head_params::b3, O_B3, 1},
};

HeadTrainState* open_state(dfd_handle* h, const char* who, int* rc) {
    if (!h) { *rc = DFD_ERR_ARG; return nullptr; }
    if (!h->head_train) { *rc = fail(h, DFD_ERR_ARG, "%s: no trainer is open on this handle (dfd_head_train_begin)", who); return nullptr; }
    *rc = DFD_OK;
    return h->head_train;
}

bool params_complete(const dfd_head_params* p, bool stats) {
    for (const Field& f : kTrainable)
        if (!(p->*f.ptr)) return false;
    return !stats || (p->rm1 && p->rv1 && p->rm2 && p->rv2);
}

// forward on `n` rows of S->feat with the parameters at `P`; train: batch statistics, dropout of this accumulate
int forward(dfd_handle* h, HeadTrainState* S, const float* P, int n, bool train) {
    hipStream_t s = h->stream;
    const float mom = S->cfg.bn_momentum, eps = 1e-5f;          // b0_arch.BN_EPS_HEAD
    if (train) {
        const uint32_t k0 = mask_key(S->cfg.seed, S->counter, 0), k1 = mask_key(S->cfg.seed, S->counter, 1),
                       k2 = mask_key(S->cfg.seed, S->counter, 2);
        const int count = n * HT_IN;
        hipLaunchKernelGGL(ht_dropout0_kernel, dim3((count + HT_THREADS - 1) / HT_THREADS), dim3(HT_THREADS), 0, s, S->feat, S->x0,
                           S->mask0, count, k0, S->thr[0], S->dscale[0]);
        hipLaunchKernelGGL((ht_layer_fwd_kernel<HT_IN, HT_H1, true>), dim3(HT_H1 / HT_SLAB), dim3(HT_THREADS), 0, s, S->x0, P + O_W1,
                           P + O_B1, P + O_G1, P + O_BE1, S->rm1, S->rv1, S->z1, S->xh1, S->istd1, S->a1, S->mask1, n, k1,
                           S->thr[1], S->dscale[1], mom, eps);
        hipLaunchKernelGGL((ht_layer_fwd_kernel<HT_H1, HT_H2, true>), dim3(HT_H2 / HT_SLAB), dim3(HT_THREADS), 0, s, S->a1, P + O_W2,
                           P + O_B2, P + O_G2, P + O_BE2, S->rm2, S->rv2, S->z2, S->xh2, S->istd2, S->a2, S->mask2, n, k2,
                           S->thr[2], S->dscale[2], mom, eps);
    } else {
        hipLaunchKernelGGL((ht_layer_fwd_kernel<HT_IN, HT_H1, false>), dim3(HT_H1 / HT_SLAB), dim3(HT_THREADS), 0, s, S->feat,
                           P + O_W1, P + O_B1, P + O_G1, P + O_BE1, S->rm1, S->rv1, nullptr, nullptr, nullptr, S->a1, nullptr, n,
                           0u, 0u, 1.f, mom, eps);
        hipLaunchKernelGGL((ht_layer_fwd_kernel<HT_H1, HT_H2, false>), dim3(HT_H2 / HT_SLAB), dim3(HT_THREADS), 0, s, S->a1,
                           P + O_W2, P + O_B2, P + O_G2, P + O_BE2, S->rm2, S->rv2, nullptr, nullptr, nullptr, S->a2, nullptr, n,
                           0u, 0u, 1.f, mom, eps);
    }
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

}  // namespace

namespace dfd {

int head_train_step(dfd_handle* h, HeadTrainState* S, int n, const float* labels_a, const float* labels_b, float lam,
                    float loss_scale, float* dfeat) {
    hipStream_t s = h->stream;
    int rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(S->ya, labels_a, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (labels_b) DFD_HIP_TRY(h, hipMemcpyAsync(S->yb, labels_b, (size_t)n * 4, hipMemcpyHostToDevice, s));
    const float* P = S->param;
    float* G = S->grad;
    if ((rc = forward(h, S, P, n, true))) return rc;
    hipLaunchKernelGGL(ht_loss_kernel, dim3(1), dim3(HT_THREADS), 0, s, S->a2, P + O_W3, P + O_B3, S->ya, labels_b ? S->yb : nullptr, lam,
                       loss_scale, S->cfg.focal_gamma, S->cfg.focal_alpha, S->cfg.label_smoothing, S->logits, S->dlogit, S->scalars,
                       G + O_W3, G + O_B3, n, 1);
    hipLaunchKernelGGL((ht_layer_bwd_kernel<1, HT_H2, true>), dim3(HT_H2 / HT_SLAB), dim3(HT_THREADS), 0, s, S->dlogit, P + O_W3, S->z2,
                       S->xh2, S->istd2, P + O_G2, S->mask2, S->dscale[2], S->dy2, G + O_G2, G + O_BE2, n);
    hipLaunchKernelGGL((ht_layer_bwd_kernel<HT_H2, HT_H1, false>), dim3(HT_H1 / HT_SLAB), dim3(HT_THREADS), 0, s, S->dy2, P + O_W2, S->z1,
                       S->xh1, S->istd1, P + O_G1, S->mask1, S->dscale[1], S->dy1, G + O_G1, G + O_BE1, n);
    if (dfeat)
        hipLaunchKernelGGL(ht_dfeat_kernel, dim3(HT_IN / HT_SLAB), dim3(HT_THREADS), 0, s, S->dy1, P + O_W1, S->mask0, S->dscale[0], dfeat, n);
    hipLaunchKernelGGL(ht_wgrad_kernel, dim3((HT_H1 + 255) / 256, HT_H2 / 16), dim3(HT_THREADS), 0, s, S->dy2, S->a1, G + O_W2, n, HT_H2, HT_H1);
    hipLaunchKernelGGL(ht_wgrad_kernel, dim3((HT_IN + 255) / 256, HT_H1 / 16), dim3(HT_THREADS), 0, s, S->dy1, S->x0, G + O_W1, n, HT_H1, HT_IN);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

int head_train_eval_step(dfd_handle* h, HeadTrainState* S, const float* P, int n) {
    int rc;
    if ((rc = forward(h, S, P, n, false))) return rc;
    hipLaunchKernelGGL(ht_loss_kernel, dim3(1), dim3(HT_THREADS), 0, h->stream, S->a2, P + O_W3, P + O_B3, nullptr, nullptr, 1.f, 1.f, 0.f,
                       0.f, 0.f, S->logits, nullptr, nullptr, nullptr, nullptr, n, 0);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

}  // namespace dfd

extern "C" {

void dfd_head_config_default(dfd_head_config* c) {
    if (!c) return;
    c->max_n = 32;
    c->seed = 0;
    c->dropout = 0.5f;
    c->beta1 = 0.9f;
    c->beta2 = 0.999f;
    c->eps = 1e-8f;
    c->weight_decay = 0.05f;
    c->focal_gamma = 2.0f;
    c->focal_alpha = 0.25f;
    c->label_smoothing = 0.1f;
    c->clip_norm = 1.0f;
    c->ema_decay = 0.999f;
    c->bn_momentum = 0.1f;
}

int dfd_head_train_begin(dfd_handle* h, const dfd_head_params* init, const dfd_head_config* cfg) {
    if (!h) return DFD_ERR_ARG;
    if (h->head_train) return fail(h, DFD_ERR_ARG, "head_train_begin: a trainer is already open on this handle");
    if (!init || !cfg || !params_complete(init, true)) return fail(h, DFD_ERR_ARG, "head_train_begin: null parameters or config");
    if (cfg->max_n < 2 || cfg->max_n > HT_MAX_N) return fail(h, DFD_ERR_ARG, "head_train_begin: max_n %d outside 2..%d", cfg->max_n, HT_MAX_N);
    if (!(cfg->dropout >= 0.f && cfg->dropout < 1.f)) return fail(h, DFD_ERR_ARG, "head_train_begin: dropout %g outside [0, 1)", (double)cfg->dropout);
    if (!(cfg->beta1 >= 0.f && cfg->beta1 < 1.f && cfg->beta2 >= 0.f && cfg->beta2 < 1.f && cfg->eps > 0.f && cfg->clip_norm > 0.f &&
          cfg->ema_decay >= 0.f && cfg->ema_decay <= 1.f && cfg->bn_momentum >= 0.f && cfg->bn_momentum <= 1.f &&
          cfg->label_smoothing >= 0.f && cfg->label_smoothing <= 1.f && cfg->focal_gamma >= 0.f))
        return fail(h, DFD_ERR_ARG, "head_train_begin: optimizer / loss setting out of range");
    {   // every float field is a finite number (eps, clip_norm and focal_gamma have no upper end above, weight_decay and
        // focal_alpha no range at all); torch.optim.AdamW refuses a negative weight_decay, FocalLoss takes any alpha
        const struct { const char* name; float v; } fields[] = {
            {"dropout", cfg->dropout}, {"beta1", cfg->beta1}, {"beta2", cfg->beta2}, {"eps", cfg->eps},
            {"weight_decay", cfg->weight_decay}, {"focal_gamma", cfg->focal_gamma}, {"focal_alpha", cfg->focal_alpha},
            {"label_smoothing", cfg->label_smoothing}, {"clip_norm", cfg->clip_norm}, {"ema_decay", cfg->ema_decay},
            {"bn_momentum", cfg->bn_momentum}};
        for (const auto& f : fields)
            if (!std::isfinite(f.v)) return fail(h, DFD_ERR_ARG, "head_train_begin: %s %g is not a finite number", f.name, (double)f.v);
        if (cfg->weight_decay < 0.f) return fail(h, DFD_ERR_ARG, "head_train_begin: weight_decay %g is negative", (double)cfg->weight_decay);
    }
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadTrainState* S = new (std::nothrow) HeadTrainState();
    if (!S) return fail(h, DFD_ERR_CAPACITY, "head_train_begin: out of host memory");
    S->cfg = *cfg;
    S->max_n = cfg->max_n;
    const double rates[3] = {1.0, 0.7, 0.5};
    for (int l = 0; l < 3; ++l) {
        S->p[l] = rates[l] * (double)cfg->dropout;
        S->thr[l] = (uint32_t)(unsigned long long)(S->p[l] * 4294967296.0);
        S->dscale[l] = (float)(1.0 / (1.0 - S->p[l]));
    }
    // one allocation, 256-byte slots
    const size_t mn = (size_t)S->max_n;
    struct Slot { void** p; size_t bytes; };
    const Slot slots[] = {
        {(void**)&S->param, (size_t)HT_COUNT * 4}, {(void**)&S->grad, (size_t)HT_COUNT * 4}, {(void**)&S->m, (size_t)HT_COUNT * 4},
        {(void**)&S->v, (size_t)HT_COUNT * 4},     {(void**)&S->ema, (size_t)HT_COUNT * 4},
        {(void**)&S->rm1, HT_H1 * 4}, {(void**)&S->rv1, HT_H1 * 4}, {(void**)&S->rm2, HT_H2 * 4}, {(void**)&S->rv2, HT_H2 * 4},
        {(void**)&S->feat, mn * HT_IN * 4}, {(void**)&S->x0, mn * HT_IN * 4},
        {(void**)&S->z1, mn * HT_H1 * 4}, {(void**)&S->xh1, mn * HT_H1 * 4}, {(void**)&S->a1, mn * HT_H1 * 4}, {(void**)&S->dy1, mn * HT_H1 * 4},
        {(void**)&S->z2, mn * HT_H2 * 4}, {(void**)&S->xh2, mn * HT_H2 * 4}, {(void**)&S->a2, mn * HT_H2 * 4}, {(void**)&S->dy2, mn * HT_H2 * 4},
        {(void**)&S->istd1, HT_H1 * 4}, {(void**)&S->istd2, HT_H2 * 4}, {(void**)&S->logits, mn * 4}, {(void**)&S->dlogit, mn * 4},
        {(void**)&S->ya, mn * 4}, {(void**)&S->yb, mn * 4}, {(void**)&S->scalars, 16}, {(void**)&S->partial, NORM_BLOCKS * 8},
        {(void**)&S->mask0, mn * HT_IN}, {(void**)&S->mask1, mn * HT_H1}, {(void**)&S->mask2, mn * HT_H2},
    };
    size_t total = 0;
    for (const Slot& sl : slots) total += (sl.bytes + 255) / 256 * 256;
    if (hipMalloc(&S->pool, total) != hipSuccess) {
        delete S;
        return fail(h, DFD_ERR_HIP, "head_train_begin: hipMalloc of %zu bytes failed", total);
    }
    size_t off = 0;
    for (const Slot& sl : slots) {
        *sl.p = static_cast<char*>(S->pool) + off;
        off += (sl.bytes + 255) / 256 * 256;
    }
    h->head_train = S;
    auto bail = [&](hipError_t e, const char* what) {
        head_train_destroy(h);
        return fail(h, DFD_ERR_HIP, "head_train_begin: %s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMemsetAsync(S->pool, 0, total, h->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
    for (const Field& f : kTrainable)
        if ((e = hipMemcpyAsync(S->param + f.off, init->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "parameter upload");
    const struct { float* d; const float* s; int c; } stats[] = {{S->rm1, init->rm1, HT_H1}, {S->rv1, init->rv1, HT_H1},
                                                                 {S->rm2, init->rm2, HT_H2}, {S->rv2, init->rv2, HT_H2}};
    for (const auto& st : stats)
        if ((e = hipMemcpyAsync(st.d, st.s, (size_t)st.c * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return bail(e, "statistics upload");
    if ((e = hipMemcpyAsync(S->ema, S->param, (size_t)HT_COUNT * 4, hipMemcpyDeviceToDevice, h->stream)) != hipSuccess) return bail(e, "shadow copy");
    if ((e = stream_sync(h)) != hipSuccess) return bail(e, "stream wait");
    return DFD_OK;
}

int dfd_head_train_accumulate(dfd_handle* h, const float* feat, int n, const float* labels_a, const float* labels_b, float lam,
                              float loss_scale, float* loss_out, float* logits_out) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_accumulate", &rc);
    if (!S) return rc;
    if (S->conv) return fail(h, DFD_ERR_ARG, "head_train_accumulate: the conv stage is unfrozen, rows are trunk rows (dfd_head_train_accumulate_trunk)");
    if (!feat || !labels_a || !loss_out) return fail(h, DFD_ERR_ARG, "head_train_accumulate: null pointer");
    if (n < 2) return fail(h, DFD_ERR_ARG, "head_train_accumulate: %d rows; batch statistics need at least 2", n);
    if (n > S->max_n) return fail(h, DFD_ERR_ARG, "head_train_accumulate: %d rows exceed the trainer's max_n %d", n, S->max_n);
    if (!head_train_mix_ok(lam, loss_scale))
        return fail(h, DFD_ERR_ARG, "head_train_accumulate: lam %g outside [0, 1] or loss_scale %g not a number", (double)lam, (double)loss_scale);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DFD_HIP_TRY(h, hipMemcpyAsync(S->feat, feat, (size_t)n * HT_IN * 4, hipMemcpyHostToDevice, s));
    if ((rc = head_train_step(h, S, n, labels_a, labels_b, lam, loss_scale, nullptr))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(loss_out, S->scalars, 4, hipMemcpyDeviceToHost, s));
    if (logits_out) DFD_HIP_TRY(h, hipMemcpyAsync(logits_out, S->logits, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));
    S->last_n = n;
    ++S->counter;
    return DFD_OK;
}

int dfd_head_train_apply(dfd_handle* h, float lr, float* grad_norm_out) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_apply", &rc);
    if (!S) return rc;
    if (!(lr >= 0.f)) return fail(h, DFD_ERR_ARG, "head_train_apply: learning rate %g", (double)lr);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const double t = (double)(S->step + 1);
    head_train_launch_sumsq(h->stream, S->grad, HT_COUNT, S->partial);
    if (S->conv) headconv_sumsq(h, S);                                          // one norm over all groups
    for (int k = 0; k < HT_STAGES && S->stage[k]; ++k) headblock_sumsq(h, S, k);
    head_train_launch_adamw(h->stream, S->param, S->grad, S->m, S->v, S->ema, HT_COUNT, head_train_norm_parts(S), S->cfg, (double)lr, t,
                            S->scalars + 1);
    if (S->conv) headconv_adamw(h, S, (double)lr, t);
    if (S->stage[0]) headblock_adamw(h, S, (double)lr, t);
    DFD_HIP_TRY(h, hipGetLastError());
    ++S->step;
    if (grad_norm_out) {
        DFD_HIP_TRY(h, hipMemcpyAsync(grad_norm_out, S->scalars + 1, 4, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, stream_sync(h));
    }
    return DFD_OK;
}

int dfd_head_train_eval(dfd_handle* h, const float* feat, int n, int use_ema, float* logits_out) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_eval", &rc);
    if (!S) return rc;
    if (S->conv) return fail(h, DFD_ERR_ARG, "head_train_eval: the conv stage is unfrozen, rows are trunk rows (dfd_head_train_eval_trunk)");
    if (!feat || !logits_out) return fail(h, DFD_ERR_ARG, "head_train_eval: null pointer");
    if (n < 1 || n > S->max_n) return fail(h, DFD_ERR_ARG, "head_train_eval: %d rows outside 1..%d", n, S->max_n);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const float* P = use_ema ? S->ema : S->param;
    DFD_HIP_TRY(h, hipMemcpyAsync(S->feat, feat, (size_t)n * HT_IN * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = head_train_eval_step(h, S, P, n))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(logits_out, S->logits, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_head_train_export(dfd_handle* h, int use_ema, dfd_head_params* out) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_export", &rc);
    if (!S) return rc;
    if (!out || !params_complete(out, true)) return fail(h, DFD_ERR_ARG, "head_train_export: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const float* P = use_ema ? S->ema : S->param;
    for (const Field& f : kTrainable)
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*f.ptr, P + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(out->rm1, S->rm1, HT_H1 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(out->rv1, S->rv1, HT_H1 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(out->rm2, S->rm2, HT_H2 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(out->rv2, S->rv2, HT_H2 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_head_train_grads(dfd_handle* h, dfd_head_params* io, int set) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_grads", &rc);
    if (!S) return rc;
    if (!io || !params_complete(io, false)) return fail(h, DFD_ERR_ARG, "head_train_grads: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    for (const Field& f : kTrainable) {
        if (set) DFD_HIP_TRY(h, hipMemcpyAsync(S->grad + f.off, io->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream));
        else DFD_HIP_TRY(h, hipMemcpyAsync(io->*f.ptr, S->grad + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_head_train_tap(dfd_handle* h, const char* name, float* out, size_t capacity) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_tap", &rc);
    if (!S) return rc;
    if (!name || !out) return fail(h, DFD_ERR_ARG, "head_train_tap: null pointer");
    if (S->last_n == 0) return fail(h, DFD_ERR_ARG, "head_train_tap: no accumulate has run yet");
    if (!strcmp(name, "cfeat") || !strcmp(name, "dfeat") || !strcmp(name, "cz")) return headconv_tap(h, S, name, out, capacity);
    if (name[0] == 'b' && name[1] == '1' && name[2] >= '1' && name[2] <= '5' && name[3] == '.') return headblock_tap(h, S, name, out, capacity);
    const uint8_t* mask = nullptr;
    const float* act = nullptr;
    int width = 0;
    if (!strcmp(name, "mask0")) { mask = S->mask0; width = HT_IN; }
    else if (!strcmp(name, "mask1")) { mask = S->mask1; width = HT_H1; }
    else if (!strcmp(name, "mask2")) { mask = S->mask2; width = HT_H2; }
    else if (!strcmp(name, "z1")) { act = S->z1; width = HT_H1; }
    else if (!strcmp(name, "z2")) { act = S->z2; width = HT_H2; }
    else if (!strcmp(name, "x0")) { act = S->x0; width = HT_IN; }
    else if (!strcmp(name, "a1")) { act = S->a1; width = HT_H1; }
    else if (!strcmp(name, "a2")) { act = S->a2; width = HT_H2; }
    else return fail(h, DFD_ERR_ARG, "head_train_tap: unknown tap '%s'", name);
    const size_t count = (size_t)S->last_n * width;
    if (capacity < count) return fail(h, DFD_ERR_ARG, "head_train_tap: '%s' holds %zu floats, capacity %zu", name, count, capacity);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, stream_sync(h));
    if (act) {
        DFD_HIP_TRY(h, hipMemcpy(out, act, count * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint8_t> bytes(count);
        DFD_HIP_TRY(h, hipMemcpy(bytes.data(), mask, count, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < count; ++i) out[i] = bytes[i] ? 1.f : 0.f;
    }
    return DFD_OK;
}

int dfd_head_train_commit(dfd_handle* h, int use_ema) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_commit", &rc);
    if (!S) return rc;
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    if (S->stage[0] && (rc = headblock_commit(h, S, use_ema))) return rc;      // the blocks' BatchNorms folded, b15.* .. b11.*
    if (S->conv && (rc = headconv_commit(h, S, use_ema))) return rc;           // _bn1 folded into _conv_head, head.w / head.b
    std::vector<float> P(HT_COUNT), rm1(HT_H1), rv1(HT_H1), rm2(HT_H2), rv2(HT_H2);
    DFD_HIP_TRY(h, hipMemcpyAsync(P.data(), use_ema ? S->ema : S->param, (size_t)HT_COUNT * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(rm1.data(), S->rm1, HT_H1 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(rv1.data(), S->rv1, HT_H1 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(rm2.data(), S->rm2, HT_H2 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(rv2.data(), S->rv2, HT_H2 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    // weights._fold: a = g / sqrt(var + eps); w' = w a; b' = b a + (beta - mu a), float64, rounded once
    auto fold = [&](int ow, int ob, int og, int obe, const std::vector<float>& mu, const std::vector<float>& var, int N, int K,
                    std::vector<float>& w, std::vector<float>& b) {
        w.resize((size_t)N * K);
        b.resize(N);
        for (int o = 0; o < N; ++o) {
            const double a = (double)P[og + o] / std::sqrt((double)var[o] + 1e-5);
            for (int k = 0; k < K; ++k) w[(size_t)o * K + k] = (float)((double)P[ow + (size_t)o * K + k] * a);
            b[o] = (float)((double)P[ob + o] * a + ((double)P[obe + o] - (double)mu[o] * a));
        }
    };
    std::vector<float> w1, b1, w2, b2;
    fold(O_W1, O_B1, O_G1, O_BE1, rm1, rv1, HT_H1, HT_IN, w1, b1);
    fold(O_W2, O_B2, O_G2, O_BE2, rm2, rv2, HT_H2, HT_H1, w2, b2);
    const B0Plan& B = h->b0;
    const struct { const float* dst; const float* src; size_t count; } ups[] = {
        {B.fc1_w, w1.data(), w1.size()}, {B.fc1_b, b1.data(), b1.size()}, {B.fc2_w, w2.data(), w2.size()},
        {B.fc2_b, b2.data(), b2.size()}, {B.fc3_w, P.data() + O_W3, (size_t)HT_H2}, {B.fc3_b, P.data() + O_B3, 1}};
    for (const auto& u : ups)
        DFD_HIP_TRY(h, hipMemcpyAsync(const_cast<float*>(u.dst), u.src, u.count * 4, hipMemcpyHostToDevice, h->stream));
    // the three-plane bf16 splits the split GEMM multiplies with are cached by weight pointer: rebuild them in place
    const struct { const float* w; int N, K; } splits[] = {{B.fc1_w, HT_H1, HT_IN}, {B.fc2_w, HT_H2, HT_H1}};
    for (const auto& sp : splits) {
        auto it = h->wsplit.find(sp.w);
        if (it != h->wsplit.end()) launch_split_weights(sp.w, it->second, sp.N, sp.K, h->stream, false);
    }
    DFD_HIP_TRY(h, hipGetLastError());
    DFD_HIP_TRY(h, stream_sync(h));                             // the host staging above lives until here
    return DFD_OK;
}

int dfd_head_train_end(dfd_handle* h) {
    int rc;
    HeadTrainState* S = open_state(h, "head_train_end", &rc);
    if (!S) return rc;
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, stream_sync(h));
    head_train_destroy(h);
    return DFD_OK;
}

}  // extern "C"

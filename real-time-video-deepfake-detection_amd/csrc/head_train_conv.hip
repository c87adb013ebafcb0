// The conv stage of the head trainer: net._conv_head (320 -> 1280, 1 x 1, no bias), net._bn1 in train mode, swish and the
// 7 x 7 average pool, trained together with the MLP head (reference train.py:863-924: the unfrozen backbone is a second
// AdamW group at lr_scale x lr).  Input: block 15's output, "trunk rows" [n][49][320] fp32 NHWC (dfd_extract_trunk); with
// m = 49 n rows
//   Z = X W^T                                   [m][1280]   hc_gemm_fwd_kernel
//   mean, biased variance per channel over m    two passes  hc_colstat_kernel<0 / 1> + hc_finalize_kernel<0 / 1>
//   y = (Z - mean) istd gamma + beta, a = y sigmoid(y), feat = mean over the 49 positions   hc_swish_pool_kernel
// then head_train.hip's forward, loss and backward on feat (head_train_step), which also returns dfeat = dLoss / dfeat, and
//   dA = dfeat / 49, dy = dA s (1 + y (1 - s)), sum dy and sum dy xhat per channel   hc_colstat_kernel<2> + hc_finalize_kernel<2>
//   dW += dZ^T X, dZ = gamma istd (dy - sum dy / m - xhat sum dy xhat / m)           hc_wgrad_kernel + hc_wreduce_kernel
// dZ is never stored: the weight-gradient kernel forms its A operand from Z, the channel's constants and dfeat as it loads.
// Block 15 is frozen, so there is no gradient with respect to X.
//
// Both GEMMs run on the fp64 MFMA (v_mfma_f64_16x16x4_f64, the form of head_train.hip's forward): products of floats are
// exact in double and the sums carry 53 bits, so Z is the dot product rounded once to fp32 and a weight gradient is its
// 12544-row sum rounded once when it is added to the gradient buffer - whatever the split of the rows.  BatchNorm divides
// by the channel's standard deviation and the loss sits behind three BatchNorms; the exact fp32 MFMA's sequential fp32
// sums over 320 (forward) and up to 12544 (weight gradient) terms would be the largest error of the step.  Per element
// everything else (normalisation, swish, its derivative) is computed in double from the stored fp32 Z and rounded once.
//
// Every reduction has a fixed order and no atomics: column statistics are partial sums over 256-row chunks added in chunk
// order, the weight gradient partial sums over 512-row chunks added in chunk order, all in double.  Rows past m are masked
// to zero at the load and never read.  Built with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "b0_kernels.h"
#include "dfd_common.h"
#include "head_train_gemm.h"
#include "head_train_state.h"
#include "kernel_util.h"

using namespace dfd;

namespace {

constexpr int HC_K = 320, HC_N = 1280, HC_HW = 49, HC_ROW = HC_HW * HC_K;
constexpr int CO_W = 0, CO_G = HC_N * HC_K, CO_BE = CO_G + HC_N, CV_COUNT = CO_BE + HC_N;   // the conv group's arena
constexpr int HC_FWD_COLS = 80;           // columns of one block of the forward GEMM: 5 tiles per wave, 1280 = 16 x 80
constexpr int HC_STAT_ROWS = 256;         // rows of one partial sum of a channel statistic
constexpr int HC_WG_ROWS = 512;           // rows of one partial weight gradient
constexpr int HC_WG_COLS = 160;           // input channels of one wave of the weight gradient: 10 tiles, 320 = 2 x 160
static_assert(HC_N % HC_FWD_COLS == 0 && HC_FWD_COLS % 16 == 0 && HC_K % 16 == 0 && HC_K % HC_WG_COLS == 0, "tiles");
static_assert(HC_N == HT_IN, "the pooled row is the head's input");

typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------- forward
// Z [m][1280] = X [m][320] . W [1280][320]^T.  grid (16, ceil(m / 64)); a wave owns 16 rows x 80 columns.  Lane (r, q)
// loads 4 consecutive k of row r of X and of 5 rows of W (16-byte loads) and issues 4 MFMAs per tile on them, both
// operands with the same k per lane; the 5 tiles are 5 independent chains.  D: col = lane & 15, row = (lane >> 4) + 4 reg.
__global__ __launch_bounds__(HT_THREADS) void hc_gemm_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                                 float* __restrict__ Z, int m) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.y * 4 + wv) * 16, col0 = blockIdx.x * HC_FWD_COLS;
    if (row0 >= m) return;                                      // wave-uniform
    constexpr int J = HC_FWD_COLS / 16;
    const int row = row0 + r16;
    const bool ok = row < m;
    const float* xrow = X + (size_t)(ok ? row : 0) * HC_K + 4 * q;
    const float* wrow = W + (size_t)(col0 + r16) * HC_K + 4 * q;
    d4 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < HC_K; k0 += 16) {
        f4 a = *reinterpret_cast<const f4*>(xrow + k0);
        if (!ok) a = (f4){0.f, 0.f, 0.f, 0.f};
        f4 b[J];
#pragma unroll
        for (int j = 0; j < J; ++j) b[j] = *reinterpret_cast<const f4*>(wrow + (size_t)j * 16 * HC_K + k0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[kk], (double)b[j][kk], acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = row0 + q + 4 * e;
            if (r < m) Z[(size_t)r * HC_N + col0 + j * 16 + r16] = (float)acc[j][e];
        }
    }
}

// One element of the train-mode stage from its stored fp32 z, in double: xhat, y (the fp32 BatchNorm output the forward
// stores) and, from the gradient of the pooled feature, dy = dLoss / dy.  The statistics pass and the weight gradient call
// the same function, so both see the same bits.
__device__ __forceinline__ float hc_bn(float z, double mean, double istd, double g, double be, double* xh) {
    *xh = ((double)z - mean) * istd;
    return (float)(*xh * g + be);
}
__device__ __forceinline__ double hc_sigmoid(double y) { return 1.0 / (1.0 + exp(-y)); }
__device__ __forceinline__ double hc_dy(float y, float dfeat) {
    const double yd = (double)y, s = hc_sigmoid(yd);
    return ((double)dfeat / (double)HC_HW) * (s * (1.0 + yd * (1.0 - s)));
}

// Partial sums of a channel statistic over rows [256 chunk, 256 (chunk + 1)) n [0, m): grid (1280 / 64, chunks).  Thread
// (col, g) adds rows g, g + 4, .. of its column in double, then the 4 row groups are added in order.
//   MODE 0: sum z      MODE 1: sum (z - mean)^2      MODE 2: sum dy -> part, sum dy xhat -> part2
template <int MODE>
__global__ __launch_bounds__(HT_THREADS) void hc_colstat_kernel(const float* __restrict__ Z, const double* __restrict__ mean,
                                                                const double* __restrict__ istd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ dfeat,
                                                                double* __restrict__ part, double* __restrict__ part2, int m) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const int r0 = blockIdx.y * HC_STAT_ROWS, r1 = min(m, r0 + HC_STAT_ROWS);
    double mu = 0.0, is = 0.0, ga = 0.0, be = 0.0;
    if constexpr (MODE >= 1) mu = mean[c];
    if constexpr (MODE == 2) { is = istd[c]; ga = (double)gamma[c]; be = (double)beta[c]; }
    double s0 = 0.0, s1 = 0.0;
    for (int r = r0 + g; r < r1; r += 4) {
        const float z = Z[(size_t)r * HC_N + c];
        if constexpr (MODE == 0) s0 += (double)z;
        if constexpr (MODE == 1) { const double d = (double)z - mu; s0 += d * d; }
        if constexpr (MODE == 2) {
            double xh;
            const float y = hc_bn(z, mu, is, ga, be, &xh);
            const double dy = hc_dy(y, dfeat[(size_t)(r / HC_HW) * HC_N + c]);
            s0 += dy;
            s1 += dy * xh;
        }
    }
    red[0][g][cl] = s0;
    red[1][g][cl] = s1;
    __syncthreads();
    if (g == 0) {
        part[(size_t)blockIdx.y * HC_N + c] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        if constexpr (MODE == 2) part2[(size_t)blockIdx.y * HC_N + c] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

// The chunks' partial sums added in chunk order, one thread per channel (grid 1280 / 256):
//   MODE 0: mean = sum / m
//   MODE 1: var = sum / m (biased: what normalises), istd = 1 / sqrt(var + eps); running statistics as BatchNorm2d updates
//           them (m / (m - 1) var into the running variance), in the head trainer's fp32 form
//   MODE 2: sdy = sum dy, sdx = sum dy xhat (kept in double for the weight gradient), added to the gradients of beta / gamma
template <int MODE>
__global__ __launch_bounds__(HT_THREADS) void hc_finalize_kernel(const double* __restrict__ part, const double* __restrict__ part2,
                                                                 int chunks, int m, double* __restrict__ out, double* __restrict__ out2,
                                                                 float* __restrict__ fa, float* __restrict__ fb, float momentum,
                                                                 double eps) {
    const int c = blockIdx.x * HT_THREADS + threadIdx.x;
    if (c >= HC_N) return;
    double s = 0.0, s2 = 0.0;
    for (int k = 0; k < chunks; ++k) {
        s += part[(size_t)k * HC_N + c];
        if constexpr (MODE == 2) s2 += part2[(size_t)k * HC_N + c];
    }
    if constexpr (MODE == 0) {
        out[c] = s / m;
    } else if constexpr (MODE == 1) {
        const double var = s / m, mu = out2[c];                 // out2 = the means of MODE 0
        out[c] = 1.0 / sqrt(var + eps);
        const float unb = (float)(var * ((double)m / (double)(m - 1)));
        fa[c] = (1.f - momentum) * fa[c] + momentum * (float)mu;            // running mean
        fb[c] = (1.f - momentum) * fb[c] + momentum * unb;                  // running variance
    } else {
        out[c] = s;
        out2[c] = s2;
        fa[c] += (float)s2;                                     // dgamma
        fb[c] += (float)s;                                      // dbeta
    }
}

// BatchNorm + swish + mean over the 49 positions: grid (1280 / 256, n), one thread per (image, channel).  TRAIN: the batch
// statistics of this call and y stored for the "cz" tap; else the running statistics (per row: any chunking of the rows
// gives the same bits).  feat = the sum of the 49 double swish values / 49, rounded once.
template <bool TRAIN>
__global__ __launch_bounds__(HT_THREADS) void hc_swish_pool_kernel(const float* __restrict__ Z, const double* __restrict__ mean,
                                                                   const double* __restrict__ istd, const float* __restrict__ rmean,
                                                                   const float* __restrict__ rvar, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, double eps, float* __restrict__ Y,
                                                                   float* __restrict__ feat) {
    const int c = blockIdx.x * HT_THREADS + threadIdx.x, i = blockIdx.y;
    if (c >= HC_N) return;
    double mu, is;
    if constexpr (TRAIN) { mu = mean[c]; is = istd[c]; }
    else { mu = (double)rmean[c]; is = 1.0 / sqrt((double)rvar[c] + eps); }
    const double ga = (double)gamma[c], be = (double)beta[c];
    double s = 0.0;
    for (int p = 0; p < HC_HW; ++p) {
        const size_t o = ((size_t)i * HC_HW + p) * HC_N + c;
        double xh;
        const float y = hc_bn(Z[o], mu, is, ga, be, &xh);
        if constexpr (TRAIN) Y[o] = y;
        s += (double)y * hc_sigmoid((double)y);
    }
    feat[(size_t)i * HC_N + c] = (float)(s / (double)HC_HW);
}

// ---------------------------------------------------------------------------------------------- backward
// Partial weight gradient of rows [512 chunk, 512 (chunk + 1)) n [0, m): P [chunk][1280][320] = dZ^T . X over those rows,
// in double.  grid (40, chunks): wave w of the grid owns channels 16 (w / 2) .. + 16 and inputs 160 (w % 2) .. + 160 (10
// tiles, 10 independent chains).  Lane (r, q) forms A[channel r][row q] = dZ of its element as it loads Z (see the head of
// the file) and loads B[row q][input r] per tile; a row past the end contributes zeros and is read at row 0 instead.
__global__ __launch_bounds__(HT_THREADS) void hc_wgrad_kernel(const float* __restrict__ Z, const float* __restrict__ X,
                                                              const float* __restrict__ dfeat, const double* __restrict__ mean,
                                                              const double* __restrict__ istd, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const double* __restrict__ sdy,
                                                              const double* __restrict__ sdx, double* __restrict__ P, int m) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int gw = blockIdx.x * 4 + wv, o0 = (gw >> 1) * 16, i0 = (gw & 1) * HC_WG_COLS;
    constexpr int J = HC_WG_COLS / 16;
    const int r0 = blockIdx.y * HC_WG_ROWS, r1 = min(m, r0 + HC_WG_ROWS);
    const int c = o0 + r16;
    const double mu = mean[c], is = istd[c], ga = (double)gamma[c], be = (double)beta[c];
    const double gi = ga * is, mdy = sdy[c] / m, mdx = sdx[c] / m;
    d4 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = r0; k0 < r1; k0 += 4) {
        const int row = k0 + q;
        const bool ok = row < r1;
        const size_t rr = ok ? (size_t)row : 0;
        double xh;
        const float y = hc_bn(Z[rr * HC_N + c], mu, is, ga, be, &xh);
        const double dy = hc_dy(y, dfeat[(rr / HC_HW) * HC_N + c]);
        const double a = ok ? gi * ((dy - mdy) - xh * mdx) : 0.0;
        const float* xr = X + rr * HC_K + i0 + r16;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            float b = xr[j * 16];
            if (!ok) b = 0.f;
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)b, acc[j], 0, 0, 0);
        }
    }
    double* out = P + (size_t)blockIdx.y * (HC_N * HC_K);
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[(size_t)(o0 + q + 4 * e) * HC_K + i0 + j * 16 + r16] = acc[j][e];
    }
}

// second stage: G [1280][320] += the chunks' partials added in chunk order, rounded once
__global__ __launch_bounds__(HT_THREADS) void hc_wreduce_kernel(const double* __restrict__ P, int chunks, float* __restrict__ G) {
    const int i = blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= HC_N * HC_K) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += P[(size_t)k * (HC_N * HC_K) + i];
    G[i] += (float)s;
}

// The stage's dZ as a gradient source of head_train_gemm.h's dY . W form (block 15's stage: dX15 = dZ . W): the element
// functions above, so the input gradient sees the bits the weight gradient sees.
struct ConvGrad {
    typedef ht64::BnK K;
    ht64::BnC bn;
    const float *Z, *dfeat;
    __device__ __forceinline__ K load(int c) const { return bn.load(c); }
    __device__ __forceinline__ void dy_xh(const K& k, size_t row, int c, double* dy, double* xh) const {
        const float y = hc_bn(Z[row * HC_N + c], k.mean, k.istd, k.gamma, k.beta, xh);
        *dy = hc_dy(y, dfeat[(row / HC_HW) * HC_N + c]);
    }
};
constexpr int HC_DX_J = 5;                // 80 columns of dX a workgroup: every dZ is formed four times
static_assert(HC_K % (16 * HC_DX_J) == 0 && HC_N % 16 == 0, "tiles");

}  // namespace

// ---------------------------------------------------------------------------------------------- host
namespace dfd {

struct HeadConvState {
    float lr_scale = 0.1f, momentum = 0.01f;
    double eps = 1e-3;
    float *param = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *ema = nullptr, *rm = nullptr, *rv = nullptr;
    float *x = nullptr, *z = nullptr, *y = nullptr, *dfeat = nullptr;
    double *mean = nullptr, *istd = nullptr, *sdy = nullptr, *sdx = nullptr, *spart = nullptr, *spart2 = nullptr, *wpart = nullptr,
           *partial = nullptr;
    void* pool = nullptr;
};

void headconv_destroy(HeadTrainState* S) {
    HeadConvState* C = S->conv;
    if (!C) return;
    if (C->pool) hipFree(C->pool);
    delete C;
    S->conv = nullptr;
}

const double* headconv_sumsq(dfd_handle* h, HeadTrainState* S) {
    HeadConvState* C = S->conv;
    head_train_launch_sumsq(h->stream, C->grad, CV_COUNT, C->partial);
    return C->partial;
}

void headconv_adamw(dfd_handle* h, HeadTrainState* S, double lr, double t) {
    HeadConvState* C = S->conv;
    // S->partial comes first in the norm's sum, as in the head's own launch: both launches see the same norm
    head_train_launch_adamw(h->stream, C->param, C->grad, C->m, C->v, C->ema, CV_COUNT, head_train_norm_parts(S), S->cfg,
                            lr * (double)C->lr_scale, t, S->scalars + 2);
}

int headconv_commit(dfd_handle* h, HeadTrainState* S, int use_ema) {
    HeadConvState* C = S->conv;
    std::vector<float> P(CV_COUNT), rm(HC_N), rv(HC_N);
    DFD_HIP_TRY(h, hipMemcpyAsync(P.data(), use_ema ? C->ema : C->param, (size_t)CV_COUNT * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(rm.data(), C->rm, HC_N * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(rv.data(), C->rv, HC_N * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    // weights._fold without a conv bias: a = g / sqrt(var + eps); w' = w a; b' = 0 a + (beta - mu a), float64, rounded once
    std::vector<float> w((size_t)HC_N * HC_K), b(HC_N);
    for (int o = 0; o < HC_N; ++o) {
        const double a = (double)P[CO_G + o] / std::sqrt((double)rv[o] + C->eps);
        for (int k = 0; k < HC_K; ++k) w[(size_t)o * HC_K + k] = (float)((double)P[CO_W + (size_t)o * HC_K + k] * a);
        b[o] = (float)(0.0 * a + ((double)P[CO_BE + o] - (double)rm[o] * a));
    }
    const B0Plan& B = h->b0;
    DFD_HIP_TRY(h, hipMemcpyAsync(const_cast<float*>(B.head_w), w.data(), w.size() * 4, hipMemcpyHostToDevice, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(const_cast<float*>(B.head_b), b.data(), b.size() * 4, hipMemcpyHostToDevice, h->stream));
    // readers of head.w: b0_forward's head GEMM and Grad-CAM's un-activated one (b0_head_preact), both through the split
    // cached by weight pointer - rebuilt in place, so plan and tile-table pointers stay valid
    auto it = h->wsplit.find(B.head_w);
    if (it != h->wsplit.end()) launch_split_weights(B.head_w, it->second, HC_N, HC_K, h->stream, false);
    DFD_HIP_TRY(h, hipGetLastError());
    DFD_HIP_TRY(h, stream_sync(h));                             // the host staging above lives until here
    return DFD_OK;
}

int headconv_tap(dfd_handle* h, HeadTrainState* S, const char* name, float* out, size_t capacity) {
    HeadConvState* C = S->conv;
    if (!C) return fail(h, DFD_ERR_ARG, "head_train_tap: '%s' needs the conv stage (dfd_head_train_unfreeze_conv)", name);
    const float* src = !strcmp(name, "cfeat") ? S->feat : !strcmp(name, "dfeat") ? C->dfeat : C->y;
    const size_t count = (size_t)S->last_n * (src == C->y ? (size_t)HC_HW * HC_N : (size_t)HC_N);
    if (capacity < count) return fail(h, DFD_ERR_ARG, "head_train_tap: '%s' holds %zu floats, capacity %zu", name, count, capacity);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipMemcpy(out, src, count * 4, hipMemcpyDeviceToHost));
    return DFD_OK;
}

}  // namespace dfd

namespace {

struct CField { float* dfd_headconv_params::*ptr; int off, count; };
const CField kConvTrainable[] = {{&dfd_headconv_params::w, CO_W, HC_N * HC_K}, {&dfd_headconv_params::g, CO_G, HC_N},
                                 {&dfd_headconv_params::be, CO_BE, HC_N}};

HeadTrainState* open_conv(dfd_handle* h, const char* who, bool want_stage, int* rc) {
    if (!h) { *rc = DFD_ERR_ARG; return nullptr; }
    HeadTrainState* S = h->head_train;
    if (!S) { *rc = fail(h, DFD_ERR_ARG, "%s: no trainer is open on this handle (dfd_head_train_begin)", who); return nullptr; }
    if (want_stage && !S->conv) { *rc = fail(h, DFD_ERR_ARG, "%s: the conv stage is not unfrozen (dfd_head_train_unfreeze_conv)", who); return nullptr; }
    *rc = DFD_OK;
    return S;
}

int stat_chunks(int m) { return (m + HC_STAT_ROWS - 1) / HC_STAT_ROWS; }
int wg_chunks(int m) { return (m + HC_WG_ROWS - 1) / HC_WG_ROWS; }

// X (C->x, n trunk rows) -> S->feat with the conv parameters at P; train: batch statistics, running update, y kept
int conv_forward(dfd_handle* h, HeadTrainState* S, const float* P, int n, bool train) {
    HeadConvState* C = S->conv;
    hipStream_t s = h->stream;
    const int m = n * HC_HW;
    const dim3 blk(HT_THREADS), chan((HC_N + HT_THREADS - 1) / HT_THREADS);
    hipLaunchKernelGGL(hc_gemm_fwd_kernel, dim3(HC_N / HC_FWD_COLS, (m + 63) / 64), blk, 0, s, C->x, P + CO_W, C->z, m);
    if (train) {
        const int ch = stat_chunks(m);
        const dim3 sg(HC_N / 64, ch);
        hipLaunchKernelGGL(hc_colstat_kernel<0>, sg, blk, 0, s, C->z, nullptr, nullptr, nullptr, nullptr, nullptr, C->spart, nullptr, m);
        hipLaunchKernelGGL(hc_finalize_kernel<0>, chan, blk, 0, s, C->spart, nullptr, ch, m, C->mean, nullptr, nullptr, nullptr, 0.f, 0.0);
        hipLaunchKernelGGL(hc_colstat_kernel<1>, sg, blk, 0, s, C->z, C->mean, nullptr, nullptr, nullptr, nullptr, C->spart, nullptr, m);
        hipLaunchKernelGGL(hc_finalize_kernel<1>, chan, blk, 0, s, C->spart, nullptr, ch, m, C->istd, C->mean, C->rm, C->rv, C->momentum, C->eps);
        hipLaunchKernelGGL(hc_swish_pool_kernel<true>, dim3(chan.x, n), blk, 0, s, C->z, C->mean, C->istd, nullptr, nullptr, P + CO_G,
                           P + CO_BE, C->eps, C->y, S->feat);
    } else {
        hipLaunchKernelGGL(hc_swish_pool_kernel<false>, dim3(chan.x, n), blk, 0, s, C->z, nullptr, nullptr, C->rm, C->rv, P + CO_G,
                           P + CO_BE, C->eps, nullptr, S->feat);
    }
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

}  // namespace

namespace dfd {

float* headconv_rows(HeadTrainState* S) { return S->conv->x; }
float headconv_lr_scale(HeadTrainState* S) { return S->conv->lr_scale; }
const double* headconv_partial(HeadTrainState* S) { return S->conv->partial; }

int headconv_step(dfd_handle* h, HeadTrainState* S, int n, const float* labels_a, const float* labels_b, float lam, float loss_scale,
                  float* dx) {
    HeadConvState* C = S->conv;
    hipStream_t s = h->stream;
    const int m = n * HC_HW;
    int rc;
    const float* P = C->param;
    if ((rc = conv_forward(h, S, P, n, true))) return rc;
    if ((rc = head_train_step(h, S, n, labels_a, labels_b, lam, loss_scale, C->dfeat))) return rc;
    const dim3 blk(HT_THREADS);
    const int sch = stat_chunks(m), wch = wg_chunks(m);
    hipLaunchKernelGGL(hc_colstat_kernel<2>, dim3(HC_N / 64, sch), blk, 0, s, C->z, C->mean, C->istd, P + CO_G, P + CO_BE, C->dfeat,
                       C->spart, C->spart2, m);
    hipLaunchKernelGGL(hc_finalize_kernel<2>, dim3((HC_N + HT_THREADS - 1) / HT_THREADS), blk, 0, s, C->spart, C->spart2, sch, m, C->sdy,
                       C->sdx, C->grad + CO_G, C->grad + CO_BE, 0.f, 0.0);
    hipLaunchKernelGGL(hc_wgrad_kernel, dim3(HC_N / 16 * (HC_K / HC_WG_COLS) / 4, wch), blk, 0, s, C->z, C->x, C->dfeat, C->mean, C->istd,
                       P + CO_G, P + CO_BE, C->sdy, C->sdx, C->wpart, m);
    hipLaunchKernelGGL(hc_wreduce_kernel, dim3((HC_N * HC_K + HT_THREADS - 1) / HT_THREADS), blk, 0, s, C->wpart, wch, C->grad + CO_W);
    if (dx) {                                                  // dX = dZ . W [1280][320], for the stage below
        const ConvGrad g{{C->mean, C->istd, C->sdy, C->sdx, P + CO_G, P + CO_BE, m}, C->z, C->dfeat};
        hipLaunchKernelGGL((ht64::gemm_dyw_kernel<HC_DX_J, ConvGrad>), dim3(HC_K / (16 * HC_DX_J), (m + 15) / 16), blk, 0, s, g, P + CO_W,
                           dx, m, HC_N, HC_K);
    }
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

int headconv_eval_step(dfd_handle* h, HeadTrainState* S, int use_ema, int n) {
    HeadConvState* C = S->conv;
    int rc;
    if ((rc = conv_forward(h, S, use_ema ? C->ema : C->param, n, false))) return rc;
    return head_train_eval_step(h, S, use_ema ? S->ema : S->param, n);
}

}  // namespace dfd

extern "C" {

int dfd_head_train_unfreeze_conv(dfd_handle* h, const dfd_headconv_params* init, float lr_scale, float bn_momentum, float bn_eps) {
    int rc;
    HeadTrainState* S = open_conv(h, "head_train_unfreeze_conv", false, &rc);
    if (!S) return rc;
    if (S->conv) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_conv: the conv stage is already unfrozen");
    if (S->counter) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_conv: the trainer has accumulated already; unfreeze right after begin");
    if (!init || !init->w || !init->g || !init->be || !init->rm || !init->rv) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_conv: null parameters");
    if (!(lr_scale >= 0.f && bn_momentum >= 0.f && bn_momentum <= 1.f && bn_eps > 0.f))
        return fail(h, DFD_ERR_ARG, "head_train_unfreeze_conv: lr_scale %g, bn_momentum %g or bn_eps %g out of range", (double)lr_scale,
                    (double)bn_momentum, (double)bn_eps);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadConvState* C = new (std::nothrow) HeadConvState();
    if (!C) return fail(h, DFD_ERR_CAPACITY, "head_train_unfreeze_conv: out of host memory");
    C->lr_scale = lr_scale;
    C->momentum = bn_momentum;
    C->eps = bn_eps == 1e-3f ? 1e-3 : (double)bn_eps;          // the backbone's eps (weights._fold's double), not its float neighbour
    const size_t mm = (size_t)S->max_n * HC_HW, sch = (size_t)stat_chunks((int)mm), wch = (size_t)wg_chunks((int)mm);
    struct Slot { void** p; size_t bytes; };
    const Slot slots[] = {
        {(void**)&C->param, (size_t)CV_COUNT * 4}, {(void**)&C->grad, (size_t)CV_COUNT * 4}, {(void**)&C->m, (size_t)CV_COUNT * 4},
        {(void**)&C->v, (size_t)CV_COUNT * 4},     {(void**)&C->ema, (size_t)CV_COUNT * 4},
        {(void**)&C->rm, HC_N * 4}, {(void**)&C->rv, HC_N * 4},
        {(void**)&C->x, mm * HC_K * 4}, {(void**)&C->z, mm * HC_N * 4}, {(void**)&C->y, mm * HC_N * 4},
        {(void**)&C->dfeat, (size_t)S->max_n * HC_N * 4},
        {(void**)&C->mean, HC_N * 8}, {(void**)&C->istd, HC_N * 8}, {(void**)&C->sdy, HC_N * 8}, {(void**)&C->sdx, HC_N * 8},
        {(void**)&C->spart, sch * HC_N * 8}, {(void**)&C->spart2, sch * HC_N * 8}, {(void**)&C->wpart, wch * HC_N * HC_K * 8},
        {(void**)&C->partial, NORM_BLOCKS * 8},
    };
    size_t total = 0;
    for (const Slot& sl : slots) total += (sl.bytes + 255) / 256 * 256;
    if (hipMalloc(&C->pool, total) != hipSuccess) {
        delete C;
        return fail(h, DFD_ERR_HIP, "head_train_unfreeze_conv: hipMalloc of %zu bytes failed", total);
    }
    size_t off = 0;
    for (const Slot& sl : slots) {
        *sl.p = static_cast<char*>(C->pool) + off;
        off += (sl.bytes + 255) / 256 * 256;
    }
    S->conv = C;
    auto bail = [&](hipError_t e, const char* what) {
        headconv_destroy(S);
        return fail(h, DFD_ERR_HIP, "head_train_unfreeze_conv: %s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMemsetAsync(C->pool, 0, total, h->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
    for (const CField& f : kConvTrainable)
        if ((e = hipMemcpyAsync(C->param + f.off, init->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "parameter upload");
    if ((e = hipMemcpyAsync(C->rm, init->rm, HC_N * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return bail(e, "statistics upload");
    if ((e = hipMemcpyAsync(C->rv, init->rv, HC_N * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return bail(e, "statistics upload");
    if ((e = hipMemcpyAsync(C->ema, C->param, (size_t)CV_COUNT * 4, hipMemcpyDeviceToDevice, h->stream)) != hipSuccess) return bail(e, "shadow copy");
    if ((e = stream_sync(h)) != hipSuccess) return bail(e, "stream wait");
    return DFD_OK;
}

int dfd_head_train_accumulate_trunk(dfd_handle* h, const float* trunk, int n, const float* labels_a, const float* labels_b, float lam,
                                    float loss_scale, float* loss_out, float* logits_out) {
    int rc;
    HeadTrainState* S = open_conv(h, "head_train_accumulate_trunk", true, &rc);
    if (!S) return rc;
    if (S->stage[0]) return fail(h, DFD_ERR_ARG, "head_train_accumulate_trunk: block 15 is unfrozen, rows are block 14's output (dfd_head_train_accumulate_block)");
    if (!trunk || !labels_a || !loss_out) return fail(h, DFD_ERR_ARG, "head_train_accumulate_trunk: null pointer");
    if (n < 2) return fail(h, DFD_ERR_ARG, "head_train_accumulate_trunk: %d rows; batch statistics need at least 2", n);
    if (n > S->max_n) return fail(h, DFD_ERR_ARG, "head_train_accumulate_trunk: %d rows exceed the trainer's max_n %d", n, S->max_n);
    if (!head_train_mix_ok(lam, loss_scale))
        return fail(h, DFD_ERR_ARG, "head_train_accumulate_trunk: lam %g outside [0, 1] or loss_scale %g not a number", (double)lam, (double)loss_scale);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadConvState* C = S->conv;
    hipStream_t s = h->stream;
    DFD_HIP_TRY(h, hipMemcpyAsync(C->x, trunk, (size_t)n * HC_ROW * 4, hipMemcpyHostToDevice, s));
    if ((rc = headconv_step(h, S, n, labels_a, labels_b, lam, loss_scale, nullptr))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(loss_out, S->scalars, 4, hipMemcpyDeviceToHost, s));
    if (logits_out) DFD_HIP_TRY(h, hipMemcpyAsync(logits_out, S->logits, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));
    S->last_n = n;
    ++S->counter;
    return DFD_OK;
}

int dfd_head_train_eval_trunk(dfd_handle* h, const float* trunk, int n, int use_ema, float* logits_out) {
    int rc;
    HeadTrainState* S = open_conv(h, "head_train_eval_trunk", true, &rc);
    if (!S) return rc;
    if (S->stage[0]) return fail(h, DFD_ERR_ARG, "head_train_eval_trunk: block 15 is unfrozen, rows are block 14's output (dfd_head_train_eval_block)");
    if (!trunk || !logits_out) return fail(h, DFD_ERR_ARG, "head_train_eval_trunk: null pointer");
    if (n < 1 || n > S->max_n) return fail(h, DFD_ERR_ARG, "head_train_eval_trunk: %d rows outside 1..%d", n, S->max_n);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadConvState* C = S->conv;
    DFD_HIP_TRY(h, hipMemcpyAsync(C->x, trunk, (size_t)n * HC_ROW * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = headconv_eval_step(h, S, use_ema, n))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(logits_out, S->logits, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_head_train_export_conv(dfd_handle* h, int use_ema, dfd_headconv_params* out) {
    int rc;
    HeadTrainState* S = open_conv(h, "head_train_export_conv", true, &rc);
    if (!S) return rc;
    if (!out || !out->w || !out->g || !out->be || !out->rm || !out->rv) return fail(h, DFD_ERR_ARG, "head_train_export_conv: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadConvState* C = S->conv;
    const float* P = use_ema ? C->ema : C->param;
    for (const CField& f : kConvTrainable)
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*f.ptr, P + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(out->rm, C->rm, HC_N * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(out->rv, C->rv, HC_N * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_head_train_conv_grads(dfd_handle* h, dfd_headconv_params* io, int set) {
    int rc;
    HeadTrainState* S = open_conv(h, "head_train_conv_grads", true, &rc);
    if (!S) return rc;
    if (!io || !io->w || !io->g || !io->be) return fail(h, DFD_ERR_ARG, "head_train_conv_grads: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadConvState* C = S->conv;
    for (const CField& f : kConvTrainable) {
        if (set) DFD_HIP_TRY(h, hipMemcpyAsync(C->grad + f.off, io->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream));
        else DFD_HIP_TRY(h, hipMemcpyAsync(io->*f.ptr, C->grad + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

}  // extern "C"

// Block 15 of the backbone under the head trainer: net._blocks.15 (MBConv k3, stride 1, 192 -> 1152 -> 320, squeeze-excite
// 48, 7 x 7, no skip) in train mode in front of the conv stage (head_train_conv.hip) and the MLP head (head_train.hip),
// reference train.py:863-924 - the unfrozen backbone is one AdamW group at lr_scale x lr.  Input: block 14's output,
// [n][7][7][192] fp32 NHWC; with m = 49 n rows
//   Ze = X We^T            gemm_fwd<6, false>    BN0 (batch statistics), ae = swish(ye)      bk_bn_swish_kernel
//   Zd = depthwise 3 x 3   bk_dw_fwd_kernel      BN1, ad = swish(yd), s = mean over 49       bk_bn_swish_pool_kernel
//   gate = sigmoid(W2 swish(W1 s + b1) + b2)                                                 bk_se_fwd_kernel
//   Zp = (ad * gate) Wp^T  gemm_fwd<5, true>     BN2 -> x15, written into the conv stage's rows   bk_bn_kernel
// then headconv_step (conv stage, head, loss, their backward), which also returns dX15 = dZh . Wh, and
//   BN2 backward: dZp formed at the load;  dWp += dZp^T t   wgrad<6, true>;   dt = dZp . Wp   gemm_dyw<6>
//   dgate, du, dq, dr, ds per crop   bk_se_bwd_kernel;   dW2, db2, dW1, db1 over the crops in order   bk_se_wgrad_kernel
//   dyd = (dt gate + ds / 49) swish'(yd), BN1 backward -> dZd (stored over dt)                bk_dz_store_kernel
//   dWd   bk_dw_wgrad_kernel + bk_dw_wreduce_kernel;   dae = dZd correlated with the flipped kernel   bk_dw_bwd_kernel
//   dye = dae swish'(ye), BN0 backward: dZe formed at the load;  dWe += dZe^T X   wgrad<6, false>
// Block 14 is frozen: no gradient with respect to X.
//
// Arithmetic as head_train_conv.hip: the GEMMs run on the fp64 MFMA with fp32 operands widened at the load
// (head_train_gemm.h), every other element is computed in double from stored fp32 values and rounded once where it is
// stored.  ye, yd, t = ad * gate and the dZ of the three BatchNorms are never stored; the small squeeze-excite vectors
// (r, q, du, dr, ds) stay in double.  Every reduction has a fixed order and no atomics: channel statistics over 256-row
// chunks, weight gradients over 512-row chunks, the depthwise weight gradient over 8-crop chunks, the squeeze-excite
// weight gradients over the crops one by one - added in that order, in double.  Built with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "b0_kernels.h"
#include "dfd_common.h"
#include "head_train_gemm.h"
#include "head_train_state.h"
#include "kernel_util.h"

using namespace dfd;
using namespace dfd::ht64;

namespace {

constexpr int BK_IN = 192, BK_EXP = 1152, BK_SE = 48, BK_OUT = 320, BK_HW = 49, BK_H = 7, BK_ROW = BK_HW * BK_IN, BK_INDEX = 15;
// the block group's arena (floats); every offset a multiple of 4
constexpr int BO_WE = 0, BO_WD = BO_WE + BK_EXP * BK_IN, BO_W1 = BO_WD + BK_EXP * 9, BO_B1 = BO_W1 + BK_SE * BK_EXP;
constexpr int BO_W2 = BO_B1 + BK_SE, BO_B2 = BO_W2 + BK_EXP * BK_SE, BO_WP = BO_B2 + BK_EXP, BO_G0 = BO_WP + BK_OUT * BK_EXP;
constexpr int BO_BE0 = BO_G0 + BK_EXP, BO_G1 = BO_BE0 + BK_EXP, BO_BE1 = BO_G1 + BK_EXP, BO_G2 = BO_BE1 + BK_EXP;
constexpr int BO_BE2 = BO_G2 + BK_OUT, BK_COUNT = BO_BE2 + BK_OUT;
static_assert(BK_COUNT == 717232, "trainable floats of block 15");
constexpr int BK_JE = 6, BK_JP = 5;       // column tiles a wave: 1152 = 12 x 96, 320 = 4 x 80
constexpr int BK_DW_CROPS = 8;            // crops of one partial depthwise weight gradient
static_assert(BK_EXP % (16 * BK_JE) == 0 && BK_OUT % (16 * BK_JP) == 0 && BK_IN % 16 == 0 && BK_EXP % 64 == 0 && BK_OUT % 64 == 0, "tiles");
static_assert((BK_OUT / 16 * (BK_EXP / (16 * BK_JE))) % 4 == 0 && (BK_EXP / 16 * (BK_IN / (16 * BK_JE))) % 4 == 0, "weight-gradient grids");
static_assert(BK_OUT % 16 == 0, "gemm_dyw splits its channels over four waves");
static_assert(BK_OUT == 320 && DFD_TRUNK_ROW == BK_HW * BK_OUT, "the block's output is the conv stage's row");
const int kBnC[3] = {BK_EXP, BK_EXP, BK_OUT};

// ---------------------------------------------------------------------------------------------- forward
// ae = swish(BN(Ze)), one thread per element
__global__ __launch_bounds__(HT_THREADS) void bk_bn_swish_kernel(const float* __restrict__ Z, BnC bn, float* __restrict__ out,
                                                                 size_t total, int C) {
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const BnK k = bn.load(c);
    out[i] = (float)swish((((double)Z[i] - k.mean) * k.istd) * k.gamma + k.beta);
}

// x15 = BN(Zp): no activation
__global__ __launch_bounds__(HT_THREADS) void bk_bn_kernel(const float* __restrict__ Z, BnC bn, float* __restrict__ out, size_t total,
                                                           int C) {
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const BnK k = bn.load(c);
    out[i] = (float)((((double)Z[i] - k.mean) * k.istd) * k.gamma + k.beta);
}

// eval mode: the running statistics in the place of the batch's
__global__ __launch_bounds__(HT_THREADS) void bk_eval_consts_kernel(const float* __restrict__ rm, const float* __restrict__ rv, double eps,
                                                                    double* __restrict__ mean, double* __restrict__ istd, int C) {
    const int c = blockIdx.x * HT_THREADS + threadIdx.x;
    if (c >= C) return;
    mean[c] = (double)rm[c];
    istd[c] = 1.0 / sqrt((double)rv[c] + eps);
}

// Depthwise 3 x 3, pad 1, on [n][7][7][1152]: one thread per output element, channels fastest; the 9 taps in (ky, kx)
// order in double.  W [c][ky][kx] (torch's layout).
__global__ __launch_bounds__(HT_THREADS) void bk_dw_fwd_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                               float* __restrict__ Z, size_t total) {
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % BK_EXP), p = (int)((i / BK_EXP) % BK_HW), y = p / BK_H, x = p % BK_H;
    const size_t base = i - (size_t)p * BK_EXP;                  // position 0 of this crop, channel c
    double s = 0.0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            if (yy < 0 || yy >= BK_H || xx < 0 || xx >= BK_H) continue;
            s += (double)A[base + (size_t)(yy * BK_H + xx) * BK_EXP] * (double)W[c * 9 + ky * 3 + kx];
        }
    }
    Z[i] = (float)s;
}

// ad = swish(BN(Zd)) and its mean over the 49 positions: grid (ceil(1152 / 256), n), one thread per (crop, channel).  The
// pooled value is the sum of the stored fp32 ad in position order / 49, rounded once.
__global__ __launch_bounds__(HT_THREADS) void bk_bn_swish_pool_kernel(const float* __restrict__ Z, BnC bn, float* __restrict__ AD,
                                                                      float* __restrict__ pooled) {
    const int c = blockIdx.x * HT_THREADS + threadIdx.x, i = blockIdx.y;
    if (c >= BK_EXP) return;
    const BnK k = bn.load(c);
    double s = 0.0;
    for (int p = 0; p < BK_HW; ++p) {
        const size_t o = ((size_t)i * BK_HW + p) * BK_EXP + c;
        const float a = (float)swish((((double)Z[o] - k.mean) * k.istd) * k.gamma + k.beta);
        AD[o] = a;
        s += (double)a;
    }
    pooled[(size_t)i * BK_EXP + c] = (float)(s / (double)BK_HW);
}

// lanes' values added in a fixed tree; every lane must call
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return __shfl(v, 0, 64);
}

// Squeeze-excite forward, one block per crop: r = W1 s + b1 [48], q = swish(r), u = W2 q + b2 [1152], gate = sigmoid(u).
// A wave owns 12 of the 48 r: lanes take the 1152 terms 64 apart, then the fixed tree.  r, q stay in double.
__global__ __launch_bounds__(HT_THREADS) void bk_se_fwd_kernel(const float* __restrict__ pooled, const float* __restrict__ W1,
                                                               const float* __restrict__ B1, const float* __restrict__ W2,
                                                               const float* __restrict__ B2, double* __restrict__ R,
                                                               double* __restrict__ Q, float* __restrict__ gate) {
    __shared__ double qs[BK_SE];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* s = pooled + (size_t)i * BK_EXP;
    for (int j = wv * (BK_SE / 4); j < (wv + 1) * (BK_SE / 4); ++j) {
        double a = 0.0;
        for (int k = lane; k < BK_EXP; k += 64) a += (double)W1[(size_t)j * BK_EXP + k] * (double)s[k];
        a = wave_sum(a) + (double)B1[j];
        if (lane == 0) {
            const double q = swish(a);
            qs[j] = q;
            R[(size_t)i * BK_SE + j] = a;
            Q[(size_t)i * BK_SE + j] = q;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < BK_EXP; c += HT_THREADS) {
        double u = 0.0;
        for (int j = 0; j < BK_SE; ++j) u += (double)W2[(size_t)c * BK_SE + j] * qs[j];
        gate[(size_t)i * BK_EXP + c] = (float)sigmoid(u + (double)B2[c]);
    }
}

// ---------------------------------------------------------------------------------------------- gradient sources
// BN2: dy is the stored dX15
struct Grad2 {
    typedef BnK K;
    BnC bn;
    const float *Zp, *dX;
    __device__ __forceinline__ K load(int c) const { return bn.load(c); }
    __device__ __forceinline__ void dy_xh(const K& k, size_t row, int c, double* dy, double* xh) const {
        const size_t o = row * BK_OUT + c;
        *xh = ((double)Zp[o] - k.mean) * k.istd;
        *dy = (double)dX[o];
    }
};
// BN1: dad = dt gate + ds / 49 through swish'(yd)
struct Grad1 {
    typedef BnK K;
    BnC bn;
    const float *Zd, *dT, *gate;
    const double* dS;
    __device__ __forceinline__ K load(int c) const { return bn.load(c); }
    __device__ __forceinline__ void dy_xh(const K& k, size_t row, int c, double* dy, double* xh) const {
        const size_t o = row * BK_EXP + c, g = (row / BK_HW) * BK_EXP + c;
        *xh = ((double)Zd[o] - k.mean) * k.istd;
        const double dad = (double)dT[o] * (double)gate[g] + dS[g] / (double)BK_HW;
        *dy = dad * swish_grad(*xh * k.gamma + k.beta);
    }
};
// BN0: the stored dae through swish'(ye)
struct Grad0 {
    typedef BnK K;
    BnC bn;
    const float *Ze, *dA;
    __device__ __forceinline__ K load(int c) const { return bn.load(c); }
    __device__ __forceinline__ void dy_xh(const K& k, size_t row, int c, double* dy, double* xh) const {
        const size_t o = row * BK_EXP + c;
        *xh = ((double)Ze[o] - k.mean) * k.istd;
        *dy = (double)dA[o] * swish_grad(*xh * k.gamma + k.beta);
    }
};

// ---------------------------------------------------------------------------------------------- backward
// Squeeze-excite backward, one block per crop: dgate = sum over 49 of dt ad (position order), du = dgate gate (1 - gate),
// dq = du . W2, dr = dq swish'(r), ds = dr . W1.  du, dr, ds are kept per crop, in double, for bk_se_wgrad_kernel and Grad1.
__global__ __launch_bounds__(HT_THREADS) void bk_se_bwd_kernel(const float* __restrict__ dT, const float* __restrict__ AD,
                                                               const float* __restrict__ gate, const double* __restrict__ R,
                                                               const float* __restrict__ W1, const float* __restrict__ W2,
                                                               double* __restrict__ dU, double* __restrict__ dR, double* __restrict__ dS) {
    __shared__ double du[BK_EXP];
    __shared__ double dr[BK_SE];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < BK_EXP; c += HT_THREADS) {
        double s = 0.0;
        for (int p = 0; p < BK_HW; ++p) {
            const size_t o = ((size_t)i * BK_HW + p) * BK_EXP + c;
            s += (double)dT[o] * (double)AD[o];
        }
        const double g = (double)gate[(size_t)i * BK_EXP + c], u = s * g * (1.0 - g);
        du[c] = u;
        dU[(size_t)i * BK_EXP + c] = u;
    }
    __syncthreads();
    for (int j = wv * (BK_SE / 4); j < (wv + 1) * (BK_SE / 4); ++j) {
        double a = 0.0;
        for (int c = lane; c < BK_EXP; c += 64) a += du[c] * (double)W2[(size_t)c * BK_SE + j];
        a = wave_sum(a);
        if (lane == 0) {
            const double v = a * swish_grad(R[(size_t)i * BK_SE + j]);
            dr[j] = v;
            dR[(size_t)i * BK_SE + j] = v;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < BK_EXP; k += HT_THREADS) {
        double s = 0.0;
        for (int j = 0; j < BK_SE; ++j) s += dr[j] * (double)W1[(size_t)j * BK_EXP + k];
        dS[(size_t)i * BK_EXP + k] = s;
    }
}

// The squeeze-excite weight gradients, one thread per gradient element, the crops added one by one in double:
//   dW2 [c][j] += sum_i du[i][c] q[i][j],  dW1 [j][k] += sum_i dr[i][j] s[i][k],  db2 [c] += sum_i du[i][c],  db1 [j] += sum_i dr[i][j]
__global__ __launch_bounds__(HT_THREADS) void bk_se_wgrad_kernel(const double* __restrict__ dU, const double* __restrict__ dR,
                                                                 const double* __restrict__ Q, const float* __restrict__ pooled,
                                                                 float* __restrict__ gW1, float* __restrict__ gB1,
                                                                 float* __restrict__ gW2, float* __restrict__ gB2, int n) {
    constexpr int NW = BK_EXP * BK_SE;
    int e = blockIdx.x * HT_THREADS + threadIdx.x;
    double s = 0.0;
    if (e < NW) {
        const int c = e / BK_SE, j = e % BK_SE;
        for (int i = 0; i < n; ++i) s += dU[(size_t)i * BK_EXP + c] * Q[(size_t)i * BK_SE + j];
        gW2[e] += (float)s;
    } else if ((e -= NW) < NW) {
        const int j = e / BK_EXP, k = e % BK_EXP;
        for (int i = 0; i < n; ++i) s += dR[(size_t)i * BK_SE + j] * (double)pooled[(size_t)i * BK_EXP + k];
        gW1[e] += (float)s;
    } else if ((e -= NW) < BK_EXP) {
        for (int i = 0; i < n; ++i) s += dU[(size_t)i * BK_EXP + e];
        gB2[e] += (float)s;
    } else if ((e -= BK_EXP) < BK_SE) {
        for (int i = 0; i < n; ++i) s += dR[(size_t)i * BK_SE + e];
        gB1[e] += (float)s;
    }
}

// dZd of BN1, stored over dt (every thread reads its own element of dt before it writes it)
__global__ __launch_bounds__(HT_THREADS) void bk_dz_store_kernel(Grad1 g, float* out, size_t total) {
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % BK_EXP);
    const BnK k = g.load(c);
    out[i] = (float)bn_dz(g, k, i / BK_EXP, c);
}

// dae [y][x] = sum over (ky, kx) of dZd [y - ky + 1][x - kx + 1] W [ky][kx]: the correlation with the flipped kernel, pad 1
__global__ __launch_bounds__(HT_THREADS) void bk_dw_bwd_kernel(const float* __restrict__ dZ, const float* __restrict__ W,
                                                               float* __restrict__ dA, size_t total) {
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % BK_EXP), p = (int)((i / BK_EXP) % BK_HW), y = p / BK_H, x = p % BK_H;
    const size_t base = i - (size_t)p * BK_EXP;
    double s = 0.0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y - ky + 1, xx = x - kx + 1;
            if (yy < 0 || yy >= BK_H || xx < 0 || xx >= BK_H) continue;
            s += (double)dZ[base + (size_t)(yy * BK_H + xx) * BK_EXP] * (double)W[c * 9 + ky * 3 + kx];
        }
    }
    dA[i] = (float)s;
}

// Partial depthwise weight gradient of crops [8 chunk, 8 (chunk + 1)) n [0, n): P [chunk][tap][c] = sum over those crops
// and the positions (crop, then position order) of dZd [y][x] ae [y + ky - 1][x + kx - 1].  grid (ceil(1152 / 256), 9, chunks).
__global__ __launch_bounds__(HT_THREADS) void bk_dw_wgrad_kernel(const float* __restrict__ dZ, const float* __restrict__ A,
                                                                 double* __restrict__ P, int n) {
    const int c = blockIdx.x * HT_THREADS + threadIdx.x, tap = blockIdx.y, ky = tap / 3, kx = tap % 3;
    if (c >= BK_EXP) return;
    const int i0 = blockIdx.z * BK_DW_CROPS, i1 = min(n, i0 + BK_DW_CROPS);
    double s = 0.0;
    for (int i = i0; i < i1; ++i) {
        const size_t base = (size_t)i * BK_HW * BK_EXP + c;
        for (int y = 0; y < BK_H; ++y) {
            const int yy = y + ky - 1;
            if (yy < 0 || yy >= BK_H) continue;
            for (int x = 0; x < BK_H; ++x) {
                const int xx = x + kx - 1;
                if (xx < 0 || xx >= BK_H) continue;
                s += (double)dZ[base + (size_t)(y * BK_H + x) * BK_EXP] * (double)A[base + (size_t)(yy * BK_H + xx) * BK_EXP];
            }
        }
    }
    P[((size_t)blockIdx.z * 9 + tap) * BK_EXP + c] = s;
}

// G [c][tap] += the chunks' partials added in chunk order, rounded once
__global__ __launch_bounds__(HT_THREADS) void bk_dw_wreduce_kernel(const double* __restrict__ P, int chunks, float* __restrict__ G) {
    const int e = blockIdx.x * HT_THREADS + threadIdx.x;
    if (e >= BK_EXP * 9) return;
    const int tap = e / BK_EXP, c = e % BK_EXP;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += P[((size_t)k * 9 + tap) * BK_EXP + c];
    G[c * 9 + tap] += (float)s;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- host
namespace dfd {

struct HeadBlockState {
    float momentum = 0.01f;
    double eps = 1e-3;
    float *param = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *ema = nullptr;
    float *rm[3] = {nullptr, nullptr, nullptr}, *rv[3] = {nullptr, nullptr, nullptr};
    // fp32 tensors of m rows: the input, Ze, ae, Zd, ad, dt then dZd (d1), dae (d2), Zp, dX15; per crop: the pooled s, gate
    float *x = nullptr, *ze = nullptr, *ae = nullptr, *zd = nullptr, *ad = nullptr, *d1 = nullptr, *d2 = nullptr, *zp = nullptr,
          *dx15 = nullptr, *pooled = nullptr, *gate = nullptr;
    double *mean[3] = {nullptr, nullptr, nullptr}, *istd[3] = {nullptr, nullptr, nullptr}, *sdy[3] = {nullptr, nullptr, nullptr},
           *sdx[3] = {nullptr, nullptr, nullptr};
    double *spart = nullptr, *spart2 = nullptr, *wpart = nullptr, *dwpart = nullptr, *partial = nullptr;
    double *r = nullptr, *q = nullptr, *du = nullptr, *dr = nullptr, *ds = nullptr;
    void* pool = nullptr;
};

void headblock_destroy(HeadTrainState* S) {
    HeadBlockState* K = S->block;
    if (!K) return;
    if (K->pool) hipFree(K->pool);
    delete K;
    S->block = nullptr;
}

const double* headblock_sumsq(dfd_handle* h, HeadTrainState* S) {
    head_train_launch_sumsq(h->stream, S->block->grad, BK_COUNT, S->block->partial);
    return S->block->partial;
}

const double* headblock_partial(HeadTrainState* S) { return S->block->partial; }

void headblock_adamw(dfd_handle* h, HeadTrainState* S, double lr, double t) {
    HeadBlockState* K = S->block;
    // the three arenas' partials in the order of the other two launches: all three see the same norm
    head_train_launch_adamw(h->stream, K->param, K->grad, K->m, K->v, K->ema, BK_COUNT, S->partial, headconv_partial(S), K->partial,
                            S->cfg, lr * (double)headconv_lr_scale(S), t, S->scalars + 3);
}

int headblock_tap(dfd_handle* h, HeadTrainState* S, const char* name, float* out, size_t capacity) {
    HeadBlockState* K = S->block;
    if (!K) return fail(h, DFD_ERR_ARG, "head_train_tap: '%s' needs block 15's stage (dfd_head_train_unfreeze_block)", name);
    const float* src = nullptr;
    size_t per = 0;
    if (!strcmp(name, "b15.out")) { src = headconv_rows(S); per = (size_t)BK_HW * BK_OUT; }
    else if (!strcmp(name, "b15.gate")) { src = K->gate; per = BK_EXP; }
    else if (!strcmp(name, "b15.ad")) { src = K->ad; per = (size_t)BK_HW * BK_EXP; }
    else if (!strcmp(name, "b15.dout")) { src = K->dx15; per = (size_t)BK_HW * BK_OUT; }
    else if (!strcmp(name, "b15.dae")) { src = K->d2; per = (size_t)BK_HW * BK_EXP; }
    else return fail(h, DFD_ERR_ARG, "head_train_tap: unknown tap '%s'", name);
    const size_t count = (size_t)S->last_n * per;
    if (capacity < count) return fail(h, DFD_ERR_ARG, "head_train_tap: '%s' holds %zu floats, capacity %zu", name, count, capacity);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipMemcpy(out, src, count * 4, hipMemcpyDeviceToHost));
    return DFD_OK;
}

// Block 15's ten tensors of the inference plan, rewritten in place from the trained parameters (live or EMA) and the
// running statistics: weights._fold's arithmetic (a = g / sqrt(var + eps); w' = w a; b' = 0 a + (beta - mu a), float64,
// rounded once) and weights.pack_b0_tensors' layouts (dw.w [ky][kx][c], se.w2 [48][1152]).  Readers of these pointers:
// b0_forward's block loop - launch_mbconv_front (mbconv_late_kernel / mbconv_k5_kernel: exp.w through its cached split
// AND the fp32 tensor, exp.b, dw.w, dw.b), the unfused pointwise_t (exp.w / proj.w: the cached split under the split GEMM
// and under "bf16_activations", the fp32 tensor in launch_pointwise), launch_depthwise (dw.w, dw.b), launch_se (se.*) and
// the projection's bias (proj.b).  The two cached splits are rebuilt in place, so plan and tile-table pointers stay valid.
int headblock_commit(dfd_handle* h, HeadTrainState* S, int use_ema) {
    HeadBlockState* K = S->block;
    if ((int)h->b0.blocks.size() != BK_INDEX + 1) return fail(h, DFD_ERR_STATE, "head_train_commit: the plan has no block %d", BK_INDEX);
    const B0Block& b = h->b0.blocks[BK_INDEX];
    if (b.c_in != BK_IN || b.c_exp != BK_EXP || b.c_se != BK_SE || b.c_out != BK_OUT || b.kernel != 3)
        return fail(h, DFD_ERR_STATE, "head_train_commit: block %d of the plan is not 192 -> 1152 -> 320, k3", BK_INDEX);
    std::vector<float> P(BK_COUNT), rm[3], rv[3];
    DFD_HIP_TRY(h, hipMemcpyAsync(P.data(), use_ema ? K->ema : K->param, (size_t)BK_COUNT * 4, hipMemcpyDeviceToHost, h->stream));
    for (int l = 0; l < 3; ++l) {
        rm[l].resize(kBnC[l]);
        rv[l].resize(kBnC[l]);
        DFD_HIP_TRY(h, hipMemcpyAsync(rm[l].data(), K->rm[l], (size_t)kBnC[l] * 4, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, hipMemcpyAsync(rv[l].data(), K->rv[l], (size_t)kBnC[l] * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    const int og[3] = {BO_G0, BO_G1, BO_G2}, obe[3] = {BO_BE0, BO_BE1, BO_BE2};
    auto scale = [&](int l, int o) { return (double)P[og[l] + o] / std::sqrt((double)rv[l][o] + K->eps); };
    auto bias = [&](int l, int o, double a) { return (float)(0.0 * a + ((double)P[obe[l] + o] - (double)rm[l][o] * a)); };
    std::vector<float> ew((size_t)BK_EXP * BK_IN), eb(BK_EXP), dw((size_t)9 * BK_EXP), db(BK_EXP), w2((size_t)BK_SE * BK_EXP),
        pw((size_t)BK_OUT * BK_EXP), pb(BK_OUT);
    for (int o = 0; o < BK_EXP; ++o) {
        const double a0 = scale(0, o), a1 = scale(1, o);
        for (int k = 0; k < BK_IN; ++k) ew[(size_t)o * BK_IN + k] = (float)((double)P[BO_WE + (size_t)o * BK_IN + k] * a0);
        eb[o] = bias(0, o, a0);
        for (int t = 0; t < 9; ++t) dw[(size_t)t * BK_EXP + o] = (float)((double)P[BO_WD + o * 9 + t] * a1);
        db[o] = bias(1, o, a1);
        for (int j = 0; j < BK_SE; ++j) w2[(size_t)j * BK_EXP + o] = P[BO_W2 + (size_t)o * BK_SE + j];
    }
    for (int o = 0; o < BK_OUT; ++o) {
        const double a2 = scale(2, o);
        for (int k = 0; k < BK_EXP; ++k) pw[(size_t)o * BK_EXP + k] = (float)((double)P[BO_WP + (size_t)o * BK_EXP + k] * a2);
        pb[o] = bias(2, o, a2);
    }
    const struct { const float* dst; const float* src; size_t count; } ups[] = {
        {b.exp_w, ew.data(), ew.size()}, {b.exp_b, eb.data(), eb.size()}, {b.dw_w, dw.data(), dw.size()}, {b.dw_b, db.data(), db.size()},
        {b.se_w1, P.data() + BO_W1, (size_t)BK_SE * BK_EXP}, {b.se_b1, P.data() + BO_B1, (size_t)BK_SE}, {b.se_w2, w2.data(), w2.size()},
        {b.se_b2, P.data() + BO_B2, (size_t)BK_EXP}, {b.proj_w, pw.data(), pw.size()}, {b.proj_b, pb.data(), pb.size()}};
    for (const auto& u : ups)
        DFD_HIP_TRY(h, hipMemcpyAsync(const_cast<float*>(u.dst), u.src, u.count * 4, hipMemcpyHostToDevice, h->stream));
    const struct { const float* w; int N, Kd; } splits[] = {{b.exp_w, BK_EXP, BK_IN}, {b.proj_w, BK_OUT, BK_EXP}};
    for (const auto& sp : splits) {
        auto it = h->wsplit.find(sp.w);
        if (it != h->wsplit.end()) launch_split_weights(sp.w, it->second, sp.N, sp.Kd, h->stream, false);
    }
    DFD_HIP_TRY(h, hipGetLastError());
    DFD_HIP_TRY(h, stream_sync(h));                             // the host staging above lives until here
    return DFD_OK;
}

}  // namespace dfd

namespace {

struct BField { float* dfd_mbconv_params::*ptr; int off, count; };
const BField kBlockTrainable[] = {
    {&dfd_mbconv_params::exp_w, BO_WE, BK_EXP * BK_IN},   {&dfd_mbconv_params::dw_w, BO_WD, BK_EXP * 9},
    {&dfd_mbconv_params::se_w1, BO_W1, BK_SE * BK_EXP},   {&dfd_mbconv_params::se_b1, BO_B1, BK_SE},
    {&dfd_mbconv_params::se_w2, BO_W2, BK_EXP * BK_SE},   {&dfd_mbconv_params::se_b2, BO_B2, BK_EXP},
    {&dfd_mbconv_params::proj_w, BO_WP, BK_OUT * BK_EXP}, {&dfd_mbconv_params::g0, BO_G0, BK_EXP},
    {&dfd_mbconv_params::be0, BO_BE0, BK_EXP},            {&dfd_mbconv_params::g1, BO_G1, BK_EXP},
    {&dfd_mbconv_params::be1, BO_BE1, BK_EXP},            {&dfd_mbconv_params::g2, BO_G2, BK_OUT},
    {&dfd_mbconv_params::be2, BO_BE2, BK_OUT},
};
struct BStat { float* dfd_mbconv_params::*rm; float* dfd_mbconv_params::*rv; };
const BStat kBlockStats[3] = {{&dfd_mbconv_params::rm0, &dfd_mbconv_params::rv0}, {&dfd_mbconv_params::rm1, &dfd_mbconv_params::rv1},
                              {&dfd_mbconv_params::rm2, &dfd_mbconv_params::rv2}};

bool block_complete(const dfd_mbconv_params* p, bool stats) {
    for (const BField& f : kBlockTrainable)
        if (!(p->*f.ptr)) return false;
    if (stats)
        for (const BStat& st : kBlockStats)
            if (!(p->*st.rm) || !(p->*st.rv)) return false;
    return true;
}

HeadTrainState* open_block(dfd_handle* h, const char* who, bool want_stage, int* rc) {
    if (!h) { *rc = DFD_ERR_ARG; return nullptr; }
    HeadTrainState* S = h->head_train;
    if (!S) { *rc = fail(h, DFD_ERR_ARG, "%s: no trainer is open on this handle (dfd_head_train_begin)", who); return nullptr; }
    if (want_stage && !S->block) { *rc = fail(h, DFD_ERR_ARG, "%s: block 15 is not unfrozen (dfd_head_train_unfreeze_block)", who); return nullptr; }
    *rc = DFD_OK;
    return S;
}

BnC bn_consts(const HeadBlockState* K, const float* P, int l, int m, bool backward) {
    const int og[3] = {BO_G0, BO_G1, BO_G2}, obe[3] = {BO_BE0, BO_BE1, BO_BE2};
    return BnC{K->mean[l], K->istd[l], backward ? K->sdy[l] : nullptr, backward ? K->sdx[l] : nullptr, P + og[l], P + obe[l], m};
}

dim3 flat(size_t total) { return dim3((unsigned)((total + HT_THREADS - 1) / HT_THREADS)); }

// mean and istd of BatchNorm l over the m rows of Z: the batch's (train; running statistics updated) or the running ones
void bn_statistics(HeadBlockState* K, int l, const float* Z, int m, bool train, hipStream_t s) {
    const int C = kBnC[l];
    const dim3 blk(HT_THREADS), chan((C + HT_THREADS - 1) / HT_THREADS);
    if (!train) {
        hipLaunchKernelGGL(bk_eval_consts_kernel, chan, blk, 0, s, K->rm[l], K->rv[l], K->eps, K->mean[l], K->istd[l], C);
        return;
    }
    const int ch = stat_chunks(m);
    const dim3 sg(C / 64, ch);
    hipLaunchKernelGGL((colstat_kernel<0, NoGrad>), sg, blk, 0, s, NoGrad{}, Z, nullptr, K->spart, nullptr, m, C);
    hipLaunchKernelGGL(finalize_kernel<0>, chan, blk, 0, s, K->spart, nullptr, ch, m, C, K->mean[l], nullptr, nullptr, nullptr, 0.f, 0.0);
    hipLaunchKernelGGL((colstat_kernel<1, NoGrad>), sg, blk, 0, s, NoGrad{}, Z, K->mean[l], K->spart, nullptr, m, C);
    hipLaunchKernelGGL(finalize_kernel<1>, chan, blk, 0, s, K->spart, nullptr, ch, m, C, K->istd[l], K->mean[l], K->rm[l], K->rv[l],
                       K->momentum, K->eps);
}

// sum dy and sum dy xhat of BatchNorm l from its gradient source; adds the gradients of gamma and beta
template <class G>
void bn_backward_statistics(HeadBlockState* K, int l, const G& g, int m, hipStream_t s) {
    const int C = kBnC[l], ch = stat_chunks(m);
    const int og[3] = {BO_G0, BO_G1, BO_G2}, obe[3] = {BO_BE0, BO_BE1, BO_BE2};
    const dim3 blk(HT_THREADS);
    hipLaunchKernelGGL((colstat_kernel<2, G>), dim3(C / 64, ch), blk, 0, s, g, nullptr, nullptr, K->spart, K->spart2, m, C);
    hipLaunchKernelGGL(finalize_kernel<2>, dim3((C + HT_THREADS - 1) / HT_THREADS), blk, 0, s, K->spart, K->spart2, ch, m, C, K->sdy[l],
                       K->sdx[l], K->grad + og[l], K->grad + obe[l], 0.f, 0.0);
}

// X (K->x, n rows of block 14's output) -> x15 in the conv stage's rows, with the block's parameters at P
int block_forward(dfd_handle* h, HeadTrainState* S, const float* P, int n, bool train) {
    HeadBlockState* K = S->block;
    hipStream_t s = h->stream;
    const int m = n * BK_HW;
    const dim3 blk(HT_THREADS);
    const size_t te = (size_t)m * BK_EXP, to = (size_t)m * BK_OUT;
    hipLaunchKernelGGL((gemm_fwd_kernel<BK_JE, false>), dim3(BK_EXP / (16 * BK_JE), (m + 63) / 64), blk, 0, s, K->x, nullptr, P + BO_WE,
                       K->ze, m, BK_IN, BK_EXP, BK_HW);
    bn_statistics(K, 0, K->ze, m, train, s);
    hipLaunchKernelGGL(bk_bn_swish_kernel, flat(te), blk, 0, s, K->ze, bn_consts(K, P, 0, m, false), K->ae, te, BK_EXP);
    hipLaunchKernelGGL(bk_dw_fwd_kernel, flat(te), blk, 0, s, K->ae, P + BO_WD, K->zd, te);
    bn_statistics(K, 1, K->zd, m, train, s);
    hipLaunchKernelGGL(bk_bn_swish_pool_kernel, dim3((BK_EXP + HT_THREADS - 1) / HT_THREADS, n), blk, 0, s, K->zd,
                       bn_consts(K, P, 1, m, false), K->ad, K->pooled);
    hipLaunchKernelGGL(bk_se_fwd_kernel, dim3(n), blk, 0, s, K->pooled, P + BO_W1, P + BO_B1, P + BO_W2, P + BO_B2, K->r, K->q, K->gate);
    hipLaunchKernelGGL((gemm_fwd_kernel<BK_JP, true>), dim3(BK_OUT / (16 * BK_JP), (m + 63) / 64), blk, 0, s, K->ad, K->gate, P + BO_WP,
                       K->zp, m, BK_EXP, BK_OUT, BK_HW);
    bn_statistics(K, 2, K->zp, m, train, s);
    hipLaunchKernelGGL(bk_bn_kernel, flat(to), blk, 0, s, K->zp, bn_consts(K, P, 2, m, false), headconv_rows(S), to, BK_OUT);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

// from dX15 (K->dx15) back to the gradients of the block's parameters
int block_backward(dfd_handle* h, HeadTrainState* S, int n) {
    HeadBlockState* K = S->block;
    hipStream_t s = h->stream;
    const int m = n * BK_HW, wch = wg_chunks(m);
    const dim3 blk(HT_THREADS);
    const float* P = K->param;
    float* G = K->grad;
    const size_t te = (size_t)m * BK_EXP;
    // BN2, project
    Grad2 g2{bn_consts(K, P, 2, m, true), K->zp, K->dx15};
    bn_backward_statistics(K, 2, g2, m, s);
    hipLaunchKernelGGL((wgrad_kernel<BK_JE, true, Grad2>), dim3(BK_OUT / 16 * (BK_EXP / (16 * BK_JE)) / 4, wch), blk, 0, s, g2, K->ad,
                       K->gate, K->wpart, m, BK_OUT, BK_EXP, BK_HW);
    hipLaunchKernelGGL(wreduce_kernel, flat((size_t)BK_OUT * BK_EXP), blk, 0, s, K->wpart, wch, BK_OUT * BK_EXP, G + BO_WP);
    hipLaunchKernelGGL((gemm_dyw_kernel<BK_JE, Grad2>), dim3(BK_EXP / (16 * BK_JE), (m + 15) / 16), blk, 0, s, g2, P + BO_WP, K->d1, m,
                       BK_OUT, BK_EXP);
    // squeeze-excite
    hipLaunchKernelGGL(bk_se_bwd_kernel, dim3(n), blk, 0, s, K->d1, K->ad, K->gate, K->r, P + BO_W1, P + BO_W2, K->du, K->dr, K->ds);
    hipLaunchKernelGGL(bk_se_wgrad_kernel, flat((size_t)2 * BK_EXP * BK_SE + BK_EXP + BK_SE), blk, 0, s, K->du, K->dr, K->q, K->pooled,
                       G + BO_W1, G + BO_B1, G + BO_W2, G + BO_B2, n);
    // BN1, depthwise
    Grad1 g1{bn_consts(K, P, 1, m, true), K->zd, K->d1, K->gate, K->ds};
    bn_backward_statistics(K, 1, g1, m, s);
    hipLaunchKernelGGL(bk_dz_store_kernel, flat(te), blk, 0, s, g1, K->d1, te);
    const int dch = (n + BK_DW_CROPS - 1) / BK_DW_CROPS;
    hipLaunchKernelGGL(bk_dw_wgrad_kernel, dim3((BK_EXP + HT_THREADS - 1) / HT_THREADS, 9, dch), blk, 0, s, K->d1, K->ae, K->dwpart, n);
    hipLaunchKernelGGL(bk_dw_wreduce_kernel, flat((size_t)BK_EXP * 9), blk, 0, s, K->dwpart, dch, G + BO_WD);
    hipLaunchKernelGGL(bk_dw_bwd_kernel, flat(te), blk, 0, s, K->d1, P + BO_WD, K->d2, te);
    // BN0, expand
    Grad0 g0{bn_consts(K, P, 0, m, true), K->ze, K->d2};
    bn_backward_statistics(K, 0, g0, m, s);
    hipLaunchKernelGGL((wgrad_kernel<BK_JE, false, Grad0>), dim3(BK_EXP / 16 * (BK_IN / (16 * BK_JE)) / 4, wch), blk, 0, s, g0, K->x, nullptr,
                       K->wpart, m, BK_EXP, BK_IN, BK_HW);
    hipLaunchKernelGGL(wreduce_kernel, flat((size_t)BK_EXP * BK_IN), blk, 0, s, K->wpart, wch, BK_EXP * BK_IN, G + BO_WE);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

}  // namespace

extern "C" {

int dfd_head_train_unfreeze_block(dfd_handle* h, int block, const dfd_mbconv_params* init, float bn_momentum, float bn_eps) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_unfreeze_block", false, &rc);
    if (!S) return rc;
    if (block != BK_INDEX)
        return fail(h, DFD_ERR_UNSUPPORTED, "head_train_unfreeze_block: block %d; only the last block (%d) can be unfrozen", block, BK_INDEX);
    if (!S->conv) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: the conv stage comes first (dfd_head_train_unfreeze_conv)");
    if (S->block) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: block %d is already unfrozen", BK_INDEX);
    if (S->counter) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: the trainer has accumulated already; unfreeze right after begin");
    if (!init || !block_complete(init, true)) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: null parameters");
    if (!(bn_momentum >= 0.f && bn_momentum <= 1.f && bn_eps > 0.f))
        return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: bn_momentum %g or bn_eps %g out of range", (double)bn_momentum, (double)bn_eps);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadBlockState* K = new (std::nothrow) HeadBlockState();
    if (!K) return fail(h, DFD_ERR_CAPACITY, "head_train_unfreeze_block: out of host memory");
    K->momentum = bn_momentum;
    K->eps = bn_eps == 1e-3f ? 1e-3 : (double)bn_eps;          // the backbone's eps (weights._fold's double), not its float neighbour
    const size_t mn = (size_t)S->max_n, mm = mn * BK_HW, sch = (size_t)stat_chunks((int)mm), wch = (size_t)wg_chunks((int)mm),
                 dch = (mn + BK_DW_CROPS - 1) / BK_DW_CROPS;
    struct Slot { void** p; size_t bytes; };
    std::vector<Slot> slots = {
        {(void**)&K->param, (size_t)BK_COUNT * 4}, {(void**)&K->grad, (size_t)BK_COUNT * 4}, {(void**)&K->m, (size_t)BK_COUNT * 4},
        {(void**)&K->v, (size_t)BK_COUNT * 4},     {(void**)&K->ema, (size_t)BK_COUNT * 4},
        {(void**)&K->x, mm * BK_IN * 4},   {(void**)&K->ze, mm * BK_EXP * 4}, {(void**)&K->ae, mm * BK_EXP * 4},
        {(void**)&K->zd, mm * BK_EXP * 4}, {(void**)&K->ad, mm * BK_EXP * 4}, {(void**)&K->d1, mm * BK_EXP * 4},
        {(void**)&K->d2, mm * BK_EXP * 4}, {(void**)&K->zp, mm * BK_OUT * 4}, {(void**)&K->dx15, mm * BK_OUT * 4},
        {(void**)&K->pooled, mn * BK_EXP * 4}, {(void**)&K->gate, mn * BK_EXP * 4},
        {(void**)&K->spart, sch * BK_EXP * 8}, {(void**)&K->spart2, sch * BK_EXP * 8},
        {(void**)&K->wpart, wch * (size_t)BK_OUT * BK_EXP * 8}, {(void**)&K->dwpart, dch * 9 * BK_EXP * 8},
        {(void**)&K->partial, NORM_BLOCKS * 8},
        {(void**)&K->r, mn * BK_SE * 8}, {(void**)&K->q, mn * BK_SE * 8}, {(void**)&K->du, mn * BK_EXP * 8},
        {(void**)&K->dr, mn * BK_SE * 8}, {(void**)&K->ds, mn * BK_EXP * 8},
    };
    for (int l = 0; l < 3; ++l) {
        const size_t c = (size_t)kBnC[l];
        slots.push_back({(void**)&K->rm[l], c * 4});
        slots.push_back({(void**)&K->rv[l], c * 4});
        slots.push_back({(void**)&K->mean[l], c * 8});
        slots.push_back({(void**)&K->istd[l], c * 8});
        slots.push_back({(void**)&K->sdy[l], c * 8});
        slots.push_back({(void**)&K->sdx[l], c * 8});
    }
    size_t total = 0;
    for (const Slot& sl : slots) total += (sl.bytes + 255) / 256 * 256;
    if (hipMalloc(&K->pool, total) != hipSuccess) {
        delete K;
        return fail(h, DFD_ERR_HIP, "head_train_unfreeze_block: hipMalloc of %zu bytes failed", total);
    }
    size_t off = 0;
    for (const Slot& sl : slots) {
        *sl.p = static_cast<char*>(K->pool) + off;
        off += (sl.bytes + 255) / 256 * 256;
    }
    S->block = K;
    auto bail = [&](hipError_t e, const char* what) {
        headblock_destroy(S);
        return fail(h, DFD_ERR_HIP, "head_train_unfreeze_block: %s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMemsetAsync(K->pool, 0, total, h->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
    for (const BField& f : kBlockTrainable)
        if ((e = hipMemcpyAsync(K->param + f.off, init->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "parameter upload");
    for (int l = 0; l < 3; ++l) {
        if ((e = hipMemcpyAsync(K->rm[l], init->*kBlockStats[l].rm, (size_t)kBnC[l] * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "statistics upload");
        if ((e = hipMemcpyAsync(K->rv[l], init->*kBlockStats[l].rv, (size_t)kBnC[l] * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "statistics upload");
    }
    if ((e = hipMemcpyAsync(K->ema, K->param, (size_t)BK_COUNT * 4, hipMemcpyDeviceToDevice, h->stream)) != hipSuccess) return bail(e, "shadow copy");
    if ((e = stream_sync(h)) != hipSuccess) return bail(e, "stream wait");
    return DFD_OK;
}

int dfd_head_train_accumulate_block(dfd_handle* h, const float* rows, int n, const float* labels_a, const float* labels_b, float lam,
                                    float loss_scale, float* loss_out, float* logits_out) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_accumulate_block", true, &rc);
    if (!S) return rc;
    if (!rows || !labels_a || !loss_out) return fail(h, DFD_ERR_ARG, "head_train_accumulate_block: null pointer");
    if (n < 2) return fail(h, DFD_ERR_ARG, "head_train_accumulate_block: %d rows; batch statistics need at least 2", n);
    if (n > S->max_n) return fail(h, DFD_ERR_ARG, "head_train_accumulate_block: %d rows exceed the trainer's max_n %d", n, S->max_n);
    if (!head_train_mix_ok(lam, loss_scale))
        return fail(h, DFD_ERR_ARG, "head_train_accumulate_block: lam %g outside [0, 1] or loss_scale %g not a number", (double)lam, (double)loss_scale);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadBlockState* K = S->block;
    hipStream_t s = h->stream;
    DFD_HIP_TRY(h, hipMemcpyAsync(K->x, rows, (size_t)n * BK_ROW * 4, hipMemcpyHostToDevice, s));
    if ((rc = block_forward(h, S, K->param, n, true))) return rc;
    if ((rc = headconv_step(h, S, n, labels_a, labels_b, lam, loss_scale, K->dx15))) return rc;
    if ((rc = block_backward(h, S, n))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(loss_out, S->scalars, 4, hipMemcpyDeviceToHost, s));
    if (logits_out) DFD_HIP_TRY(h, hipMemcpyAsync(logits_out, S->logits, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));
    S->last_n = n;
    ++S->counter;
    return DFD_OK;
}

int dfd_head_train_eval_block(dfd_handle* h, const float* rows, int n, int use_ema, float* logits_out) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_eval_block", true, &rc);
    if (!S) return rc;
    if (!rows || !logits_out) return fail(h, DFD_ERR_ARG, "head_train_eval_block: null pointer");
    if (n < 1 || n > S->max_n) return fail(h, DFD_ERR_ARG, "head_train_eval_block: %d rows outside 1..%d", n, S->max_n);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadBlockState* K = S->block;
    DFD_HIP_TRY(h, hipMemcpyAsync(K->x, rows, (size_t)n * BK_ROW * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = block_forward(h, S, use_ema ? K->ema : K->param, n, false))) return rc;
    if ((rc = headconv_eval_step(h, S, use_ema, n))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(logits_out, S->logits, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_head_train_export_block(dfd_handle* h, int use_ema, dfd_mbconv_params* out) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_export_block", true, &rc);
    if (!S) return rc;
    if (!out || !block_complete(out, true)) return fail(h, DFD_ERR_ARG, "head_train_export_block: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadBlockState* K = S->block;
    const float* P = use_ema ? K->ema : K->param;
    for (const BField& f : kBlockTrainable)
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*f.ptr, P + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    for (int l = 0; l < 3; ++l) {
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*kBlockStats[l].rm, K->rm[l], (size_t)kBnC[l] * 4, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*kBlockStats[l].rv, K->rv[l], (size_t)kBnC[l] * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_head_train_block_grads(dfd_handle* h, dfd_mbconv_params* io, int set) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_block_grads", true, &rc);
    if (!S) return rc;
    if (!io || !block_complete(io, false)) return fail(h, DFD_ERR_ARG, "head_train_block_grads: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    HeadBlockState* K = S->block;
    for (const BField& f : kBlockTrainable) {
        if (set) DFD_HIP_TRY(h, hipMemcpyAsync(K->grad + f.off, io->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream));
        else DFD_HIP_TRY(h, hipMemcpyAsync(io->*f.ptr, K->grad + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

}  // extern "C"

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
// Without block 14's stage no gradient with respect to X is formed.
//
// Block 14 (dfd_head_train_unfreeze_block_at): net._blocks.14 (MBConv k5, pad 2, 192 -> 1152 -> 192, the identity skip with
// per-crop drop-connect) runs the same launches in front of block 15 on a second state, through the geometry parameter
// (Geo: kernel size, output width, skip) the host functions below are instantiated with.  Its last forward launch
// (bk_bn_skip_kernel) writes out = x13 + (BN2(Zp) / keep_prob) b_i into block 15's input buffer; block 15's backward then
// ends with dOut14 = dZe15 . We15 (gemm_dyw<6, Grad0>), and block 14's BN2 takes dOut14 b_i / keep_prob as its gradient
// source (Grad2<true>).
//
// Blocks 13 and 12 (the same entry, once the block above is unfrozen) have block 14's geometry exactly and run block 14's
// instantiations on a third and a fourth state; the block's index is a run-time field that only names taps, plan entries
// and messages.  Block b writes its output into block b + 1's input buffer.  A trained skip block with a trained block
// below it hands down dX_b = dOut_b + dZe_b . We_b (gemm_dyw<6, Grad0, true>: the skip path added to the branch in double,
// one rounding) into that block's dx; the deepest trained block hands nothing down.  Block b draws its drop-connect mask
// from the trainer's hash with layer 17 - b.
//
// Block 11 (the same entry, once block 12 is unfrozen): net._blocks.11 (MBConv k5 at stride 2 with TF-"SAME" padding 1 before
// and 2 after, 112 -> 672 -> 192, squeeze-excite 28, 14 x 14 -> 7 x 7, no skip and so no drop-connect) runs the same chain on
// a fifth state through the geometry G11: m0 = 196 n rows in front of the depthwise conv (X, Ze, ae, dae, BN0's statistics),
// m1 = 49 n after it; the depthwise conv, its input gradient (a gather per input element) and its weight gradient are the
// bk_dws_* kernels; the channel statistics over 672 channels and the expand's weight gradient (42 waves) run the guarded
// instances of head_train_gemm.h.  Its last forward launch (bk_bn_kernel) writes BN2(Zp) into block 12's input buffer, block
// 12 hands dX12 = dOut12 + dZe12 . We12 into its dx, and it forms no input gradient itself: block 10 is frozen.
//
// Arithmetic as head_train_conv.hip: the GEMMs run on the fp64 MFMA with fp32 operands widened at the load
// (head_train_gemm.h), every other element is computed in double from stored fp32 values and rounded once where it is
// stored.  ye, yd, t = ad * gate and the dZ of the three BatchNorms are never stored; the small squeeze-excite vectors
// (r, q, du, dr, ds) stay in double.  Every reduction has a fixed order and no atomics: channel statistics over 256-row
// chunks, weight gradients over 512-row chunks, the depthwise weight gradient over 8-crop chunks, the squeeze-excite
// weight gradients over the crops one by one - added in that order, in double.  Built with -ffp-contract=off.
#include <algorithm>
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

// What the blocks of one width share: input width, expanded width, squeeze width, the input's edge and the depthwise
// conv's stride.  HW_IN positions a crop in front of the depthwise conv (the rows of X, Ze, ae, dae), HW after it (Zd, ad,
// dt, Zp, the output); the two are one number at stride 1.  The kernels that index by these take the shape as a parameter.
template <int IN_, int EXP_, int SE_, int H_IN_, int STRIDE_>
struct Shape {
    static constexpr int IN = IN_, EXP = EXP_, SE = SE_, H_IN = H_IN_, STRIDE = STRIDE_;
    static constexpr int H = (H_IN_ + STRIDE_ - 1) / STRIDE_, HW_IN = H_IN * H_IN, HW = H * H, ROW = HW_IN * IN;
    static_assert(SE % 4 == 0, "a wave of the squeeze-excite kernels owns SE / 4 of the squeezed values");
};
typedef Shape<192, 1152, 48, 7, 1> S7;    // blocks 12-15: 192 -> 1152, squeeze-excite 48, 7 x 7
typedef Shape<112, 672, 28, 14, 2> S14;   // block 11: 112 -> 672, squeeze-excite 28, 14 x 14 -> 7 x 7
constexpr int BK_DW_CROPS = 8;            // crops of one partial depthwise weight gradient
// A block's geometry: its shape, its depthwise kernel size and low pad (the high pad follows from TF-"SAME"), output width,
// whether it has the identity skip, and the column tiles a wave takes: JP in the projection's forward GEMM, JE in the
// expand's forward GEMM, gemm_dyw and the projection's weight gradient (EXP = 96 x ..), JW over the input width in the
// expand's weight gradient.  The block group's arena (floats); every offset a multiple of 4.
template <class S_, int KS_, int PAD_, int OUT_, bool SKIP_, int JP_, int JE_, int JW_>
struct Geo {
    typedef S_ S;
    static constexpr int IN = S::IN, EXP = S::EXP, SE = S::SE, HW_IN = S::HW_IN, HW = S::HW, STRIDE = S::STRIDE;
    static constexpr int KS = KS_, TAPS = KS_ * KS_, PAD = PAD_, OUT = OUT_, JP = JP_, JE = JE_, JW = JW_;
    static constexpr bool SKIP = SKIP_;
    static constexpr int O_WE = 0, O_WD = O_WE + EXP * IN, O_W1 = O_WD + EXP * TAPS, O_B1 = O_W1 + SE * EXP;
    static constexpr int O_W2 = O_B1 + SE, O_B2 = O_W2 + EXP * SE, O_WP = O_B2 + EXP, O_G0 = O_WP + OUT * EXP;
    static constexpr int O_BE0 = O_G0 + EXP, O_G1 = O_BE0 + EXP, O_BE1 = O_G1 + EXP, O_G2 = O_BE1 + EXP;
    static constexpr int O_BE2 = O_G2 + OUT, COUNT = O_BE2 + OUT;
    // waves of the two weight-gradient launches; the expand's may be no multiple of 4 (the guarded instance takes it)
    static constexpr int WP_WAVES = OUT / 16 * (EXP / (16 * JE)), WE_WAVES = EXP / 16 * (IN / (16 * JW));
    static constexpr bool WE_GUARD = WE_WAVES % 4 != 0;
    static_assert(EXP % (16 * JE) == 0 && OUT % (16 * JP) == 0 && IN % (16 * JW) == 0 && IN % 16 == 0 && EXP % 16 == 0, "tiles");
    static_assert(WP_WAVES % 4 == 0, "the projection's weight-gradient grid");
    static_assert(OUT % 16 == 0, "gemm_dyw splits its channels over four waves");
    static_assert(O_WD % 4 == 0 && O_W1 % 4 == 0 && O_W2 % 4 == 0 && O_WP % 4 == 0, "weight rows must stay 16-byte aligned");
    static_assert(!SKIP || (STRIDE == 1 && OUT == IN), "the identity skip");
    static_assert(PAD == (S::H * STRIDE + KS - STRIDE - S::H_IN) / 2, "TF-SAME: the smaller half of the padding comes first");
};
typedef Geo<S7, 3, 1, 320, false, 5, 6, 6> G15;     // block 15; 320 = 4 x 80, 1152 = 12 x 96, 192 = 2 x 96
typedef Geo<S7, 5, 2, 192, true, 6, 6, 6> G14;      // blocks 14, 13 and 12; 192 = 2 x 96
typedef Geo<S14, 5, 1, 192, false, 6, 6, 7> G11;    // block 11: stride 2, pad 1 / 2; 672 = 7 x 96, 112 = 7 x 16
constexpr int BK_LAST = 15, BK_FIRST = BK_LAST - (HT_STAGES - 1);   // the blocks a trainer can hold: stage k = block 15 - k
constexpr int BK_STRIDED = 11;            // the one block of the range with G11's geometry; 12 .. 14 have G14's
static_assert(BK_FIRST == BK_STRIDED, "the deepest stage is block 11");
static_assert(G15::COUNT == 717232, "trainable floats of block 15");
static_assert(G14::COUNT == 587952, "trainable floats of each of blocks 14, 13 and 12");
static_assert(G11::COUNT == 262492, "trainable floats of block 11");
static_assert(!G15::WE_GUARD && !G14::WE_GUARD && G11::WE_GUARD && G11::WE_WAVES == 42, "only block 11's expand needs the guarded weight gradient");
static_assert(DFD_TRUNK_ROW == S7::HW * G15::OUT, "block 15's output is the conv stage's row");
static_assert(G14::OUT == S7::IN && S7::IN % (16 * G14::JE) == 0, "a skip block's output is the next block's input; dOut = dZe . We in 96-column tiles");
static_assert(G11::OUT == S7::IN && G11::HW == S7::HW_IN, "block 11's output is block 12's input");
// the same at run time, for the host code that only moves tensors
struct Layout {
    int index, ks, taps, out;
    bool skip;
    int o_we, o_wd, o_w1, o_b1, o_w2, o_b2, o_wp, o_g[3], o_be[3], count, bnc[3];
    int in, exp, se, hw_in, hw, stride;
};
template <class G>
Layout layout_of(int index) {
    return Layout{index, G::KS, G::TAPS, G::OUT, G::SKIP, G::O_WE, G::O_WD, G::O_W1, G::O_B1, G::O_W2, G::O_B2, G::O_WP,
                  {G::O_G0, G::O_G1, G::O_G2}, {G::O_BE0, G::O_BE1, G::O_BE2}, G::COUNT, {G::EXP, G::EXP, G::OUT},
                  G::IN, G::EXP, G::SE, G::HW_IN, G::HW, G::STRIDE};
}

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

// A skip block's output: out = x + (BN(Zp) / keep_prob) b_i (efficientnet_pytorch's drop_connect), in double, rounded once.
// keep [crop] != 0 where b_i = 1 (null: every crop kept - eval, with keep_prob = 1); a dropped crop's output is its input
// row bit for bit.  X and out are different buffers.
template <class S>
__global__ __launch_bounds__(HT_THREADS) void bk_bn_skip_kernel(const float* __restrict__ Z, BnC bn, const float* __restrict__ X,
                                                                const float* __restrict__ keep, double keep_prob,
                                                                float* __restrict__ out, size_t total, int C) {
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    if (keep && keep[i / ((size_t)S::HW * C)] == 0.f) {
        out[i] = X[i];
        return;
    }
    const int c = (int)(i % C);
    const BnK k = bn.load(c);
    const double y = (((double)Z[i] - k.mean) * k.istd) * k.gamma + k.beta;
    out[i] = (float)((double)X[i] + y / keep_prob);
}

// eval mode: the running statistics in the place of the batch's
__global__ __launch_bounds__(HT_THREADS) void bk_eval_consts_kernel(const float* __restrict__ rm, const float* __restrict__ rv, double eps,
                                                                    double* __restrict__ mean, double* __restrict__ istd, int C) {
    const int c = blockIdx.x * HT_THREADS + threadIdx.x;
    if (c >= C) return;
    mean[c] = (double)rm[c];
    istd[c] = 1.0 / sqrt((double)rv[c] + eps);
}

// Depthwise KS x KS at stride 1, pad KS / 2, on [n][7][7][1152]: one thread per output element, channels fastest; the KS KS taps in
// (ky, kx) order in double, taps outside the 7 x 7 left out (at KS = 5 every position has some, 16 of 25 in the corners).
// W [c][ky][kx] (torch's layout).
template <class S, int KS>
__global__ __launch_bounds__(HT_THREADS) void bk_dw_fwd_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                               float* __restrict__ Z, size_t total) {
    static_assert(S::STRIDE == 1, "the strided form is bk_dws_fwd_kernel");
    constexpr int BK_EXP = S::EXP, BK_HW = S::HW, BK_H = S::H;
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % BK_EXP), p = (int)((i / BK_EXP) % BK_HW), y = p / BK_H, x = p % BK_H;
    const size_t base = i - (size_t)p * BK_EXP;                  // position 0 of this crop, channel c
    double s = 0.0;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int yy = y + ky - KS / 2, xx = x + kx - KS / 2;
            if (yy < 0 || yy >= BK_H || xx < 0 || xx >= BK_H) continue;
            s += (double)A[base + (size_t)(yy * BK_H + xx) * BK_EXP] * (double)W[c * (KS * KS) + ky * KS + kx];
        }
    }
    Z[i] = (float)s;
}

// The same at a stride (block 11: 5 x 5, stride 2, pad 1 before and 2 after, [n][14][14][672] -> [n][7][7][672]): one thread
// per OUTPUT element; output (oy, ox) reads input (STRIDE oy - PAD + ky, STRIDE ox - PAD + kx), the taps in (ky, kx) order in
// double, taps outside the input left out (9 live taps of 25 in the corner (6, 6), 16 in (0, 0)).  total = n HW EXP.
template <class S, int KS, int PAD>
__global__ __launch_bounds__(HT_THREADS) void bk_dws_fwd_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                                float* __restrict__ Z, size_t total) {
    constexpr int EXP = S::EXP, H = S::H, H_IN = S::H_IN;
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % EXP), p = (int)((i / EXP) % S::HW), oy = p / H, ox = p % H;
    const size_t base = (i / ((size_t)S::HW * EXP)) * ((size_t)S::HW_IN * EXP) + c;      // input position 0 of this crop, channel c
    double s = 0.0;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int yy = S::STRIDE * oy - PAD + ky, xx = S::STRIDE * ox - PAD + kx;
            if (yy < 0 || yy >= H_IN || xx < 0 || xx >= H_IN) continue;
            s += (double)A[base + (size_t)(yy * H_IN + xx) * EXP] * (double)W[c * (KS * KS) + ky * KS + kx];
        }
    }
    Z[i] = (float)s;
}

// ad = swish(BN(Zd)) and its mean over the HW output positions (49): grid (ceil(EXP / 256), n), one thread per (crop,
// channel).  The pooled value is the sum of the stored fp32 ad in position order / 49, rounded once.
template <class S>
__global__ __launch_bounds__(HT_THREADS) void bk_bn_swish_pool_kernel(const float* __restrict__ Z, BnC bn, float* __restrict__ AD,
                                                                      float* __restrict__ pooled) {
    constexpr int BK_EXP = S::EXP, BK_HW = S::HW;
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

// Squeeze-excite forward, one block per crop: r = W1 s + b1 [SE], q = swish(r), u = W2 q + b2 [EXP], gate = sigmoid(u).
// A wave owns SE / 4 of the r (12 of 48; 7 of 28): lanes take the EXP terms 64 apart (at 672 the upper half of the lanes
// one term fewer), then the fixed tree.  r, q stay in double.
template <class S>
__global__ __launch_bounds__(HT_THREADS) void bk_se_fwd_kernel(const float* __restrict__ pooled, const float* __restrict__ W1,
                                                               const float* __restrict__ B1, const float* __restrict__ W2,
                                                               const float* __restrict__ B2, double* __restrict__ R,
                                                               double* __restrict__ Q, float* __restrict__ gate) {
    constexpr int BK_EXP = S::EXP, BK_SE = S::SE;
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
// BN2: dy is the stored gradient of the block's output (dX15); with the skip (SKIP) that gradient times the crop's
// drop-connect factor, dOut14 b_i / keep_prob: exactly zero on a dropped crop
template <bool SKIP, int BK_HW = S7::HW>
struct Grad2 {
    typedef BnK K;
    BnC bn;
    const float *Zp, *dX;
    int out;
    const float* keep;
    double keep_prob;
    __device__ __forceinline__ K load(int c) const { return bn.load(c); }
    __device__ __forceinline__ void dy_xh(const K& k, size_t row, int c, double* dy, double* xh) const {
        const size_t o = row * out + c;
        *xh = ((double)Zp[o] - k.mean) * k.istd;
        if constexpr (SKIP) *dy = keep[row / BK_HW] == 0.f ? 0.0 : (double)dX[o] / keep_prob;
        else *dy = (double)dX[o];
    }
};
// BN1: dad = dt gate + ds / 49 through swish'(yd)
template <class S>
struct Grad1 {
    static constexpr int BK_EXP = S::EXP, BK_HW = S::HW;
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
template <class S>
struct Grad0 {
    static constexpr int BK_EXP = S::EXP;
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
template <class S>
__global__ __launch_bounds__(HT_THREADS) void bk_se_bwd_kernel(const float* __restrict__ dT, const float* __restrict__ AD,
                                                               const float* __restrict__ gate, const double* __restrict__ R,
                                                               const float* __restrict__ W1, const float* __restrict__ W2,
                                                               double* __restrict__ dU, double* __restrict__ dR, double* __restrict__ dS) {
    constexpr int BK_EXP = S::EXP, BK_SE = S::SE, BK_HW = S::HW;
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
template <class S>
__global__ __launch_bounds__(HT_THREADS) void bk_se_wgrad_kernel(const double* __restrict__ dU, const double* __restrict__ dR,
                                                                 const double* __restrict__ Q, const float* __restrict__ pooled,
                                                                 float* __restrict__ gW1, float* __restrict__ gB1,
                                                                 float* __restrict__ gW2, float* __restrict__ gB2, int n) {
    constexpr int BK_EXP = S::EXP, BK_SE = S::SE, NW = BK_EXP * BK_SE;
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
template <class S>
__global__ __launch_bounds__(HT_THREADS) void bk_dz_store_kernel(Grad1<S> g, float* out, size_t total) {
    constexpr int BK_EXP = S::EXP;
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % BK_EXP);
    const BnK k = g.load(c);
    out[i] = (float)bn_dz(g, k, i / BK_EXP, c);
}

// dae [y][x] = sum over (ky, kx) of dZd [y - ky + KS / 2][x - kx + KS / 2] W [ky][kx]: the correlation with the flipped
// kernel, pad KS / 2
template <class S, int KS>
__global__ __launch_bounds__(HT_THREADS) void bk_dw_bwd_kernel(const float* __restrict__ dZ, const float* __restrict__ W,
                                                               float* __restrict__ dA, size_t total) {
    static_assert(S::STRIDE == 1, "the strided form is bk_dws_bwd_kernel");
    constexpr int BK_EXP = S::EXP, BK_HW = S::HW, BK_H = S::H;
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % BK_EXP), p = (int)((i / BK_EXP) % BK_HW), y = p / BK_H, x = p % BK_H;
    const size_t base = i - (size_t)p * BK_EXP;
    double s = 0.0;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int yy = y - ky + KS / 2, xx = x - kx + KS / 2;
            if (yy < 0 || yy >= BK_H || xx < 0 || xx >= BK_H) continue;
            s += (double)dZ[base + (size_t)(yy * BK_H + xx) * BK_EXP] * (double)W[c * (KS * KS) + ky * KS + kx];
        }
    }
    dA[i] = (float)s;
}

// The same at a stride, as a gather (no atomics, no scatter): one thread per INPUT element (iy, ix); it collects the taps
// with STRIDE oy - PAD + ky = iy, in (ky, kx) order - at stride 2 and pad 1 an even iy takes ky in {1, 3}, an odd one ky in
// {0, 2, 4}, so an element sums 4, 6 or 9 taps before the border removes those whose output lies outside the 7 x 7.
// dZ [n][HW][EXP] -> dA [n][HW_IN][EXP]; total = n HW_IN EXP.
template <class S, int KS, int PAD>
__global__ __launch_bounds__(HT_THREADS) void bk_dws_bwd_kernel(const float* __restrict__ dZ, const float* __restrict__ W,
                                                                float* __restrict__ dA, size_t total) {
    constexpr int EXP = S::EXP, H = S::H, H_IN = S::H_IN, ST = S::STRIDE;
    const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % EXP), p = (int)((i / EXP) % S::HW_IN), iy = p / H_IN, ix = p % H_IN;
    const size_t base = (i / ((size_t)S::HW_IN * EXP)) * ((size_t)S::HW * EXP) + c;      // output position 0 of this crop, channel c
    double s = 0.0;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
        const int ty = iy + PAD - ky;                            // = STRIDE oy
        if (ty < 0 || ty % ST != 0 || ty / ST >= H) continue;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int tx = ix + PAD - kx;
            if (tx < 0 || tx % ST != 0 || tx / ST >= H) continue;
            s += (double)dZ[base + (size_t)((ty / ST) * H + tx / ST) * EXP] * (double)W[c * (KS * KS) + ky * KS + kx];
        }
    }
    dA[i] = (float)s;
}

// Partial depthwise weight gradient of crops [8 chunk, 8 (chunk + 1)) n [0, n): P [chunk][tap][c] = sum over those crops
// and the positions (crop, then position order) of dZd [y][x] ae [y + ky - KS / 2][x + kx - KS / 2].
// grid (ceil(1152 / 256), KS KS, chunks).
template <class S, int KS>
__global__ __launch_bounds__(HT_THREADS) void bk_dw_wgrad_kernel(const float* __restrict__ dZ, const float* __restrict__ A,
                                                                 double* __restrict__ P, int n) {
    static_assert(S::STRIDE == 1, "the strided form is bk_dws_wgrad_kernel");
    constexpr int BK_EXP = S::EXP, BK_HW = S::HW, BK_H = S::H;
    const int c = blockIdx.x * HT_THREADS + threadIdx.x, tap = blockIdx.y, ky = tap / KS, kx = tap % KS;
    if (c >= BK_EXP) return;
    const int i0 = blockIdx.z * BK_DW_CROPS, i1 = min(n, i0 + BK_DW_CROPS);
    double s = 0.0;
    for (int i = i0; i < i1; ++i) {
        const size_t base = (size_t)i * BK_HW * BK_EXP + c;
        for (int y = 0; y < BK_H; ++y) {
            const int yy = y + ky - KS / 2;
            if (yy < 0 || yy >= BK_H) continue;
            for (int x = 0; x < BK_H; ++x) {
                const int xx = x + kx - KS / 2;
                if (xx < 0 || xx >= BK_H) continue;
                s += (double)dZ[base + (size_t)(y * BK_H + x) * BK_EXP] * (double)A[base + (size_t)(yy * BK_H + xx) * BK_EXP];
            }
        }
    }
    P[((size_t)blockIdx.z * (KS * KS) + tap) * BK_EXP + c] = s;
}

// The same at a stride: P [chunk][tap][c] = sum over the chunk's crops and the OUTPUT positions (crop, then position order)
// of dZd [oy][ox] ae [STRIDE oy - PAD + ky][STRIDE ox - PAD + kx], positions whose tap lies outside the input left out.
template <class S, int KS, int PAD>
__global__ __launch_bounds__(HT_THREADS) void bk_dws_wgrad_kernel(const float* __restrict__ dZ, const float* __restrict__ A,
                                                                  double* __restrict__ P, int n) {
    constexpr int EXP = S::EXP, H = S::H, H_IN = S::H_IN, ST = S::STRIDE;
    const int c = blockIdx.x * HT_THREADS + threadIdx.x, tap = blockIdx.y, ky = tap / KS, kx = tap % KS;
    if (c >= EXP) return;
    const int i0 = blockIdx.z * BK_DW_CROPS, i1 = min(n, i0 + BK_DW_CROPS);
    double s = 0.0;
    for (int i = i0; i < i1; ++i) {
        const size_t zb = (size_t)i * S::HW * EXP + c, ab = (size_t)i * S::HW_IN * EXP + c;
        for (int oy = 0; oy < H; ++oy) {
            const int yy = ST * oy - PAD + ky;
            if (yy < 0 || yy >= H_IN) continue;
            for (int ox = 0; ox < H; ++ox) {
                const int xx = ST * ox - PAD + kx;
                if (xx < 0 || xx >= H_IN) continue;
                s += (double)dZ[zb + (size_t)(oy * H + ox) * EXP] * (double)A[ab + (size_t)(yy * H_IN + xx) * EXP];
            }
        }
    }
    P[((size_t)blockIdx.z * (KS * KS) + tap) * EXP + c] = s;
}

// G [c][tap] += the chunks' partials added in chunk order, rounded once
template <class S>
__global__ __launch_bounds__(HT_THREADS) void bk_dw_wreduce_kernel(const double* __restrict__ P, int chunks, float* __restrict__ G,
                                                                   int taps) {
    constexpr int BK_EXP = S::EXP;
    const int e = blockIdx.x * HT_THREADS + threadIdx.x;
    if (e >= BK_EXP * taps) return;
    const int tap = e / BK_EXP, c = e % BK_EXP;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += P[((size_t)k * taps + tap) * BK_EXP + c];
    G[c * taps + tap] += (float)s;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- host
namespace dfd {

struct HeadBlockState {
    Layout L{};
    float momentum = 0.01f;
    double eps = 1e-3;
    float *param = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *ema = nullptr;
    float *rm[3] = {nullptr, nullptr, nullptr}, *rv[3] = {nullptr, nullptr, nullptr};
    // fp32 tensors of m rows: the input, Ze, ae, Zd, ad, dt then dZd (d1), dae (d2), Zp, the gradient of the block's output
    // (dx: dX15, or dOut14); per crop: the pooled s, gate
    float *x = nullptr, *ze = nullptr, *ae = nullptr, *zd = nullptr, *ad = nullptr, *d1 = nullptr, *d2 = nullptr, *zp = nullptr,
          *dx = nullptr, *pooled = nullptr, *gate = nullptr;
    double *mean[3] = {nullptr, nullptr, nullptr}, *istd[3] = {nullptr, nullptr, nullptr}, *sdy[3] = {nullptr, nullptr, nullptr},
           *sdx[3] = {nullptr, nullptr, nullptr};
    double *spart = nullptr, *spart2 = nullptr, *wpart = nullptr, *dwpart = nullptr, *partial = nullptr;
    double *r = nullptr, *q = nullptr, *du = nullptr, *dr = nullptr, *ds = nullptr;
    // the skip's drop-connect (blocks 14, 13, 12): rate, 1 - rate, floor(rate 2^32); per crop the factor of the last accumulate,
    // 0 or 1 / keep_prob ("b14.keep"), on the device and as it was uploaded; the norm this arena's AdamW launch writes
    double drop_p = 0.0, keep_prob = 1.0;
    uint32_t drop_thr = 0;
    float *keep = nullptr, *norm = nullptr;
    std::vector<float> keep_host;
    void* pool = nullptr;
};

namespace {
void destroy_one(HeadBlockState** slot) {
    HeadBlockState* K = *slot;
    if (!K) return;
    if (K->pool) hipFree(K->pool);
    delete K;
    *slot = nullptr;
}
// the stage of block 15 .. 11, or null where it is not unfrozen (or the trainer holds no such block)
HeadBlockState* stage_of(HeadTrainState* S, int block) {
    return block >= BK_FIRST && block <= BK_LAST ? S->stage[BK_LAST - block] : nullptr;
}
const char* unfreeze_entry(int block) { return block == BK_LAST ? "dfd_head_train_unfreeze_block" : "dfd_head_train_unfreeze_block_at"; }
}  // namespace

void headblock_destroy(HeadTrainState* S) {
    for (int k = HT_STAGES - 1; k >= 0; --k) destroy_one(&S->stage[k]);
}

const double* headblock_sumsq(dfd_handle* h, HeadTrainState* S, int k) {
    HeadBlockState* K = S->stage[k];
    head_train_launch_sumsq(h->stream, K->grad, K->L.count, K->partial);
    return K->partial;
}

const double* headblock_partial(HeadTrainState* S, int k) {
    HeadBlockState* K = S->stage[k];
    return K ? K->partial : nullptr;
}

void headblock_adamw(dfd_handle* h, HeadTrainState* S, double lr, double t) {
    // the arenas' partials in the order of the other launches (head, conv, block 15, 14, 13, 12, 11): all see the same norm
    const NormParts parts = head_train_norm_parts(S);
    for (int k = 0; k < HT_STAGES && S->stage[k]; ++k) {
        HeadBlockState* K = S->stage[k];
        head_train_launch_adamw(h->stream, K->param, K->grad, K->m, K->v, K->ema, K->L.count, parts, S->cfg,
                                lr * (double)headconv_lr_scale(S), t, k == 0 ? S->scalars + 3 : K->norm);
    }
}

int headblock_tap(dfd_handle* h, HeadTrainState* S, const char* name, float* out, size_t capacity) {
    const int block = 10 + (name[2] - '0'), k = BK_LAST - block;             // "b15." .. "b11.": the caller checked the prefix
    const bool below = block != BK_LAST;                        // a block under block 15: its output is the next stage's input
    HeadBlockState* K = stage_of(S, block);
    if (!K)
        return fail(h, DFD_ERR_ARG, "head_train_tap: '%s' needs block %d's stage (%s)", name, block, unfreeze_entry(block));
    const float* src = nullptr;
    size_t per = 0;
    const char* what = name + 4;
    // a block's output lives in the next stage's input buffer
    const Layout& L = K->L;
    if (!strcmp(what, "out")) { src = below ? S->stage[k - 1]->x : headconv_rows(S); per = (size_t)L.hw * L.out; }
    else if (!strcmp(what, "gate")) { src = K->gate; per = L.exp; }
    else if (!strcmp(what, "ad")) { src = K->ad; per = (size_t)L.hw * L.exp; }
    else if (!strcmp(what, "dout")) { src = K->dx; per = (size_t)L.hw * L.out; }
    else if (!strcmp(what, "dae")) { src = K->d2; per = (size_t)L.hw_in * L.exp; }
    else if (L.skip && !strcmp(what, "keep")) { src = K->keep; per = 1; }      // block 11 has no skip: no "b11.keep"
    else return fail(h, DFD_ERR_ARG, "head_train_tap: unknown tap '%s'", name);
    const size_t count = (size_t)S->last_n * per;
    if (capacity < count) return fail(h, DFD_ERR_ARG, "head_train_tap: '%s' holds %zu floats, capacity %zu", name, count, capacity);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipMemcpy(out, src, count * 4, hipMemcpyDeviceToHost));
    return DFD_OK;
}

// A trained block's ten tensors of the inference plan, rewritten in place from the trained parameters (live or EMA) and the
// running statistics: weights._fold's arithmetic (a = g / sqrt(var + eps); w' = w a; b' = 0 a + (beta - mu a), float64,
// rounded once) and weights.pack_b0_tensors' layouts (dw.w [ky][kx][c] with 9 or 25 taps, se.w2 [SE][EXP]).  Readers of
// these pointers, for blocks 15, 14, 13 and 12 alike (b0_forward's block loop treats all four as "late" 7 x 7 blocks):
// launch_mbconv_front (mbconv_late_kernel for k3, and for k5 the fused front launch mbconv_k5_kernel in its modes 1 and 2:
// exp.w through its cached split AND the fp32 tensor, exp.b, dw.w, dw.b), the unfused pointwise_t (exp.w / proj.w: the
// cached split under the split GEMM and, in the bf16-activation instances under "bf16_activations", always; the fp32 tensor
// in launch_pointwise), launch_depthwise (dw.w, dw.b; fp32 and bf16 instances), launch_se (se.w1, se.b1, se.w2, se.b2) and
// the projection's bias (proj.b); the projections of blocks 14, 13 and 12 also add their input (the skip), which is no weight.  The two cached
// splits are rebuilt in place, so plan and tile-table pointers stay valid.
// Block 11 (112 -> 672 -> 192, k5 at stride 2, 14 x 14 -> 7 x 7) is no "late" 7 x 7 block.  Readers of its ten tensors in
// b0_forward's block loop: launch_mbconv_front with mbconv_k5_kernel as the per-image instance of "fuse_k5" (block 11 has no
// mbconv_late_kernel form, so always mode 2: exp.w through its cached split AND the fp32 tensor, exp.b, dw.w, dw.b) and the
// other fused front modes (mbconv_kernel under "fuse_expand": the same five pointers); the standalone expand GEMM
// (pointwise_t on exp.w / exp.b: the cached split under the split GEMM, the fp32 tensor in launch_pointwise); the unfused
// launch_depthwise (dw.w, dw.b) and launch_se (se.w1, se.b1, se.w2, se.b2); the projection (pointwise_t on proj.w through
// its cached split, proj.b; no skip input); and the bf16-activation instances of all of these, which always read the
// cached splits.  Every one of them reads through the plan's pointers or h->wsplit's entry for that pointer at launch time;
// nothing holds a copy, so the in-place writes below reach all of them.
static int commit_one(dfd_handle* h, HeadBlockState* K, int use_ema) {
    const Layout& L = K->L;
    if ((int)h->b0.blocks.size() <= L.index) return fail(h, DFD_ERR_STATE, "head_train_commit: the plan has no block %d", L.index);
    const B0Block& b = h->b0.blocks[L.index];
    if (b.c_in != L.in || b.c_exp != L.exp || b.c_se != L.se || b.c_out != L.out || b.kernel != L.ks || (b.skip != 0) != L.skip ||
        b.stride != L.stride)
        return fail(h, DFD_ERR_STATE, "head_train_commit: block %d of the plan is not %d -> %d -> %d, k%d at stride %d", L.index, L.in, L.exp,
                    L.out, L.ks, L.stride);
    const int T = L.taps, OUT = L.out, BK_IN = L.in, BK_EXP = L.exp, BK_SE = L.se;
    std::vector<float> P(L.count), rm[3], rv[3];
    DFD_HIP_TRY(h, hipMemcpyAsync(P.data(), use_ema ? K->ema : K->param, (size_t)L.count * 4, hipMemcpyDeviceToHost, h->stream));
    for (int l = 0; l < 3; ++l) {
        rm[l].resize(L.bnc[l]);
        rv[l].resize(L.bnc[l]);
        DFD_HIP_TRY(h, hipMemcpyAsync(rm[l].data(), K->rm[l], (size_t)L.bnc[l] * 4, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, hipMemcpyAsync(rv[l].data(), K->rv[l], (size_t)L.bnc[l] * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    auto scale = [&](int l, int o) { return (double)P[L.o_g[l] + o] / std::sqrt((double)rv[l][o] + K->eps); };
    auto bias = [&](int l, int o, double a) { return (float)(0.0 * a + ((double)P[L.o_be[l] + o] - (double)rm[l][o] * a)); };
    std::vector<float> ew((size_t)BK_EXP * BK_IN), eb(BK_EXP), dw((size_t)T * BK_EXP), db(BK_EXP), w2((size_t)BK_SE * BK_EXP),
        pw((size_t)OUT * BK_EXP), pb(OUT);
    for (int o = 0; o < BK_EXP; ++o) {
        const double a0 = scale(0, o), a1 = scale(1, o);
        for (int k = 0; k < BK_IN; ++k) ew[(size_t)o * BK_IN + k] = (float)((double)P[L.o_we + (size_t)o * BK_IN + k] * a0);
        eb[o] = bias(0, o, a0);
        for (int t = 0; t < T; ++t) dw[(size_t)t * BK_EXP + o] = (float)((double)P[L.o_wd + o * T + t] * a1);
        db[o] = bias(1, o, a1);
        for (int j = 0; j < BK_SE; ++j) w2[(size_t)j * BK_EXP + o] = P[L.o_w2 + (size_t)o * BK_SE + j];
    }
    for (int o = 0; o < OUT; ++o) {
        const double a2 = scale(2, o);
        for (int k = 0; k < BK_EXP; ++k) pw[(size_t)o * BK_EXP + k] = (float)((double)P[L.o_wp + (size_t)o * BK_EXP + k] * a2);
        pb[o] = bias(2, o, a2);
    }
    const struct { const float* dst; const float* src; size_t count; } ups[] = {
        {b.exp_w, ew.data(), ew.size()}, {b.exp_b, eb.data(), eb.size()}, {b.dw_w, dw.data(), dw.size()}, {b.dw_b, db.data(), db.size()},
        {b.se_w1, P.data() + L.o_w1, (size_t)BK_SE * BK_EXP}, {b.se_b1, P.data() + L.o_b1, (size_t)BK_SE}, {b.se_w2, w2.data(), w2.size()},
        {b.se_b2, P.data() + L.o_b2, (size_t)BK_EXP}, {b.proj_w, pw.data(), pw.size()}, {b.proj_b, pb.data(), pb.size()}};
    for (const auto& u : ups)
        DFD_HIP_TRY(h, hipMemcpyAsync(const_cast<float*>(u.dst), u.src, u.count * 4, hipMemcpyHostToDevice, h->stream));
    const struct { const float* w; int N, Kd; } splits[] = {{b.exp_w, BK_EXP, BK_IN}, {b.proj_w, OUT, BK_EXP}};
    for (const auto& sp : splits) {
        auto it = h->wsplit.find(sp.w);
        if (it != h->wsplit.end()) launch_split_weights(sp.w, it->second, sp.N, sp.Kd, h->stream, false);
    }
    DFD_HIP_TRY(h, hipGetLastError());
    DFD_HIP_TRY(h, stream_sync(h));                             // the host staging above lives until here
    return DFD_OK;
}

int headblock_commit(dfd_handle* h, HeadTrainState* S, int use_ema) {
    int rc = DFD_OK;
    for (int k = 0; k < HT_STAGES && S->stage[k] && !rc; ++k) rc = commit_one(h, S->stage[k], use_ema);
    return rc;
}

}  // namespace dfd

namespace {

struct BField { float* dfd_mbconv_params::*ptr; int off, count; };
// the 13 trainable tensors of a block with their places in its arena
std::vector<BField> trainable_fields(const Layout& L) {
    const int BK_IN = L.in, BK_EXP = L.exp, BK_SE = L.se;
    return {
        {&dfd_mbconv_params::exp_w, L.o_we, BK_EXP * BK_IN},   {&dfd_mbconv_params::dw_w, L.o_wd, BK_EXP * L.taps},
        {&dfd_mbconv_params::se_w1, L.o_w1, BK_SE * BK_EXP},   {&dfd_mbconv_params::se_b1, L.o_b1, BK_SE},
        {&dfd_mbconv_params::se_w2, L.o_w2, BK_EXP * BK_SE},   {&dfd_mbconv_params::se_b2, L.o_b2, BK_EXP},
        {&dfd_mbconv_params::proj_w, L.o_wp, L.out * BK_EXP},  {&dfd_mbconv_params::g0, L.o_g[0], BK_EXP},
        {&dfd_mbconv_params::be0, L.o_be[0], BK_EXP},          {&dfd_mbconv_params::g1, L.o_g[1], BK_EXP},
        {&dfd_mbconv_params::be1, L.o_be[1], BK_EXP},          {&dfd_mbconv_params::g2, L.o_g[2], L.out},
        {&dfd_mbconv_params::be2, L.o_be[2], L.out},
    };
}
struct BStat { float* dfd_mbconv_params::*rm; float* dfd_mbconv_params::*rv; };
const BStat kBlockStats[3] = {{&dfd_mbconv_params::rm0, &dfd_mbconv_params::rv0}, {&dfd_mbconv_params::rm1, &dfd_mbconv_params::rv1},
                              {&dfd_mbconv_params::rm2, &dfd_mbconv_params::rv2}};

bool block_complete(const dfd_mbconv_params* p, bool stats) {
    for (const BField& f : trainable_fields(layout_of<G15>(BK_LAST)))
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
    if (want_stage && !S->stage[0]) { *rc = fail(h, DFD_ERR_ARG, "%s: block 15 is not unfrozen (dfd_head_train_unfreeze_block)", who); return nullptr; }
    *rc = DFD_OK;
    return S;
}

BnC bn_consts(const HeadBlockState* K, const float* P, int l, int m, bool backward) {
    return BnC{K->mean[l], K->istd[l], backward ? K->sdy[l] : nullptr, backward ? K->sdx[l] : nullptr, P + K->L.o_g[l], P + K->L.o_be[l], m};
}

// the place of the deepest unfrozen block in S->stage (block 15 is unfrozen)
int deepest(const HeadTrainState* S) {
    int k = 0;
    while (k + 1 < HT_STAGES && S->stage[k + 1]) ++k;
    return k;
}

constexpr int K11 = BK_LAST - BK_STRIDED;                       // block 11's place in S->stage
// floats of one input row of a stage: [7][7][192], or block 11's [14][14][112]
size_t row_floats(const HeadBlockState* K) { return (size_t)K->L.hw_in * K->L.in; }

dim3 flat(size_t total) { return dim3((unsigned)((total + HT_THREADS - 1) / HT_THREADS)); }

// mean and istd of BatchNorm l over the m rows of Z: the batch's (train; running statistics updated) or the running ones
void bn_statistics(HeadBlockState* K, int l, const float* Z, int m, bool train, hipStream_t s) {
    const int C = K->L.bnc[l];
    const dim3 blk(HT_THREADS), chan((C + HT_THREADS - 1) / HT_THREADS);
    if (!train) {
        hipLaunchKernelGGL(bk_eval_consts_kernel, chan, blk, 0, s, K->rm[l], K->rv[l], K->eps, K->mean[l], K->istd[l], C);
        return;
    }
    const int ch = stat_chunks(m);
    const bool guard = C % 64 != 0;                             // 672 channels: the guarded instance on ceil(C / 64) blocks
    const dim3 sg((C + 63) / 64, ch);
    if (guard) hipLaunchKernelGGL((colstat_kernel<0, NoGrad, true>), sg, blk, 0, s, NoGrad{}, Z, nullptr, K->spart, nullptr, m, C);
    else hipLaunchKernelGGL((colstat_kernel<0, NoGrad>), sg, blk, 0, s, NoGrad{}, Z, nullptr, K->spart, nullptr, m, C);
    hipLaunchKernelGGL(finalize_kernel<0>, chan, blk, 0, s, K->spart, nullptr, ch, m, C, K->mean[l], nullptr, nullptr, nullptr, 0.f, 0.0);
    if (guard) hipLaunchKernelGGL((colstat_kernel<1, NoGrad, true>), sg, blk, 0, s, NoGrad{}, Z, K->mean[l], K->spart, nullptr, m, C);
    else hipLaunchKernelGGL((colstat_kernel<1, NoGrad>), sg, blk, 0, s, NoGrad{}, Z, K->mean[l], K->spart, nullptr, m, C);
    hipLaunchKernelGGL(finalize_kernel<1>, chan, blk, 0, s, K->spart, nullptr, ch, m, C, K->istd[l], K->mean[l], K->rm[l], K->rv[l],
                       K->momentum, K->eps);
}

// sum dy and sum dy xhat of BatchNorm l from its gradient source; adds the gradients of gamma and beta
template <class G>
void bn_backward_statistics(HeadBlockState* K, int l, const G& g, int m, hipStream_t s) {
    const int C = K->L.bnc[l], ch = stat_chunks(m);
    const dim3 blk(HT_THREADS);
    if (C % 64 != 0) hipLaunchKernelGGL((colstat_kernel<2, G, true>), dim3((C + 63) / 64, ch), blk, 0, s, g, nullptr, nullptr, K->spart, K->spart2, m, C);
    else hipLaunchKernelGGL((colstat_kernel<2, G>), dim3(C / 64, ch), blk, 0, s, g, nullptr, nullptr, K->spart, K->spart2, m, C);
    hipLaunchKernelGGL(finalize_kernel<2>, dim3((C + HT_THREADS - 1) / HT_THREADS), blk, 0, s, K->spart, K->spart2, ch, m, C, K->sdy[l],
                       K->sdx[l], K->grad + K->L.o_g[l], K->grad + K->L.o_be[l], 0.f, 0.0);
}

// X (K->x, n rows of the block below) -> the block's output in `out` (the next stage's input rows), with the block's
// parameters at P.  With the skip: out = X + the branch times the crop's drop-connect factor (`masked`: K->keep, else none).
// m0 = HW_IN n rows in front of the depthwise conv, m1 = HW n rows after it (one number at stride 1).
template <class GEO>
int block_forward(dfd_handle* h, HeadBlockState* K, const float* P, int n, bool train, float* out, bool masked) {
    typedef typename GEO::S S;
    hipStream_t s = h->stream;
    const int m0 = n * GEO::HW_IN, m1 = n * GEO::HW;
    const dim3 blk(HT_THREADS);
    const size_t te0 = (size_t)m0 * GEO::EXP, te1 = (size_t)m1 * GEO::EXP, to = (size_t)m1 * GEO::OUT;
    hipLaunchKernelGGL((gemm_fwd_kernel<GEO::JE, false>), dim3(GEO::EXP / (16 * GEO::JE), (m0 + 63) / 64), blk, 0, s, K->x, nullptr,
                       P + GEO::O_WE, K->ze, m0, GEO::IN, GEO::EXP, GEO::HW_IN);
    bn_statistics(K, 0, K->ze, m0, train, s);
    hipLaunchKernelGGL(bk_bn_swish_kernel, flat(te0), blk, 0, s, K->ze, bn_consts(K, P, 0, m0, false), K->ae, te0, GEO::EXP);
    if constexpr (GEO::STRIDE == 1)
        hipLaunchKernelGGL((bk_dw_fwd_kernel<S, GEO::KS>), flat(te1), blk, 0, s, K->ae, P + GEO::O_WD, K->zd, te1);
    else
        hipLaunchKernelGGL((bk_dws_fwd_kernel<S, GEO::KS, GEO::PAD>), flat(te1), blk, 0, s, K->ae, P + GEO::O_WD, K->zd, te1);
    bn_statistics(K, 1, K->zd, m1, train, s);
    hipLaunchKernelGGL(bk_bn_swish_pool_kernel<S>, dim3((GEO::EXP + HT_THREADS - 1) / HT_THREADS, n), blk, 0, s, K->zd,
                       bn_consts(K, P, 1, m1, false), K->ad, K->pooled);
    hipLaunchKernelGGL(bk_se_fwd_kernel<S>, dim3(n), blk, 0, s, K->pooled, P + GEO::O_W1, P + GEO::O_B1, P + GEO::O_W2, P + GEO::O_B2, K->r,
                       K->q, K->gate);
    hipLaunchKernelGGL((gemm_fwd_kernel<GEO::JP, true>), dim3(GEO::OUT / (16 * GEO::JP), (m1 + 63) / 64), blk, 0, s, K->ad, K->gate,
                       P + GEO::O_WP, K->zp, m1, GEO::EXP, GEO::OUT, GEO::HW);
    bn_statistics(K, 2, K->zp, m1, train, s);
    if constexpr (GEO::SKIP)
        hipLaunchKernelGGL(bk_bn_skip_kernel<S>, flat(to), blk, 0, s, K->zp, bn_consts(K, P, 2, m1, false), K->x, masked ? K->keep : nullptr,
                           masked ? K->keep_prob : 1.0, out, to, GEO::OUT);
    else
        hipLaunchKernelGGL(bk_bn_kernel, flat(to), blk, 0, s, K->zp, bn_consts(K, P, 2, m1, false), out, to, GEO::OUT);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

// from the gradient of the block's output (K->dx) back to the gradients of the block's parameters; dx_below (or null):
// the gradient with respect to the block's input for a trained block below: dZe . We, and with the skip K->dx + dZe . We
template <class GEO>
int block_backward(dfd_handle* h, HeadBlockState* K, int n, float* dx_below) {
    typedef typename GEO::S S;
    hipStream_t s = h->stream;
    const int m0 = n * GEO::HW_IN, m1 = n * GEO::HW, wch0 = wg_chunks(m0), wch1 = wg_chunks(m1);
    const dim3 blk(HT_THREADS);
    const float* P = K->param;
    float* G = K->grad;
    const size_t te0 = (size_t)m0 * GEO::EXP, te1 = (size_t)m1 * GEO::EXP;
    typedef Grad2<GEO::SKIP> G2;
    typedef Grad1<S> G1;
    typedef Grad0<S> G0;
    // BN2, project
    G2 g2{bn_consts(K, P, 2, m1, true), K->zp, K->dx, GEO::OUT, K->keep, K->keep_prob};
    bn_backward_statistics(K, 2, g2, m1, s);
    hipLaunchKernelGGL((wgrad_kernel<GEO::JE, true, G2>), dim3(GEO::WP_WAVES / 4, wch1), blk, 0, s, g2, K->ad, K->gate, K->wpart, m1, GEO::OUT,
                       GEO::EXP, GEO::HW);
    hipLaunchKernelGGL(wreduce_kernel, flat((size_t)GEO::OUT * GEO::EXP), blk, 0, s, K->wpart, wch1, GEO::OUT * GEO::EXP, G + GEO::O_WP);
    hipLaunchKernelGGL((gemm_dyw_kernel<GEO::JE, G2>), dim3(GEO::EXP / (16 * GEO::JE), (m1 + 15) / 16), blk, 0, s, g2, P + GEO::O_WP, K->d1, m1,
                       GEO::OUT, GEO::EXP);
    // squeeze-excite
    hipLaunchKernelGGL(bk_se_bwd_kernel<S>, dim3(n), blk, 0, s, K->d1, K->ad, K->gate, K->r, P + GEO::O_W1, P + GEO::O_W2, K->du, K->dr, K->ds);
    hipLaunchKernelGGL(bk_se_wgrad_kernel<S>, flat((size_t)2 * GEO::EXP * GEO::SE + GEO::EXP + GEO::SE), blk, 0, s, K->du, K->dr, K->q, K->pooled,
                       G + GEO::O_W1, G + GEO::O_B1, G + GEO::O_W2, G + GEO::O_B2, n);
    // BN1, depthwise
    G1 g1{bn_consts(K, P, 1, m1, true), K->zd, K->d1, K->gate, K->ds};
    bn_backward_statistics(K, 1, g1, m1, s);
    hipLaunchKernelGGL(bk_dz_store_kernel<S>, flat(te1), blk, 0, s, g1, K->d1, te1);
    const int dch = (n + BK_DW_CROPS - 1) / BK_DW_CROPS;
    const dim3 dwg((GEO::EXP + HT_THREADS - 1) / HT_THREADS, GEO::TAPS, dch);
    if constexpr (GEO::STRIDE == 1)
        hipLaunchKernelGGL((bk_dw_wgrad_kernel<S, GEO::KS>), dwg, blk, 0, s, K->d1, K->ae, K->dwpart, n);
    else
        hipLaunchKernelGGL((bk_dws_wgrad_kernel<S, GEO::KS, GEO::PAD>), dwg, blk, 0, s, K->d1, K->ae, K->dwpart, n);
    hipLaunchKernelGGL(bk_dw_wreduce_kernel<S>, flat((size_t)GEO::EXP * GEO::TAPS), blk, 0, s, K->dwpart, dch, G + GEO::O_WD, GEO::TAPS);
    if constexpr (GEO::STRIDE == 1)
        hipLaunchKernelGGL((bk_dw_bwd_kernel<S, GEO::KS>), flat(te0), blk, 0, s, K->d1, P + GEO::O_WD, K->d2, te0);
    else
        hipLaunchKernelGGL((bk_dws_bwd_kernel<S, GEO::KS, GEO::PAD>), flat(te0), blk, 0, s, K->d1, P + GEO::O_WD, K->d2, te0);
    // BN0, expand
    G0 g0{bn_consts(K, P, 0, m0, true), K->ze, K->d2};
    bn_backward_statistics(K, 0, g0, m0, s);
    hipLaunchKernelGGL((wgrad_kernel<GEO::JW, false, G0, GEO::WE_GUARD>), dim3((GEO::WE_WAVES + 3) / 4, wch0), blk, 0, s, g0, K->x, nullptr,
                       K->wpart, m0, GEO::EXP, GEO::IN, GEO::HW_IN);
    hipLaunchKernelGGL(wreduce_kernel, flat((size_t)GEO::EXP * GEO::IN), blk, 0, s, K->wpart, wch0, GEO::EXP * GEO::IN, G + GEO::O_WE);
    if constexpr (GEO::STRIDE == 1) {
        if (dx_below) {                                         // dOut of the block below: IN columns, reduction over EXP
            const dim3 grid(GEO::IN / (16 * GEO::JE), (m0 + 15) / 16);
            if constexpr (GEO::SKIP)                            // the skip path K->dx (another buffer than dx_below) + the branch
                hipLaunchKernelGGL((gemm_dyw_kernel<GEO::JE, G0, true>), grid, blk, 0, s, g0, P + GEO::O_WE, dx_below, m0, GEO::EXP, GEO::IN, K->dx);
            else
                hipLaunchKernelGGL((gemm_dyw_kernel<GEO::JE, G0>), grid, blk, 0, s, g0, P + GEO::O_WE, dx_below, m0, GEO::EXP, GEO::IN, nullptr);
        }
    } else if (dx_below) {                                      // block 11 forms no dX: block 10 is frozen
        return fail(h, DFD_ERR_STATE, "block %d hands no gradient down", K->L.index);
    }
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

// a skip block's drop-connect factors of accumulate number `counter`, drawn with layer 17 - its index (block 14: 3):
// head_training.drop_connect_keep is the specification
int draw_keep(dfd_handle* h, HeadTrainState* S, HeadBlockState* K, int n) {
    const uint32_t key = mask_key(S->cfg.seed, S->counter, 17 - K->L.index);
    const float scale = (float)(1.0 / K->keep_prob);
    for (int i = 0; i < n; ++i) K->keep_host[i] = mask_keep(key, (uint32_t)i, K->drop_thr) ? scale : 0.f;
    DFD_HIP_TRY(h, hipMemcpyAsync(K->keep, K->keep_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    return DFD_OK;
}

// Allocates a block's stage for max_n crops in ONE hipMalloc and uploads `init`
int create_stage(dfd_handle* h, HeadTrainState* S, const char* who, const Layout& L, const dfd_mbconv_params* init, float bn_momentum,
                 float bn_eps, HeadBlockState** slot) {
    HeadBlockState* K = new (std::nothrow) HeadBlockState();
    if (!K) return fail(h, DFD_ERR_CAPACITY, "%s: out of host memory", who);
    K->L = L;
    K->momentum = bn_momentum;
    K->eps = bn_eps == 1e-3f ? 1e-3 : (double)bn_eps;          // the backbone's eps (weights._fold's double), not its float neighbour
    // mm0 rows in front of the depthwise conv (x, Ze, ae, dae), mm1 after it; the chunked partials are sized by the larger
    const size_t BK_IN = (size_t)L.in, BK_EXP = (size_t)L.exp, BK_SE = (size_t)L.se;
    const size_t mn = (size_t)S->max_n, mm0 = mn * L.hw_in, mm1 = mn * L.hw, sch = (size_t)stat_chunks((int)mm0),
                 dch = (mn + BK_DW_CROPS - 1) / BK_DW_CROPS, cnt = (size_t)L.count, out = (size_t)L.out,
                 wmax = std::max((size_t)wg_chunks((int)mm1) * out * BK_EXP, (size_t)wg_chunks((int)mm0) * BK_EXP * BK_IN);
    struct Slot { void** p; size_t bytes; };
    std::vector<Slot> slots = {
        {(void**)&K->param, cnt * 4}, {(void**)&K->grad, cnt * 4}, {(void**)&K->m, cnt * 4},
        {(void**)&K->v, cnt * 4},     {(void**)&K->ema, cnt * 4},
        {(void**)&K->x, mm0 * BK_IN * 4},   {(void**)&K->ze, mm0 * BK_EXP * 4}, {(void**)&K->ae, mm0 * BK_EXP * 4},
        {(void**)&K->zd, mm1 * BK_EXP * 4}, {(void**)&K->ad, mm1 * BK_EXP * 4}, {(void**)&K->d1, mm1 * BK_EXP * 4},
        {(void**)&K->d2, mm0 * BK_EXP * 4}, {(void**)&K->zp, mm1 * out * 4}, {(void**)&K->dx, mm1 * out * 4},
        {(void**)&K->pooled, mn * BK_EXP * 4}, {(void**)&K->gate, mn * BK_EXP * 4},
        {(void**)&K->spart, sch * BK_EXP * 8}, {(void**)&K->spart2, sch * BK_EXP * 8},
        {(void**)&K->wpart, wmax * 8}, {(void**)&K->dwpart, dch * L.taps * BK_EXP * 8},
        {(void**)&K->partial, NORM_BLOCKS * 8},
        {(void**)&K->r, mn * BK_SE * 8}, {(void**)&K->q, mn * BK_SE * 8}, {(void**)&K->du, mn * BK_EXP * 8},
        {(void**)&K->dr, mn * BK_SE * 8}, {(void**)&K->ds, mn * BK_EXP * 8},
    };
    for (int l = 0; l < 3; ++l) {
        const size_t c = (size_t)L.bnc[l];
        slots.push_back({(void**)&K->rm[l], c * 4});
        slots.push_back({(void**)&K->rv[l], c * 4});
        slots.push_back({(void**)&K->mean[l], c * 8});
        slots.push_back({(void**)&K->istd[l], c * 8});
        slots.push_back({(void**)&K->sdy[l], c * 8});
        slots.push_back({(void**)&K->sdx[l], c * 8});
    }
    if (L.skip) {
        slots.push_back({(void**)&K->keep, mn * 4});
        K->keep_host.assign(mn, 0.f);
    }
    if (L.index != BK_LAST) slots.push_back({(void**)&K->norm, 4});          // block 15's launch writes the trainer's own scalar
    size_t total = 0;
    for (const Slot& sl : slots) total += (sl.bytes + 255) / 256 * 256;
    if (hipMalloc(&K->pool, total) != hipSuccess) {
        delete K;
        return fail(h, DFD_ERR_HIP, "%s: hipMalloc of %zu bytes failed", who, total);
    }
    size_t off = 0;
    for (const Slot& sl : slots) {
        *sl.p = static_cast<char*>(K->pool) + off;
        off += (sl.bytes + 255) / 256 * 256;
    }
    *slot = K;
    auto bail = [&](hipError_t e, const char* what) {
        destroy_one(slot);
        return fail(h, DFD_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMemsetAsync(K->pool, 0, total, h->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
    for (const BField& f : trainable_fields(L))
        if ((e = hipMemcpyAsync(K->param + f.off, init->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "parameter upload");
    for (int l = 0; l < 3; ++l) {
        if ((e = hipMemcpyAsync(K->rm[l], init->*kBlockStats[l].rm, (size_t)L.bnc[l] * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "statistics upload");
        if ((e = hipMemcpyAsync(K->rv[l], init->*kBlockStats[l].rv, (size_t)L.bnc[l] * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return bail(e, "statistics upload");
    }
    if ((e = hipMemcpyAsync(K->ema, K->param, cnt * 4, hipMemcpyDeviceToDevice, h->stream)) != hipSuccess) return bail(e, "shadow copy");
    if ((e = stream_sync(h)) != hipSuccess) return bail(e, "stream wait");
    return DFD_OK;
}

int export_stage(dfd_handle* h, HeadBlockState* K, int use_ema, dfd_mbconv_params* out) {
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const float* P = use_ema ? K->ema : K->param;
    for (const BField& f : trainable_fields(K->L))
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*f.ptr, P + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    for (int l = 0; l < 3; ++l) {
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*kBlockStats[l].rm, K->rm[l], (size_t)K->L.bnc[l] * 4, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, hipMemcpyAsync(out->*kBlockStats[l].rv, K->rv[l], (size_t)K->L.bnc[l] * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int stage_grads(dfd_handle* h, HeadBlockState* K, dfd_mbconv_params* io, int set) {
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    for (const BField& f : trainable_fields(K->L)) {
        if (set) DFD_HIP_TRY(h, hipMemcpyAsync(K->grad + f.off, io->*f.ptr, (size_t)f.count * 4, hipMemcpyHostToDevice, h->stream));
        else DFD_HIP_TRY(h, hipMemcpyAsync(io->*f.ptr, K->grad + f.off, (size_t)f.count * 4, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

// the stage of `block` (11 .. 15) for the _at entries
HeadBlockState* stage_at(dfd_handle* h, HeadTrainState* S, const char* who, int block, int* rc) {
    if (block < BK_FIRST || block > BK_LAST) {
        *rc = fail(h, DFD_ERR_UNSUPPORTED, "%s: block %d; %d .. %d", who, block, BK_FIRST, BK_LAST);
        return nullptr;
    }
    HeadBlockState* K = stage_of(S, block);
    if (!K)                                                     // 13, 12 and 11 frozen: not served, as before they could be unfrozen
        *rc = fail(h, block < 14 ? DFD_ERR_UNSUPPORTED : DFD_ERR_ARG, "%s: block %d is not unfrozen (%s)", who, block, unfreeze_entry(block));
    return K;
}

}  // namespace

extern "C" {

int dfd_head_train_unfreeze_block(dfd_handle* h, int block, const dfd_mbconv_params* init, float bn_momentum, float bn_eps) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_unfreeze_block", false, &rc);
    if (!S) return rc;
    if (block != BK_LAST)
        return fail(h, DFD_ERR_UNSUPPORTED, "head_train_unfreeze_block: block %d; only the last block (%d) can be unfrozen", block, BK_LAST);
    if (!S->conv) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: the conv stage comes first (dfd_head_train_unfreeze_conv)");
    if (S->stage[0]) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: block %d is already unfrozen", BK_LAST);
    if (S->counter) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: the trainer has accumulated already; unfreeze right after begin");
    if (!init || !block_complete(init, true)) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: null parameters");
    if (!(bn_momentum >= 0.f && bn_momentum <= 1.f && bn_eps > 0.f))
        return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block: bn_momentum %g or bn_eps %g out of range", (double)bn_momentum, (double)bn_eps);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    return create_stage(h, S, "head_train_unfreeze_block", layout_of<G15>(BK_LAST), init, bn_momentum, bn_eps, &S->stage[0]);
}

int dfd_head_train_unfreeze_block_at(dfd_handle* h, int block, const dfd_mbconv_params* init, float bn_momentum, float bn_eps,
                                     float drop_connect) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_unfreeze_block_at", false, &rc);
    if (!S) return rc;
    if (block < BK_FIRST || block >= BK_LAST)
        return fail(h, DFD_ERR_UNSUPPORTED, "head_train_unfreeze_block_at: block %d; only blocks %d .. %d can be unfrozen below block 15", block,
                    BK_FIRST, BK_LAST - 1);
    const int k = BK_LAST - block;
    if (S->stage[k]) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block_at: block %d is already unfrozen", block);
    if (!S->stage[k - 1])                                       // the blocks come from the top down: 15, 14, 13, 12, 11
        return k == 1 ? fail(h, DFD_ERR_ARG, "head_train_unfreeze_block_at: block 15 comes first (dfd_head_train_unfreeze_block)")
                      : fail(h, DFD_ERR_UNSUPPORTED, "head_train_unfreeze_block_at: block %d cannot be unfrozen while block %d is frozen", block,
                             block + 1);
    if (S->counter) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block_at: the trainer has accumulated already; unfreeze right after begin");
    if (!init || !block_complete(init, true)) return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block_at: null parameters");
    if (!(bn_momentum >= 0.f && bn_momentum <= 1.f && bn_eps > 0.f))
        return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block_at: bn_momentum %g or bn_eps %g out of range", (double)bn_momentum, (double)bn_eps);
    if (!(drop_connect >= 0.f && drop_connect < 1.f))
        return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block_at: drop_connect %g outside [0, 1)", (double)drop_connect);
    if (block == BK_STRIDED && drop_connect != 0.f)
        return fail(h, DFD_ERR_ARG, "head_train_unfreeze_block_at: drop_connect %g for block %d, which has no skip; 0", (double)drop_connect, block);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const Layout L = block == BK_STRIDED ? layout_of<G11>(block) : layout_of<G14>(block);
    if ((rc = create_stage(h, S, "head_train_unfreeze_block_at", L, init, bn_momentum, bn_eps, &S->stage[k]))) return rc;
    HeadBlockState* K = S->stage[k];
    K->drop_p = (double)drop_connect;                           // the double of the float32 argument, as the head's dropout rates
    K->keep_prob = 1.0 - K->drop_p;
    K->drop_thr = (uint32_t)(unsigned long long)(K->drop_p * 4294967296.0);
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
    HeadBlockState** T = S->stage;
    HeadBlockState* K = T[0];
    hipStream_t s = h->stream;
    const int deep = deepest(S), skips = std::min(deep, K11 - 1);            // stages 1 .. skips are the skip blocks 14 .. 12
    // the rows are the input of the deepest unfrozen block; every block below block 15 writes into the input of the block above it
    DFD_HIP_TRY(h, hipMemcpyAsync(T[deep]->x, rows, (size_t)n * row_floats(T[deep]) * 4, hipMemcpyHostToDevice, s));
    if (deep == K11 && (rc = block_forward<G11>(h, T[K11], T[K11]->param, n, true, T[K11 - 1]->x, false))) return rc;
    for (int k = skips; k >= 1; --k) {
        if ((rc = draw_keep(h, S, T[k], n))) return rc;
        if ((rc = block_forward<G14>(h, T[k], T[k]->param, n, true, T[k - 1]->x, true))) return rc;
    }
    if ((rc = block_forward<G15>(h, K, K->param, n, true, headconv_rows(S), false))) return rc;
    if ((rc = headconv_step(h, S, n, labels_a, labels_b, lam, loss_scale, K->dx))) return rc;
    if ((rc = block_backward<G15>(h, K, n, deep >= 1 ? T[1]->dx : nullptr))) return rc;
    for (int k = 1; k <= skips; ++k)                            // the deepest block hands nothing down: the block below it is frozen
        if ((rc = block_backward<G14>(h, T[k], n, k < deep ? T[k + 1]->dx : nullptr))) return rc;
    if (deep == K11 && (rc = block_backward<G11>(h, T[K11], n, nullptr))) return rc;
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
    HeadBlockState** T = S->stage;
    HeadBlockState* K = T[0];
    const int deep = deepest(S), skips = std::min(deep, K11 - 1);
    DFD_HIP_TRY(h, hipMemcpyAsync(T[deep]->x, rows, (size_t)n * row_floats(T[deep]) * 4, hipMemcpyHostToDevice, h->stream));
    if (deep == K11 && (rc = block_forward<G11>(h, T[K11], use_ema ? T[K11]->ema : T[K11]->param, n, false, T[K11 - 1]->x, false))) return rc;
    for (int k = skips; k >= 1; --k)                            // no drop-connect
        if ((rc = block_forward<G14>(h, T[k], use_ema ? T[k]->ema : T[k]->param, n, false, T[k - 1]->x, false))) return rc;
    if ((rc = block_forward<G15>(h, K, use_ema ? K->ema : K->param, n, false, headconv_rows(S), false))) return rc;
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
    return export_stage(h, S->stage[0], use_ema, out);
}

int dfd_head_train_block_grads(dfd_handle* h, dfd_mbconv_params* io, int set) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_block_grads", true, &rc);
    if (!S) return rc;
    if (!io || !block_complete(io, false)) return fail(h, DFD_ERR_ARG, "head_train_block_grads: null pointer");
    return stage_grads(h, S->stage[0], io, set);
}

int dfd_head_train_export_block_at(dfd_handle* h, int block, int use_ema, dfd_mbconv_params* out) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_export_block_at", false, &rc);
    if (!S) return rc;
    HeadBlockState* K = stage_at(h, S, "head_train_export_block_at", block, &rc);
    if (!K) return rc;
    if (!out || !block_complete(out, true)) return fail(h, DFD_ERR_ARG, "head_train_export_block_at: null pointer");
    return export_stage(h, K, use_ema, out);
}

int dfd_head_train_block_grads_at(dfd_handle* h, int block, dfd_mbconv_params* io, int set) {
    int rc;
    HeadTrainState* S = open_block(h, "head_train_block_grads_at", false, &rc);
    if (!S) return rc;
    HeadBlockState* K = stage_at(h, S, "head_train_block_grads_at", block, &rc);
    if (!K) return rc;
    if (!io || !block_complete(io, false)) return fail(h, DFD_ERR_ARG, "head_train_block_grads_at: null pointer");
    return stage_grads(h, K, io, set);
}

}  // extern "C"

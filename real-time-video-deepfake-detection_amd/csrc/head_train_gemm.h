// The head trainer's fp64-MFMA GEMMs and channel statistics over any (K, N): the forms of head_train_conv.hip's
// 320 -> 1280 kernels (hc_gemm_fwd / hc_wgrad / hc_wreduce / hc_colstat / hc_finalize, which keep their own tiling and
// bits) for block 15's shapes (head_train_block.hip), plus the dY . W form both files need for an input gradient.
// v_mfma_f64_16x16x4_f64: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// D[row = (lane >> 4) + 4 reg][col = lane & 15].  fp32 operands are widened at the load, products of floats are exact in
// double, so every result is its sum rounded once at the store.  Rows past m are masked at the load and never read.
// Reductions over rows are partial sums over fixed chunks added in chunk order, in double; no atomics.
//
// A gradient source `G` describes one train-mode BatchNorm's upstream gradient:
//   G::K  k = g.load(c)                      the channel's constants
//   g.dy_xh(k, row, c, &dy, &xh)             dLoss / dy of the element and its xhat, in double
// and bn_dz() turns it into dZ = gamma istd (dy - sum dy / m - xhat sum(dy xhat) / m), formed at the load, never stored.
#pragma once
#include "head_train_state.h"

namespace dfd {
namespace ht64 {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int STAT_ROWS = 256;            // rows of one partial sum of a channel statistic
constexpr int WG_ROWS = 512;              // rows of one partial weight gradient

__device__ __forceinline__ double sigmoid(double y) { return 1.0 / (1.0 + exp(-y)); }
__device__ __forceinline__ double swish(double y) { return y * sigmoid(y); }
__device__ __forceinline__ double swish_grad(double y) {
    const double s = sigmoid(y);
    return s * (1.0 + y * (1.0 - s));
}

// the constants of one channel of a train-mode BatchNorm and of its backward
struct BnK { double mean, istd, gamma, beta, mdy, mdx; };
struct BnC {
    const double *mean, *istd, *sdy, *sdx;    // sdy / sdx: sum dy, sum dy xhat (null before the backward's statistics)
    const float *gamma, *beta;
    int m;
    __device__ __forceinline__ BnK load(int c) const {
        BnK k;
        k.mean = mean[c];
        k.istd = istd[c];
        k.gamma = (double)gamma[c];
        k.beta = (double)beta[c];
        k.mdy = sdy ? sdy[c] / m : 0.0;
        k.mdx = sdx ? sdx[c] / m : 0.0;
        return k;
    }
};

template <class G>
__device__ __forceinline__ double bn_dz(const G& g, const typename G::K& k, size_t row, int c) {
    double dy, xh;
    g.dy_xh(k, row, c, &dy, &xh);
    return (k.gamma * k.istd) * ((dy - k.mdy) - xh * k.mdx);
}

// ---------------------------------------------------------------------------------------------- forward
// Z [m][N] = A [m][K] . W [N][K]^T, A = X or (GATED) X * gate[row / hw] in double.  grid (N / (16 J), ceil(m / 64)); a wave
// owns 16 rows x 16 J columns, J independent chains.  K % 16 == 0.
template <int J, bool GATED>
__global__ __launch_bounds__(HT_THREADS) void gemm_fwd_kernel(const float* __restrict__ X, const float* __restrict__ gate,
                                                              const float* __restrict__ W, float* __restrict__ Z, int m, int K,
                                                              int N, int hw) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.y * 4 + wv) * 16, col0 = blockIdx.x * (16 * J);
    if (row0 >= m) return;                                      // wave-uniform
    const int row = row0 + r16;
    const bool ok = row < m;
    const size_t rr = ok ? (size_t)row : 0;
    const float* xrow = X + rr * K + 4 * q;
    const float* grow = GATED ? gate + (rr / hw) * K + 4 * q : nullptr;
    const float* wrow = W + (size_t)(col0 + r16) * K + 4 * q;
    d4 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 16) {
        const f4 a = *reinterpret_cast<const f4*>(xrow + k0);
        d4 ad = (d4){(double)a[0], (double)a[1], (double)a[2], (double)a[3]};
        if constexpr (GATED) {
            const f4 g = *reinterpret_cast<const f4*>(grow + k0);
            ad = (d4){ad[0] * (double)g[0], ad[1] * (double)g[1], ad[2] * (double)g[2], ad[3] * (double)g[3]};
        }
        if (!ok) ad = (d4){0.0, 0.0, 0.0, 0.0};
        f4 b[J];
#pragma unroll
        for (int j = 0; j < J; ++j) b[j] = *reinterpret_cast<const f4*>(wrow + (size_t)j * 16 * K + k0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[kk], (double)b[j][kk], acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = row0 + q + 4 * e;
            if (r < m) Z[(size_t)r * N + col0 + j * 16 + r16] = (float)acc[j][e];
        }
    }
}

// ---------------------------------------------------------------------------------------------- input gradient
// dX [m][NC] = dZ [m][R] . W [R][NC], dZ formed from the gradient source as it loads.  grid (NC / (16 J), ceil(m / 16)); a
// workgroup owns 16 rows x 16 J columns and each of its 4 waves a quarter of the R channels, walked 4 at a time; the four
// partial tiles are added in wave order through LDS (6 J KB) and rounded once.  R % 16 == 0.
// ADD: dX = add + dZ . W, the gradient an identity skip hands down (add [m][NC]: the gradient of the block's output, a
// buffer other than dX); the stored value is the double sum (add + the four partial tiles), rounded once.
template <int J, class G, bool ADD = false>
__global__ __launch_bounds__(HT_THREADS) void gemm_dyw_kernel(G g, const float* __restrict__ W, float* __restrict__ dX, int m,
                                                              int R, int NC, const float* __restrict__ add = nullptr) {
    __shared__ double red[3][J][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int row0 = blockIdx.y * 16, col0 = blockIdx.x * (16 * J);
    const int row = row0 + r16;
    const bool ok = row < m;
    const size_t rr = ok ? (size_t)row : 0;
    d4 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
    const int quarter = R / 4, c_end = (wv + 1) * quarter;
    for (int c0 = wv * quarter; c0 < c_end; c0 += 4) {
        const int c = c0 + q;
        const typename G::K k = g.load(c);
        double a = bn_dz(g, k, rr, c);
        if (!ok) a = 0.0;
        const float* wr = W + (size_t)c * NC + col0 + r16;
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)wr[j * 16], acc[j], 0, 0, 0);
    }
    if (wv > 0) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wv - 1][j][e][lane] = acc[j][e];
        }
    }
    __syncthreads();
    if (wv > 0) return;
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = row0 + q + 4 * e;
            double s = ((acc[j][e] + red[0][j][e][lane]) + red[1][j][e][lane]) + red[2][j][e][lane];
            if (r < m) {
                const size_t o = (size_t)r * NC + col0 + j * 16 + r16;
                if constexpr (ADD) s = (double)add[o] + s;
                dX[o] = (float)s;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- weight gradient
// P [chunk][NO][NI] = dZ^T . B over rows [512 chunk, 512 (chunk + 1)) n [0, m), in double; B = X or (GATED) X * gate.
// grid (NO / 16 * NI / (16 J) / 4, chunks): wave w owns channels 16 (w / (NI / 16 J)) .. + 16 and inputs 16 J (w % ..) .. + 16 J.
// GUARD: the instance for a wave count that is no multiple of 4 (672 x 112 at J = 7: 42 waves), grid ceil(waves / 4); a
// wave whose tile lies past channel NO returns before any load or store (wave-uniform; the kernel has no barrier).  The
// instances without it keep their instruction stream.
template <int J, bool GATED, class G, bool GUARD = false>
__global__ __launch_bounds__(HT_THREADS) void wgrad_kernel(G g, const float* __restrict__ X, const float* __restrict__ gate,
                                                           double* __restrict__ P, int m, int NO, int NI, int hw) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int groups = NI / (16 * J), gw = blockIdx.x * 4 + wv, o0 = (gw / groups) * 16, i0 = (gw % groups) * (16 * J);
    if constexpr (GUARD) {
        if (o0 >= NO) return;
    }
    const int r0 = blockIdx.y * WG_ROWS, r1 = min(m, r0 + WG_ROWS);
    const int c = o0 + r16;
    const typename G::K k = g.load(c);
    d4 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = r0; k0 < r1; k0 += 4) {
        const int row = k0 + q;
        const bool ok = row < r1;
        const size_t rr = ok ? (size_t)row : 0;
        double a = bn_dz(g, k, rr, c);
        if (!ok) a = 0.0;
        const float* xr = X + rr * NI + i0 + r16;
        const float* gr = GATED ? gate + (rr / hw) * NI + i0 + r16 : nullptr;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            double b = (double)xr[j * 16];
            if constexpr (GATED) b *= (double)gr[j * 16];
            if (!ok) b = 0.0;
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
        }
    }
    double* out = P + (size_t)blockIdx.y * ((size_t)NO * NI);
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[(size_t)(o0 + q + 4 * e) * NI + i0 + j * 16 + r16] = acc[j][e];
    }
}

// second stage: G [count] += the chunks' partials added in chunk order, rounded once
static __global__ __launch_bounds__(HT_THREADS) void wreduce_kernel(const double* __restrict__ P, int chunks, int count, float* __restrict__ G) {
    const int i = blockIdx.x * HT_THREADS + threadIdx.x;
    if (i >= count) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += P[(size_t)k * count + i];
    G[i] += (float)s;
}

// ---------------------------------------------------------------------------------------------- channel statistics
// Partial sums over rows [256 chunk, 256 (chunk + 1)) n [0, m): grid (C / 64, chunks).  Thread (col, g) adds rows g, g + 4, ..
// of its column in double, then the 4 row groups are added in order.
//   MODE 0: sum z      MODE 1: sum (z - mean)^2      MODE 2: sum dy -> part, sum dy xhat -> part2 (gradient source G)
// GUARD: the instance for a C that is no multiple of 64 (672 = 10.5 x 64), grid (ceil(C / 64), chunks): a thread whose
// column lies past C loads and stores nothing but still meets the barrier (a wave is 64 columns of one row group, so the
// last block's waves are half past the end: the guard is per lane).  The instances without it keep their instruction stream.
struct NoGrad {
    typedef BnK K;
    __device__ __forceinline__ K load(int) const { return K{}; }
    __device__ __forceinline__ void dy_xh(const K&, size_t, int, double* dy, double* xh) const { *dy = 0.0; *xh = 0.0; }
};
template <int MODE, class G, bool GUARD = false>
__global__ __launch_bounds__(HT_THREADS) void colstat_kernel(G g, const float* __restrict__ Z, const double* __restrict__ mean,
                                                             double* __restrict__ part, double* __restrict__ part2, int m, int C) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, gr = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const bool live = !GUARD || c < C;
    const int r0 = blockIdx.y * STAT_ROWS, r1 = live ? min(m, r0 + STAT_ROWS) : r0;
    double mu = 0.0;
    if constexpr (MODE == 1) {
        if (live) mu = mean[c];
    }
    typename G::K k{};
    if constexpr (MODE == 2) {
        if (live) k = g.load(c);
    }
    double s0 = 0.0, s1 = 0.0;
    for (int r = r0 + gr; r < r1; r += 4) {
        if constexpr (MODE == 0) s0 += (double)Z[(size_t)r * C + c];
        if constexpr (MODE == 1) { const double d = (double)Z[(size_t)r * C + c] - mu; s0 += d * d; }
        if constexpr (MODE == 2) {
            double dy, xh;
            g.dy_xh(k, (size_t)r, c, &dy, &xh);
            s0 += dy;
            s1 += dy * xh;
        }
    }
    red[0][gr][cl] = s0;
    red[1][gr][cl] = s1;
    __syncthreads();
    if (gr == 0 && live) {
        part[(size_t)blockIdx.y * C + c] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        if constexpr (MODE == 2) part2[(size_t)blockIdx.y * C + c] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

// The chunks' partial sums added in chunk order, one thread per channel (grid ceil(C / 256)):
//   MODE 0: mean = sum / m
//   MODE 1: var = sum / m (biased: what normalises), istd = 1 / sqrt(var + eps); running statistics as BatchNorm2d updates
//           them (m / (m - 1) var into the running variance), in fp32
//   MODE 2: sdy = sum dy, sdx = sum dy xhat (kept in double), added to the gradients of beta / gamma
template <int MODE>
__global__ __launch_bounds__(HT_THREADS) void finalize_kernel(const double* __restrict__ part, const double* __restrict__ part2,
                                                              int chunks, int m, int C, double* __restrict__ out,
                                                              double* __restrict__ out2, float* __restrict__ fa, float* __restrict__ fb,
                                                              float momentum, double eps) {
    const int c = blockIdx.x * HT_THREADS + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, s2 = 0.0;
    for (int k = 0; k < chunks; ++k) {
        s += part[(size_t)k * C + c];
        if constexpr (MODE == 2) s2 += part2[(size_t)k * C + c];
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

inline int stat_chunks(int m) { return (m + STAT_ROWS - 1) / STAT_ROWS; }
inline int wg_chunks(int m) { return (m + WG_ROWS - 1) / WG_ROWS; }

}  // namespace ht64
}  // namespace dfd

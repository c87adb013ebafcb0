// Frequency-domain analysis at any size: the 2-D DFT of face windows at their own h x w (DeepfakeDetector.analyze_frequency_domain,
// reference deepfake_detection.py:457-487) and compute_frequency_features at any even size (reference model.py:105-149).
//
//   fd_gather_kernel   n windows of a uint8 frame (BGR or gray, row stride) -> packed gray planes [hp][wp]
//   fd_rows_kernel     pass 1: out[k][row] = sum_n W_w[k n] g[row][n], transposed, [wp][hp]
//   fd_cols_kernel     pass 2: X[k1][k2] = sum_row in[k1][row] W_h[row k2]; epilogues: sum |X| (total, outside the mask),
//                      the spectrum itself (test tap), log1p|X| at the fftshift position + min / max (features)
//   fd_sums_kernel     a window's tile partials, in tile order -> (high, total)
//   fd_dct_kernel      DCT-II, orthonormal (cv2.dct), one real pass; run twice
//   fd_minmax_norm_kernel
//
// X = W_h G W_w as two dense products on v_mfma_f32_16x16x4_f32, in the structure of dft_rows_kernel / dft_band_kernel
// (forensic_kernels.hip; operand layout, chunked double accumulation and row centring are described there).  What is new
// is the rectangle: sides are any 1 <= h, w <= 4096, several windows of different sizes share one launch set, and the
// planes are padded to multiples of 16 so that every load is an aligned vector load.  The rules the padding sets:
//   - the table exp(-2 pi i j / N) has the TRUE length N and is indexed by (k n) mod N; padded output rows k >= N walk
//     it with k mod N and are stored as zeros;
//   - a padded K element contributes exactly 0: the operand is 0, not 0 - c0 (c0 = the element the row is centred on);
//   - the bin-0 correction is N c0 with the true N;
//   - pass 1 stores its whole padded [wp][hp] array, zeros outside k < w, row < h, so pass 2 reads it unmasked
//     (x0 of a padded row is 0) and masks only the K elements row >= h, which would otherwise become 0 - x0;
//   - results are stored, summed and min / max-ed for k1 < w, k2 < h only.
// The grid of both passes runs over a tile table: pre[i] = 16-row tiles of the windows before window i (both passes tile
// the w axis, so they share it); a block finds its window by bisection.  Each window's arithmetic is independent of the
// other windows of the call, and its tile partials are added in tile order: one window gives the same bits alone, among
// others, and in any chunk of a call.
#include <algorithm>
#include <cmath>
#include <map>

#include "dfd_common.h"
#include "freq_domain.h"
#include "kernel_util.h"

namespace dfd {

// device view of a window: FdWin + its two tables
struct FdWinDev {
    FdWin g;
    const float2 *tw_w, *tw_h;      // exp(-2 pi i j / w), exp(-2 pi i j / h)
};

__device__ __forceinline__ int fd_find(const int* __restrict__ pre, int n, int tile) {
    int lo = 0, hi = n;                                           // pre[lo] <= tile < pre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

// block (x, y): rows 16 x .. 16 x + 15 of window y's padded plane; zero outside the window
__global__ __launch_bounds__(256) void fd_gather_kernel(const uint8_t* __restrict__ frame, size_t stride, int channels,
                                                        const FdWinDev* __restrict__ wins, uint8_t* __restrict__ gray) {
    const FdWin W = wins[blockIdx.y].g;
    const int r0 = blockIdx.x * 16;
    if (r0 >= W.hp) return;
    uint8_t* dst = gray + W.gray_off;
    const int vec = W.wp >> 2;
    for (int i = threadIdx.x; i < 16 * vec; i += 256) {
        const int row = r0 + i / vec, c = (i % vec) * 4;
        uint8_t e[4] = {0, 0, 0, 0};
        if (row < W.h) {
            const uint8_t* p = frame + (size_t)(W.y + row) * stride + (size_t)(W.x + c) * channels;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < W.w) e[k] = channels == 3 ? bgr_to_gray_u8(p[3 * k], p[3 * k + 1], p[3 * k + 2]) : p[k];
        }
        *reinterpret_cast<uchar4*>(dst + (size_t)row * W.wp + c) = make_uchar4(e[0], e[1], e[2], e[3]);
    }
}

// pass 1.  A = the table (row k of the tile), B = the pixels (column = image row); wave w walks the 64-row groups
// w, w + 4, ... of the plane.
__global__ __launch_bounds__(256) void fd_rows_kernel(const uint8_t* __restrict__ gray, float2* __restrict__ rows,
                                                      const FdWinDev* __restrict__ wins, const int* __restrict__ pre, int n) {
    extern __shared__ float2 fd_tw[];
    const int tid = threadIdx.x;
    const int wi = fd_find(pre, n, blockIdx.x);                   // (block-uniform)
    const FdWinDev WD = wins[wi];
    const FdWin W = WD.g;
    const int N = W.w, wp = W.wp, hp = W.hp;
    for (int i = tid; i < N; i += 256) fd_tw[i] = WD.tw_w[i];
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, j = l & 15, q = l >> 4;
    const uint8_t* g = gray + W.gray_off;
    float2* out = rows + W.rows_off;
    const int k0 = (blockIdx.x - pre[wi]) * 16, kf = (k0 + j) % N;    // this lane's A row (a padded row: any row, never stored)
    const int jump = (13 * kf) % N;                               // from k = 4q + 3 of one chunk to 4q of the next
    const int ngroups = (hp + 63) >> 6;
    for (int grp = wave; grp < ngroups; grp += 4) {
        const int row0 = grp * 64;
        const int nt = min(4, (hp - row0) >> 4);                  // (wave-uniform)
        double dre[4][4], dim[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dre[t][r] = dim[t][r] = 0.0;
        int idx = (kf * 4 * q) % N;
        int c0[4] = {0, 0, 0, 0};                                 // first pixel of this lane's image row, per tile
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt) c0[t] = g[(size_t)(row0 + 16 * t + j) * wp];
        for (int n0 = 0; n0 < wp; n0 += 16) {
            uchar4 bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt) bv[t] = *reinterpret_cast<const uchar4*>(g + (size_t)(row0 + 16 * t + j) * wp + n0 + 4 * q);
            v4f are[4], aim[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { are[t] = v4f{0.f, 0.f, 0.f, 0.f}; aim[t] = v4f{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float2 w = fd_tw[idx];
                const bool live = n0 + 4 * q + e < N;             // a padded pixel is 0 after centring, not 0 - c0
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) {
                        const int px = e == 0 ? bv[t].x : e == 1 ? bv[t].y : e == 2 ? bv[t].z : bv[t].w;
                        const float b = live ? (float)(px - c0[t]) : 0.f;
                        are[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b, are[t], 0, 0, 0);
                        aim[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b, aim[t], 0, 0, 0);
                    }
                idx += e < 3 ? kf : jump;
                if (idx >= N) idx -= N;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { dre[t][r] += (double)are[t][r]; dim[t][r] += (double)aim[t][r]; }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = k0 + 4 * q + r;
                    if (k == 0) dre[t][r] += (double)(c0[t] * N);     // bin 0 of the row (D column j = B column j); exact
                    // rows >= h of the plane are zeros with c0 = 0: their outputs are zeros already
                    out[(size_t)k * hp + row0 + 16 * t + j] = k < N ? make_float2((float)dre[t][r], (float)dim[t][r]) : make_float2(0.f, 0.f);
                }
    }
}

// pass 2.  A = pass 1's rows (row k1 of the tile), B = the table (column k2).  FEAT = false: |X| of every bin summed in
// double into (high, total) of the block's tile, part [tiles][2]; spec_out / mag_out are the test taps, compact [w][h] at
// the window's tap_off, null on every production launch.  FEAT = true (one square window): log1pf|X| stored at the
// fftshift position of feat_out [S][S] ([ky][kx]; the kernel's k1 is kx), min / max of the block in fpart [tiles][2].
template <bool FEAT>
__global__ __launch_bounds__(256) void fd_cols_kernel(const float2* __restrict__ rows, const FdWinDev* __restrict__ wins,
                                                      const int* __restrict__ pre, int n, double* __restrict__ part,
                                                      float2* __restrict__ spec_out, float* __restrict__ mag_out,
                                                      float* __restrict__ feat_out, float* __restrict__ fpart) {
    extern __shared__ float2 fd_tw[];
    __shared__ double red[4 * 2];
    const int tid = threadIdx.x;
    const int wi = fd_find(pre, n, blockIdx.x);
    const FdWinDev WD = wins[wi];
    const FdWin W = WD.g;
    const int N = W.h, hp = W.hp;
    for (int i = tid; i < N; i += 256) fd_tw[i] = WD.tw_h[i];
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, j = l & 15, q = l >> 4;
    const int k0 = (blockIdx.x - pre[wi]) * 16;
    const float2* in = rows + W.rows_off;
    const float2* src = in + (size_t)(k0 + j) * hp;               // this lane's A row (zeros when k0 + j >= w)
    const float2 x0 = src[0];                                     // ... centred on its first element
    const int m = min(W.h, W.w) >> 2, half_w = (W.w + 1) >> 1, half_h = (W.h + 1) >> 1;
    double total = 0.0, high = 0.0;
    float lo = 3.4e38f, hi = -3.4e38f;
    const int ngroups = (hp + 63) >> 6;
    for (int grp = wave; grp < ngroups; grp += 4) {
        const int col0 = grp * 64;
        const int nt = min(4, (hp - col0) >> 4);                  // (wave-uniform)
        int idx[4], step[4], jump[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k2 = (col0 + 16 * t + j) % N;               // (padded columns: any column, never used)
            step[t] = k2;
            jump[t] = (13 * k2) % N;
            idx[t] = (k2 * 4 * q) % N;
        }
        double dre[4][4], dim[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dre[t][r] = dim[t][r] = 0.0;
        for (int r0 = 0; r0 < hp; r0 += 16) {
            const float4 a01 = *reinterpret_cast<const float4*>(src + r0 + 4 * q);
            const float4 a23 = *reinterpret_cast<const float4*>(src + r0 + 4 * q + 2);
            v4f fre[4], fim[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { fre[t] = v4f{0.f, 0.f, 0.f, 0.f}; fim[t] = v4f{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool live = r0 + 4 * q + e < N;             // a padded element is 0 after centring, not 0 - x0
                const float tr = live ? (e == 0 ? a01.x : e == 1 ? a01.z : e == 2 ? a23.x : a23.z) - x0.x : 0.f;
                const float ti = live ? (e == 0 ? a01.y : e == 1 ? a01.w : e == 2 ? a23.y : a23.w) - x0.y : 0.f;
                float2 w[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) {
                        w[t] = fd_tw[idx[t]];
                        idx[t] += e < 3 ? step[t] : jump[t];
                        if (idx[t] >= N) idx[t] -= N;
                    }
                // every accumulator gets one MFMA before any gets its next (32-cycle issue, 40-cycle dependent latency)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) fre[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(tr, w[t].x, fre[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) fim[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(tr, w[t].y, fim[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) fre[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ti, -w[t].y, fre[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) fim[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ti, w[t].x, fim[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { dre[t][r] += (double)fre[t][r]; dim[t][r] += (double)fim[t][r]; }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k1 = k0 + 4 * q + r, k2 = col0 + 16 * t + j;
                    if (k1 >= W.w || k2 >= W.h) continue;
                    double re = dre[t][r], im = dim[t][r];
                    if (k2 == 0) {                                    // bin 0 of row k1: h times the element it was centred on
                        const float2 z = in[(size_t)k1 * hp];
                        re += (double)z.x * (double)N;
                        im += (double)z.y * (double)N;
                    }
                    const float xr = (float)re, xi = (float)im;
                    const float mg = hypotf(xr, xi);
                    if (!FEAT) {
                        if (spec_out) {                               // (wave-uniform)
                            const size_t o = (size_t)W.tap_off + (size_t)k1 * W.h + k2;
                            spec_out[o] = make_float2(xr, xi);
                            mag_out[o] = mg;
                        }
                        // signed frequencies; the reference zeroes [c - m, c + m) of the shifted spectrum on both axes
                        const int s1 = k1 < half_w ? k1 : k1 - W.w, s2 = k2 < half_h ? k2 : k2 - W.h;
                        total += (double)mg;
                        if (!(s1 >= -m && s1 < m && s2 >= -m && s2 < m)) high += (double)mg;
                    } else {
                        const int S = W.h, y = (k2 + (S >> 1)) % S, x = (k1 + (S >> 1)) % S;
                        const float v = log1pf(mg);
                        feat_out[(size_t)y * S + x] = v;
                        if (spec_out) spec_out[(size_t)k1 * S + k2] = make_float2(xr, xi);
                        lo = fminf(lo, v);
                        hi = fmaxf(hi, v);
                    }
                }
    }
    if (!FEAT) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { high += __shfl_xor(high, off); total += __shfl_xor(total, off); }
        if (l == 0) { red[2 * wave] = high; red[2 * wave + 1] = total; }
        __syncthreads();
        if (tid < 2) part[(size_t)blockIdx.x * 2 + tid] = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
    } else {
        float* fred = reinterpret_cast<float*>(red);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off)); hi = fmaxf(hi, __shfl_xor(hi, off)); }
        if (l == 0) { fred[2 * wave] = lo; fred[2 * wave + 1] = hi; }
        __syncthreads();
        if (tid == 0) {
            fpart[(size_t)blockIdx.x * 2] = fminf(fminf(fred[0], fred[2]), fminf(fred[4], fred[6]));
            fpart[(size_t)blockIdx.x * 2 + 1] = fmaxf(fmaxf(fred[1], fred[3]), fmaxf(fred[5], fred[7]));
        }
    }
}

// out [n][2] = (high, total): the window's tile partials added in tile order
__global__ __launch_bounds__(256) void fd_sums_kernel(const double* __restrict__ part, const int* __restrict__ pre, int n,
                                                      double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double high = 0.0, total = 0.0;
    for (int t = pre[i]; t < pre[i + 1]; ++t) { high += part[2 * (size_t)t]; total += part[2 * (size_t)t + 1]; }
    out[2 * (size_t)i] = high;
    out[2 * (size_t)i + 1] = total;
}

// DCT-II, orthonormal, one pass over a padded square plane [Sp][Sp] of true edge S:
//   out[k][row] = a_k sum_n in[row][n] cos(pi (2n + 1) k / 2S),  a_0 = sqrt(1/S), a_k = sqrt(2/S)
// on the structure of pass 1: the 4S-entry table cos(pi j / 2S) in LDS, indexed by ((2n + 1) k) mod 4S; rows centred on
// their first element (the cosines of a row k > 0 sum to 0, those of row 0 to S).  FINAL = false: out is the padded
// [Sp][Sp] array, zeros outside k, row < S.  FINAL = true (the second pass: out is [ky][kx]): log1pf|.| stored compact
// [S][S] with the block's min / max in fpart; tap (or null): the coefficients themselves, compact.
template <bool FINAL>
__global__ __launch_bounds__(256) void fd_dct_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                     const float* __restrict__ ctab, int S, int Sp, float* __restrict__ fpart,
                                                     float* __restrict__ tap) {
    extern __shared__ float fd_ct[];
    __shared__ float fred[4 * 2];
    const int tid = threadIdx.x, M = 4 * S;
    for (int i = tid; i < M; i += 256) fd_ct[i] = ctab[i];
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, j = l & 15, q = l >> 4;
    const int k0 = blockIdx.x * 16, kf = (k0 + j) % M;
    const int step = (2 * kf) % M, jump = (26 * kf) % M;          // n -> n + 1, and n = 4q + 3 -> 4q + 16
    const double a0 = sqrt(1.0 / (double)S), ak = sqrt(2.0 / (double)S);
    float lo = 3.4e38f, hi = -3.4e38f;
    const int ngroups = (Sp + 63) >> 6;
    for (int grp = wave; grp < ngroups; grp += 4) {
        const int row0 = grp * 64;
        const int nt = min(4, (Sp - row0) >> 4);                  // (wave-uniform)
        double acc[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
        int idx = ((8 * q + 1) * kf) % M;
        float c0[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt) c0[t] = in[(size_t)(row0 + 16 * t + j) * Sp];
        for (int n0 = 0; n0 < Sp; n0 += 16) {
            float4 bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt) bv[t] = *reinterpret_cast<const float4*>(in + (size_t)(row0 + 16 * t + j) * Sp + n0 + 4 * q);
            v4f f[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) f[t] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float w = fd_ct[idx];
                const bool live = n0 + 4 * q + e < S;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) {
                        const float px = e == 0 ? bv[t].x : e == 1 ? bv[t].y : e == 2 ? bv[t].z : bv[t].w;
                        f[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, live ? px - c0[t] : 0.f, f[t], 0, 0, 0);
                    }
                idx += e < 3 ? step : jump;
                if (idx >= M) idx -= M;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t][r] += (double)f[t][r];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = k0 + 4 * q + r, row = row0 + 16 * t + j;
                    const bool inside = k < S && row < S;
                    double d = acc[t][r];
                    if (k == 0) d += (double)c0[t] * (double)S;
                    const float v = (float)(d * (k == 0 ? a0 : ak));
                    if (!FINAL) {
                        out[(size_t)k * Sp + row] = inside ? v : 0.f;
                    } else if (inside) {
                        if (tap) tap[(size_t)k * S + row] = v;    // (wave-uniform)
                        const float lv = log1pf(fabsf(v));
                        out[(size_t)k * S + row] = lv;
                        lo = fminf(lo, lv);
                        hi = fmaxf(hi, lv);
                    }
                }
    }
    if (FINAL) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off)); hi = fmaxf(hi, __shfl_xor(hi, off)); }
        if (l == 0) { fred[2 * wave] = lo; fred[2 * wave + 1] = hi; }
        __syncthreads();
        if (tid == 0) {
            fpart[(size_t)blockIdx.x * 2] = fminf(fminf(fred[0], fred[2]), fminf(fred[4], fred[6]));
            fpart[(size_t)blockIdx.x * 2 + 1] = fmaxf(fmaxf(fred[1], fred[3]), fmaxf(fred[5], fred[7]));
        }
    }
}

// minmax_norm_kernel's rule at a run-time size
__global__ __launch_bounds__(256) void fd_minmax_norm_kernel(float* __restrict__ v, const float* __restrict__ part, int nparts, int count) {
    float lo = 3.4e38f, hi = -3.4e38f;
    for (int p = 0; p < nparts; ++p) { lo = fminf(lo, part[2 * p]); hi = fmaxf(hi, part[2 * p + 1]); }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    v[i] = (hi - lo > 1e-6f) ? (v[i] - lo) / (hi - lo) : 0.f;
}

// ------------------------------------------------------------------------------------------------ host side
struct FreqDomainState {
    std::map<int, const float2*> dft;       // length -> exp(-2 pi i j / N) on the device, made on first use
    std::map<int, const float*> dct;        // edge S -> cos(pi j / 2S), j < 4S
    DevBuf gray, rows, desc, part, sums, tap_spec, tap_mag;      // windows
    DevBuf gray_full, gray_s, fwork, feat;                       // features
};

void freq_domain_destroy(dfd_handle* h) {
    delete h->freq_domain;
    h->freq_domain = nullptr;
}

namespace {

constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr int kFdMaxWindows = 32768;        // windows of one launch set (the gather's grid.y)

FreqDomainState& fd_state(dfd_handle* h) {
    if (!h->freq_domain) h->freq_domain = new FreqDomainState();
    return *h->freq_domain;
}

// table entries are the float32 roundings of the float64 values, the quarter turns exact: transforms of length 1, 2 and 4
// are then exact, as through an FFT
int fd_dft_table(dfd_handle* h, int N, const float2** out) {
    FreqDomainState& F = fd_state(h);
    auto it = F.dft.find(N);
    if (it == F.dft.end()) {
        std::vector<float2> tw(N);
        for (int j = 0; j < N; ++j) {
            const double a = -2.0 * M_PI * (double)j / (double)N;
            tw[j] = make_float2((float)std::cos(a), (float)std::sin(a));
            if (4 * j % N == 0) {                                 // cos / sin of the rounded pi leave 6e-17 where the value is 0
                const float2 quarter[4] = {{1.f, 0.f}, {0.f, -1.f}, {-1.f, 0.f}, {0.f, 1.f}};
                tw[j] = quarter[4 * j / N];
            }
        }
        void* d = nullptr;
        DFD_HIP_TRY(h, hipMalloc(&d, tw.size() * sizeof(float2)));
        h->owned.push_back(d);
        DFD_HIP_TRY(h, hipMemcpy(d, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        it = F.dft.emplace(N, static_cast<const float2*>(d)).first;
    }
    *out = it->second;
    return DFD_OK;
}

int fd_dct_table(dfd_handle* h, int S, const float** out) {
    FreqDomainState& F = fd_state(h);
    auto it = F.dct.find(S);
    if (it == F.dct.end()) {
        std::vector<float> ct(4 * (size_t)S);
        const float quarter[4] = {1.f, 0.f, -1.f, 0.f};
        for (int j = 0; j < 4 * S; ++j) ct[j] = j % S == 0 ? quarter[j / S] : (float)std::cos(M_PI * (double)j / (2.0 * (double)S));
        void* d = nullptr;
        DFD_HIP_TRY(h, hipMalloc(&d, ct.size() * sizeof(float)));
        h->owned.push_back(d);
        DFD_HIP_TRY(h, hipMemcpy(d, ct.data(), ct.size() * sizeof(float), hipMemcpyHostToDevice));
        it = F.dct.emplace(S, static_cast<const float*>(d)).first;
    }
    *out = it->second;
    return DFD_OK;
}

int pad16(int v) { return (v + 15) & ~15; }

// windows [first, first + cnt) of `boxes` as one launch set on the handle's stream; results into F.sums [cnt][2].
// The host tables of the set live in `wins` / `pre` until the caller's stream wait.
int fd_launch_set(dfd_handle* h, const uint8_t* frame_dev, size_t stride, int channels, const int32_t* boxes, int cnt, bool tap,
                  std::vector<FdWinDev>& wins, std::vector<int>& pre) {
    FreqDomainState& F = fd_state(h);
    wins.assign(cnt, FdWinDev{});
    pre.assign(cnt + 1, 0);
    size_t gray_bytes = 0, rows_elems = 0, tap_elems = 0;
    int max_hp = 0, max_w = 0, max_h = 0;
    for (int i = 0; i < cnt; ++i) {
        FdWin& g = wins[i].g;
        g.x = boxes[4 * i]; g.y = boxes[4 * i + 1]; g.w = boxes[4 * i + 2]; g.h = boxes[4 * i + 3];
        g.wp = pad16(g.w); g.hp = pad16(g.h);
        g.gray_off = (long long)gray_bytes;
        g.rows_off = (long long)rows_elems;
        g.tap_off = (long long)tap_elems;
        gray_bytes += al((size_t)g.hp * g.wp);
        rows_elems += (size_t)g.wp * g.hp;
        tap_elems += (size_t)g.w * g.h;
        pre[i + 1] = pre[i] + g.wp / 16;
        max_hp = std::max(max_hp, g.hp); max_w = std::max(max_w, g.w); max_h = std::max(max_h, g.h);
        int rc;
        if ((rc = fd_dft_table(h, g.w, &wins[i].tw_w))) return rc;
        if ((rc = fd_dft_table(h, g.h, &wins[i].tw_h))) return rc;
    }
    const int tiles = pre[cnt];
    const size_t o_pre = al(wins.size() * sizeof(FdWinDev));
    int rc;
    if ((rc = ensure(h, &F.gray, gray_bytes))) return rc;
    if ((rc = ensure(h, &F.rows, rows_elems * sizeof(float2)))) return rc;
    if ((rc = ensure(h, &F.desc, o_pre + pre.size() * sizeof(int)))) return rc;
    if ((rc = ensure(h, &F.part, (size_t)tiles * 2 * sizeof(double)))) return rc;
    if ((rc = ensure(h, &F.sums, (size_t)cnt * 2 * sizeof(double)))) return rc;
    if (tap) {
        if ((rc = ensure(h, &F.tap_spec, tap_elems * sizeof(float2)))) return rc;
        if ((rc = ensure(h, &F.tap_mag, tap_elems * sizeof(float)))) return rc;
    }
    hipStream_t s = h->stream;
    const FdWinDev* d_wins = (const FdWinDev*)F.desc.p;
    const int* d_pre = (const int*)((char*)F.desc.p + o_pre);
    DFD_HIP_TRY(h, hipMemcpyAsync(F.desc.p, wins.data(), wins.size() * sizeof(FdWinDev), hipMemcpyHostToDevice, s));
    DFD_HIP_TRY(h, hipMemcpyAsync((char*)F.desc.p + o_pre, pre.data(), pre.size() * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(fd_gather_kernel, dim3(max_hp / 16, cnt), dim3(256), 0, s, frame_dev, stride, channels, d_wins, (uint8_t*)F.gray.p);
    hipLaunchKernelGGL(fd_rows_kernel, dim3(tiles), dim3(256), (size_t)max_w * sizeof(float2), s, (const uint8_t*)F.gray.p,
                       (float2*)F.rows.p, d_wins, d_pre, cnt);
    hipLaunchKernelGGL(fd_cols_kernel<false>, dim3(tiles), dim3(256), (size_t)max_h * sizeof(float2), s, (const float2*)F.rows.p, d_wins,
                       d_pre, cnt, (double*)F.part.p, tap ? (float2*)F.tap_spec.p : nullptr, tap ? (float*)F.tap_mag.p : nullptr,
                       (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(fd_sums_kernel, dim3((cnt + 255) / 256), dim3(256), 0, s, (const double*)F.part.p, d_pre, cnt, (double*)F.sums.p);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

int fd_check_boxes(dfd_handle* h, const char* what, int hh, int ww, const int32_t* boxes, int n) {
    for (int i = 0; i < n; ++i) {
        const long long x = boxes[4 * i], y = boxes[4 * i + 1], w = boxes[4 * i + 2], b = boxes[4 * i + 3];
        if (w < 1 || b < 1 || x < 0 || y < 0 || x + w > ww || y + b > hh)
            return fail(h, DFD_ERR_ARG, "%s: box %d (%lld, %lld, %lld, %lld) is empty or leaves the %d x %d frame", what, i, x, y, w, b, ww, hh);
    }
    for (int i = 0; i < n; ++i)
        if (boxes[4 * i + 2] > kFdMaxSide || boxes[4 * i + 3] > kFdMaxSide)
            return fail(h, DFD_ERR_UNSUPPORTED, "%s: box %d is %d x %d; a side above %d is not supported (its table would not fit the LDS)", what, i,
                        boxes[4 * i + 2], boxes[4 * i + 3], kFdMaxSide);
    return DFD_OK;
}

// every window of a device-resident frame -> out [n][2] on the host; launch sets of the windows that fit the work budget
int fd_run(dfd_handle* h, const char* what, const uint8_t* frame_dev, int hh, int ww, size_t stride, int channels, const int32_t* boxes,
           int n, double* out) {
    const int32_t whole[4] = {0, 0, ww, hh};
    if (!boxes) { boxes = whole; n = 1; }
    int rc = fd_check_boxes(h, what, hh, ww, boxes, n);
    if (rc) return rc;
    FreqDomainState& F = fd_state(h);
    std::vector<FdWinDev> wins;
    std::vector<int> pre;
    for (int first = 0; first < n;) {
        size_t bytes = 0;
        int cnt = 0;
        while (first + cnt < n && cnt < kFdMaxWindows) {
            const size_t px = (size_t)pad16(boxes[4 * (first + cnt) + 2]) * pad16(boxes[4 * (first + cnt) + 3]);
            const size_t need = al(px) + px * sizeof(float2);
            if (cnt > 0 && bytes + need > h->forensic_chunk_bytes) break;     // one window at least
            bytes += need;
            ++cnt;
        }
        if ((rc = fd_launch_set(h, frame_dev, stride, channels, boxes + 4 * (size_t)first, cnt, false, wins, pre))) return rc;
        DFD_HIP_TRY(h, hipMemcpyAsync(out + 2 * (size_t)first, F.sums.p, (size_t)cnt * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, stream_sync(h));
        first += cnt;
    }
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

bool fd_geometry_ok(const void* img, int hh, int ww, int stride, int channels) {
    return img && hh > 0 && ww > 0 && (channels == 1 || channels == 3) && stride >= ww * channels;
}

// the feature chain on the frame in h->frame_buf; `tap_name` (or null) names the buffer copied to tap_out instead of the features
int fd_features(dfd_handle* h, const char* what, const uint8_t* img, int hh, int ww, int stride, int channels, int S, float* out,
                const char* tap_name, void* tap_out, size_t capacity) {
    if (!fd_geometry_ok(img, hh, ww, stride, channels)) return fail(h, DFD_ERR_ARG, "%s: bad pointer or geometry", what);
    if (S < 2 || S > kFdMaxFeatureSize || (S & 1))
        return fail(h, DFD_ERR_ARG, "%s: size %d; supported are even sizes in 2..%d (cv2.dct refuses odd sizes)", what, S, kFdMaxFeatureSize);
    const size_t PL = (size_t)S * S;
    int tap = 0;                                                  // 1 gray, 2 spectrum, 3 dct
    if (tap_name) {
        tap = !strcmp(tap_name, "gray") ? 1 : !strcmp(tap_name, "spectrum") ? 2 : !strcmp(tap_name, "dct") ? 3 : 0;
        if (!tap) return fail(h, DFD_ERR_ARG, "%s: unknown buffer '%s'", what, tap_name);
        const size_t need = PL * (tap == 1 ? 1 : tap == 2 ? sizeof(float2) : sizeof(float));
        if (!tap_out || capacity < need) return fail(h, DFD_ERR_ARG, "%s: '%s' needs %zu bytes", what, tap_name, need);
    } else if (!out) {
        return fail(h, DFD_ERR_ARG, "%s: null output", what);
    }
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    FreqDomainState& F = fd_state(h);
    const int Sp = pad16(S), tiles = Sp / 16;
    const size_t PP = (size_t)Sp * Sp;
    const float2* tw = nullptr;
    const float* ct = nullptr;
    int rc;
    if ((rc = fd_dft_table(h, S, &tw))) return rc;
    if ((rc = fd_dct_table(h, S, &ct))) return rc;
    if ((rc = ensure(h, &h->frame_buf, (size_t)hh * stride))) return rc;
    if ((rc = ensure(h, &F.gray_full, (size_t)hh * ww))) return rc;
    if ((rc = ensure(h, &F.gray_s, PL))) return rc;
    if ((rc = ensure(h, &F.gray, al(PP)))) return rc;
    if ((rc = ensure(h, &F.rows, PP * sizeof(float2)))) return rc;
    // float work: plane | pass A of the DCT | dct tap | min / max partials of both channels
    const size_t o_a = al(PP * 4), o_tap = o_a + al(PP * 4), o_part = o_tap + al(PL * 4), work = o_part + al((size_t)tiles * 4 * 4);
    if ((rc = ensure(h, &F.fwork, work))) return rc;
    if ((rc = ensure(h, &F.feat, 2 * PL * 4))) return rc;
    if ((rc = ensure(h, &F.desc, al(sizeof(FdWinDev)) + 2 * sizeof(int)))) return rc;
    if (tap == 2 && (rc = ensure(h, &F.tap_spec, PL * sizeof(float2)))) return rc;
    char* fw = (char*)F.fwork.p;
    float *plane = (float*)fw, *pass_a = (float*)(fw + o_a), *dct_tap = (float*)(fw + o_tap), *part0 = (float*)(fw + o_part), *part1 = part0 + 2 * tiles;
    float *o0 = (float*)F.feat.p, *o1 = o0 + PL;
    FdWinDev win{};
    win.g = FdWin{0, 0, S, S, Sp, Sp, 0, 0, 0};
    win.tw_w = win.tw_h = tw;
    const int pre[2] = {0, tiles};
    const FdWinDev* d_win = (const FdWinDev*)F.desc.p;
    const int* d_pre = (const int*)((char*)F.desc.p + al(sizeof(FdWinDev)));
    hipStream_t s = h->stream;
    DFD_HIP_TRY(h, hipMemcpyAsync(h->frame_buf.p, img, (size_t)hh * stride, hipMemcpyHostToDevice, s));
    DFD_HIP_TRY(h, hipMemcpyAsync(F.desc.p, &win, sizeof(win), hipMemcpyHostToDevice, s));
    DFD_HIP_TRY(h, hipMemcpyAsync((char*)F.desc.p + al(sizeof(FdWinDev)), pre, sizeof(pre), hipMemcpyHostToDevice, s));
    launch_gray_full((const uint8_t*)h->frame_buf.p, hh, ww, (size_t)stride, channels, (uint8_t*)F.gray_full.p, s);
    launch_resize_gray((const uint8_t*)F.gray_full.p, hh, ww, (uint8_t*)F.gray_s.p, S, S, s);      // cv2.resize(gray, (S, S))
    hipLaunchKernelGGL(fd_gather_kernel, dim3(tiles, 1), dim3(256), 0, s, (const uint8_t*)F.gray_s.p, (size_t)S, 1, d_win, (uint8_t*)F.gray.p);
    // channel 0: fft2 -> fftshift -> log1p|.| -> min-max
    hipLaunchKernelGGL(fd_rows_kernel, dim3(tiles), dim3(256), (size_t)S * sizeof(float2), s, (const uint8_t*)F.gray.p, (float2*)F.rows.p, d_win, d_pre, 1);
    hipLaunchKernelGGL(fd_cols_kernel<true>, dim3(tiles), dim3(256), (size_t)S * sizeof(float2), s, (const float2*)F.rows.p, d_win, d_pre, 1,
                       (double*)nullptr, tap == 2 ? (float2*)F.tap_spec.p : nullptr, (float*)nullptr, o0, part0);
    const int nb = (int)((PL + 255) / 256);
    hipLaunchKernelGGL(fd_minmax_norm_kernel, dim3(nb), dim3(256), 0, s, o0, part0, tiles, (int)PL);
    // channel 1: dct2(gray / 255) -> log1p|.| -> min-max
    u8_to_float((const uint8_t*)F.gray.p, plane, (int)PP, 1.0f / 255.0f, s);
    hipLaunchKernelGGL(fd_dct_kernel<false>, dim3(tiles), dim3(256), (size_t)S * 16, s, plane, pass_a, ct, S, Sp, (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(fd_dct_kernel<true>, dim3(tiles), dim3(256), (size_t)S * 16, s, pass_a, o1, ct, S, Sp, part1, tap == 3 ? dct_tap : nullptr);
    hipLaunchKernelGGL(fd_minmax_norm_kernel, dim3(nb), dim3(256), 0, s, o1, part1, tiles, (int)PL);
    if (tap == 1) DFD_HIP_TRY(h, hipMemcpyAsync(tap_out, F.gray_s.p, PL, hipMemcpyDeviceToHost, s));
    else if (tap == 2) DFD_HIP_TRY(h, hipMemcpyAsync(tap_out, F.tap_spec.p, PL * sizeof(float2), hipMemcpyDeviceToHost, s));
    else if (tap == 3) DFD_HIP_TRY(h, hipMemcpyAsync(tap_out, dct_tap, PL * 4, hipMemcpyDeviceToHost, s));
    else DFD_HIP_TRY(h, hipMemcpyAsync(out, o0, 2 * PL * 4, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

}  // namespace
}  // namespace dfd

using namespace dfd;

extern "C" int dfd_frequency_domain_device(dfd_handle* h, const uint8_t* img_dev, int hh, int ww, int stride, int channels,
                                           const int32_t* boxes, int n, double* out) {
    if (!h) return DFD_ERR_ARG;
    if (!fd_geometry_ok(img_dev, hh, ww, stride, channels) || !out || (boxes && n < 1))
        return fail(h, DFD_ERR_ARG, "frequency_domain_device: bad pointer or geometry");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    return fd_run(h, "frequency_domain_device", img_dev, hh, ww, (size_t)stride, channels, boxes, n, out);
}

extern "C" int dfd_frequency_domain(dfd_handle* h, const uint8_t* img, int hh, int ww, int stride, int channels, const int32_t* boxes,
                                    int n, double* out) {
    if (!h) return DFD_ERR_ARG;
    if (!fd_geometry_ok(img, hh, ww, stride, channels) || !out || (boxes && n < 1))
        return fail(h, DFD_ERR_ARG, "frequency_domain: bad pointer or geometry");
    const int32_t whole[4] = {0, 0, ww, hh};
    int rc = fd_check_boxes(h, "frequency_domain", hh, ww, boxes ? boxes : whole, boxes ? n : 1);     // before the upload
    if (rc) return rc;
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ensure(h, &h->frame_buf, (size_t)hh * stride))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(h->frame_buf.p, img, (size_t)hh * stride, hipMemcpyHostToDevice, h->stream));
    return fd_run(h, "frequency_domain", (const uint8_t*)h->frame_buf.p, hh, ww, (size_t)stride, channels, boxes, n, out);
}

extern "C" int dfd_frequency_domain_tap(dfd_handle* h, const uint8_t* gray, int hh, int ww, const char* name, void* out, size_t capacity) {
    if (!h) return DFD_ERR_ARG;
    if (!gray || hh < 1 || ww < 1 || !name || !out) return fail(h, DFD_ERR_ARG, "frequency_domain_tap: bad pointer or geometry");
    const int32_t box[4] = {0, 0, ww, hh};
    int rc = fd_check_boxes(h, "frequency_domain_tap", hh, ww, box, 1);
    if (rc) return rc;
    const size_t px = (size_t)hh * ww;
    const int which = !strcmp(name, "rows") ? 0 : !strcmp(name, "spectrum") ? 1 : !strcmp(name, "mag") ? 2 : !strcmp(name, "sums") ? 3 : -1;
    if (which < 0) return fail(h, DFD_ERR_ARG, "frequency_domain_tap: unknown buffer '%s'", name);
    const size_t need = which <= 1 ? px * sizeof(float2) : which == 2 ? px * sizeof(float) : 2 * sizeof(double);
    if (capacity < need) return fail(h, DFD_ERR_ARG, "frequency_domain_tap: '%s' needs %zu bytes", name, need);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = ensure(h, &h->frame_buf, px))) return rc;
    hipStream_t s = h->stream;
    DFD_HIP_TRY(h, hipMemcpyAsync(h->frame_buf.p, gray, px, hipMemcpyHostToDevice, s));
    std::vector<FdWinDev> wins;
    std::vector<int> pre;
    if ((rc = fd_launch_set(h, (const uint8_t*)h->frame_buf.p, (size_t)ww, 1, box, 1, true, wins, pre))) return rc;
    FreqDomainState& F = *h->freq_domain;
    if (which == 0)           // the padded [wp][hp] array -> [w][h]
        DFD_HIP_TRY(h, hipMemcpy2DAsync(out, (size_t)hh * sizeof(float2), F.rows.p, (size_t)wins[0].g.hp * sizeof(float2),
                                        (size_t)hh * sizeof(float2), (size_t)ww, hipMemcpyDeviceToHost, s));
    else if (which == 1) DFD_HIP_TRY(h, hipMemcpyAsync(out, F.tap_spec.p, need, hipMemcpyDeviceToHost, s));
    else if (which == 2) DFD_HIP_TRY(h, hipMemcpyAsync(out, F.tap_mag.p, need, hipMemcpyDeviceToHost, s));
    else DFD_HIP_TRY(h, hipMemcpyAsync(out, F.sums.p, need, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

extern "C" int dfd_frequency_features_sized(dfd_handle* h, const uint8_t* img, int hh, int ww, int stride, int channels, int size,
                                            float* out) {
    if (!h) return DFD_ERR_ARG;
    return fd_features(h, "frequency_features_sized", img, hh, ww, stride, channels, size, out, nullptr, nullptr, 0);
}

extern "C" int dfd_frequency_features_tap(dfd_handle* h, const uint8_t* img, int hh, int ww, int stride, int channels, int size,
                                          const char* name, void* out, size_t capacity) {
    if (!h) return DFD_ERR_ARG;
    if (!name) return fail(h, DFD_ERR_ARG, "frequency_features_tap: null buffer name");
    return fd_features(h, "frequency_features_tap", img, hh, ww, stride, channels, size, nullptr, name, out, capacity);
}

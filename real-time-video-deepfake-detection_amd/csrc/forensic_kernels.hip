// Forensic-signal kernels on the S x S analysis image (S % 16 == 0, 32 <= S <= 1024; gfx950).  Apart from the general
// spectrum, HBM/latency-bound integer or fp32 byte work without MFMA.  One launch handles a batch of frames (blockIdx.y
// or blockIdx.z = frame); every reduction is written as per-row or per-block partials and summed in a fixed order by
// stats_finalize_kernel, so results are run-to-run and batch-size identical (no float atomics).
//
// Every stage is written once, as template <int CS>: CS = 256 is the benchmarked 256x256 chain, whose S, S * S, S / 32,
// i / S and row loops fold to constants; CS = 0 takes the edge from the run-time argument (the general chain).  Only the
// spectrum is two algorithms: a radix-2 fp32 FFT at 256, a dense two-pass DFT on the fp32 MFMA at any S (no
// power-of-two FFT serves S = 80, 224, 272).
//
//   gray_kernel            BGR->GRAY fixed point                          frame_analysis.py:136,188,...
//   fft256_kernel          256-point complex FFT rows (LDS radix-2)       frame_analysis.py:139-141
//   fft_band_kernel        second FFT pass + log1p|X| band sums           frame_analysis.py:141-165
//   dft_rows_kernel        row DFT, v_mfma_f32_16x16x4_f32, transposed    frame_analysis.py:139-141
//   dft_band_kernel        column DFT + log1p|X| band sums (fused)        frame_analysis.py:141-165
//   noise_block_kernel     gray - GaussianBlur5 -> 32x32 block std        frame_analysis.py:188-202
//   jpeg_block_kernel      q90 4:2:0 islow DCT round trip per block       frame_analysis.py:233-236
//   ela_block_kernel       fancy upsample + YCC->RGB + absdiff stats      frame_analysis.py:242-253
//   sobel_lap_kernel       Sobel dx/dy + Laplacian sums                   frame_analysis.py:289-294
//   canny_nms_kernel       fixed-point non-maximum suppression            frame_analysis.py:289
//   canny_hyst_kernel      8-connected hysteresis in LDS + edge count     frame_analysis.py:289-290
//   hsv_stats_kernel       BGR->HSV integer + S/V moments + hue set       frame_analysis.py:318-338
//   absdiff_kernel         sum |gray - prev gray|                         frame_analysis.py:363-364
//   absdiff_prev_kernel    the same for frames of many streams and edges, one launch (the batched stream entries)
//   copy_planes_kernel     every stream's last gray plane to its stored slot, one launch
//
// Compiled with -ffp-contract=off (operation orders restate OpenCV's float filters).
#include "forensic_kernels.h"

#include <cmath>

#include "forensic_device.h"
#include "jpeg_sample.h"

namespace dfd {

constexpr int FS = 256;            // edge of the FFT pair and of absdiff_pairs_kernel
constexpr int FPIX = FS * FS;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

// the analysis edge in use: the compile-time CS, or the run-time argument when CS = 0
template <int CS>
__device__ __forceinline__ int edge_of(int s_arg) { return CS ? CS : s_arg; }

__device__ __forceinline__ int r101(int i, int S) { i = i < 0 ? -i : i; return i >= S ? 2 * (S - 1) - i : i; }

// one block-wide sum; result valid in thread 0
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    double a[1] = {v};
    block_sum_n<NT, 1>(a, sh);
    return a[0];
}

}  // namespace

// ---------------------------------------------------------------------------------- gray
// S * S is a multiple of 256: the grid covers the plane exactly
template <int CS>
__global__ __launch_bounds__(256) void gray_kernel(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ gray, int s_arg) {
    const int S = edge_of<CS>(s_arg);
    const size_t i = (size_t)blockIdx.y * S * S + (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint8_t* p = bgr + i * 3;
    gray[i] = (uint8_t)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14);
}

// ---------------------------------------------------------------------------------- FFT (the 256x256 chain)
// 256-point radix-2 DIT in LDS, 128 threads = one butterfly each per stage.
__device__ __forceinline__ void fft256_lds(float2* x, const float2* __restrict__ tw, int tid) {
    for (int half = 1; half < 256; half <<= 1) {
        const int pos = tid & (half - 1);
        const int i0 = ((tid - pos) << 1) + pos, i1 = i0 + half;
        const float2 w = tw[pos * (128 / half)];
        const float2 a = x[i0], b = x[i1];
        const float2 t = make_float2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x);
        x[i0] = make_float2(a.x + t.x, a.y + t.y);
        x[i1] = make_float2(a.x - t.x, a.y - t.y);
        __syncthreads();
    }
}

// pass 1: FFT of each image row (real input); output stored transposed [k][row]
__global__ __launch_bounds__(128) void fft256_kernel(const uint8_t* __restrict__ gray, float2* __restrict__ out,
                                                     const float2* __restrict__ tw) {
    __shared__ float2 x[256];
    const int tid = threadIdx.x, row = blockIdx.x;
    const uint8_t* g = gray + (size_t)blockIdx.y * FPIX + row * FS;
    for (int i = tid; i < 256; i += 128) x[__brev((unsigned)i) >> 24] = make_float2((float)g[i], 0.f);
    __syncthreads();
    fft256_lds(x, tw, tid);
    float2* o = out + (size_t)blockIdx.y * FPIX;
    for (int k = tid; k < 256; k += 128) o[(size_t)k * FS + row] = x[k];
}

// pass 2: FFT along the other axis, then log1p|X| accumulated into the three radial bands.
// The band masks depend on k1^2+k2^2 only, so working on the transposed array changes nothing.
// spec_out / logmag_out: test taps ([frame][k1][k2], the layout of `in`), null on every production launch.
__global__ __launch_bounds__(128) void fft_band_kernel(const float2* __restrict__ in, double* __restrict__ part,
                                                       const float2* __restrict__ tw, float2* __restrict__ spec_out,
                                                       float* __restrict__ logmag_out) {
    __shared__ float2 x[256];
    __shared__ double red[2 * 7];
    const int tid = threadIdx.x, k1 = blockIdx.x;
    const float2* src = in + (size_t)blockIdx.y * FPIX + (size_t)k1 * FS;
    for (int i = tid; i < 256; i += 128) x[__brev((unsigned)i) >> 24] = src[i];
    __syncthreads();
    fft256_lds(x, tw, tid);
    const int s1 = k1 < 128 ? k1 : k1 - 256;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};      // low sum,cnt | mid sum,sumsq,cnt | high sum,cnt
    for (int k2 = tid; k2 < 256; k2 += 128) {
        const int s2 = k2 < 128 ? k2 : k2 - 256;
        const int d2 = s1 * s1 + s2 * s2;
        const float m = log1pf(hypotf(x[k2].x, x[k2].y));
        if (spec_out) {                                       // (wave-uniform)
            const size_t o = (size_t)blockIdx.y * FPIX + (size_t)k1 * FS + k2;
            spec_out[o] = x[k2];
            logmag_out[o] = m;
        }
        if (d2 <= 32 * 32) { acc[0] += m; acc[1] += 1.0; }
        else if (d2 <= 64 * 64) { acc[2] += m; acc[3] += (double)m * m; acc[4] += 1.0; }
        else if (d2 <= 128 * 128) { acc[5] += m; acc[6] += 1.0; }
    }
    double* p = part + ((size_t)blockIdx.y * FS + k1) * 7;
    block_sum_n<128, 7>(acc, red);
    if (tid == 0)
#pragma unroll
        for (int j = 0; j < 7; ++j) p[j] = acc[j];
}

// ---------------------------------------------------------------------------------- DFT (the general chain)
// X = W G W as two dense products on v_mfma_f32_16x16x4_f32 (A[i][k] on lane i = l & 15, k = l >> 4; B[k][j] on lane
// j = l & 15, k = l >> 4; D[i][j] on lane j = l & 15, register r, i = 4 (l >> 4) + r).  A block of four waves owns 16
// output rows; wave w walks the 64-column groups w, w + 4, ... with four 16x16 accumulators per part.  The lane's
// k-group q supplies the four consecutive k = 4q .. 4q + 3 of a 16-wide K chunk (one 4-byte or two 16-byte loads) to
// MFMAs e = 0..3 - the same permutation of k on both operands.  The S-entry table exp(-2 pi i j / S) sits in LDS and is
// indexed by (k n) mod S, carried forward by additions and one conditional subtraction, so the argument is exact for
// any S.  Accuracy: every 16-wide K chunk is summed in fp32 by the MFMA and added to a double accumulator (a 1024-term
// fp32 chain would cost ~K / sqrt(2) roundings of the partial sum; the chunks cost 11 each and add in quadrature), and
// each transformed row is centred on its own first element x[0]: the row's transform differs only by S x[0] in bin 0,
// added back in the epilogue (exact in pass 1, where x is an integer), so constant rows - a constant frame, a vertical
// ramp - transform to exact zeros off bin 0 as they do through an FFT, instead of to the rounding residue of S terms.
//
// pass 1: out[k][row] = sum_n W[k n] g[row][n], stored transposed so pass 2 reads rows.
__global__ __launch_bounds__(256) void dft_rows_kernel(const uint8_t* __restrict__ gray, float2* __restrict__ out,
                                                       const float2* __restrict__ table, int S) {
    extern __shared__ float2 dft_tw[];
    const int tid = threadIdx.x;
    for (int i = tid; i < S; i += 256) dft_tw[i] = table[i];
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, j = l & 15, q = l >> 4;
    const size_t fo = (size_t)blockIdx.y * S * S;
    const uint8_t* g = gray + fo;
    const int k0 = blockIdx.x * 16, kf = k0 + j;                  // this lane's A row
    const int jump = (13 * kf) % S;                               // from k = 4q + 3 of one chunk to 4q of the next
    const int ngroups = (S + 63) >> 6;
    for (int grp = wave; grp < ngroups; grp += 4) {
        const int row0 = grp * 64;
        const int nt = min(4, (S - row0) >> 4);                   // (wave-uniform)
        double dre[4][4], dim[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dre[t][r] = dim[t][r] = 0.0;
        int idx = (kf * 4 * q) % S;
        int c0[4] = {0, 0, 0, 0};                                 // first pixel of this lane's image row, per tile
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt) c0[t] = g[(size_t)(row0 + 16 * t + j) * S];
        for (int n0 = 0; n0 < S; n0 += 16) {
            uchar4 bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt) bv[t] = *reinterpret_cast<const uchar4*>(g + (size_t)(row0 + 16 * t + j) * S + n0 + 4 * q);
            v4f are[4], aim[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { are[t] = v4f{0.f, 0.f, 0.f, 0.f}; aim[t] = v4f{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float2 w = dft_tw[idx];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) {
                        const int px = e == 0 ? bv[t].x : e == 1 ? bv[t].y : e == 2 ? bv[t].z : bv[t].w;
                        const float b = (float)(px - c0[t]);
                        are[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b, are[t], 0, 0, 0);
                        aim[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b, aim[t], 0, 0, 0);
                    }
                idx += e < 3 ? kf : jump;
                if (idx >= S) idx -= S;
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
                    if (k0 + 4 * q + r == 0) dre[t][r] += (double)(c0[t] * S);      // bin 0 of the row (D column j = B column j)
                    out[fo + (size_t)(k0 + 4 * q + r) * S + row0 + 16 * t + j] = make_float2((float)dre[t][r], (float)dim[t][r]);
                }
    }
}

// pass 2: X[k1][k2] = sum_row in[k1][row] W[row k2] (complex x complex: four real products), then log1pf(hypotf()) of
// every bin accumulated into the three radial bands of its row k1 - the spectrum leaves the registers only through the
// test taps (spec_out / logmag_out, null on every production launch).  The masks depend on s1^2 + s2^2 alone (s = the
// signed frequency, the fftshift index minus S / 2), so the transposed layout changes nothing.
// part [n][S][7]: low sum, count | mid sum, sum of squares, count | high sum, count.
__global__ __launch_bounds__(256) void dft_band_kernel(const float2* __restrict__ in, double* __restrict__ part,
                                                       const float2* __restrict__ table, int S,
                                                       float2* __restrict__ spec_out, float* __restrict__ logmag_out) {
    extern __shared__ float2 dft_tw[];
    __shared__ double red[4 * 16 * 7];
    const int tid = threadIdx.x;
    for (int i = tid; i < S; i += 256) dft_tw[i] = table[i];
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, j = l & 15, q = l >> 4;
    const size_t fo = (size_t)blockIdx.y * S * S;
    const int k0 = blockIdx.x * 16;
    const float2* src = in + fo + (size_t)(k0 + j) * S;           // this lane's A row
    const float2 x0 = src[0];                                     // ... centred on its first element
    const int half = S >> 1, r_in = S >> 3, r_mid = S >> 2, r_out = S >> 1;
    double acc[4][7];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 7; ++c) acc[r][c] = 0.0;
    const int ngroups = (S + 63) >> 6;
    for (int grp = wave; grp < ngroups; grp += 4) {
        const int col0 = grp * 64;
        const int nt = min(4, (S - col0) >> 4);                   // (wave-uniform)
        int idx[4], step[4], jump[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k2 = (col0 + 16 * t + j) % S;               // (tiles past nt are never used)
            step[t] = k2;
            jump[t] = (13 * k2) % S;
            idx[t] = (k2 * 4 * q) % S;
        }
        double dre[4][4], dim[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dre[t][r] = dim[t][r] = 0.0;
        for (int r0 = 0; r0 < S; r0 += 16) {
            const float4 a01 = *reinterpret_cast<const float4*>(src + r0 + 4 * q);
            const float4 a23 = *reinterpret_cast<const float4*>(src + r0 + 4 * q + 2);
            v4f fre[4], fim[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { fre[t] = v4f{0.f, 0.f, 0.f, 0.f}; fim[t] = v4f{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float tr = (e == 0 ? a01.x : e == 1 ? a01.z : e == 2 ? a23.x : a23.z) - x0.x;
                const float ti = (e == 0 ? a01.y : e == 1 ? a01.w : e == 2 ? a23.y : a23.w) - x0.y;
                float2 w[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) {
                        w[t] = dft_tw[idx[t]];
                        idx[t] += e < 3 ? step[t] : jump[t];
                        if (idx[t] >= S) idx[t] -= S;
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
                    double re = dre[t][r], im = dim[t][r];
                    if (k2 == 0) {                                    // bin 0 of row k1: S times the element it was centred on
                        const float2 z = in[fo + (size_t)k1 * S];
                        re += (double)z.x * (double)S;
                        im += (double)z.y * (double)S;
                    }
                    const float xr = (float)re, xi = (float)im;
                    const float m = log1pf(hypotf(xr, xi));
                    if (spec_out) {                                   // (wave-uniform)
                        const size_t o = fo + (size_t)k1 * S + k2;
                        spec_out[o] = make_float2(xr, xi);
                        logmag_out[o] = m;
                    }
                    const int s1 = k1 < half ? k1 : k1 - S, s2 = k2 < half ? k2 : k2 - S;
                    const int d2 = s1 * s1 + s2 * s2;
                    if (d2 <= r_in * r_in) { acc[r][0] += m; acc[r][1] += 1.0; }
                    else if (d2 <= r_mid * r_mid) { acc[r][2] += m; acc[r][3] += (double)m * m; acc[r][4] += 1.0; }
                    else if (d2 <= r_out * r_out) { acc[r][5] += m; acc[r][6] += 1.0; }
                }
    }
    // the 16 lanes of a k-group hold the columns of rows 4q + r: butterfly over j, then the four waves in order
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            double v = acc[r][c];
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (j == 0) red[(wave * 16 + 4 * q + r) * 7 + c] = v;
        }
    __syncthreads();
    if (tid < 16 * 7) {
        double v = 0.0;
        for (int w = 0; w < 4; ++w) v += red[w * 16 * 7 + tid];
        part[((size_t)blockIdx.y * S + k0) * 7 + tid] = v;
    }
}

// --------------------------------------------------------------------------------- noise
// residual = gray - blur5(gray) (separable [1,4,6,4,1]/16, reflect-101 at S - 1, fp32 in OpenCV's symmetric-filter
// order); population std of each 32x32 block at i, j in range(0, S - 31, 32).
__device__ __forceinline__ float blur_row(const uint8_t* g, int y, int x, int S) {
    const uint8_t* r = g + y * S;                           // inside one plane: below 2^20
    float s = 0.375f * (float)r[x];
    s = s + 0.25f * ((float)r[r101(x - 1, S)] + (float)r[r101(x + 1, S)]);
    s = s + 0.0625f * ((float)r[r101(x - 2, S)] + (float)r[r101(x + 2, S)]);
    return s;
}

template <int CS>
__global__ __launch_bounds__(256) void noise_block_kernel(const uint8_t* __restrict__ gray, double* __restrict__ stds, int s_arg) {
    __shared__ float res[1024];
    __shared__ double red[4];
    __shared__ double mean_sh;
    const int S = edge_of<CS>(s_arg);
    const int tid = threadIdx.x, blk = blockIdx.x, nb = S >> 5;
    const uint8_t* g = gray + (size_t)blockIdx.y * S * S;
    const int by = (blk / nb) * 32, bx = (blk % nb) * 32;
    double s = 0.0;
    for (int i = tid; i < 1024; i += 256) {
        const int y = by + (i >> 5), x = bx + (i & 31);
        float o = 0.375f * blur_row(g, y, x, S);
        o = o + 0.25f * (blur_row(g, r101(y - 1, S), x, S) + blur_row(g, r101(y + 1, S), x, S));
        o = o + 0.0625f * (blur_row(g, r101(y - 2, S), x, S) + blur_row(g, r101(y + 2, S), x, S));
        const float r = (float)g[y * S + x] - o;
        res[i] = r;
        s += r;
    }
    const double tot = block_sum<256>(s, red);
    if (tid == 0) mean_sh = tot / 1024.0;
    __syncthreads();
    const double mean = mean_sh;
    double q = 0.0;
    for (int i = tid; i < 1024; i += 256) { const double d = (double)res[i] - mean; q += d * d; }
    const double ss = block_sum<256>(q, red);
    if (tid == 0) stds[(size_t)blockIdx.y * nb * nb + blk] = sqrt(ss / 1024.0);
}

// ---------------------------------------------------------------------------------- JPEG
// libjpeg integer pipeline per 8x8 block, one thread per block (64 coefficients in registers): the arithmetic of
// jpeg_sample.h with the quantiser of quality 90, every divisor a compile-time constant after unrolling.
// The two block loads below are jpeg420_luma_block / jpeg420_chroma_block written out.  Calling the shared loaders gives
// the same IR after inlining but another register allocation at this kernel's 256 VGPRs: jpeg_block_kernel<256> grew
// from 12,945 to 13,206-13,670 instructions and took 41.6-42.3 us against 40.1-40.5 us for 16 frames on the MI355X, twice
// in two shapes of the helper, outside the 0.4 us spread of the same build.  Written out, both
// instantiations compile to the instructions they had.
//
// grid x: ceil((S/8)^2 / 64) blocks of luma 8x8 blocks, then ceil(2 (S/16)^2 / 64) blocks of chroma ones (Cb, then Cr),
// so a wave is all luma or all chroma (at 256: 16 + 8 blocks)
template <int CS>
__global__ __launch_bounds__(64) void jpeg_block_kernel(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ yp,
                                                        uint8_t* __restrict__ cbp, uint8_t* __restrict__ crp, int s_arg) {
    const int S = edge_of<CS>(s_arg);
    const int ly = S >> 3, lc = S >> 4, n_y = ly * ly, n_c = lc * lc, gy = (n_y + 63) >> 6;
    const size_t fpix = (size_t)S * S;
    const uint8_t* img = bgr + (size_t)blockIdx.y * fpix * 3;
    int d[64];
    if ((int)blockIdx.x < gy) {
        const int b = blockIdx.x * 64 + threadIdx.x;
        if (b >= n_y) return;
        const int by = (b / ly) * 8, bx = (b % ly) * 8;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const uint8_t* p = img + ((size_t)(by + (i >> 3)) * S + bx + (i & 7)) * 3;
            d[i] = ycc_y(p[2], p[1], p[0]) - 128;
        }
        jpeg_roundtrip(d, [](int i) { return jpeg_quant_value(0, i, jpeg_quality_scale(90)); },
                       yp + (size_t)blockIdx.y * fpix + (size_t)by * S + bx, S);
    } else {
        const int b = (blockIdx.x - gy) * 64 + threadIdx.x;
        if (b >= 2 * n_c) return;
        const bool is_cr = b >= n_c;
        const int c = is_cr ? b - n_c : b, hs = S >> 1;
        const int by = (c / lc) * 8, bx = (c % lc) * 8;          // in the S/2 x S/2 chroma plane
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const int cy = by + (i >> 3), cx = bx + (i & 7);
            int s = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* p = img + ((size_t)(2 * cy + (k >> 1)) * S + 2 * cx + (k & 1)) * 3;
                s += is_cr ? ycc_cr(p[2], p[1], p[0]) : ycc_cb(p[2], p[1], p[0]);
            }
            d[i] = ((s + ((cx & 1) ? 2 : 1)) >> 2) - 128;          // h2v2_downsample, bias 1,2,1,2,...
        }
        jpeg_roundtrip(d, [](int i) { return jpeg_quant_value(1, i, jpeg_quality_scale(90)); },
                       (is_cr ? crp : cbp) + (size_t)blockIdx.y * (fpix / 4) + (size_t)by * hs + bx, hs);
    }
}

// per 32x32 block: sum of gray(|frame - decoded|); exact integers.  The chroma planes are hs = S / 2 >= 16 samples wide:
// fancy_h2v2's cw > 2 holds
template <int CS>
__global__ __launch_bounds__(256) void ela_block_kernel(const uint8_t* __restrict__ bgr, const uint8_t* __restrict__ yp,
                                                        const uint8_t* __restrict__ cbp, const uint8_t* __restrict__ crp,
                                                        double* __restrict__ means, int s_arg) {
    __shared__ double red[4];
    const int S = edge_of<CS>(s_arg);
    const int tid = threadIdx.x, blk = blockIdx.x, nb = S >> 5, hs = S >> 1;
    const size_t f = blockIdx.y, fpix = (size_t)S * S;
    const int by = (blk / nb) * 32, bx = (blk % nb) * 32;
    long long s = 0;
    for (int i = tid; i < 1024; i += 256) {
        const int y = by + (i >> 5), x = bx + (i & 31);
        const size_t o = f * fpix + (size_t)y * S + x;
        const int Yv = yp[o];
        const int cb = fancy_h2v2(cbp + f * (fpix / 4), hs, hs, hs, y, x) - 128, cr = fancy_h2v2(crp + f * (fpix / 4), hs, hs, hs, y, x) - 128;
        int r, g, b;
        ycc_to_rgb(Yv, cb, cr, r, g, b);
        const uint8_t* p = bgr + o * 3;
        const int db = abs((int)p[0] - b), dg = abs((int)p[1] - g), dr = abs((int)p[2] - r);
        s += (db * 1868 + dg * 9617 + dr * 4899 + (1 << 13)) >> 14;
    }
    const double tot = block_sum<256>((double)s, red);
    if (tid == 0) means[f * nb * nb + blk] = tot / 1024.0;
}

// --------------------------------------------------------------------------------- edges
// One block per image row.  Sobel (BORDER_REPLICATE) dx,dy as int16 pairs + Laplacian ([0 1 0;1 -4 1;0 1 0],
// reflect-101) sums of the row (sum, sum of squares as exact integers).
template <int CS>
__global__ __launch_bounds__(256) void sobel_lap_kernel(const uint8_t* __restrict__ gray, short2* __restrict__ grad,
                                                        double* __restrict__ part, int s_arg) {
    __shared__ double red[4 * 2];
    const int S = edge_of<CS>(s_arg);
    const int tid = threadIdx.x, y = blockIdx.x;
    const size_t fo = (size_t)blockIdx.y * S * S;
    const uint8_t* g = gray + fo;
    const int ym = y > 0 ? y - 1 : 0, yp = y < S - 1 ? y + 1 : S - 1;
    const uint8_t *rm = g + (size_t)ym * S, *rc = g + (size_t)y * S, *rp = g + (size_t)yp * S;
    const uint8_t *lm = g + (size_t)r101(y - 1, S) * S, *lp = g + (size_t)r101(y + 1, S) * S;
    double ss[2] = {0.0, 0.0};
    for (int x = tid; x < S; x += 256) {
        const int xm = x > 0 ? x - 1 : 0, xp = x < S - 1 ? x + 1 : S - 1;
        const int a = rm[xm], b = rm[x], c = rm[xp];
        const int d = rc[xm], e = rc[x], f = rc[xp];
        const int h = rp[xm], k = rp[x], l = rp[xp];
        const int dx = (c + 2 * f + l) - (a + 2 * d + h), dy = (h + 2 * k + l) - (a + 2 * b + c);
        grad[fo + (size_t)y * S + x] = make_short2((short)dx, (short)dy);
        const int lap = lm[x] + lp[x] + rc[r101(x - 1, S)] + rc[r101(x + 1, S)] - 4 * e;
        ss[0] += (double)lap;
        ss[1] += (double)lap * (double)lap;
    }
    block_sum_n<256, 2>(ss, red);
    if (tid == 0) {
        part[((size_t)blockIdx.y * S + y) * 2] = ss[0];
        part[((size_t)blockIdx.y * S + y) * 2 + 1] = ss[1];
    }
}

__device__ __forceinline__ int mag_at(const short2* g, int y, int x, int S) {
    if ((unsigned)y >= (unsigned)S || (unsigned)x >= (unsigned)S) return 0;    // OpenCV's zero mag border
    const short2 v = g[(size_t)y * S + x];
    return abs((int)v.x) + abs((int)v.y);
}

// map: 1 = not an edge, 0 = candidate (passed NMS, above low), 2 = strong (above high)
template <int CS>
__global__ __launch_bounds__(256) void canny_nms_kernel(const short2* __restrict__ grad, uint8_t* __restrict__ map,
                                                        int low, int high, int s_arg) {
    const int S = edge_of<CS>(s_arg);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t fo = (size_t)blockIdx.y * S * S;
    const short2* g = grad + fo;
    const int y = i / S, x = i - y * S;
    const int xs = g[i].x, ys = g[i].y;
    const int m = abs(xs) + abs(ys);
    uint8_t lab = 1;
    if (m > low) {
        const int ax = abs(xs), ay = abs(ys) << 15;
        const int tg22 = ax * 13573;
        bool keep;
        if (ay < tg22) keep = m > mag_at(g, y, x - 1, S) && m >= mag_at(g, y, x + 1, S);
        else {
            const int tg67 = tg22 + (ax << 16);
            if (ay > tg67) keep = m > mag_at(g, y - 1, x, S) && m >= mag_at(g, y + 1, x, S);
            else {
                const int s = (xs ^ ys) < 0 ? -1 : 1;
                keep = m > mag_at(g, y - 1, x - s, S) && m > mag_at(g, y + 1, x + s, S);
            }
        }
        if (keep) lab = m > high ? 2 : 0;
    }
    map[fo + i] = lab;
}

// Hysteresis.  One 1024-thread block per frame; strong pixels and weak candidates as bitboards, one 64-pixel word of a
// row per bit set, rows of wpr = ceil(S / 64) words.  The whole strong board of a frame sits in the block's LDS - 8 KiB
// at 256, 128 KiB of the CU's 160 KiB at S = 1024 - with one guard row of zero words above and below; a thread owns
// words tid, tid + 1024, ... (at most 16; exactly one at 256) and keeps their weak bits and their current strong bits in
// registers.  A row's last word holds S - 64 (wpr - 1) valid bits; the bits past the row end are never set in the
// strong or weak sets, so neither the dilation (ANDed with the weak set) nor the fill along the row (inside
// strong | weak) can reach them.  A sweep ORs the three rows around a word, dilates by one column (with the edge bits of
// the neighbouring words), ANDs with the weak set and then floods along the row inside the word (Kogge-Stone occluded
// fill, both directions); a barrier separates a sweep's reads from its writes, and sweeps repeat until no word
// changes.  The fixpoint - weak pixels 8-connected to a strong one - is the set OpenCV's stack-based flood fill reaches,
// whatever the visiting order.  (The byte-map version of this kernel scanned 64 pixels x 9 LDS reads per thread and
// sweep: 480 us per 64 frames, more than the other nine forensic kernels together.)
// edges_out: test tap, the final edge set as one byte (0 / 1) per pixel, written by the TAP = true instantiations only
// (with the store compiled in behind a run-time test of the pointer alone, the 256 kernel measured 36 -> 40 us per 64
// frames with the branch never taken).
constexpr int HYST_MAXW = 16;                               // words per thread at S = 1024: 1024 * 16 / 1024

template <int CS, bool TAP>
__global__ __launch_bounds__(1024) void canny_hyst_kernel(const uint8_t* __restrict__ map, double* __restrict__ count,
                                                          uint8_t* __restrict__ edges_out, int s_arg) {
    extern __shared__ unsigned long long hyst_board[];      // [wpr guards][S * wpr][wpr guards], then 16 doubles
    const int S = edge_of<CS>(s_arg);
    const int tid = threadIdx.x, wpr = (S + 63) >> 6, W = S * wpr, nk = (W + 1023) >> 10;
    unsigned long long* Sw = hyst_board + wpr;
    double* red = reinterpret_cast<double*>(hyst_board + W + 2 * wpr);
    const size_t fo = (size_t)blockIdx.x * S * S;
    unsigned long long wk[HYST_MAXW], nw[HYST_MAXW];        // weak bits and current strong bits of this thread's words
    unsigned long long pk[HYST_MAXW];                       // strong | weak at load (read by the compile-time edge only)
    unsigned has_l = 0, has_r = 0;                          // bit k: word k of this thread has a left / right neighbour word
#pragma unroll
    for (int k = 0; k < HYST_MAXW; ++k) {
        wk[k] = 0ull;
        pk[k] = 0ull;
        nw[k] = 0ull;
        const int wi = tid + 1024 * k;
        if (k < nk && wi < W) {
            const int row = wi / wpr, wd = wi - row * wpr;
            if (wd > 0) has_l |= 1u << k;
            if (wd < wpr - 1) has_r |= 1u << k;
            const int nv = min(64, S - wd * 64) >> 4;       // 16-pixel groups of this word inside the row
            const uint4* src = reinterpret_cast<const uint4*>(map + fo + (size_t)row * S + wd * 64);
            unsigned long long s = 0ull, w = 0ull;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (g < nv) {
                    const uint4 v = src[g];
                    const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const unsigned lab = (wv[qd] >> (8 * b)) & 0xFFu;
                            const int bit = g * 16 + qd * 4 + b;
                            s |= (unsigned long long)(lab == 2u) << bit;
                            w |= (unsigned long long)(lab == 0u) << bit;
                        }
                }
            wk[k] = w;
            pk[k] = s | w;
            nw[k] = s;
            Sw[wi] = s;
        }
    }
    if (tid < wpr) { hyst_board[tid] = 0ull; Sw[W + tid] = 0ull; }
    __syncthreads();
    for (int iter = 0; iter < S * S; ++iter) {              // bounded: each productive sweep adds >= 1 edge
        int changed = 0;
#pragma unroll
        for (int k = 0; k < HYST_MAXW; ++k) {
            const int wi = tid + 1024 * k;
            if (k < nk && wi < W) {
                const unsigned long long s = nw[k];         // = Sw[wi]: nobody else writes this thread's words
                const unsigned long long v = Sw[wi - wpr] | s | Sw[wi + wpr];
                // edge bits of the horizontal neighbour words (rows above / below included); none beyond the row ends
                const unsigned long long vl = (has_l >> k) & 1u ? (Sw[wi - wpr - 1] | Sw[wi - 1] | Sw[wi + wpr - 1]) : 0ull;
                const unsigned long long vr = (has_r >> k) & 1u ? (Sw[wi - wpr + 1] | Sw[wi + 1] | Sw[wi + wpr + 1]) : 0ull;
                const unsigned long long dil = v | (v << 1) | (v >> 1) | (vl >> 63) | (vr << 63);
                // strong | weak never changes: a sweep only moves weak bits into the strong set.  With the one word per
                // thread of the compile-time edge it stays in registers and fill_row's propagate masks leave the sweep
                // loop (30 of its 167 instructions); for 16 words those masks do not fit the register file (1.2 KiB of
                // scratch per lane when tried), so the run-time edge rebuilds it from the current strong bits
                const unsigned long long pass = CS ? pk[k] : s | wk[k];
                nw[k] = fill_row(s | (wk[k] & dil), pass);
                changed |= nw[k] != s;
            }
        }
        const int any = __syncthreads_or(changed);          // also: every read of this sweep is done
#pragma unroll
        for (int k = 0; k < HYST_MAXW; ++k) {
            const int wi = tid + 1024 * k;
            if (k < nk && wi < W) Sw[wi] = nw[k];
        }
        __syncthreads();
        if (!any) break;
    }
    double pop = 0.0;
#pragma unroll
    for (int k = 0; k < HYST_MAXW; ++k) {
        const int wi = tid + 1024 * k;
        if (k < nk && wi < W) {
            const unsigned long long s = nw[k];
            pop += (double)__popcll(s);
            if (TAP) {                                      // one byte (0 / 1) per pixel
                const int row = wi / wpr, wd = wi - row * wpr;
                const int nv = min(64, S - wd * 64) >> 4;
                uint4* dst = reinterpret_cast<uint4*>(edges_out + fo + (size_t)row * S + wd * 64);
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (g < nv) {
                        unsigned wv[4];
#pragma unroll
                        for (int qd = 0; qd < 4; ++qd) {
                            const unsigned nib = (unsigned)(s >> (g * 16 + qd * 4)) & 0xFu;
                            wv[qd] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
                        }
                        dst[g] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
                    }
            }
        }
    }
    const double tot = block_sum<1024>(pop, red);
    if (tid == 0) count[blockIdx.x] = tot;
}

// --------------------------------------------------------------------------------- colour
// one block per image row
template <int CS>
__global__ __launch_bounds__(256) void hsv_stats_kernel(const uint8_t* __restrict__ bgr, double* __restrict__ part,
                                                        unsigned* __restrict__ hue_bits, ColorTables T, int s_arg) {
    __shared__ double red[4 * 4];
    __shared__ unsigned bits[6];
    const int S = edge_of<CS>(s_arg);
    const int tid = threadIdx.x, y = blockIdx.x;
    if (tid < 6) bits[tid] = 0;
    __syncthreads();
    const uint8_t* row = bgr + ((size_t)blockIdx.y * S * S + (size_t)y * S) * 3;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int x = tid; x < S; x += 256) {
        const uint8_t* p = row + x * 3;
        const int b = p[0], g = p[1], r = p[2];
        const int v = max(max(b, g), r), vmin = min(min(b, g), r), diff = v - vmin;
        const int s = (diff * T.hsv_sdiv[v] + (1 << 11)) >> 12;
        int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
        h = (h * T.hsv_hdiv[diff] + (1 << 11)) >> 12;
        if (h < 0) h += 180;
        atomicOr(&bits[h >> 5], 1u << (h & 31));
        acc[0] += (double)s; acc[1] += (double)s * s; acc[2] += (double)v; acc[3] += (double)v * v;
    }
    double* o = part + ((size_t)blockIdx.y * S + y) * 4;
    block_sum_n<256, 4>(acc, red);
    if (tid == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = acc[j];
    __syncthreads();
    if (tid < 6 && bits[tid]) atomicOr(&hue_bits[(size_t)blockIdx.y * 6 + tid], bits[tid]);   // integer OR: order-free
}

// ------------------------------------------------------------------------------- temporal
// one block per image row: part [S]
template <int CS>
__global__ __launch_bounds__(256) void absdiff_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ prev,
                                                      double* __restrict__ part, int s_arg) {
    __shared__ double red[4];
    const int S = edge_of<CS>(s_arg);
    const size_t o = (size_t)blockIdx.x * S;
    double d = 0.0;
    for (int x = threadIdx.x; x < S; x += 256) d += (double)abs((int)gray[o + x] - (int)prev[o + x]);
    const double t = block_sum<256>(d, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// frame-sharded streams on the 256x256 chain: frame f against frame prev_index[f] of the same batch (gray planes
// [n][65536]); prev_index < 0 = no predecessor (partial sums 0).  part: [n][256].
__global__ __launch_bounds__(256) void absdiff_pairs_kernel(const uint8_t* __restrict__ gray, const int* __restrict__ prev_index,
                                                            double* __restrict__ part) {
    __shared__ double red[4];
    const int f = blockIdx.y, pf = prev_index[f];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int d = pf < 0 ? 0 : abs((int)gray[(size_t)f * FPIX + i] - (int)gray[(size_t)pf * FPIX + i]);
    const double t = block_sum<256>((double)d, red);
    if (threadIdx.x == 0) part[(size_t)f * 256 + blockIdx.x] = t;
}

// frames of many streams and analysis edges in one launch: table row blockIdx.y is one frame (its gray plane, the plane
// of its predecessor or null, its edge S and its S partial sums), a wave owns one image row and a lane 16 bytes of it (a
// row is at most EDGE_MAX = 64 x 16 bytes, and a multiple of 16: whole 16-byte loads, none past the row).  The sums are
// integers below 2^18, exact in every order - the same doubles absdiff_kernel writes for the frame.  Null predecessor:
// partial sums 0.
__global__ __launch_bounds__(256) void absdiff_prev_kernel(const DiffRow* __restrict__ rows) {
    const DiffRow r = rows[blockIdx.y];
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= r.S) return;                                       // (wave-uniform)
    unsigned d = 0;
    if (r.prev && 16 * lane < r.S) {
        const size_t o = (size_t)y * r.S + 16 * lane;
        const uint4 a = *reinterpret_cast<const uint4*>(r.gray + o);
        const uint4 b = *reinterpret_cast<const uint4*>(r.prev + o);
        d = __builtin_amdgcn_sad_u8(a.x, b.x, d);
        d = __builtin_amdgcn_sad_u8(a.y, b.y, d);
        d = __builtin_amdgcn_sad_u8(a.z, b.z, d);
        d = __builtin_amdgcn_sad_u8(a.w, b.w, d);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (lane == 0) r.part[y] = (double)d;
}

// one plane of `bytes` (S * S, a multiple of 256) per table entry, 16 bytes per thread
__global__ __launch_bounds__(256) void copy_planes_kernel(const PlaneCopy* __restrict__ copies) {
    const PlaneCopy pc = copies[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i * 16 < pc.bytes) reinterpret_cast<uint4*>(pc.dst)[i] = reinterpret_cast<const uint4*>(pc.src)[i];
}

// ------------------------------------------------------------------------------- finalize
// stats layout per frame (doubles): ForensicStat, forensic_score.h
// One wave per frame: lane l folds partial rows l, l + 64, ... below S (in that order; at 256: l, l + 64, l + 128,
// l + 192), then a butterfly over the lanes - a fixed order, so the sums are run-to-run and batch-size invariant.  Edge
// density and the moments divide by S^2.  (One thread per frame walking all 256 rows was 3,300 dependent L2 round trips:
// 69 us, the longest forensic kernel once the hysteresis was fixed.)
template <int CS>
__global__ __launch_bounds__(64) void stats_finalize_kernel(ForensicBuffers B, int full, int nframes, int s_arg) {
    const int S = edge_of<CS>(s_arg);
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= nframes) return;
    double* st = B.stats + (size_t)f * FORENSIC_STATS;
    double a[7] = {0, 0, 0, 0, 0, 0, 0}, l1 = 0, l2 = 0, s1 = 0, s2 = 0, v1 = 0, v2 = 0;
    for (int row = lane; row < S; row += 64) {
        const size_t r = (size_t)f * S + row;
#pragma unroll
        for (int j = 0; j < 7; ++j) a[j] += B.fft_part[r * 7 + j];
        l1 += B.lap_part[r * 2];
        l2 += B.lap_part[r * 2 + 1];
        if (full) {
            const double* p = B.hsv_part + r * 4;
            s1 += p[0]; s2 += p[1]; v1 += p[2]; v2 += p[3];
        }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[j] += __shfl_xor(a[j], off);
    double* six[6] = {&l1, &l2, &s1, &s2, &v1, &v2};
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) *six[j] += __shfl_xor(*six[j], off);
    if (lane != 0) return;
    const double npix = (double)S * (double)S;
    const double mid_mean = a[2] / a[4];
    st[ST_FREQ_LOW] = a[0] / a[1];
    st[ST_FREQ_MID] = mid_mean;
    st[ST_FREQ_HIGH] = a[5] / a[6];
    const double var = a[3] / a[4] - mid_mean * mid_mean;
    st[ST_FREQ_MID_STD] = sqrt(var > 0 ? var : 0);
    const double lm = l1 / npix;
    st[ST_LAP_VAR] = l2 / npix - lm * lm;
    st[ST_EDGE_COUNT] = B.edge_count[f];
    if (full) {
        const double sm = s1 / npix, vm = v1 / npix;
        const double sv = s2 / npix - sm * sm, vv = v2 / npix - vm * vm;
        st[ST_SAT_STD] = sqrt(sv > 0 ? sv : 0);
        st[ST_VAL_STD] = sqrt(vv > 0 ? vv : 0);
        int hues = 0;
        for (int w = 0; w < 6; ++w) hues += __popc(B.hue_bits[(size_t)f * 6 + w]);
        st[ST_HUES] = hues;
    }
}

// ------------------------------------------------------------------------------- launchers
namespace {

template <int CS, bool TAP>
hipError_t launch_hyst(const ForensicBuffers& B, int S, int n, uint8_t* edges, hipStream_t s) {
    const int wpr = (S + 63) / 64;
    const size_t lds = ((size_t)S * wpr + 2 * wpr) * 8 + 16 * 8;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(canny_hyst_kernel<CS, TAP>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((canny_hyst_kernel<CS, TAP>), dim3(n), dim3(1024), lds, s, B.map, B.edge_count, edges, S);
    return hipSuccess;
}

// the chain with the kernels of one instantiation: CS = 256 with the FFT pair, CS = 0 with the DFT pair
template <int CS>
hipError_t launch_chain(const ForensicBuffers& B, int S, int n, bool full, const ColorTables& T, const float2* table, hipStream_t s,
                        int gray_only, ForensicStart start, const ForensicTaps* taps) {
    const int pix_blocks = S * S / 256, nb = edge_blocks(S);
    if (start == FROM_RS) hipLaunchKernelGGL(gray_kernel<CS>, dim3(pix_blocks, n + gray_only), dim3(256), 0, s, B.rs, B.gray, S);
    if (n <= 0) return hipGetLastError();
    if (start <= FROM_GRAY) {
        float2* spectrum = taps ? taps->spectrum : nullptr;
        float* logmag = taps ? taps->logmag : nullptr;
        if (CS == FS) {
            hipLaunchKernelGGL(fft256_kernel, dim3(FS, n), dim3(128), 0, s, B.gray, B.fft_tmp, table);
            hipLaunchKernelGGL(fft_band_kernel, dim3(FS, n), dim3(128), 0, s, B.fft_tmp, B.fft_part, table, spectrum, logmag);
        } else {
            const size_t tw_bytes = (size_t)S * sizeof(float2);
            hipLaunchKernelGGL(dft_rows_kernel, dim3(S / 16, n), dim3(256), tw_bytes, s, B.gray, B.fft_tmp, table, S);
            hipLaunchKernelGGL(dft_band_kernel, dim3(S / 16, n), dim3(256), tw_bytes, s, B.fft_tmp, B.fft_part, table, S, spectrum, logmag);
        }
        hipLaunchKernelGGL(sobel_lap_kernel<CS>, dim3(S, n), dim3(256), 0, s, B.gray, B.grad, B.lap_part, S);
    }
    if (start <= FROM_GRAD) hipLaunchKernelGGL(canny_nms_kernel<CS>, dim3(pix_blocks, n), dim3(256), 0, s, B.grad, B.map, 50, 150, S);
    const hipError_t eh = taps && taps->edges ? launch_hyst<CS, true>(B, S, n, taps->edges, s) : launch_hyst<CS, false>(B, S, n, nullptr, s);
    if (eh != hipSuccess) return eh;
    if (start >= FROM_GRAD) return hipGetLastError();
    if (full) hipLaunchKernelGGL(noise_block_kernel<CS>, dim3(nb, n), dim3(256), 0, s, B.gray, B.stats_noise, S);
    if (start != FROM_RS) full = false;
    if (full) {
        const int n_y = (S / 8) * (S / 8), n_c = (S / 16) * (S / 16);
        hipLaunchKernelGGL(jpeg_block_kernel<CS>, dim3((n_y + 63) / 64 + (2 * n_c + 63) / 64, n), dim3(64), 0, s, B.rs, B.jy, B.jcb, B.jcr, S);
        hipLaunchKernelGGL(ela_block_kernel<CS>, dim3(nb, n), dim3(256), 0, s, B.rs, B.jy, B.jcb, B.jcr, B.stats_ela, S);
        const hipError_t e = hipMemsetAsync(B.hue_bits, 0, (size_t)n * 6 * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hsv_stats_kernel<CS>, dim3(S, n), dim3(256), 0, s, B.rs, B.hsv_part, B.hue_bits, T, S);
    }
    hipLaunchKernelGGL(stats_finalize_kernel<CS>, dim3(n), dim3(64), 0, s, B, full ? 1 : 0, n, S);
    return hipGetLastError();
}

}  // namespace

// `start` / `taps` are the test entries' (dfd_forensic_tap, dfd_forensic_tap_sized): production callers pass neither.
// From FROM_GRAY on, only the kernels downstream of that buffer run: nothing that reads `rs` (JPEG, ELA, HSV), and no
// statistics from FROM_GRAD on.  Without a frame that gets the signals (n <= 0) only the gray pass of the `gray_only`
// frames runs; without any frame at all nothing is launched.
hipError_t launch_forensics(const ForensicBuffers& B, bool general, int S, int n, bool full, const ColorTables& T, const float2* table,
                            hipStream_t s, int gray_only, ForensicStart start, const ForensicTaps* taps) {
    if (!edge_ok(S) || (!general && S != FS) || n < 0 || gray_only < 0 || n + gray_only <= 0) return hipErrorInvalidValue;
    return general ? launch_chain<0>(B, S, n, full, T, table, s, gray_only, start, taps)
                   : launch_chain<FS>(B, S, n, full, T, table, s, gray_only, start, taps);
}

void launch_absdiff(const uint8_t* gray, const uint8_t* prev, double* part, int S, hipStream_t s) {
    if (S == FS) hipLaunchKernelGGL(absdiff_kernel<FS>, dim3(S), dim3(256), 0, s, gray, prev, part, S);
    else hipLaunchKernelGGL(absdiff_kernel<0>, dim3(S), dim3(256), 0, s, gray, prev, part, S);
}

void launch_absdiff_pairs(const uint8_t* gray, const int* prev_index, double* part, int n, hipStream_t s) {
    hipLaunchKernelGGL(absdiff_pairs_kernel, dim3(256, n), dim3(256), 0, s, gray, prev_index, part);
}

void launch_absdiff_prev(const DiffRow* rows_dev, int n, int max_S, hipStream_t s) {
    hipLaunchKernelGGL(absdiff_prev_kernel, dim3((max_S + 3) / 4, n), dim3(256), 0, s, rows_dev);
}

void launch_copy_planes(const PlaneCopy* copies_dev, int n, int max_S, hipStream_t s) {
    const size_t vecs = (size_t)max_S * max_S / 16;
    hipLaunchKernelGGL(copy_planes_kernel, dim3((unsigned)((vecs + 255) / 256), n), dim3(256), 0, s, copies_dev);
}

void forensic_table(int S, float2* out) {
    for (int j = 0; j < S; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)S;
        out[j] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
}

namespace {
constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

// arrays are frame-major ([n][...]): each kind gets one contiguous region of n * size bytes, carved per call
size_t forensic_bytes_per_frame(int S) {
    const size_t pix = (size_t)S * S, nb = edge_blocks(S);
    const size_t each[] = {pix * 3, pix, pix * sizeof(float2), (size_t)S * 7 * 8, pix * sizeof(short2), (size_t)S * 2 * 8, pix, 8,
                           pix, pix / 4, pix / 4, (size_t)S * 4 * 8, 6 * 4, FORENSIC_STATS * 8, nb * 8, nb * 8};
    size_t total = 0;
    for (size_t e : each) total += al(e);
    return total;
}

void forensic_carve(void* base, int S, int n, ForensicBuffers* o) {
    const size_t pix = (size_t)S * S, nb = edge_blocks(S);
    char* p = static_cast<char*>(base);
    auto take = [&](size_t exact_per_frame) { char* r = p; p += al(exact_per_frame * n); return r; };
    o->rs = (uint8_t*)take(pix * 3);
    o->gray = (uint8_t*)take(pix);
    o->fft_tmp = (float2*)take(pix * sizeof(float2));
    o->fft_part = (double*)take((size_t)S * 7 * 8);
    o->grad = (short2*)take(pix * sizeof(short2));
    o->lap_part = (double*)take((size_t)S * 2 * 8);
    o->map = (uint8_t*)take(pix);
    o->edge_count = (double*)take(8);
    o->jy = (uint8_t*)take(pix);
    o->jcb = (uint8_t*)take(pix / 4);
    o->jcr = (uint8_t*)take(pix / 4);
    o->hsv_part = (double*)take((size_t)S * 4 * 8);
    o->hue_bits = (unsigned*)take(6 * 4);
    o->stats = (double*)take(FORENSIC_STATS * 8);
    o->stats_noise = (double*)take(nb * 8);
    o->stats_ela = (double*)take(nb * 8);
}

}  // namespace dfd

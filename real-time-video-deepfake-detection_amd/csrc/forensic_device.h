// __device__ helpers of the forensic kernels (forensic_kernels.hip) that do not depend on the analysis edge.  Internal to
// that file; all __forceinline__.
#pragma once
#include <hip/hip_runtime.h>

namespace dfd {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// N block-wide sums at once: the same shuffle tree and the same wave-order fold per value as a single block-wide sum (identical bits),
// one barrier pair for all of them instead of one per value (fft_band: 7, hsv_stats: 4, sobel_lap: 2 - the barriers were
// most of what these 256-pixel blocks did after their loads).  Results valid in thread 0.
template <int NT, int N>
__device__ __forceinline__ void block_sum_n(double (&v)[N], double* sh) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[j] += __shfl_xor(v[j], off);
    if ((tid & 63) == 0)
#pragma unroll
        for (int j = 0; j < N; ++j) sh[(tid >> 6) * N + j] = v[j];
    __syncthreads();
    if (tid == 0)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double r = 0.0;
            for (int i = 0; i < NT / 64; ++i) r += sh[i * N + j];
            v[j] = r;
        }
    __syncthreads();
}

// libjpeg quantise + dequantise of one 8x8 block at quality 90, the divisors as compile-time constants (the tables as
// constexpr: after unrolling every `/ dv` is a multiply-shift; with the divisor read from __constant__ memory each of
// the 64 divisions per block was a ~25-instruction sequence - a quarter of the JPEG kernel's instructions)
template <bool CHROMA>
__device__ __forceinline__ void jpeg_quant_q90(int* d) {
    constexpr int L[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                           69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                           81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    constexpr int C[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                           99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
#pragma unroll
    for (int i = 0; i < 64; ++i) {                                // quality 90: scale = 200 - 2*90 = 20
        const int q0 = CHROMA ? C[i] : L[i];
        int qv = (q0 * 20 + 50) / 100;
        qv = qv < 1 ? 1 : (qv > 255 ? 255 : qv);
        const int dv = qv << 3, a = d[i] < 0 ? -d[i] : d[i];
        const int lev = (a + (dv >> 1)) / dv;
        d[i] = (d[i] < 0 ? -lev : lev) * qv;                       // quantise, then dequantise
    }
}

// Kogge-Stone occluded fill of one 64-pixel bitboard word along its row, both directions: the bits of `pro` connected
// to a bit of `gen` (the hysteresis kernels' flood inside a word)
__device__ __forceinline__ unsigned long long fill_row(unsigned long long gen, unsigned long long pro) {
    unsigned long long g = gen, p = pro;                    // towards higher columns
    g |= p & (g << 1);  p &= p << 1;
    g |= p & (g << 2);  p &= p << 2;
    g |= p & (g << 4);  p &= p << 4;
    g |= p & (g << 8);  p &= p << 8;
    g |= p & (g << 16); p &= p << 16;
    g |= p & (g << 32);
    unsigned long long h = gen;                             // towards lower columns
    p = pro;
    h |= p & (h >> 1);  p &= p >> 1;
    h |= p & (h >> 2);  p &= p >> 2;
    h |= p & (h >> 4);  p &= p >> 4;
    h |= p & (h >> 8);  p &= p >> 8;
    h |= p & (h >> 16); p &= p >> 16;
    h |= p & (h >> 32);
    return g | h;
}

}  // namespace dfd

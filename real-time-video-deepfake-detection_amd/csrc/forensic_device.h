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

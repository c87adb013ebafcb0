// Pillow's 8-bit bilinear Image.resize (src/libImaging/Resample.c), shared by the MTCNN face extraction and the train-time
// augmentation chain: the coefficient tables on the host, the fixed-point tap sum of one output element on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

namespace dfd {

// precompute_coeffs + normalize_coeffs_8bpc of Pillow's bilinear filter (src/libImaging/Resample.c)
inline void pil_coeffs(int in_size, int out_size, std::vector<int>* coeff, std::vector<int>* bounds, int* ksize_out) {
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    coeff->assign((size_t)out_size * ksize, 0);
    bounds->assign((size_t)out_size * 2, 0);
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale, ss = 1.0 / fs;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? k[x] / ww : k[x];
            (*coeff)[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
        }
        (*bounds)[2 * xx] = xmin;
        (*bounds)[2 * xx + 1] = xmax;
    }
    *ksize_out = ksize;
}

// one output element of a pass: `cnt` taps `step` bytes apart, coefficients in 22-bit fixed point
__device__ __forceinline__ uint8_t pil_tap_sum(const uint8_t* __restrict__ p, size_t step, const int* __restrict__ kk, int cnt) {
    int ss = 1 << 21;
    for (int k = 0; k < cnt; ++k) ss += kk[k] * (int)p[(size_t)k * step];
    int v = ss >> 22;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace dfd

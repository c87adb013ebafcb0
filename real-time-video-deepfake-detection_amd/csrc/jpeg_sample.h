// libjpeg's sample-domain arithmetic, restated once for the four JPEG paths: the ELA round trip (forensic_kernels.hip,
// reference frame_analysis.py:233-236), the decoder at the HTTP edge (jpeg_decode.hip, reference backend_server.py:139-145),
// the encoder (jpeg_encode.hip) and the training augment's round trip (train_augment.hip).  In pipeline order:
// RGB -> YCbCr (jccolor.c, 16-bit fixed point) and the 8x8 blocks of a 4:2:0 image (jcsample.c h2v2_downsample), the
// jfdctint.c / jidctint.c ("islow") passes, the round trip of a block through a quantiser, fancy upsampling (jdsample.c),
// YCbCr -> RGB (jdcolor.c).  The tables are jpeg_tables.h.  What only one caller meets stays with that caller: chroma
// planes one or two samples wide (decoder), edge replication and h2v1 downsampling (encoder).
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_tables.h"

namespace dfd {

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

#define JFIX(x) ((int)((x) * 65536.0 + 0.5))
__device__ __forceinline__ int ycc_y(int r, int g, int b) { return (JFIX(0.29900) * r + JFIX(0.58700) * g + JFIX(0.11400) * b + 32768) >> 16; }
__device__ __forceinline__ int ycc_cb(int r, int g, int b) { return (-JFIX(0.16874) * r - JFIX(0.33126) * g + JFIX(0.50000) * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int ycc_cr(int r, int g, int b) { return (JFIX(0.50000) * r - JFIX(0.41869) * g - JFIX(0.08131) * b + (128 << 16) + 32767) >> 16; }

// jdcolor.c ycc_rgb_convert; cb, cr without their bias of 128
__device__ __forceinline__ void ycc_to_rgb(int Y, int cb, int cr, int& r, int& g, int& b) {
    r = clamp_u8(Y + ((JFIX(1.40200) * cr + 32768) >> 16));
    g = clamp_u8(Y + ((-JFIX(0.34414) * cb + 32768 - JFIX(0.71414) * cr) >> 16));
    b = clamp_u8(Y + ((JFIX(1.77200) * cb + 32768) >> 16));
}

// The 8x8 block of level-shifted luma samples at (by, bx) of a packed 3-byte image with `pitch` pixels per row; R and B sit
// at bytes ir and ib of a pixel.  The image is whole blocks: no edge replication here.  (The ELA kernel keeps these two
// loops written out, for a measured reason given there.)
__device__ __forceinline__ void jpeg420_luma_block(const uint8_t* img, int pitch, int ir, int ib, int by, int bx, int* d) {
    const uint8_t* org = img + ((size_t)by * pitch + bx) * 3;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const uint8_t* p = org + ((size_t)(i >> 3) * pitch + (i & 7)) * 3;
        d[i] = ycc_y(p[ir], p[1], p[ib]) - 128;
    }
}

// The same of Cb (or Cr) at (by, bx) of the half-size chroma plane: jcsample.c h2v2_downsample of the converted samples
__device__ __forceinline__ void jpeg420_chroma_block(const uint8_t* img, int pitch, int ir, int ib, bool is_cr, int by, int bx, int* d) {
    const uint8_t* org = img + ((size_t)2 * by * pitch + 2 * bx) * 3;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int cx = bx + (i & 7);
        int s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t* p = org + ((size_t)(2 * (i >> 3) + (k >> 1)) * pitch + 2 * (i & 7) + (k & 1)) * 3;
            s += is_cr ? ycc_cr(p[ir], p[1], p[ib]) : ycc_cb(p[ir], p[1], p[ib]);
        }
        d[i] = ((s + ((cx & 1) ? 2 : 1)) >> 2) - 128;          // bias 1,2,1,2,...
    }
}

__host__ __device__ __forceinline__ int dsc(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c one pass over 8 values with stride `st`
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* d, int st) {
    const int t0 = d[0] + d[7 * st], t7 = d[0] - d[7 * st], t1 = d[st] + d[6 * st], t6 = d[st] - d[6 * st];
    const int t2 = d[2 * st] + d[5 * st], t5 = d[2 * st] - d[5 * st], t3 = d[3 * st] + d[4 * st], t4 = d[3 * st] - d[4 * st];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15;
    d[0] = FIRST ? (t10 + t11) << 2 : dsc(t10 + t11, 2);
    d[4 * st] = FIRST ? (t10 - t11) << 2 : dsc(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2 * st] = dsc(z1 + t13 * 6270, n);
    d[6 * st] = dsc(z1 + t12 * (-15137), n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * (-16069) + z5; z4 = z4 * (-3196) + z5;
    d[7 * st] = dsc(a4 + z1 + z3, n);
    d[5 * st] = dsc(a5 + z2 + z4, n);
    d[3 * st] = dsc(a6 + z2 + z3, n);
    d[st] = dsc(a7 + z1 + z4, n);
}

// jidctint.c one pass
template <bool FIRST>
__device__ __forceinline__ void idct8(int* v, int st) {
    int z2 = v[2 * st], z3 = v[6 * st];
    int z1 = (z2 + z3) * 4433;
    int t2 = z1 + z3 * (-15137), t3 = z1 + z2 * 6270;
    int t0 = (v[0] + v[4 * st]) << 13, t1 = (v[0] - v[4 * st]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = v[7 * st]; t1 = v[5 * st]; t2 = v[3 * st]; t3 = v[st];
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * (-16069) + z5; z4 = z4 * (-3196) + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr int n = FIRST ? 11 : 18;
    v[0] = dsc(t10 + t3, n); v[7 * st] = dsc(t10 - t3, n);
    v[st] = dsc(t11 + t2, n); v[6 * st] = dsc(t11 - t2, n);
    v[2 * st] = dsc(t12 + t1, n); v[5 * st] = dsc(t12 - t1, n);
    v[3 * st] = dsc(t13 + t0, n); v[4 * st] = dsc(t13 - t0, n);
}

// One 8x8 block of level-shifted samples through FDCT, quantiser (jcdctmgr.c: the FDCT output is scaled by 8), dequantiser
// and IDCT, to dst.  qv_of(i): entry i of the quantisation table, natural order.  Where it is a constant expression every
// division below becomes a multiply and shift after unrolling; a table read at run time costs ~25 instructions per division.
template <class Q>
__device__ __forceinline__ void jpeg_roundtrip(int* d, Q qv_of, uint8_t* dst, int dstride) {
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct8<true>(d + 8 * r, 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct8<false>(d + c, 8);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int qv = qv_of(i), dv = qv << 3, a = d[i] < 0 ? -d[i] : d[i];
        const int lev = (a + (dv >> 1)) / dv;
        d[i] = (d[i] < 0 ? -lev : lev) * qv;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) idct8<true>(d + c, 8);
#pragma unroll
    for (int r = 0; r < 8; ++r) idct8<false>(d + 8 * r, 1);
#pragma unroll
    for (int i = 0; i < 64; ++i) dst[(size_t)(i >> 3) * dstride + (i & 7)] = (uint8_t)clamp_u8(d[i] + 128);
}

// jdsample.c h2v2_fancy_upsample: the chroma sample for pixel (Y, X) from a plane of cw x ch real samples, row stride cs.
// As in libjpeg, cw > 2: jinit_upsampler replicates a narrower plane, and the caller that can meet one does so
// (jpeg_decode.hip).
__device__ __forceinline__ int fancy_h2v2(const uint8_t* p, int cs, int cw, int ch, int Y, int X) {
    const int i = Y >> 1, c = X >> 1;
    const int nb = (Y & 1) ? (i + 1 < ch ? i + 1 : ch - 1) : (i > 0 ? i - 1 : 0);
    const uint8_t *r0 = p + (size_t)i * cs, *r1 = p + (size_t)nb * cs;
    const int cur = 3 * r0[c] + r1[c];
    if ((X & 1) == 0) {
        if (c == 0) return (4 * cur + 8) >> 4;
        return (3 * cur + (3 * r0[c - 1] + r1[c - 1]) + 8) >> 4;
    }
    if (c == cw - 1) return (4 * cur + 7) >> 4;
    return (3 * cur + (3 * r0[c + 1] + r1[c + 1]) + 7) >> 4;
}

// jdsample.c h2v1_fancy_upsample, cw > 2 likewise
__device__ __forceinline__ int fancy_h2v1(const uint8_t* p, int cs, int cw, int Y, int X) {
    const uint8_t* r = p + (size_t)Y * cs;
    const int c = X >> 1;
    if ((X & 1) == 0) return c == 0 ? r[0] : (3 * r[c] + r[c - 1] + 1) >> 2;
    return c == cw - 1 ? r[c] : (3 * r[c] + r[c + 1] + 2) >> 2;
}


}  // namespace dfd

// Train-time image augmentation on the device (include/dfd_hip.h "train-time image augmentation"): the
// reference's training transform (train.py:462-489, 298-349) as one launch per stage over the whole batch, grid =
// (tiles, images).  A row of `dfd_train_aug_image` per image carries the flags and the parameters the host drew; a block
// of an image that skips a stage returns at once (stage in place) or copies (stage out of place).
//
//   aug_jpeg_block/_color libjpeg 4:2:0 round trip at the row's quality: colour conversion, h2v2 downsampling, islow FDCT,
//                         quantise / dequantise, islow IDCT per 8 x 8 block; fancy upsampling + YCC -> RGB per pixel
//   aug_resize_h / _v     Pillow bilinear Image.resize, 8-bit fixed point (pil_resize.h), to (T+20)^2 or straight to T^2
//   aug_crop              RandomCrop + RandomHorizontalFlip (index arithmetic)
//   aug_lsum, aug_jitter  one ColorJitter slot: Image.blend against black / mean(L) / L, or Pillow's HSV round trip
//   aug_gray              convert("L") on three channels
//   aug_axis, aug_warp_nearest  Pillow AFFINE, NEAREST: affine_fixed (16.16) or, without rotation terms, ImagingScaleAffine
//   aug_perspective       Pillow PERSPECTIVE, BILINEAR, double arithmetic, truncated
//   aug_blur              3 x 3 Gaussian, reflect padding, double accumulation, round half to even
//   aug_norm              ToTensor + Normalize -> planar float32 (IEEE divisions)
//   aug_erase / aug_noise RandomErasing, GaussianNoise + clamp(0, 1) (on the NORMALISED tensor, as the reference does)
//   aug_mix               Mixup / CutMix against the partner image
//   aug_gather            a shuffled batch out of a training set resident in HBM (dfd_train_augment_gather)
//
// Every operation order below restates Pillow's or torch's; the file is built with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "dfd_common.h"
#include "jpeg_sample.h"
#include "pil_resize.h"
#include "train_augment.h"

namespace dfd {
namespace {

typedef dfd_train_aug_image Row;
static_assert(sizeof(Row) == 240, "dfd_train_aug_image layout (train_augment.ROW_DTYPE mirrors it)");
static_assert(sizeof(dfd_train_aug_batch) == 48, "dfd_train_aug_batch layout (train_augment.BATCH_DTYPE mirrors it)");

constexpr int kMargin = 20;        // Resize(T + 20) before RandomCrop(T)
constexpr int kMaxT = 492, kMinT = 12;

// tables of the four resize passes: W -> T+20, H -> T+20, W -> T, H -> T (offsets in ints into the table buffer)
struct ResizeTabs { int coeff[4], bounds[4], ksize[4]; };

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ void copy_image(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int bytes) {
    for (int t = blockIdx.x * 256 + threadIdx.x; t < bytes; t += gridDim.x * 256) d[t] = s[t];
}

// ------------------------------------------------------------------------------------------------ JPEG round trip
// a thread per 8 x 8 block: grid x = the luma blocks of an image in groups of 64, then its Cb and Cr blocks (a wave is all
// luma or all chroma).  planes: per image Y [H][W], Cb [H/2][W/2], Cr [H/2][W/2].  The reference hands its RGB array to an
// encoder that reads BGR: unless DFD_AUG_JPEG_RGB is set the encoder's R is the image's B.
__global__ __launch_bounds__(64) void aug_jpeg_block_kernel(const uint8_t* __restrict__ src, const Row* __restrict__ rows,
                                                            uint8_t* __restrict__ planes, int H, int W) {
    const int img = blockIdx.y;
    const Row& r = rows[img];
    if (!(r.flags & DFD_AUG_JPEG)) return;
    const int quality = r.jpeg_quality, scale = jpeg_quality_scale(quality);
    const int ir = (r.flags & DFD_AUG_JPEG_RGB) ? 0 : 2, ib = 2 - ir;
    const int lw = W >> 3, n_y = lw * (H >> 3), cw = W >> 4, n_c = cw * (H >> 4), gy = (n_y + 63) >> 6, hw = W >> 1;
    const size_t fpix = (size_t)H * W;
    const uint8_t* im = src + (size_t)img * fpix * 3;
    uint8_t* yp = planes + (size_t)img * (fpix + fpix / 2);
    int d[64];
    if ((int)blockIdx.x < gy) {
        const int b = blockIdx.x * 64 + threadIdx.x;
        if (b >= n_y) return;
        const int by = (b / lw) * 8, bx = (b % lw) * 8;
        jpeg420_luma_block(im, W, ir, ib, by, bx, d);
        jpeg_roundtrip(d, [scale](int i) { return jpeg_quant_value(0, i, scale); }, yp + (size_t)by * W + bx, W);
    } else {
        const int b = (blockIdx.x - gy) * 64 + threadIdx.x;
        if (b >= 2 * n_c) return;
        const bool is_cr = b >= n_c;
        const int c = is_cr ? b - n_c : b;
        const int by = (c / cw) * 8, bx = (c % cw) * 8;          // in the H/2 x W/2 chroma plane
        jpeg420_chroma_block(im, W, ir, ib, is_cr, by, bx, d);
        jpeg_roundtrip(d, [scale](int i) { return jpeg_quant_value(1, i, scale); },
                       yp + fpix + (is_cr ? fpix / 4 : 0) + (size_t)by * hw + bx, hw);
    }
}

// decoded planes -> RGB (jdcolor.c); an image without the stage is copied
__global__ __launch_bounds__(256) void aug_jpeg_color_kernel(const uint8_t* __restrict__ src, const Row* __restrict__ rows,
                                                             const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst, int H, int W) {
    const int img = blockIdx.y;
    const size_t fpix = (size_t)H * W;
    const uint8_t* s = src + (size_t)img * fpix * 3;
    uint8_t* d = dst + (size_t)img * fpix * 3;
    if (!(rows[img].flags & DFD_AUG_JPEG)) {
        copy_image(s, d, (int)(fpix * 3));
        return;
    }
    const uint8_t* yp = planes + (size_t)img * (fpix + fpix / 2);
    const uint8_t *cbp = yp + fpix, *crp = cbp + fpix / 4;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < (int)fpix; t += gridDim.x * 256) {
        const int y = t / W, x = t % W;
        const int Yv = yp[t];
        const int hh = H >> 1, hw = W >> 1;                          // W >= 32 (aug_check): fancy_h2v2's cw > 2 holds
        const int cb = fancy_h2v2(cbp, hw, hw, hh, y, x) - 128, cr = fancy_h2v2(crp, hw, hw, hh, y, x) - 128;
        int r, g, b;
        ycc_to_rgb(Yv, cb, cr, r, g, b);
        d[3 * t] = (uint8_t)r;
        d[3 * t + 1] = (uint8_t)g;
        d[3 * t + 2] = (uint8_t)b;
    }
}

// ------------------------------------------------------------------------------------------------ resize, crop
__global__ __launch_bounds__(256) void aug_resize_h_kernel(const uint8_t* __restrict__ src, const Row* __restrict__ rows,
                                                           const int* __restrict__ tables, ResizeTabs tb, uint8_t* __restrict__ tmp,
                                                           int H, int W, int A, int T) {
    const int img = blockIdx.y;
    const bool crop = rows[img].flags & DFD_AUG_CROP;
    const int S = crop ? A : T, k = crop ? 0 : 2;
    const int* coeff = tables + tb.coeff[k];
    const int* bounds = tables + tb.bounds[k];
    const int ks = tb.ksize[k];
    const uint8_t* s = src + (size_t)img * H * W * 3;
    uint8_t* d = tmp + (size_t)img * H * A * 3;
    const int total = H * S * 3;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        const int c = t % 3, col = (t / 3) % S, row = t / 3 / S;
        const int xmin = bounds[2 * col], cnt = bounds[2 * col + 1];
        d[t] = pil_tap_sum(s + ((size_t)row * W + xmin) * 3 + c, 3, coeff + (size_t)col * ks, cnt);
    }
}

__global__ __launch_bounds__(256) void aug_resize_v_kernel(const uint8_t* __restrict__ tmp, const Row* __restrict__ rows,
                                                           const int* __restrict__ tables, ResizeTabs tb, uint8_t* __restrict__ dst,
                                                           int H, int A, int T) {
    const int img = blockIdx.y;
    const bool crop = rows[img].flags & DFD_AUG_CROP;
    const int S = crop ? A : T, k = crop ? 1 : 3;
    const int* coeff = tables + tb.coeff[k];
    const int* bounds = tables + tb.bounds[k];
    const int ks = tb.ksize[k];
    const uint8_t* s = tmp + (size_t)img * H * A * 3;
    uint8_t* d = dst + (size_t)img * A * A * 3;
    const int total = S * S * 3;
    const size_t sstride = (size_t)S * 3;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        const int c = t % 3, col = (t / 3) % S, row = t / 3 / S;
        const int ymin = bounds[2 * row], cnt = bounds[2 * row + 1];
        d[t] = pil_tap_sum(s + (size_t)ymin * sstride + (size_t)col * 3 + c, sstride, coeff + (size_t)row * ks, cnt);
    }
}

__global__ __launch_bounds__(256) void aug_crop_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const Row* __restrict__ rows, int A, int T) {
    const int img = blockIdx.y;
    const Row& r = rows[img];
    const bool crop = r.flags & DFD_AUG_CROP, flip = r.flags & DFD_AUG_FLIP;
    const int S = crop ? A : T, cx = crop ? r.crop_x : 0, cy = crop ? r.crop_y : 0;
    const uint8_t* s = src + (size_t)img * A * A * 3;
    uint8_t* d = dst + (size_t)img * T * T * 3;
    const int total = T * T * 3;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        const int c = t % 3, x = (t / 3) % T, y = t / 3 / T;
        const int sx = cx + (flip ? T - 1 - x : x);
        d[t] = s[((size_t)(cy + y) * S + sx) * 3 + c];
    }
}

// ------------------------------------------------------------------------------------------------ colour
// exact sum of L over an image whose jitter slot `slot` is the contrast op (ImageStat.Stat(convert("L")).mean needs it)
__global__ __launch_bounds__(256) void aug_lsum_kernel(const uint8_t* __restrict__ imgs, const Row* __restrict__ rows,
                                                       unsigned int* __restrict__ sums, int slot, int T) {
    const int img = blockIdx.y;
    if (rows[img].jitter_op[slot] != DFD_JITTER_CONTRAST) return;
    const uint8_t* p = imgs + (size_t)img * T * T * 3;
    unsigned int acc = 0;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T * T; t += gridDim.x * 256) acc += luma(p[3 * t], p[3 * t + 1], p[3 * t + 2]);
    __shared__ unsigned int part[256];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(&sums[img * 4 + slot], part[0]);
}

// Image.blend(degenerate, image, f): float32 d + f (v - d), clamped, truncated
__device__ __forceinline__ uint8_t blend(int d, int v, float f) {
    const float o = (float)d + f * (float)(v - d);
    return o <= 0.f ? 0 : (o >= 255.f ? 255 : (uint8_t)o);
}

// Pillow Convert.c rgb2hsv followed by the uint8 hue shift and hsv2rgb, with the C code's float / double promotions
__device__ __forceinline__ void hue_shift(uint8_t* px, int shift) {
    const int r = px[0], g = px[1], b = px[2];
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
        int ih = (int)((double)h * 255.0), is = (int)((double)s * 255.0);
        uh = ih < 0 ? 0 : (ih > 255 ? 255 : ih);
        us = is < 0 ? 0 : (is > 255 ? 255 : is);
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        px[0] = px[1] = px[2] = (uint8_t)uv;
        return;
    }
    const double hh = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hh);
    const float f = (float)(hh - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double v = (double)(float)uv;
    int p = (int)round(v * (1.0 - (double)fs));
    int q = (int)round(v * (1.0 - (double)(fs * f)));
    int t = (int)round(v * (1.0 - (double)fs * (1.0 - (double)f)));
    p = p < 0 ? 0 : (p > 255 ? 255 : p);
    q = q < 0 ? 0 : (q > 255 ? 255 : q);
    t = t < 0 ? 0 : (t > 255 ? 255 : t);
    int R, G, B;
    switch (i % 6) {
        case 0: R = uv; G = t; B = p; break;
        case 1: R = q; G = uv; B = p; break;
        case 2: R = p; G = uv; B = t; break;
        case 3: R = p; G = q; B = uv; break;
        case 4: R = t; G = p; B = uv; break;
        default: R = uv; G = p; B = q; break;
    }
    px[0] = (uint8_t)R; px[1] = (uint8_t)G; px[2] = (uint8_t)B;
}

__global__ __launch_bounds__(256) void aug_jitter_kernel(uint8_t* __restrict__ imgs, const Row* __restrict__ rows,
                                                         const unsigned int* __restrict__ sums, int slot, int T) {
    const int img = blockIdx.y;
    const int op = rows[img].jitter_op[slot];
    if (op == DFD_JITTER_NONE) return;
    const float f = rows[img].jitter_factor[slot];
    uint8_t* p = imgs + (size_t)img * T * T * 3;
    int mean = 0, shift = 0;
    if (op == DFD_JITTER_CONTRAST) mean = (int)((double)sums[img * 4 + slot] / (double)(T * T) + 0.5);
    if (op == DFD_JITTER_HUE) shift = (int)((double)f * 255.0) & 255;   // numpy: uint8(int32(hue * 255)), the product in double
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T * T; t += gridDim.x * 256) {
        uint8_t px[3] = {p[3 * t], p[3 * t + 1], p[3 * t + 2]};
        if (op == DFD_JITTER_HUE) hue_shift(px, shift);
        else {
            const int d = op == DFD_JITTER_BRIGHTNESS ? 0 : (op == DFD_JITTER_CONTRAST ? mean : luma(px[0], px[1], px[2]));
            px[0] = blend(d, px[0], f); px[1] = blend(d, px[1], f); px[2] = blend(d, px[2], f);
        }
        p[3 * t] = px[0]; p[3 * t + 1] = px[1]; p[3 * t + 2] = px[2];
    }
}

__global__ __launch_bounds__(256) void aug_gray_kernel(uint8_t* __restrict__ imgs, const Row* __restrict__ rows, int T) {
    const int img = blockIdx.y;
    if (!(rows[img].flags & DFD_AUG_GRAY)) return;
    uint8_t* p = imgs + (size_t)img * T * T * 3;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T * T; t += gridDim.x * 256) {
        const uint8_t l = (uint8_t)luma(p[3 * t], p[3 * t + 1], p[3 * t + 2]);
        p[3 * t] = l; p[3 * t + 1] = l; p[3 * t + 2] = l;
    }
}

// ------------------------------------------------------------------------------------------------ warps
__device__ __forceinline__ int fix16(double v) { return (int)floor(v * 65536.0 + 0.5); }
__device__ __forceinline__ int coord(double v) { return v < 0.0 ? -1 : (int)v; }

// ImagingScaleAffine's two coordinate tables of an image, [2][512] ints (-1 = outside): the running sums are sequential
// by definition, so one lane per axis builds them once per image instead of once per block of the warp
__global__ __launch_bounds__(128) void aug_axis_kernel(const Row* __restrict__ rows, int* __restrict__ axes, int which, int T) {
    const int img = blockIdx.x;
    const Row& r = rows[img];
    if (!(r.flags & (which ? DFD_AUG_AFFINE : DFD_AUG_ROTATE))) return;
    const double* m = which ? r.affine : r.rotate;
    if (!(m[1] == 0.0 && m[3] == 0.0) || (threadIdx.x != 0 && threadIdx.x != 64)) return;
    const int axis = threadIdx.x >> 6;
    int* tab = axes + ((size_t)img * 2 + axis) * 512;
    const double step = axis ? m[4] : m[0];
    double o = (axis ? m[5] : m[2]) + step * 0.5;
    for (int k = 0; k < T; ++k) {
        const int c = coord(o);
        tab[k] = c >= 0 && c < T ? c : -1;
        o += step;
    }
}

// Pillow Geometry.c ImagingTransformAffine with NEAREST: a matrix without rotation terms takes ImagingScaleAffine (source
// coordinates accumulated in double along each axis: aug_axis_kernel's tables), any other affine_fixed (16.16 fixed point).
// which: 0 rotate, 1 affine
__global__ __launch_bounds__(256) void aug_warp_nearest_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const Row* __restrict__ rows, const int* __restrict__ axes, int which, int T) {
    const int img = blockIdx.y;
    const Row& r = rows[img];
    const uint8_t* s = src + (size_t)img * T * T * 3;
    uint8_t* d = dst + (size_t)img * T * T * 3;
    if (!(r.flags & (which ? DFD_AUG_AFFINE : DFD_AUG_ROTATE))) {
        copy_image(s, d, T * T * 3);
        return;
    }
    const double* m = which ? r.affine : r.rotate;
    const bool scale_only = m[1] == 0.0 && m[3] == 0.0;
    const int* xtab = axes + (size_t)img * 1024;
    const int* ytab = xtab + 512;
    const int a0 = fix16(m[0]), a1 = fix16(m[1]), a3 = fix16(m[3]), a4 = fix16(m[4]);
    const int a2 = fix16(m[2] + m[0] * 0.5 + m[1] * 0.5), a5 = fix16(m[5] + m[3] * 0.5 + m[4] * 0.5);
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T * T; t += gridDim.x * 256) {
        const int x = t % T, y = t / T;
        int xi, yi;
        if (scale_only) {
            xi = xtab[x];
            yi = ytab[y];
        } else {
            // the C loop adds a0 / a3 per column and a1 / a4 per row in int: the same value mod 2^32
            xi = (int)((unsigned)a2 + (unsigned)x * (unsigned)a0 + (unsigned)y * (unsigned)a1) >> 16;
            yi = (int)((unsigned)a5 + (unsigned)x * (unsigned)a3 + (unsigned)y * (unsigned)a4) >> 16;
        }
        uint8_t o0 = 0, o1 = 0, o2 = 0;
        if (xi >= 0 && xi < T && yi >= 0 && yi < T) {
            const uint8_t* q = s + ((size_t)yi * T + xi) * 3;
            o0 = q[0]; o1 = q[1]; o2 = q[2];
        }
        d[3 * t] = o0; d[3 * t + 1] = o1; d[3 * t + 2] = o2;
    }
}

// Pillow perspective_transform + bilinear_filter32RGB: per-pixel double division, result truncated to uint8
__global__ __launch_bounds__(256) void aug_perspective_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const Row* __restrict__ rows, int T) {
    const int img = blockIdx.y;
    const Row& r = rows[img];
    const uint8_t* s = src + (size_t)img * T * T * 3;
    uint8_t* d = dst + (size_t)img * T * T * 3;
    if (!(r.flags & DFD_AUG_PERSPECTIVE)) {
        copy_image(s, d, T * T * 3);
        return;
    }
    const double c0 = r.perspective[0], c1 = r.perspective[1], c2 = r.perspective[2], c3 = r.perspective[3],
                 c4 = r.perspective[4], c5 = r.perspective[5], c6 = r.perspective[6], c7 = r.perspective[7];
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T * T; t += gridDim.x * 256) {
        const double xs = (double)(t % T) + 0.5, ys = (double)(t / T) + 0.5;
        const double den = c6 * xs + c7 * ys + 1.0;
        double xin = (c0 * xs + c1 * ys + c2) / den, yin = (c3 * xs + c4 * ys + c5) / den;
        uint8_t o[3] = {0, 0, 0};
        if (!(xin < 0.0 || xin >= (double)T || yin < 0.0 || yin >= (double)T)) {
            xin -= 0.5;
            yin -= 0.5;
            const int x = (int)floor(xin), y = (int)floor(yin);
            const double dx = xin - (double)x, dy = yin - (double)y;
            const int x0 = min(max(x, 0), T - 1), x1 = min(max(x + 1, 0), T - 1), y0 = min(max(y, 0), T - 1);
            const uint8_t* ra = s + (size_t)y0 * T * 3;
            const bool two = y + 1 >= 0 && y + 1 < T;
            const uint8_t* rb = s + (size_t)(two ? y + 1 : y0) * T * 3;
            for (int c = 0; c < 3; ++c) {
                const double a = (double)ra[x0 * 3 + c], b = (double)ra[x1 * 3 + c];
                const double v1 = a + (b - a) * dx;
                double v2 = v1;
                if (two) {
                    const double e = (double)rb[x0 * 3 + c], g = (double)rb[x1 * 3 + c];
                    v2 = e + (g - e) * dx;
                }
                o[c] = (uint8_t)(int)(v1 + (v2 - v1) * dy);
            }
        }
        d[3 * t] = o[0]; d[3 * t + 1] = o[1]; d[3 * t + 2] = o[2];
    }
}

// GaussianBlur(3): reflect padding, k2[i][j] = float32(k1[i] k1[j]), double accumulation in row-major tap order
__global__ __launch_bounds__(256) void aug_blur_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const Row* __restrict__ rows, int T) {
    const int img = blockIdx.y;
    const Row& r = rows[img];
    const uint8_t* s = src + (size_t)img * T * T * 3;
    uint8_t* d = dst + (size_t)img * T * T * 3;
    if (!(r.flags & DFD_AUG_BLUR)) {
        copy_image(s, d, T * T * 3);
        return;
    }
    const float k1[3] = {r.blur_k[0], r.blur_k[1], r.blur_k[0]};
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T * T * 3; t += gridDim.x * 256) {
        const int c = t % 3, x = (t / 3) % T, y = t / 3 / T;
        double acc = 0.0;
        for (int i = 0; i < 3; ++i) {
            int yy = y + i - 1;
            yy = yy < 0 ? -yy : (yy >= T ? 2 * T - 2 - yy : yy);
            for (int j = 0; j < 3; ++j) {
                int xx = x + j - 1;
                xx = xx < 0 ? -xx : (xx >= T ? 2 * T - 2 - xx : xx);
                const float k2 = k1[i] * k1[j];
                acc += (double)k2 * (double)s[((size_t)yy * T + xx) * 3 + c];
            }
        }
        const double v = rint(acc);
        d[t] = (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
    }
}

// ------------------------------------------------------------------------------------------------ tensor stages
__global__ __launch_bounds__(256) void aug_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int T) {
    const int img = blockIdx.y;
    const uint8_t* s = src + (size_t)img * T * T * 3;
    float* d = dst + (size_t)img * T * T * 3;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const int hw = T * T;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < 3 * hw; t += gridDim.x * 256) {
        const int c = t / hw, p = t % hw;
        const float v = (float)s[(size_t)p * 3 + c] / 255.0f;
        d[t] = (v - mean[c]) / sd[c];
    }
}

__global__ __launch_bounds__(256) void aug_erase_kernel(float* __restrict__ x, const Row* __restrict__ rows, int T) {
    const int img = blockIdx.y;
    const Row& r = rows[img];
    if (!(r.flags & DFD_AUG_ERASE)) return;
    const int ex = r.erase[0], ey = r.erase[1], ew = r.erase[2], eh = r.erase[3];
    float* d = x + (size_t)img * T * T * 3;
    const int total = 3 * ew * eh;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        const int c = t / (ew * eh), yy = (t / ew) % eh, xx = t % ew;
        d[(size_t)c * T * T + (size_t)(ey + yy) * T + ex + xx] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void aug_noise_kernel(float* __restrict__ x, const Row* __restrict__ rows,
                                                        unsigned long long seed, unsigned long long counter, int T) {
    const int img = blockIdx.y;
    const Row& r = rows[img];
    if (!(r.flags & DFD_AUG_NOISE)) return;
    const uint32_t key = aug_noise_key(seed, counter, img);
    const float sd = r.noise_std;
    float* d = x + (size_t)img * T * T * 3;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < 3 * T * T; t += gridDim.x * 256) {
        const uint32_t u1 = aug_noise_word(key, 2u * (uint32_t)t), u2 = aug_noise_word(key, 2u * (uint32_t)t + 1u);
        const float a = (float)((u1 >> 8) + 1u) * 5.9604644775390625e-8f;      // (0, 1], exact
        const float b = (float)(u2 >> 8) * 5.9604644775390625e-8f;             // [0, 1), exact
        const float z = sqrtf(-2.0f * logf(a)) * cosf(6.2831855f * b);
        const float v = d[t] + sd * z;
        d[t] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
}

// images [first, first + count) of the batch against their partners (any image of the batch) -> dst [count][3][T][T]
__global__ __launch_bounds__(256) void aug_mix_kernel(const float* __restrict__ x, float* __restrict__ dst, const int* __restrict__ perm,
                                                      int first, int kind, float lam, int bx1, int by1, int bx2, int by2, int T) {
    const int img = first + blockIdx.y;
    const size_t per = (size_t)3 * T * T;
    const float* a = x + (size_t)img * per;
    const float* b = x + (size_t)perm[img] * per;
    float* d = dst + (size_t)blockIdx.y * per;
    const float one_minus = 1.0f - lam;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < (int)per; t += gridDim.x * 256) {
        float v;
        if (kind == DFD_MIX_MIXUP) v = lam * a[t] + one_minus * b[t];
        else {
            const int xx = t % T, yy = (t / T) % T;
            v = (xx >= bx1 && xx < bx2 && yy >= by1 && yy < by2) ? b[t] : a[t];
        }
        d[t] = v;
    }
}

// crops idx[0 .. n) of a resident set -> a contiguous batch (fit_loop's shuffled batch of a training set kept in HBM)
__global__ __launch_bounds__(256) void aug_gather_kernel(const uint8_t* __restrict__ src, const int* __restrict__ idx,
                                                         uint8_t* __restrict__ dst, size_t crop_bytes) {
    const uint4* s = (const uint4*)(src + (size_t)idx[blockIdx.y] * crop_bytes);      // crop_bytes = 768 k: 16-byte units
    uint4* d = (uint4*)(dst + (size_t)blockIdx.y * crop_bytes);
    const size_t units = crop_bytes / 16;
    for (size_t t = blockIdx.x * 256 + threadIdx.x; t < units; t += (size_t)gridDim.x * 256) d[t] = s[t];
}

// ------------------------------------------------------------------------------------------------ host
const char* const kU8Stages[] = {"crop", "jitter0", "jitter1", "jitter2", "jitter3", "gray", "rotate", "affine", "perspective", "blur"};
const char* const kF32Stages[] = {"norm", "erase", "noise", "mix"};

bool known_stage(const char* s) {
    if (!strcmp(s, "resize") || !strcmp(s, "jpeg")) return true;
    for (const char* k : kU8Stages)
        if (!strcmp(s, k)) return true;
    for (const char* k : kF32Stages)
        if (!strcmp(s, k)) return true;
    return false;
}

int aug_check(dfd_handle* h, const void* rgb, int n, int H, int W, int T, const Row* rows, const dfd_train_aug_batch* batch) {
    if (!rgb || !rows || !batch) return fail(h, DFD_ERR_ARG, "train_augment: null pointer");
    if (n < 1) return fail(h, DFD_ERR_ARG, "train_augment: n = %d", n);
    if (H % 16 || W % 16 || H < 32 || W < 32 || H > 512 || W > 512)
        return fail(h, DFD_ERR_ARG, "train_augment: source %d x %d is not a multiple of 16 in 32..512", H, W);
    if (T < kMinT || T > kMaxT) return fail(h, DFD_ERR_ARG, "train_augment: out_size %d outside %d..%d", T, kMinT, kMaxT);
    if ((size_t)n * 3 * (T + kMargin) * std::max(T + kMargin, H) > ((size_t)1 << 31))
        return fail(h, DFD_ERR_CAPACITY, "train_augment: %d images of this size exceed the work memory of one call", n);
    for (int i = 0; i < n; ++i) {
        const Row& r = rows[i];
        if ((r.flags & DFD_AUG_JPEG) && (r.jpeg_quality < 1 || r.jpeg_quality > 100))
            return fail(h, DFD_ERR_ARG, "train_augment: JPEG quality %d of row %d outside 1..100", r.jpeg_quality, i);
        if ((r.flags & DFD_AUG_CROP) && (r.crop_x < 0 || r.crop_y < 0 || r.crop_x > kMargin || r.crop_y > kMargin))
            return fail(h, DFD_ERR_ARG, "train_augment: crop offset (%d, %d) of row %d outside 0..%d", r.crop_x, r.crop_y, i, kMargin);
        for (int k = 0; k < 4; ++k)
            if (r.jitter_op[k] < DFD_JITTER_NONE || r.jitter_op[k] > DFD_JITTER_HUE)
                return fail(h, DFD_ERR_ARG, "train_augment: jitter op %d of row %d", r.jitter_op[k], i);
        if (r.flags & DFD_AUG_ERASE) {
            const int* e = r.erase;
            if (e[0] < 0 || e[1] < 0 || e[2] < 0 || e[3] < 0 || e[0] > T || e[1] > T || e[2] > T - e[0] || e[3] > T - e[1])   // no sum: it could wrap
                return fail(h, DFD_ERR_ARG, "train_augment: erase box of row %d outside the image", i);
        }
    }
    if (batch->mix_kind < DFD_MIX_NONE || batch->mix_kind > DFD_MIX_CUTMIX) return fail(h, DFD_ERR_ARG, "train_augment: mix kind %d", batch->mix_kind);
    if (batch->mix_kind != DFD_MIX_NONE) {
        if (!batch->perm) return fail(h, DFD_ERR_ARG, "train_augment: mix without a partner permutation");
        for (int i = 0; i < n; ++i)
            if (batch->perm[i] < 0 || batch->perm[i] >= n) return fail(h, DFD_ERR_ARG, "train_augment: partner %d of image %d outside 0..%d", batch->perm[i], i, n - 1);
        const int* b = batch->box;
        if (batch->mix_kind == DFD_MIX_CUTMIX && (b[0] < 0 || b[1] < 0 || b[2] < b[0] || b[3] < b[1] || b[2] > T || b[3] > T))
            return fail(h, DFD_ERR_ARG, "train_augment: CutMix box outside the image");
    }
    return DFD_OK;
}

struct AugOut {                 // what a run leaves on the device
    float* x = nullptr;         // [n][3][T][T] after the noise stage
    const int* perm = nullptr;  // device copy of the partners (mix_kind != none)
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// the chain through the noise stage; `tap` (or null): copy the named stage's images to tap_out and stop there (*tapped)
int aug_run(dfd_handle* h, const uint8_t* rgb, int on_device, int n, int H, int W, int T, const Row* rows,
            const dfd_train_aug_batch* batch, const char* tap, void* tap_out, size_t tap_cap, bool* tapped, AugOut* out,
            bool room_for_mix = false) {
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const int A = T + kMargin;
    hipStream_t s = h->stream;
    // tables: rows, resize coefficients, luma sums, partners
    std::vector<int> tab;
    ResizeTabs tb;
    const int ins[4] = {W, H, W, H}, outs[4] = {A, A, T, T};
    for (int k = 0; k < 4; ++k) {
        std::vector<int> coeff, bounds;
        pil_coeffs(ins[k], outs[k], &coeff, &bounds, &tb.ksize[k]);
        tb.coeff[k] = (int)tab.size();
        tab.insert(tab.end(), coeff.begin(), coeff.end());
        tb.bounds[k] = (int)tab.size();
        tab.insert(tab.end(), bounds.begin(), bounds.end());
    }
    const size_t rows_bytes = align16((size_t)n * sizeof(Row)), tab_bytes = align16(tab.size() * 4), sum_bytes = align16((size_t)n * 16),
                 perm_bytes = align16((size_t)n * 4), axis_bytes = (size_t)n * 1024 * 4;
    const size_t src_bytes = on_device ? 0 : align16((size_t)n * H * W * 3);
    const size_t region = align16((size_t)n * 3 * A * std::max(A, H));
    bool any_jpeg = false;
    for (int i = 0; i < n; ++i) any_jpeg = any_jpeg || (rows[i].flags & DFD_AUG_JPEG);
    // decoded images + the Y / Cb / Cr planes of the round trip, only when a row asks for it
    const size_t jpeg_bytes = any_jpeg ? align16((size_t)n * H * W * 3) : 0, plane_bytes = any_jpeg ? align16((size_t)n * H * W * 3 / 2) : 0;
    const size_t per_f = (size_t)n * 3 * T * T;
    int rc = ensure(h, &h->aug_tab, rows_bytes + tab_bytes + sum_bytes + perm_bytes + axis_bytes);
    if (!rc) rc = ensure(h, &h->aug_u8, src_bytes + jpeg_bytes + plane_bytes + 2 * region);
    if (!rc) rc = ensure(h, &h->aug_f32, per_f * 4 * (room_for_mix ? 2 : 1));
    if (rc) return rc;
    char* tbase = (char*)h->aug_tab.p;
    Row* rows_dev = (Row*)tbase;
    int* tab_dev = (int*)(tbase + rows_bytes);
    unsigned int* sums = (unsigned int*)(tbase + rows_bytes + tab_bytes);
    int* perm_dev = (int*)(tbase + rows_bytes + tab_bytes + sum_bytes);
    int* axes = (int*)(tbase + rows_bytes + tab_bytes + sum_bytes + perm_bytes);
    // the small tables go through the pinned mailbox: copied out of the caller's memory before this returns
    rc = mailbox_h2d(h, rows_dev, rows, (size_t)n * sizeof(Row));
    if (!rc) rc = mailbox_h2d(h, tab_dev, tab.data(), tab.size() * 4);
    if (!rc && batch->mix_kind != DFD_MIX_NONE) rc = mailbox_h2d(h, perm_dev, batch->perm, (size_t)n * 4);
    if (rc) return rc;
    DFD_HIP_TRY(h, hipMemsetAsync(sums, 0, (size_t)n * 16, s));
    uint8_t* ubase = (uint8_t*)h->aug_u8.p;
    const uint8_t* src = rgb;
    if (!on_device) {
        DFD_HIP_TRY(h, hipMemcpyAsync(ubase, rgb, (size_t)n * H * W * 3, hipMemcpyHostToDevice, s));
        src = ubase;
    }
    uint8_t* cur = ubase + src_bytes + jpeg_bytes + plane_bytes;
    uint8_t* oth = cur + region;
    float* x = (float*)h->aug_f32.p;
    *tapped = false;
    // a tap: the stage's images to the host, then the call is over
    auto tap_here = [&](const char* name, const void* p, size_t bytes) -> int {
        if (!tap || strcmp(tap, name)) return 0;
        if (bytes > tap_cap) return fail(h, DFD_ERR_ARG, "train_augment_tap: stage '%s' needs %zu bytes, capacity %zu", name, bytes, tap_cap);
        DFD_HIP_TRY(h, hipGetLastError());
        DFD_HIP_TRY(h, hipMemcpyAsync(tap_out, p, bytes, hipMemcpyDeviceToHost, s));
        DFD_HIP_TRY(h, stream_sync(h));
        *tapped = true;
        return 1;
    };
#define AUG_TAP(name, p, bytes)                    \
    do {                                           \
        const int _t = tap_here(name, p, bytes);   \
        if (_t < 0) return _t;                     \
        if (_t > 0) return DFD_OK;                 \
    } while (0)
    const auto tiles = [](long long elems) { return (unsigned)std::min<long long>((elems + 255) / 256, 128); };
    const dim3 blk(256);
    const size_t img_bytes = (size_t)n * T * T * 3;
    if (any_jpeg) {
        uint8_t* decoded = ubase + src_bytes;
        uint8_t* planes = decoded + jpeg_bytes;
        const int n_y = (H >> 3) * (W >> 3), n_c = (H >> 4) * (W >> 4);
        hipLaunchKernelGGL(aug_jpeg_block_kernel, dim3((n_y + 63) / 64 + (2 * n_c + 63) / 64, n), dim3(64), 0, s, src, rows_dev, planes, H, W);
        hipLaunchKernelGGL(aug_jpeg_color_kernel, dim3(tiles((long long)H * W), n), blk, 0, s, src, rows_dev, planes, decoded, H, W);
        src = decoded;
    }
    AUG_TAP("jpeg", src, (size_t)n * H * W * 3);
    hipLaunchKernelGGL(aug_resize_h_kernel, dim3(tiles((long long)H * A * 3), n), blk, 0, s, src, rows_dev, tab_dev, tb, oth, H, W, A, T);
    hipLaunchKernelGGL(aug_resize_v_kernel, dim3(tiles((long long)A * A * 3), n), blk, 0, s, oth, rows_dev, tab_dev, tb, cur, H, A, T);
    AUG_TAP("resize", cur, (size_t)n * A * A * 3);
    hipLaunchKernelGGL(aug_crop_kernel, dim3(tiles((long long)T * T * 3), n), blk, 0, s, cur, oth, rows_dev, A, T);
    std::swap(cur, oth);
    AUG_TAP("crop", cur, img_bytes);
    const dim3 gpix(tiles((long long)T * T), n), gelem(tiles((long long)T * T * 3), n);
    for (int k = 0; k < 4; ++k) {
        hipLaunchKernelGGL(aug_lsum_kernel, gpix, blk, 0, s, cur, rows_dev, sums, k, T);
        hipLaunchKernelGGL(aug_jitter_kernel, gpix, blk, 0, s, cur, rows_dev, sums, k, T);
        AUG_TAP(kU8Stages[1 + k], cur, img_bytes);
    }
    hipLaunchKernelGGL(aug_gray_kernel, gpix, blk, 0, s, cur, rows_dev, T);
    AUG_TAP("gray", cur, img_bytes);
    for (int which = 0; which < 2; ++which) {
        hipLaunchKernelGGL(aug_axis_kernel, dim3(n), dim3(128), 0, s, rows_dev, axes, which, T);
        hipLaunchKernelGGL(aug_warp_nearest_kernel, gpix, blk, 0, s, cur, oth, rows_dev, axes, which, T);
        std::swap(cur, oth);
        AUG_TAP(which ? "affine" : "rotate", cur, img_bytes);
    }
    hipLaunchKernelGGL(aug_perspective_kernel, gpix, blk, 0, s, cur, oth, rows_dev, T);
    std::swap(cur, oth);
    AUG_TAP("perspective", cur, img_bytes);
    hipLaunchKernelGGL(aug_blur_kernel, gelem, blk, 0, s, cur, oth, rows_dev, T);
    std::swap(cur, oth);
    AUG_TAP("blur", cur, img_bytes);
    hipLaunchKernelGGL(aug_norm_kernel, gelem, blk, 0, s, cur, x, T);
    AUG_TAP("norm", x, per_f * 4);
    hipLaunchKernelGGL(aug_erase_kernel, gelem, blk, 0, s, x, rows_dev, T);
    AUG_TAP("erase", x, per_f * 4);
    hipLaunchKernelGGL(aug_noise_kernel, gelem, blk, 0, s, x, rows_dev, batch->seed, batch->counter, T);
    AUG_TAP("noise", x, per_f * 4);
#undef AUG_TAP
    DFD_HIP_TRY(h, hipGetLastError());
    out->x = x;
    out->perm = perm_dev;
    return DFD_OK;
}

void launch_mix(dfd_handle* h, const AugOut& o, const dfd_train_aug_batch* b, int first, int count, int T, float* dst) {
    const unsigned tiles = (unsigned)std::min<long long>(((long long)3 * T * T + 255) / 256, 128);
    hipLaunchKernelGGL(aug_mix_kernel, dim3(tiles, count), dim3(256), 0, h->stream, o.x, dst, o.perm, first, b->mix_kind, b->lam,
                       b->box[0], b->box[1], b->box[2], b->box[3], T);
}

// the chain with the mix -> host (out_host) or the tap
int aug_to_host(dfd_handle* h, const uint8_t* rgb, int n, int H, int W, int T, const Row* rows, const dfd_train_aug_batch* batch,
                const char* tap, void* out_host, size_t cap) {
    int rc = aug_check(h, rgb, n, H, W, T, rows, batch);
    if (rc) return rc;
    if (!out_host) return fail(h, DFD_ERR_ARG, "train_augment: null pointer");
    const size_t bytes = (size_t)n * 3 * T * T * 4;
    if (tap && !known_stage(tap)) return fail(h, DFD_ERR_ARG, "train_augment_tap: unknown stage '%s'", tap);
    if (tap && !strcmp(tap, "mix") && bytes > cap) return fail(h, DFD_ERR_ARG, "train_augment_tap: stage 'mix' needs %zu bytes, capacity %zu", bytes, cap);
    bool tapped = false;
    AugOut o;
    const bool mix_tap = tap && !strcmp(tap, "mix");
    // the mixed batch goes beside the unmixed one: partners are read from any image of the batch
    rc = aug_run(h, rgb, 0, n, H, W, T, rows, batch, mix_tap ? nullptr : tap, out_host, cap, &tapped, &o, batch->mix_kind != DFD_MIX_NONE);
    if (rc || tapped) return rc;
    const float* result = o.x;
    if (batch->mix_kind != DFD_MIX_NONE) {
        float* mixed = o.x + (size_t)n * 3 * T * T;
        launch_mix(h, o, batch, 0, n, T, mixed);
        result = mixed;
    }
    DFD_HIP_TRY(h, hipMemcpyAsync(out_host, result, bytes, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

}  // namespace
}  // namespace dfd

using namespace dfd;

extern "C" {

int dfd_train_augment(dfd_handle* h, const unsigned char* rgb_host, int n, int H, int W, int out_size,
                      const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, float* nchw_out_host) {
    if (!h) return DFD_ERR_ARG;
    return aug_to_host(h, rgb_host, n, H, W, out_size, rows, batch, nullptr, nchw_out_host, 0);
}

int dfd_train_augment_gather(dfd_handle* h, const unsigned char* rgb_dev, int n_src, int H, int W, const int* idx, int n,
                             unsigned char* out_dev) {
    if (!h) return DFD_ERR_ARG;
    if (!rgb_dev || !idx || !out_dev) return fail(h, DFD_ERR_ARG, "train_augment_gather: null pointer");
    if (n < 1 || n_src < 1) return fail(h, DFD_ERR_ARG, "train_augment_gather: n = %d of %d", n, n_src);
    if (H % 16 || W % 16 || H < 32 || W < 32 || H > 512 || W > 512)
        return fail(h, DFD_ERR_ARG, "train_augment_gather: source %d x %d is not a multiple of 16 in 32..512", H, W);
    if (((uintptr_t)rgb_dev | (uintptr_t)out_dev) & 15) return fail(h, DFD_ERR_ARG, "train_augment_gather: buffers must be 16-byte aligned");
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= n_src) return fail(h, DFD_ERR_ARG, "train_augment_gather: index %d of entry %d outside 0..%d", idx[i], i, n_src - 1);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure(h, &h->aug_idx, (size_t)n * 4);
    if (!rc) rc = mailbox_h2d(h, h->aug_idx.p, idx, (size_t)n * 4);
    if (rc) return rc;
    const size_t crop_bytes = (size_t)H * W * 3;                       // H, W multiples of 16: a multiple of 768
    const unsigned tiles = (unsigned)std::min<size_t>((crop_bytes / 16 + 255) / 256, 64);
    hipLaunchKernelGGL(aug_gather_kernel, dim3(tiles, n), dim3(256), 0, h->stream, rgb_dev, (const int*)h->aug_idx.p, out_dev, crop_bytes);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

int dfd_train_augment_noise_words(unsigned long long seed, unsigned long long counter, int row, unsigned int first,
                                  unsigned int count, unsigned int* u1_out, unsigned int* u2_out) {
    if (!u1_out || !u2_out || row < 0) return DFD_ERR_ARG;
    const uint32_t key = aug_noise_key(seed, counter, row);
    for (unsigned int i = 0; i < count; ++i) {
        const uint32_t e = first + i;
        u1_out[i] = aug_noise_word(key, 2u * e);
        u2_out[i] = aug_noise_word(key, 2u * e + 1u);
    }
    return DFD_OK;
}

int dfd_train_augment_tap(dfd_handle* h, const unsigned char* rgb_host, int n, int H, int W, int out_size,
                          const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, const char* stage_name,
                          void* out, size_t capacity) {
    if (!h) return DFD_ERR_ARG;
    if (!stage_name) return fail(h, DFD_ERR_ARG, "train_augment_tap: null pointer");
    return aug_to_host(h, rgb_host, n, H, W, out_size, rows, batch, stage_name, out, capacity);
}

// the chain at 224 on all n images, then the backbone in chunks of max_batch: pooled rows, or (trunk) block 15's output, or
// (trunk, block = 14) block 14's, or (first_block = 13: dfd_train_augment_block_out) block 13's, or (first_block = 11:
// dfd_train_augment_block_input, which checks its own range) block 11's or 12's, or (first_block = 10:
// dfd_train_augment_block_rows, likewise) block 10's, [14][14][112] a crop
static int augment_forward(dfd_handle* h, const char* who, const unsigned char* rgb, int on_device, int n, int H, int W,
                           const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, float* out_host, bool trunk,
                           int block = 15, int first_block = 14) {
    if (!h) return DFD_ERR_ARG;
    if (block < first_block || block > 15)
        return fail(h, DFD_ERR_ARG, first_block == 13 ? "%s: block %d; 13, 14 or 15" : "%s: block %d; 14 or 15", who, block);
    int rc = aug_check(h, rgb, n, H, W, DFD_CROP, rows, batch);
    if (rc) return rc;
    if (!out_host) return fail(h, DFD_ERR_ARG, "%s: null pointer", who);
    bool tapped = false;
    AugOut o;
    // partners of Mixup / CutMix may sit in another chunk: the chain runs on all n images before the first forward
    rc = aug_run(h, rgb, on_device ? 1 : 0, n, H, W, DFD_CROP, rows, batch, nullptr, nullptr, 0, &tapped, &o);
    if (rc) return rc;
    const size_t per = (size_t)3 * DFD_CROP * DFD_CROP;
    for (int first = 0; first < n; first += h->max_batch) {
        const int m = std::min(h->max_batch, n - first);
        const float* in = o.x + (size_t)first * per;
        if (batch->mix_kind != DFD_MIX_NONE) {
            launch_mix(h, o, batch, first, m, DFD_CROP, h->in_nchw);
            in = h->in_nchw;
        }
        if (trunk) {
            const size_t row = block == 15 ? DFD_TRUNK_ROW : block == 10 ? DFD_BLOCK11_INPUT_ROW : DFD_BLOCK14_ROW;
            if ((rc = b0_trunk_to_host(h, in, m, out_host + (size_t)first * row, block))) return rc;
            continue;
        }
        rc = b0_forward(h, in, m, nullptr, nullptr, nullptr);
        if (rc) return rc;
        DFD_HIP_TRY(h, hipMemcpyAsync(out_host + (size_t)first * DFD_FEATURES, h->feat, (size_t)m * DFD_FEATURES * 4,
                                      hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_train_augment_features(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                               const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, float* feat_out_host) {
    return augment_forward(h, "train_augment_features", rgb, on_device, n, H, W, rows, batch, feat_out_host, false);
}

int dfd_train_augment_trunk(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                            const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, float* trunk_out_host) {
    return augment_forward(h, "train_augment_trunk", rgb, on_device, n, H, W, rows, batch, trunk_out_host, true);
}

int dfd_train_augment_trunk_at(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                               const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host) {
    return augment_forward(h, "train_augment_trunk_at", rgb, on_device, n, H, W, rows, batch, out_host, true, block);
}

int dfd_train_augment_block_out(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                                const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host) {
    return augment_forward(h, "train_augment_block_out", rgb, on_device, n, H, W, rows, batch, out_host, true, block, 13);
}

int dfd_train_augment_block_input(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                                  const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host) {
    if (!h) return DFD_ERR_ARG;
    if (block < 12 || block > 15) return fail(h, DFD_ERR_ARG, "train_augment_block_input: block %d; 12, 13, 14 or 15", block);
    // a block's input is the output of the block below it: [7][7][192] for all four
    return augment_forward(h, "train_augment_block_input", rgb, on_device, n, H, W, rows, batch, out_host, true, block - 1, 11);
}

int dfd_train_augment_block_rows(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                                 const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host) {
    if (!h) return DFD_ERR_ARG;
    if (block < 11 || block > 15) return fail(h, DFD_ERR_ARG, "train_augment_block_rows: block %d; 11, 12, 13, 14 or 15", block);
    // dfd_train_augment_block_input with block 11 as well: its rows are block 10's output, [14][14][112]
    return augment_forward(h, "train_augment_block_rows", rgb, on_device, n, H, W, rows, batch, out_host, true, block - 1, 10);
}

}  // extern "C"

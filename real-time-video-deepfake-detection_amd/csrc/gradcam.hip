// Grad-CAM of the classifier's head conv (reference deepfake_detection.py:5-7 imports pytorch_grad_cam's GradCAM /
// ClassifierOutputTarget / show_cam_on_image; :300-311 `enable_gradcam`; model.py:100-102 names `net._conv_head` as
// the target layer).  The classifier is a HIP forward without autograd, so the gradient is restated in closed form
// (DESIGN section 2).  With z = BN(conv_head(x15)) (what the head GEMM computes before swish; BN folded into head.w /
// head.b) and A = (z - b) / s the layer's output:
//   g[n][k]   = dL/dfeat: the logit's backward through fc3, the fc2 > 0 mask, fc2, the fc1 > 0 mask and fc1
//   mu[n][k]  = mean_p swish'(z[n][p][k]),  swish'(z) = s(z) (1 + z (1 - s(z)))
//   cam[n][p] = relu( sum_k (g[n][k] * mu[n][k] / 49) * (z[n][p][k] - b[k]) )      (the BN scale cancels)
// then pytorch_grad_cam 1.3.x's scale_cam_image (min-max, cv2 INTER_LINEAR 7 -> 224), the one-layer aggregation (a
// second min-max of the 224 x 224 map) and, optionally, show_cam_on_image's JET overlay on the de-normalised input.
//
// Launches after the unchanged b0_forward: the head GEMM once more with ACT_NONE (z into expbuf, dead by then), the
// MLP backward in two kernels (D1 and G into dwbuf) and one map kernel per call.  No new HBM: host-call outputs are
// staged in headbuf and in whichever of io0 / io1 does not hold the last block's output.  Reductions run in a fixed
// order without atomics, so every output is bit-reproducible.  Compiled with -ffp-contract=off: the resize and the overlay restate numpy / cv2
// operation orders.
#include "b0_kernels.h"
#include "dfd_common.h"
#include "kernel_util.h"

using namespace dfd;

namespace {

constexpr int GC_HW = 49, GC_C = 1280, GC_F1 = 512, GC_F2 = 256, GC_S = 224, GC_PIX = GC_S * GC_S;
constexpr int GC_THREADS = 256;                 // MLP backward block
constexpr int MAP_THREADS = 640, MAP_WAVES = MAP_THREADS / 64;   // map block: two channels per thread, 10 waves per CU

// OpenCV COLORMAP_JET restated as the piecewise-linear jet (x = i / 255; B, G, R = clip(1.5 - |4x - k|, 0, 1) for
// k = 1, 2, 3), rounded to 8 bits.  PARITY WITH OPENCV UNPINNED (no cv2 to compare against).  The same table is
// luts.JET_BGR, which tests/test_gradcam_ref.py checks against this source.
__constant__ unsigned char kJetBgr[256][3] = {
    {128, 0, 0}, {132, 0, 0}, {136, 0, 0}, {140, 0, 0}, {144, 0, 0}, {147, 0, 0}, {152, 0, 0}, {156, 0, 0},
    {160, 0, 0}, {163, 0, 0}, {168, 0, 0}, {172, 0, 0}, {176, 0, 0}, {179, 0, 0}, {184, 0, 0}, {188, 0, 0},
    {192, 0, 0}, {195, 0, 0}, {200, 0, 0}, {204, 0, 0}, {208, 0, 0}, {211, 0, 0}, {216, 0, 0}, {220, 0, 0},
    {224, 0, 0}, {227, 0, 0}, {232, 0, 0}, {236, 0, 0}, {240, 0, 0}, {243, 0, 0}, {248, 0, 0}, {252, 0, 0},
    {255, 0, 0}, {255, 4, 0}, {255, 8, 0}, {255, 13, 0}, {255, 16, 0}, {255, 21, 0}, {255, 25, 0}, {255, 29, 0},
    {255, 33, 0}, {255, 36, 0}, {255, 40, 0}, {255, 45, 0}, {255, 49, 0}, {255, 53, 0}, {255, 57, 0}, {255, 61, 0},
    {255, 65, 0}, {255, 68, 0}, {255, 72, 0}, {255, 77, 0}, {255, 81, 0}, {255, 85, 0}, {255, 89, 0}, {255, 93, 0},
    {255, 97, 0}, {255, 100, 0}, {255, 104, 0}, {255, 109, 0}, {255, 113, 0}, {255, 117, 0}, {255, 121, 0}, {255, 125, 0},
    {255, 129, 0}, {255, 132, 0}, {255, 137, 0}, {255, 141, 0}, {255, 145, 0}, {255, 148, 0}, {255, 153, 0}, {255, 157, 0},
    {255, 161, 0}, {255, 164, 0}, {255, 169, 0}, {255, 173, 0}, {255, 177, 0}, {255, 180, 0}, {255, 185, 0}, {255, 189, 0},
    {255, 193, 0}, {255, 196, 0}, {255, 201, 0}, {255, 205, 0}, {255, 209, 0}, {255, 212, 0}, {255, 217, 0}, {255, 221, 0},
    {255, 225, 0}, {255, 228, 0}, {255, 233, 0}, {255, 237, 0}, {255, 241, 0}, {255, 244, 0}, {255, 249, 0}, {255, 253, 0},
    {254, 255, 1}, {250, 255, 5}, {245, 255, 10}, {242, 255, 14}, {238, 255, 17}, {234, 255, 21}, {229, 255, 26}, {226, 255, 30},
    {222, 255, 33}, {218, 255, 37}, {213, 255, 42}, {210, 255, 46}, {206, 255, 49}, {202, 255, 53}, {197, 255, 58}, {194, 255, 62},
    {190, 255, 66}, {186, 255, 69}, {181, 255, 74}, {178, 255, 78}, {174, 255, 82}, {170, 255, 85}, {165, 255, 90}, {162, 255, 94},
    {158, 255, 98}, {154, 255, 101}, {149, 255, 106}, {146, 255, 110}, {142, 255, 114}, {138, 255, 117}, {133, 255, 122}, {130, 255, 126},
    {126, 255, 130}, {122, 255, 133}, {118, 255, 137}, {114, 255, 141}, {109, 255, 146}, {105, 255, 150}, {101, 255, 154}, {98, 255, 158},
    {94, 255, 162}, {90, 255, 165}, {86, 255, 169}, {82, 255, 173}, {77, 255, 178}, {73, 255, 182}, {69, 255, 186}, {66, 255, 190},
    {62, 255, 194}, {58, 255, 197}, {54, 255, 201}, {50, 255, 205}, {45, 255, 210}, {41, 255, 214}, {37, 255, 218}, {33, 255, 222},
    {30, 255, 226}, {26, 255, 229}, {22, 255, 233}, {18, 255, 237}, {13, 255, 242}, {9, 255, 246}, {5, 255, 250}, {1, 255, 254},
    {0, 253, 255}, {0, 249, 255}, {0, 245, 255}, {0, 241, 255}, {0, 236, 255}, {0, 232, 255}, {0, 228, 255}, {0, 225, 255},
    {0, 221, 255}, {0, 217, 255}, {0, 213, 255}, {0, 209, 255}, {0, 204, 255}, {0, 200, 255}, {0, 196, 255}, {0, 193, 255},
    {0, 189, 255}, {0, 185, 255}, {0, 181, 255}, {0, 177, 255}, {0, 172, 255}, {0, 168, 255}, {0, 164, 255}, {0, 161, 255},
    {0, 157, 255}, {0, 153, 255}, {0, 149, 255}, {0, 145, 255}, {0, 140, 255}, {0, 136, 255}, {0, 132, 255}, {0, 129, 255},
    {0, 125, 255}, {0, 121, 255}, {0, 117, 255}, {0, 113, 255}, {0, 108, 255}, {0, 104, 255}, {0, 100, 255}, {0, 97, 255},
    {0, 93, 255}, {0, 89, 255}, {0, 85, 255}, {0, 81, 255}, {0, 76, 255}, {0, 72, 255}, {0, 68, 255}, {0, 65, 255},
    {0, 61, 255}, {0, 57, 255}, {0, 53, 255}, {0, 49, 255}, {0, 44, 255}, {0, 40, 255}, {0, 36, 255}, {0, 33, 255},
    {0, 29, 255}, {0, 25, 255}, {0, 21, 255}, {0, 17, 255}, {0, 12, 255}, {0, 8, 255}, {0, 4, 255}, {0, 0, 255},
    {0, 0, 252}, {0, 0, 248}, {0, 0, 244}, {0, 0, 240}, {0, 0, 235}, {0, 0, 231}, {0, 0, 227}, {0, 0, 224},
    {0, 0, 220}, {0, 0, 216}, {0, 0, 212}, {0, 0, 208}, {0, 0, 203}, {0, 0, 199}, {0, 0, 195}, {0, 0, 192},
    {0, 0, 188}, {0, 0, 184}, {0, 0, 180}, {0, 0, 176}, {0, 0, 171}, {0, 0, 167}, {0, 0, 163}, {0, 0, 160},
    {0, 0, 156}, {0, 0, 152}, {0, 0, 148}, {0, 0, 144}, {0, 0, 139}, {0, 0, 135}, {0, 0, 132}, {0, 0, 128},
};

__device__ __forceinline__ float ldz(const float* p) { return *p; }
__device__ __forceinline__ float ldz(const bf16_t* p) {
    return __builtin_bit_cast(float, (unsigned)*reinterpret_cast<const unsigned short*>(p) << 16);
}

// G (n x 1280) = D1 . W1 with D1 = (W2^T (w3 . [fc2 > 0])) . [fc1 > 0]; fc1 / fc2 hold the post-ReLU activations of the
// forward (PyTorch's ReLU backward masks on output > 0), weights are the folded [out][in] tensors.  Two small VALU
// kernels, each block MB_ROWS crops (a weight read serves all of them) x 64 output columns, the reduction dimension
// split over the block's 4 waves and summed in wave order.  The weights stay in L2.
constexpr int MB_ROWS = 8, MB_COLS = 64, MB_WAVES = GC_THREADS / 64;

// D1 [n][512]: grid (512 / 64, ceil(n / MB_ROWS))
__global__ __launch_bounds__(GC_THREADS) void gradcam_mlp_d1_kernel(const float* __restrict__ fc1, const float* __restrict__ fc2,
                                                                    const float* __restrict__ w2, const float* __restrict__ w3,
                                                                    float* __restrict__ D1, int n) {
    __shared__ __attribute__((aligned(16))) float d2[GC_F2][MB_ROWS];
    __shared__ float part[MB_WAVES][MB_ROWS][MB_COLS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int r0 = blockIdx.y * MB_ROWS, rows = min(MB_ROWS, n - r0);
#pragma unroll
    for (int r = 0; r < MB_ROWS; ++r) d2[t][r] = (r < rows && fc2[(size_t)(r0 + r) * GC_F2 + t] > 0.f) ? w3[t] : 0.f;
    __syncthreads();
    const int i = blockIdx.x * MB_COLS + lane;
    float a[MB_ROWS] = {};
    constexpr int JW = GC_F2 / MB_WAVES;
#pragma unroll 8
    for (int j = wv * JW; j < (wv + 1) * JW; ++j) {
        const float w = w2[(size_t)j * GC_F1 + i];
        const v4f lo = *reinterpret_cast<const v4f*>(&d2[j][0]), hi = *reinterpret_cast<const v4f*>(&d2[j][4]);
        a[0] += lo.x * w; a[1] += lo.y * w; a[2] += lo.z * w; a[3] += lo.w * w;
        a[4] += hi.x * w; a[5] += hi.y * w; a[6] += hi.z * w; a[7] += hi.w * w;
    }
#pragma unroll
    for (int r = 0; r < MB_ROWS; ++r) part[wv][r][lane] = a[r];
    __syncthreads();
    for (int e = t; e < MB_ROWS * MB_COLS; e += GC_THREADS) {
        const int r = e / MB_COLS, l = e % MB_COLS;
        if (r >= rows) continue;
        float v = part[0][r][l];
        for (int w = 1; w < MB_WAVES; ++w) v += part[w][r][l];
        const size_t o = (size_t)(r0 + r) * GC_F1 + blockIdx.x * MB_COLS + l;
        D1[o] = fc1[o] > 0.f ? v : 0.f;
    }
}

// G [n][1280] = D1 . W1: grid (1280 / 64, ceil(n / MB_ROWS))
__global__ __launch_bounds__(GC_THREADS) void gradcam_mlp_g_kernel(const float* __restrict__ D1, const float* __restrict__ w1,
                                                                   float* __restrict__ G, int n) {
    __shared__ __attribute__((aligned(16))) float d1[GC_F1][MB_ROWS];
    __shared__ float part[MB_WAVES][MB_ROWS][MB_COLS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int r0 = blockIdx.y * MB_ROWS, rows = min(MB_ROWS, n - r0);
    for (int e = t; e < MB_ROWS * GC_F1; e += GC_THREADS) {
        const int r = e / GC_F1, i = e % GC_F1;
        d1[i][r] = r < rows ? D1[(size_t)(r0 + r) * GC_F1 + i] : 0.f;
    }
    __syncthreads();
    const int k = blockIdx.x * MB_COLS + lane;
    float g[MB_ROWS] = {};
    constexpr int IW = GC_F1 / MB_WAVES;
#pragma unroll 8
    for (int i = wv * IW; i < (wv + 1) * IW; ++i) {
        const float w = w1[(size_t)i * GC_C + k];
        const v4f lo = *reinterpret_cast<const v4f*>(&d1[i][0]), hi = *reinterpret_cast<const v4f*>(&d1[i][4]);
        g[0] += lo.x * w; g[1] += lo.y * w; g[2] += lo.z * w; g[3] += lo.w * w;
        g[4] += hi.x * w; g[5] += hi.y * w; g[6] += hi.z * w; g[7] += hi.w * w;
    }
#pragma unroll
    for (int r = 0; r < MB_ROWS; ++r) part[wv][r][lane] = g[r];
    __syncthreads();
    for (int e = t; e < MB_ROWS * MB_COLS; e += GC_THREADS) {
        const int r = e / MB_COLS, l = e % MB_COLS;
        if (r >= rows) continue;
        float v = part[0][r][l];
        for (int w = 1; w < MB_WAVES; ++w) v += part[w][r][l];
        G[(size_t)(r0 + r) * GC_C + blockIdx.x * MB_COLS + l] = v;
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// cv2.resize INTER_LINEAR of a float map, 7 -> 224: sx = (dx + 0.5) * 7 / 224 - 0.5, fx = sx - floor(sx); sx < 0 ->
// (0, 0), sx >= 6 -> (6, 0); horizontal pass a (1 - fx) + b fx per row, then the vertical one the same way.
__device__ __forceinline__ float resize_at(const float* m7, const int* xo, const float* xf, int q) {
    const int dy = q / GC_S, dx = q - dy * GC_S;
    const int sx = xo[dx], sy = xo[dy];
    const float fx = xf[dx], fy = xf[dy];
    const int sx1 = min(sx + 1, 6), sy1 = min(sy + 1, 6);
    const float h0 = m7[sy * 7 + sx] * (1.f - fx) + m7[sy * 7 + sx1] * fx;
    const float h1 = m7[sy1 * 7 + sx] * (1.f - fx) + m7[sy1 * 7 + sx1] * fx;
    return h0 * (1.f - fy) + h1 * fy;
}

// one pixel of show_cam_on_image (1.3.x) before the division by the image max, BGR channel c:
// float32(applyColorMap(uint8(255 * mask), JET)) / 255 + clamp(x * std + mean, 0, 1)
// (jetf: kJetBgr / 255 as float, the same division numpy does)
__device__ __forceinline__ float overlay_pre(const float* xn, const float* jetf, float heat, int q, int c) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const int rgb = 2 - c;
    const int idx = min((int)(255.f * heat), 255);
    const float img = fminf(fmaxf(xn[(size_t)rgb * GC_PIX + q] * stdv[rgb] + mean[rgb], 0.f), 1.f);
    return jetf[idx * 3 + c] + img;
}

// one block per crop.  z: [n][49][1280] NHWC (channels contiguous), G: [n][1280], x: the classifier input NCHW (read
// only for the overlay).  Outputs (each may be null): cam7 [n][49] the ReLU'd map before any normalisation, heat
// [n][224][224], overlay [n][224][224][3] BGR u8.
template <typename XT>
__global__ __launch_bounds__(MAP_THREADS) void gradcam_map_kernel(const XT* __restrict__ z, const float* __restrict__ head_b,
                                                                 const float* __restrict__ G, const float* __restrict__ x,
                                                                 float* __restrict__ cam7, float* __restrict__ heat,
                                                                 uint8_t* __restrict__ overlay) {
    __shared__ float red[MAP_WAVES][GC_HW];
    __shared__ float m7[GC_HW];
    __shared__ float stat[MAP_WAVES][2];
    __shared__ int xo[GC_S];
    __shared__ float xf[GC_S];
    __shared__ float jetf[256 * 3];
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const XT* zn = z + (size_t)n * GC_HW * GC_C;
    const float* gn = G + (size_t)n * GC_C;

    // 1. channel weights and the 49 position sums: thread t owns channels t and t + 640 and keeps its partial sums
    float part[GC_HW];
#pragma unroll
    for (int p = 0; p < GC_HW; ++p) part[p] = 0.f;
    for (int k = t; k < GC_C; k += MAP_THREADS) {
        float v[GC_HW];
#pragma unroll
        for (int p = 0; p < GC_HW; ++p) v[p] = ldz(zn + (size_t)p * GC_C + k);
        float mu = 0.f;
#pragma unroll
        for (int p = 0; p < GC_HW; ++p) {
            const float s = 1.f / (1.f + __expf(-v[p]));
            mu += s * (1.f + v[p] * (1.f - s));
        }
        const float w = gn[k] * (mu / (float)GC_HW) / (float)GC_HW;
        const float b = head_b[k];
#pragma unroll
        for (int p = 0; p < GC_HW; ++p) part[p] += w * (v[p] - b);
    }
#pragma unroll
    for (int p = 0; p < GC_HW; ++p) {
        const float s = wave_sum(part[p]);
        if (lane == 0) red[wv][p] = s;
    }
    if (t < GC_S) {                                      // the resize's source offsets / weights (same for x and y)
        const float f = ((float)t + 0.5f) * (7.f / (float)GC_S) - 0.5f;
        int s = (int)floorf(f);
        float fr = f - (float)s;
        if (s < 0) { s = 0; fr = 0.f; }
        if (s >= 6) { s = 6; fr = 0.f; }
        xo[t] = s;
        xf[t] = fr;
    }
    if (overlay)
        for (int i = t; i < 256 * 3; i += MAP_THREADS) jetf[i] = (float)kJetBgr[i / 3][i % 3] / 255.f;
    __syncthreads();
    if (wv == 0) {
        // 2. ReLU, raw map out, first min-max (scale_cam_image: m - min, then / (1e-7 + max))
        float c = 0.f;
        if (lane < GC_HW) {
            float sum = red[0][lane];
            for (int w = 1; w < MAP_WAVES; ++w) sum += red[w][lane];
            c = fmaxf(sum, 0.f);
            if (cam7) cam7[(size_t)n * GC_HW + lane] = c;
        }
        const float lo = wave_min(lane < GC_HW ? c : INFINITY);
        const float hi = wave_max(lane < GC_HW ? c : -INFINITY);
        if (lane < GC_HW) m7[lane] = (c - lo) / (1e-7f + (hi - lo));
    }
    __syncthreads();
    if (!heat && !overlay) return;

    // 3. the 224 x 224 map's min / max (its second min-max); recomputed from the 49 values in every pass
    float lo = INFINITY, hi = -INFINITY;
    for (int q = t; q < GC_PIX; q += MAP_THREADS) {
        const float r = resize_at(m7, xo, xf, q);
        lo = fminf(lo, r);
        hi = fmaxf(hi, r);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (lane == 0) { stat[wv][0] = lo; stat[wv][1] = hi; }
    __syncthreads();
    lo = stat[0][0];
    hi = stat[0][1];
    for (int w = 1; w < MAP_WAVES; ++w) {
        lo = fminf(lo, stat[w][0]);
        hi = fmaxf(hi, stat[w][1]);
    }
    const float den = 1e-7f + (hi - lo);
    __syncthreads();                                     // stat is reused below

    // 4. heat out; the overlay's image max
    const float* xn = x + (size_t)n * 3 * GC_PIX;
    float vmax = -INFINITY;
    for (int q = t; q < GC_PIX; q += MAP_THREADS) {
        const float hv = (resize_at(m7, xo, xf, q) - lo) / den;
        if (heat) heat[(size_t)n * GC_PIX + q] = hv;
        if (overlay)
#pragma unroll
            for (int c = 0; c < 3; ++c) vmax = fmaxf(vmax, overlay_pre(xn, jetf, hv, q, c));
    }
    if (!overlay) return;
    vmax = wave_max(vmax);
    if (lane == 0) stat[wv][0] = vmax;
    __syncthreads();
    vmax = stat[0][0];
    for (int w = 1; w < MAP_WAVES; ++w) vmax = fmaxf(vmax, stat[w][0]);

    // 5. overlay out: uint8(255 * (v / max)), truncating
    uint8_t* on = overlay + (size_t)n * GC_PIX * 3;
    for (int q = t; q < GC_PIX; q += MAP_THREADS) {
        const float hv = (resize_at(m7, xo, xf, q) - lo) / den;
#pragma unroll
        for (int c = 0; c < 3; ++c) on[(size_t)q * 3 + c] = (uint8_t)(int)(255.f * (overlay_pre(xn, jetf, hv, q, c) / vmax));
    }
}

// The three Grad-CAM launches on h->stream, as one function of device pointers (the product path and dfd_gradcam_tap
// launch the same kernels with the same grids): z [n][49][1280] fp32 or - z_bf16 - bf16, fc1 [n][512] / fc2 [n][256] the
// forward's post-ReLU activations, x the classifier input (read only for the overlay); D1 [n][512] and G [n][1280] are
// work buffers, cam7 / heat / overlay the nullable outputs.  The weights are the handle's own.
int gradcam_launch(dfd_handle* h, const void* z, bool z_bf16, const float* fc1, const float* fc2, const float* x, int n, float* D1,
                   float* G, float* cam7, float* heat, uint8_t* overlay) {
    const B0Plan& P = h->b0;
    const unsigned row_blocks = (unsigned)((n + MB_ROWS - 1) / MB_ROWS);
    hipLaunchKernelGGL(gradcam_mlp_d1_kernel, dim3(GC_F1 / MB_COLS, row_blocks), dim3(GC_THREADS), 0, h->stream, fc1, fc2,
                       P.fc2_w, P.fc3_w, D1, n);
    hipLaunchKernelGGL(gradcam_mlp_g_kernel, dim3(GC_C / MB_COLS, row_blocks), dim3(GC_THREADS), 0, h->stream, D1, P.fc1_w, G, n);
    if (z_bf16)
        hipLaunchKernelGGL(gradcam_map_kernel<bf16_t>, dim3((unsigned)n), dim3(MAP_THREADS), 0, h->stream,
                           static_cast<const bf16_t*>(z), P.head_b, G, x, cam7, heat, overlay);
    else
        hipLaunchKernelGGL(gradcam_map_kernel<float>, dim3((unsigned)n), dim3(MAP_THREADS), 0, h->stream,
                           static_cast<const float*>(z), P.head_b, G, x, cam7, heat, overlay);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

// forward (logits into logits_dev) + the three Grad-CAM launches on h->stream; outputs are device pointers (nullable)
int gradcam_run(dfd_handle* h, const float* x_dev, int n, float* logits_dev, float* cam7, float* heat, uint8_t* overlay) {
    if (n <= 0) return fail(h, DFD_ERR_ARG, "gradcam: batch must be positive");
    if (n > h->max_batch) return fail(h, DFD_ERR_CAPACITY, "gradcam: batch %d exceeds handle capacity %d", n, h->max_batch);
    int rc;
    if ((rc = b0_forward(h, x_dev, n, logits_dev, nullptr, nullptr))) return rc;
    if ((rc = b0_head_preact(h, n, h->expbuf))) return rc;           // expbuf: >= 112*112*96 floats per crop, dead here
    float* G = h->dwbuf;                                               // dwbuf: >= 112*112*96 floats per crop, dead here
    float* D1 = h->dwbuf + (size_t)n * GC_C;
    return gradcam_launch(h, h->expbuf, h->act_bf16, h->fc1, h->fc2, x_dev, n, D1, G, cam7, heat, overlay);
}

// device staging of the host-side calls: heat in headbuf (49*1280 >= 224*224 floats per crop), cam7 and overlay in the
// activation buffer that does not hold the last block's output (112*112*32 floats per crop)
struct Staging {
    float *cam7, *heat;
    uint8_t* overlay;
};
Staging staging(dfd_handle* h, int n, bool cam7, bool heat, bool overlay) {
    float* spare = b0_last_block_out(h) == h->io0 ? h->io1 : h->io0;
    Staging s;
    s.cam7 = cam7 ? spare : nullptr;
    s.heat = heat ? h->headbuf : nullptr;
    s.overlay = overlay ? reinterpret_cast<uint8_t*>(spare + (size_t)n * GC_HW) : nullptr;
    return s;
}

// device -> host copies of the first k rows of every requested output (logits from h->logits), then a stream wait
int gradcam_download(dfd_handle* h, const Staging& s, int k, float* logits, float* cam7, float* heat, uint8_t* overlay) {
    DFD_HIP_TRY(h, hipMemcpyAsync(logits, h->logits, (size_t)k * 4, hipMemcpyDeviceToHost, h->stream));
    if (cam7) DFD_HIP_TRY(h, hipMemcpyAsync(cam7, s.cam7, (size_t)k * GC_HW * 4, hipMemcpyDeviceToHost, h->stream));
    if (heat) DFD_HIP_TRY(h, hipMemcpyAsync(heat, s.heat, (size_t)k * GC_PIX * 4, hipMemcpyDeviceToHost, h->stream));
    if (overlay) DFD_HIP_TRY(h, hipMemcpyAsync(overlay, s.overlay, (size_t)k * GC_PIX * 3, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

}  // namespace

extern "C" {

int dfd_gradcam_nchw_device(dfd_handle* h, const float* nchw_dev, int n, float* logits_dev, float* cam7_dev, float* heat_dev,
                            uint8_t* overlay_dev) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_dev || !logits_dev) return fail(h, DFD_ERR_ARG, "gradcam: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    return gradcam_run(h, nchw_dev, n, logits_dev, cam7_dev, heat_dev, overlay_dev);
}

int dfd_gradcam_nchw(dfd_handle* h, const float* nchw_host, int n, float* logits_host, float* cam7_host, float* heat_host,
                     uint8_t* overlay_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !logits_host) return fail(h, DFD_ERR_ARG, "gradcam: null pointer");
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "gradcam: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * GC_PIX * 4, hipMemcpyHostToDevice, h->stream));
    const Staging s = staging(h, n, cam7_host, heat_host, overlay_host);
    int rc = gradcam_run(h, h->in_nchw, n, h->logits, s.cam7, s.heat, s.overlay);
    if (rc) return rc;
    return gradcam_download(h, s, n, logits_host, cam7_host, heat_host, overlay_host);
}

int dfd_gradcam_crops(dfd_handle* h, const uint8_t* bgr, int hh, int ww, int stride, const int32_t* xywh, int n, int apply_clahe,
                      float* logits_out, float* cam7_out, float* heat_out, uint8_t* overlay_out) {
    if (!h) return DFD_ERR_ARG;
    if (!logits_out) return fail(h, DFD_ERR_ARG, "gradcam_crops: null output");
    if (!bgr || hh <= 0 || ww <= 0 || stride < ww * 3) return fail(h, DFD_ERR_ARG, "gradcam_crops: bad frame pointer or geometry");
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "gradcam_crops: %d boxes outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure(h, &h->frame_buf, (size_t)hh * stride);
    if (rc) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(h->frame_buf.p, bgr, (size_t)hh * stride, hipMemcpyHostToDevice, h->stream));
    // as dfd_classify_crops: crop / CLAHE / MTCNN / 224 x 224, the classifier at the batch of the crops the cascade kept
    if ((rc = preprocess_run(h, (const uint8_t*)h->frame_buf.p, hh, ww, stride, xywh, n, apply_clahe, nullptr, true))) return rc;
    const int k = h->n_compact;
    std::vector<float> lg(k), c7(cam7_out ? (size_t)k * GC_HW : 0), ht(heat_out ? (size_t)k * GC_PIX : 0);
    std::vector<uint8_t> ov(overlay_out ? (size_t)k * GC_PIX * 3 : 0);
    if (k > 0) {
        const Staging s = staging(h, k, cam7_out, heat_out, overlay_out);
        if ((rc = gradcam_run(h, h->in_nchw, k, h->logits, s.cam7, s.heat, s.overlay))) return rc;
        if ((rc = gradcam_download(h, s, k, lg.data(), cam7_out ? c7.data() : nullptr, heat_out ? ht.data() : nullptr,
                                   overlay_out ? ov.data() : nullptr))) return rc;
    } else {
        DFD_HIP_TRY(h, stream_sync(h));
    }
    // rejected crops (MTCNN found no face): NaN logit, all-zero maps
    for (int i = 0, j = 0; i < n; ++i) {
        const bool kept = h->crop_valid[i] != 0;
        logits_out[i] = kept ? lg[j] : NAN;
        if (cam7_out) {
            float* d = cam7_out + (size_t)i * GC_HW;
            if (kept) memcpy(d, c7.data() + (size_t)j * GC_HW, GC_HW * 4); else memset(d, 0, GC_HW * 4);
        }
        if (heat_out) {
            float* d = heat_out + (size_t)i * GC_PIX;
            if (kept) memcpy(d, ht.data() + (size_t)j * GC_PIX, GC_PIX * 4); else memset(d, 0, GC_PIX * 4);
        }
        if (overlay_out) {
            uint8_t* d = overlay_out + (size_t)i * GC_PIX * 3;
            if (kept) memcpy(d, ov.data() + (size_t)j * GC_PIX * 3, GC_PIX * 3); else memset(d, 0, GC_PIX * 3);
        }
        if (kept) ++j;
    }
    return DFD_OK;
}

// test entry (include/dfd_hip.h): gradcam_launch on buffers of its own, every stage copied out, D1 / G / cam7 with
// sentinel-filled guard rows behind row n - 1
int dfd_gradcam_tap(dfd_handle* h, dfd_gradcam_tap_params* p) {
    if (!h || !p) return DFD_ERR_ARG;
    const bool from_z = p->start == DFD_GRADCAM_TAP_FROM_Z;
    if (p->start != DFD_GRADCAM_TAP_FROM_X && !from_z) return fail(h, DFD_ERR_ARG, "gradcam_tap: start must be 0 (x) or 1 (z)");
    const int n = p->n;
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "gradcam_tap: batch %d outside 1..%d", n, h->max_batch);
    if (from_z ? (!p->z || !p->fc1 || !p->fc2 || (p->overlay && !p->x)) : !p->x)
        return fail(h, DFD_ERR_ARG, "gradcam_tap: null input pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const bool zb = from_z ? p->z_bf16 != 0 : h->act_bf16;
    p->z_bf16 = zb ? 1 : 0;
    const size_t rows = (size_t)n + DFD_GRADCAM_TAP_GUARD, zbytes = (size_t)n * GC_HW * GC_C * (zb ? 2 : 4);
    // one allocation, 256-byte slots: the guarded stage outputs first, then the injected inputs of start "z"
    size_t total = 0;
    auto slot = [&](size_t bytes) { const size_t at = total; total += (bytes + 255) / 256 * 256; return at; };
    const size_t od1 = slot(rows * GC_F1 * 4), og = slot(rows * GC_C * 4), oc = slot(rows * GC_HW * 4);
    const size_t oh = slot(p->heat ? (size_t)n * GC_PIX * 4 : 0), oo = slot(p->overlay ? (size_t)n * GC_PIX * 3 : 0);
    const size_t oz = slot(from_z ? zbytes : 0), o1 = slot(from_z ? (size_t)n * GC_F1 * 4 : 0), o2 = slot(from_z ? (size_t)n * GC_F2 * 4 : 0);
    const size_t ox = slot(from_z && p->x ? (size_t)n * 3 * GC_PIX * 4 : 0);
    char* base = nullptr;
    DFD_HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&base), total + 256));
    auto run = [&]() -> int {
        float *D1 = reinterpret_cast<float*>(base + od1), *G = reinterpret_cast<float*>(base + og), *cam7 = reinterpret_cast<float*>(base + oc);
        float* heat = p->heat ? reinterpret_cast<float*>(base + oh) : nullptr;
        uint8_t* overlay = p->overlay ? reinterpret_cast<uint8_t*>(base + oo) : nullptr;
        DFD_HIP_TRY(h, hipMemsetD32Async(base, (int)DFD_GRADCAM_TAP_SENTINEL, oh / 4, h->stream));     // D1, G and cam7 with their guard rows
        const void* z;
        const float *fc1, *fc2, *x;
        int rc;
        if (from_z) {
            DFD_HIP_TRY(h, hipMemcpyAsync(base + oz, p->z, zbytes, hipMemcpyHostToDevice, h->stream));
            DFD_HIP_TRY(h, hipMemcpyAsync(base + o1, p->fc1, (size_t)n * GC_F1 * 4, hipMemcpyHostToDevice, h->stream));
            DFD_HIP_TRY(h, hipMemcpyAsync(base + o2, p->fc2, (size_t)n * GC_F2 * 4, hipMemcpyHostToDevice, h->stream));
            if (p->x) DFD_HIP_TRY(h, hipMemcpyAsync(base + ox, p->x, (size_t)n * 3 * GC_PIX * 4, hipMemcpyHostToDevice, h->stream));
            z = base + oz;
            fc1 = reinterpret_cast<const float*>(base + o1);
            fc2 = reinterpret_cast<const float*>(base + o2);
            x = p->x ? reinterpret_cast<const float*>(base + ox) : nullptr;
        } else {
            // as gradcam_run: the forward, then the head GEMM once more without swish
            DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, p->x, (size_t)n * 3 * GC_PIX * 4, hipMemcpyHostToDevice, h->stream));
            if ((rc = b0_forward(h, h->in_nchw, n, h->logits, nullptr, nullptr))) return rc;
            if ((rc = b0_head_preact(h, n, h->expbuf))) return rc;
            z = h->expbuf;
            fc1 = h->fc1;
            fc2 = h->fc2;
            x = h->in_nchw;
        }
        if ((rc = gradcam_launch(h, z, zb, fc1, fc2, x, n, D1, G, cam7, heat, overlay))) return rc;
        if (!from_z) {
            if (p->z) DFD_HIP_TRY(h, hipMemcpyAsync(p->z, z, zbytes, hipMemcpyDeviceToHost, h->stream));
            if (p->fc1) DFD_HIP_TRY(h, hipMemcpyAsync(p->fc1, fc1, (size_t)n * GC_F1 * 4, hipMemcpyDeviceToHost, h->stream));
            if (p->fc2) DFD_HIP_TRY(h, hipMemcpyAsync(p->fc2, fc2, (size_t)n * GC_F2 * 4, hipMemcpyDeviceToHost, h->stream));
        }
        if (p->D1) DFD_HIP_TRY(h, hipMemcpyAsync(p->D1, D1, rows * GC_F1 * 4, hipMemcpyDeviceToHost, h->stream));
        if (p->G) DFD_HIP_TRY(h, hipMemcpyAsync(p->G, G, rows * GC_C * 4, hipMemcpyDeviceToHost, h->stream));
        if (p->cam7) DFD_HIP_TRY(h, hipMemcpyAsync(p->cam7, cam7, rows * GC_HW * 4, hipMemcpyDeviceToHost, h->stream));
        if (heat) DFD_HIP_TRY(h, hipMemcpyAsync(p->heat, heat, (size_t)n * GC_PIX * 4, hipMemcpyDeviceToHost, h->stream));
        if (overlay) DFD_HIP_TRY(h, hipMemcpyAsync(p->overlay, overlay, (size_t)n * GC_PIX * 3, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, stream_sync(h));
        return DFD_OK;
    };
    const int rc = run();
    if (rc != DFD_OK) hipStreamSynchronize(h->stream);
    hipFree(base);
    return rc;
}

}  // extern "C"

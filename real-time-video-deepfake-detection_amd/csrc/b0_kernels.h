// Launchers for the EfficientNet-B0 kernels (gfx950).  All activations are NHWC fp32.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace dfd {

// activation storage: float, or bf16_t when the handle runs with "bf16_activations" (kernel_util.h)
typedef __bf16 bf16_t;

enum Act { ACT_NONE = 0, ACT_SWISH = 1, ACT_RELU = 2, ACT_PRELU = 3 };   // PRELU: bias points at [N bias][N slope]

// stem: 3x3 stride-2 conv, NCHW (n,3,224,224) -> NHWC (n,112,112,32), folded BN + swish.
template <typename XT>
void launch_stem(const float* x_nchw, const float* w /*[3][3][3][32]*/, const float* b,
                 XT* y, int n, hipStream_t s);

// stem + block-0 depthwise fused (the stem activation stays in LDS); stem_out may be null, or a buffer
// [n][112][112][32] that receives a copy of the stem activation for parity taps.  The tile count (98) is
// that of launch_depthwise for block 0.
// (ws3: the stem weights [32][27] as three bf16 planes, `plane` elements apart, rows Kp long: the 3x3x3 -> 32 stem conv
// runs on the bf16 MFMA with split-precision operands, K = 27 padded to 32)
template <typename XT>
void launch_stem_dw(const float* x_nchw, const unsigned short* ws3, int plane, int Kp, const float* bs, const float* Wd,
                    const float* bd, XT* Y, float* P, XT* stem_out, int n, int* tiles, hipStream_t s);

// pointwise conv as GEMM: Y[m][o] = act( sum_k X[m][k]*gate[m/HW][k] * W[o][k] + b[o] ) + R[m][o]
// gate / R may be null.  X rows have stride K, Y/R rows stride N.
void launch_pointwise(const float* X, const float* W, const float* bias, const float* gate,
                      const float* R, float* Y, int M, int K, int N, int HW, int act,
                      hipStream_t s);

// geometry of an implicit-GEMM convolution on NHWC fp32 (square kernel, same stride/pad/dilation
// in both directions)
struct ConvGeom {
    int H = 0, W = 0, Ho = 0, Wo = 0, Cin = 0, ksize = 1, stride = 1, pad = 0, dil = 1;
};

// k x k convolution as implicit GEMM on the same MFMA kernel (C_in % 32 == 0; returns false
// otherwise): Y[n][oy][ox][o] = act( conv(X, W[o][ky][kx][ci]) + b[o] (+ R before act if res_first) )
bool launch_conv_gemm(const float* X, const float* W, const float* bias, const float* R, float* Y,
                      int n_img, const ConvGeom& g, int Cout, int act, bool res_first, hipStream_t s);

// Split-precision variants (gemm_split.hip): same contracts, the weight operand is the three-plane bf16 split
// of W [N][K] written by launch_split_weights (out: 3 * split_weights_count(N, K) bf16, zero-padded planes).
// fp32-exact products, fp32 accumulate.
size_t split_weights_count(int N, int K);
void launch_split_weights(const float* W, unsigned short* out, int N, int K, hipStream_t s, bool transposed = false);
bool split_gemm_supports(int K, int N);
// can a gated 1x1 conv of this shape run on pw8_kernel (weights resident in LDS; images of HW rows, HW % 16 == 0)?
bool split_gemm_thin_supports(int K, int N, int HW);
// `tab` is the handle's tile table (null: heuristic tile, nothing remembered).  A shape the table has no
// measurement for runs the heuristic tile unless the table is in tuning mode (dfd_warmup), where every
// candidate is timed on the caller's operands - the only place these launchers synchronise.  Calls whose
// activations span 2^31 bytes or more are issued as several launches over whole images (32-bit buffer offsets
// inside the kernels); false = shape not supported.
struct S6Table;
S6Table* s6_table_create();
void s6_table_destroy(S6Table* t);
void s6_table_set_force(S6Table* t, int idx);      // >= 0: run candidate idx (mod count) everywhere; -1: normal
void s6_table_set_tuning(S6Table* t, bool on);
int s6_table_measured(const S6Table* t);           // shapes with a measured tile
int s6_max_candidates();                           // largest candidate count of any call (pw8 / pw9 extras included)
// host-side bookkeeping for dfd_gemm_tap: the candidates "gemm_tile" indexes for one launch (pw8 / pw9 decided as the
// launchers decide them), the instance the table dispatched last and how many launches it has dispatched
int s6_call_candidates(bool conv, bool gated, bool bf16, int planes, int M, int K, int N, int HW, int act, bool has_res,
                       int res_first);
void s6_table_last(const S6Table* t, int out[6]);  // kind, wm, wn, mt, nt, ks
long long s6_table_dispatches(const S6Table* t);
long long s6_chunk_rows(long long M, long long row_bytes, long long HW);
std::string s6_table_export(const S6Table* t);                       // measured entries as text
int s6_table_import(S6Table* t, const char* text, size_t len);       // -> entries accepted
// XT = float: every fp32 activation is split into three bf16 terms in registers (planes must be 3);
// XT = bf16_t: bf16 activation storage in and out, `planes` = 3 (fp32-exact weights) or 1 (bf16 weights).
template <typename XT>
bool launch_pointwise_split(S6Table* tab, const XT* X, const unsigned short* W3, const float* bias, const float* gate,
                            const XT* R, XT* Y, int M, int K, int N, int HW, int act, int planes, hipStream_t s,
                            int res_first = 0);      // 1: R is added before the activation (no network asks for it)
template <typename XT>
bool launch_conv_gemm_split(S6Table* tab, const XT* X, const unsigned short* W3, const float* bias, const XT* R,
                            XT* Y, int n_img, const ConvGeom& g, int Cout, int act, bool res_first, int planes, hipStream_t s);

// depthwise kxk conv (k in {3,5}, stride in {1,2}, TF-SAME pad) + folded BN + swish, and
// per-tile channel sums for the squeeze-excite pool: P[n][tile][c].  Returns the tile count
// through *tiles.  Only the 16 shape classes of EfficientNet-B0 at 224x224 are instantiated.
template <typename XT>
bool launch_depthwise(const XT* X, const float* W /*[k][k][C]*/, const float* bias, XT* Y,
                      float* P, int n, int H, int C, int k, int stride, int pad_lo,
                      int* tiles, hipStream_t s);
int depthwise_tiles(int H, int C, int k, int stride);
// MBConv front half in one kernel: 1x1 expand (+BN+swish) computed per LDS halo tile on the bf16 MFMA with
// split-precision operands (We3 = the three bf16 planes of We [C][Cin] from launch_split_weights, `plane`
// elements apart, rows Kp long), then the depthwise conv as above.  Xin: block input [n][H][H][Cin]; be [C].
// Returns false when no instantiation covers the shape (callers then run the GEMM + launch_depthwise).
// late: the whole-image launches of blocks 6-15 (option "fuse_late"); k5: among those, fp32 blocks 6-11 through
// mbconv_k5_kernel (option "fuse_k5"): 1 = with mbconv_late_kernel's result bits, 2 = with those of expand GEMM + depthwise
// kernel (the expand bias added after the products instead of in front of them).  Block 11 has form 2 only, blocks 6 and 7
// form 1 only; a request for a form the block has no instance of returns false.
template <typename XT>
bool launch_mbconv_front(const XT* Xin, int Cin, const unsigned short* We3, int plane, int Kp, const float* Wef, const float* be,
                         const float* Wd, const float* bd, XT* Y, float* P, int n, int H, int C, int k, int stride,
                         int pad_lo, int* tiles, hipStream_t s, bool late = false, int k5 = 0);
// Block 1's front half with block 0's projection folded into its prologue (option "fuse_proj0", fp32 only): Xdw0 is block
// 0's depthwise output [n][H][H][32], gate0 its squeeze-excite gate [n][32], Wp3 / plane / Kp / bp the three bf16 planes
// of its projection weights [16][32] and the bias; the rest as launch_mbconv_front.  The block input it computes per halo
// pixel has the bits the separate projection launch stores.  `supported`: the shape is block 1's; the launcher
// returns false otherwise.
bool mbconv_proj0_supported(int H, int C, int k, int stride, int Cin, int C0);
bool launch_mbconv_front_proj0(const float* Xdw0, const float* gate0, const unsigned short* Wp3, int plane, int Kp, const float* bp,
                               const float* Wef, const float* be, const float* Wd, const float* bd, float* Y, float* P, int n,
                               int H, int C, int k, int stride, int Cin, int pad_lo, int* tiles, hipStream_t s);
// pool-tile count of the fused launch (the larger of the fp32 and bf16 kernels'), -1: none.  late: also the whole-image launches of blocks 6-15
// (mbconv_late_kernel, option "fuse_late"); k5: also a block that has no such instance but one of mbconv_k5_kernel (block 11)
int mbconv_tiles(int H, int C, int k, int stride, int Cin, bool late = false, bool k5 = false);
// the block shapes (and padding) mbconv_k5_kernel covers; launch_mbconv_front with k5 != 0 fails for any other
bool mbconv_k5_shape(int H, int C, int k, int stride, int Cin, int pad_lo);

// squeeze-excite gate: mean over tiles*pixels -> FC(c_se)+swish -> FC(C)+sigmoid.
void launch_se(const float* P, int tiles, float inv_hw, const float* w1, const float* b1,
               const float* w2t, const float* b2, float* gate, int n, int C, int c_se,
               hipStream_t s);

// global average pool over hw pixels: [n][hw][C] -> [n][C]
template <typename XT>
void launch_avgpool(const XT* X, float* Y, int n, int hw, int C, hipStream_t s);
void launch_bf16_to_f32(const bf16_t* x, float* y, size_t n, hipStream_t s);

}  // namespace dfd

// Launchers for the 8-bit image kernels (resize, CLAHE path, crop -> network input).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dfd {

// Integer LUTs of the 8-bit colour conversions (built by luts.py, uploaded at dfd_create).
struct ColorTables {
    const int *gamma, *cbrt, *L_fy, *L_y, *a_div, *b_div, *ab_xz, *inv_gamma, *hsv_sdiv, *hsv_hdiv;
    int fwd[9];        // RGB->XYZ/white, 12-bit
    long long inv[9];  // XYZ*white->RGB, 12-bit
};

struct CropDesc {
    int x, y, w, h;        // box in the frame
    size_t offset;         // byte offset of this crop's packed w*h*3 region in the scratch buffers
    size_t src_off;        // byte offset of the crop's frame inside the frame buffer (batched frames)
    size_t stride;         // row stride of that frame (frames of different widths share one batch)
};

// one frame of a ragged batch: byte offset in the frame arena, size, row stride
struct FrameDesc {
    size_t offset;
    int h, w, stride;
};

void launch_resize_bgr(const uint8_t* src, int n, int sh, int sw, size_t sstride, size_t simg,
                       uint8_t* dst, int dh, int dw, hipStream_t s);
// the same for n frames of their own sizes (frames_dev: n descriptors on the device) -> [n][dh][dw][3]
void launch_resize_bgr_ragged(const uint8_t* src, const FrameDesc* frames_dev, int n, uint8_t* dst, int dh, int dw,
                              hipStream_t s);
// single-channel cv2.resize(INTER_LINEAR) and u8 -> float (x scale)
// test-time augmentation of face crops (flip, brightness, small rotation) as the reference builds it with cv2: one row per
// output image.  src_off / dst_off: bytes from the launch's source / destination base; stride: source row stride;
// m = the inverted 2x3 affine matrix (warpAffine's internal form); tw_log2: tile width of this image (tta_tile_count)
struct TtaRow {
    size_t src_off, stride, dst_off;
    int h, w, flip, tw_log2;
    float alpha;
    double m[6];
};
// tiles (= blocks) an h x w image takes and the tile width chosen for it
int tta_tile_count(int h, int w, int* tw_log2);
// n images, `tiles` blocks in all; tile_start_dev: n + 1 running tile counts
void launch_tta_augment_batch(const uint8_t* src_base, uint8_t* dst_base, const TtaRow* rows_dev, const int* tile_start_dev, int n,
                              int tiles, hipStream_t s);
void launch_resize_gray(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, hipStream_t s);
void u8_to_float(const uint8_t* src, float* dst, int n, float scale, hipStream_t s);
// both read a crop's source rows with the row stride of its descriptor
void launch_clahe(const uint8_t* frame, const CropDesc* crops_dev, int n, uint8_t* lab,
                  uint8_t* luts, uint8_t* bgr_out, const ColorTables& T, int max_pixels, hipStream_t s);
void launch_crop_norm(const uint8_t* frame, const uint8_t* scratch, const CropDesc* crops_dev,
                      int n, float* out_nchw, bool from_scratch, hipStream_t s);

}  // namespace dfd

// The JPEG tables every path here reads (host parser and entropy decoder, device entropy decoder, encoder, ELA round
// trip, training augment), stated once: the zig-zag order, the ITU-T T.81 Annex K.1 quantisation tables and libjpeg's
// scaling of them by a quality.  Plain C++ - no HIP in here: jpeg_entropy.h includes it and builds into the sanitizer
// harness.  Device code indexes the arrays at run time and calls the constexpr functions as they stand.
#pragma once
#include <cstdint>

namespace dfd {

// position k of the zig-zag scan -> natural (row-major) index in the 8x8 block (jutils.c jpeg_natural_order)
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl (Annex K.1), natural order: [0] luma, [1] chroma
constexpr uint8_t kJpegBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// jcparam.c jpeg_quality_scaling: quality 1..100 -> percentage the base tables are scaled by
constexpr int jpeg_quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - quality * 2; }

// jpeg_add_quant_table with force_baseline: entry i (natural order) of the luma (chroma = 0) or chroma (1) table
constexpr int jpeg_quant_value(int chroma, int i, int scale) {
    const int q = (kJpegBaseQuant[chroma][i] * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

static_assert(jpeg_quant_value(0, 0, jpeg_quality_scale(90)) == 3, "quality 90, luma DC");
static_assert(jpeg_quant_value(1, 63, jpeg_quality_scale(90)) == 20, "quality 90, last chroma entry");
static_assert(jpeg_quant_value(0, 0, jpeg_quality_scale(1)) == 255 && jpeg_quant_value(1, 63, jpeg_quality_scale(1)) == 255, "quality 1 clamps to 255");
static_assert(jpeg_quant_value(0, 63, jpeg_quality_scale(100)) == 1 && jpeg_quant_value(1, 0, jpeg_quality_scale(100)) == 1, "quality 100 clamps to 1");

}  // namespace dfd

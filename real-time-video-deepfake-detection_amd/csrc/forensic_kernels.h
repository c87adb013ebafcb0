// Launchers and buffer layout of the forensic-signal kernels (256x256 analysis image).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "forensic_score.h"   // ForensicStat: the per-frame scalar statistics produced on the device
#include "imgproc_kernels.h"

namespace dfd {

struct ForensicBuffers {
    uint8_t* rs;         // [n][256][256][3] resized BGR
    uint8_t* gray;       // [n][65536]
    float2* fft_tmp;     // [n][65536] row-FFT output, transposed
    double* fft_part;    // [n][256][7]
    short2* grad;        // [n][65536] Sobel dx,dy
    double* lap_part;    // [n][256][2]
    uint8_t* map;        // [n][65536] Canny labels
    double* edge_count;  // [n]
    uint8_t *jy, *jcb, *jcr;   // decoded JPEG planes [n][65536], [n][16384] x2
    double* hsv_part;    // [n][256][4]
    unsigned* hue_bits;  // [n][6]
    double* stats;       // [n][FORENSIC_STATS]
    double* stats_noise; // [n][64] block stds of the noise residual
    double* stats_ela;   // [n][64] block means of the ELA difference
};

// test entry (dfd_forensic_tap) only: where the chain starts, and storage for what the kernels otherwise keep in LDS
enum ForensicStart { FROM_RS = 0, FROM_GRAY, FROM_GRAD, FROM_MAP };
struct ForensicTaps {
    float2* spectrum;    // [n][256][256] second FFT pass, [k1][k2] like fft_tmp
    float* logmag;       // [n][256][256] log1pf(hypotf()) of it: the values the band sums add
    uint8_t* edges;      // [n][65536] final hysteresis set, 0 / 1
};

size_t forensic_bytes_per_frame();
void forensic_carve(void* base, int n, ForensicBuffers* out);
void launch_forensics(const ForensicBuffers& B, int n, bool full, const ColorTables& T, const float2* tw, hipStream_t s,
                      int gray_only = 0, ForensicStart start = FROM_RS, const ForensicTaps* taps = nullptr);
void launch_absdiff(const uint8_t* gray, const uint8_t* prev, double* part256, hipStream_t s);
void launch_absdiff_pairs(const uint8_t* gray, const int* prev_index, double* part /*[n][256]*/, int n, hipStream_t s);
// frame f of gray [n][65536] against the plane prev_dev[f] (device pointer table; null = no predecessor, sums 0)
void launch_absdiff_prev(const uint8_t* gray, const uint8_t* const* prev_dev, double* part /*[n][256]*/, int n, hipStream_t s);
// n 65536-byte gray planes src -> dst (16-byte aligned), one launch
struct PlaneCopy { const uint8_t* src; uint8_t* dst; };
void launch_copy_planes(const PlaneCopy* pairs_dev, int n, hipStream_t s);

}  // namespace dfd

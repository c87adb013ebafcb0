// Launchers and buffer layout of the forensic-signal kernels at an analysis edge S (S % 16 == 0, 32 <= S <= 1024).
// Two instantiations of one set of kernels: the 256x256 chain (edge a compile-time constant, radix-2 FFT spectrum) and
// the general chain (edge a run-time argument, dense MFMA DFT spectrum).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "forensic_score.h"   // ForensicStat: the per-frame scalar statistics produced on the device
#include "imgproc_kernels.h"

namespace dfd {

constexpr int EDGE_MIN = 32, EDGE_MAX = 1024;
inline bool edge_ok(int S) { return S >= EDGE_MIN && S <= EDGE_MAX && S % 16 == 0; }
inline int edge_blocks(int S) { return (S / 32) * (S / 32); }    // 32x32 blocks at i, j in range(0, S - 31, 32)

struct ForensicBuffers {
    uint8_t* rs;         // [n][S][S][3] resized BGR
    uint8_t* gray;       // [n][S*S]
    float2* fft_tmp;     // [n][S*S] row-transform output, transposed
    double* fft_part;    // [n][S][7]   one partial per spectrum row
    short2* grad;        // [n][S*S] Sobel dx,dy
    double* lap_part;    // [n][S][2]   one partial per image row
    uint8_t* map;        // [n][S*S] Canny labels
    double* edge_count;  // [n]
    uint8_t *jy, *jcb, *jcr;   // decoded JPEG planes [n][S*S], [n][S/2 * S/2] x2
    double* hsv_part;    // [n][S][4]   one partial per image row
    unsigned* hue_bits;  // [n][6]
    double* stats;       // [n][FORENSIC_STATS]
    double* stats_noise; // [n][edge_blocks(S)] block stds of the noise residual
    double* stats_ela;   // [n][edge_blocks(S)] block means of the ELA difference
};

// test entries (dfd_forensic_tap, dfd_forensic_tap_sized) only: where the chain starts, and storage for what the kernels
// otherwise keep in LDS or registers
enum ForensicStart { FROM_RS = 0, FROM_GRAY, FROM_GRAD, FROM_MAP };
struct ForensicTaps {
    float2* spectrum;    // [n][S][S] second transform pass, [k1][k2] like fft_tmp
    float* logmag;       // [n][S][S] log1pf(hypotf()) of it: the values the band sums add
    uint8_t* edges;      // [n][S*S] final hysteresis set, 0 / 1
};

size_t forensic_bytes_per_frame(int S);
void forensic_carve(void* base, int S, int n, ForensicBuffers* out);
// S entries exp(-2 pi i j / S), computed in double: the DFT reads all of them, the 256-point FFT the first half
void forensic_table(int S, float2* host_out);
// general = false: the 256x256 chain (S is 256); true: the general chain at edge S.  n frames get every signal;
// `gray_only` further frames (behind them in the buffers) only their gray plane.
hipError_t launch_forensics(const ForensicBuffers& B, bool general, int S, int n, bool full, const ColorTables& T, const float2* table,
                            hipStream_t s, int gray_only = 0, ForensicStart start = FROM_RS, const ForensicTaps* taps = nullptr);
// sum |gray - prev| per image row: part [S]
void launch_absdiff(const uint8_t* gray, const uint8_t* prev, double* part, int S, hipStream_t s);
void launch_absdiff_pairs(const uint8_t* gray, const int* prev_index, double* part /*[n][256]*/, int n, hipStream_t s);
// frames of many streams and edges (device table, one row per frame; max_S: the largest edge in it): frame `gray`
// against `prev` - an earlier frame of its stream in the call, the stream's stored plane, or null (sums 0) - into its S
// partial sums `part`, the doubles launch_absdiff writes.  One launch.
struct DiffRow { const uint8_t* gray; const uint8_t* prev; double* part; int S; int pad; };
void launch_absdiff_prev(const DiffRow* rows_dev, int n, int max_S, hipStream_t s);
// bytes = S * S of the plane (16-byte aligned); one launch for every entry
struct PlaneCopy { const uint8_t* src; uint8_t* dst; size_t bytes; };
void launch_copy_planes(const PlaneCopy* copies_dev, int n, int max_S, hipStream_t s);

}  // namespace dfd

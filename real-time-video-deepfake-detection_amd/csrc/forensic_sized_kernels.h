// Launchers of the forensic-signal kernels at a run-time analysis edge S (S % 16 == 0, 32 <= S <= 1024).
// The buffers are ForensicBuffers / ForensicTaps (forensic_kernels.h) with S in place of 256:
//   rs [n][S][S][3], gray / map / jy [n][S*S], fft_tmp [n][S*S] (transposed row DFT), grad [n][S*S],
//   jcb / jcr [n][S/2 * S/2], fft_part [n][S][7], lap_part [n][S][2], hsv_part [n][S][4] (one partial per image row or
//   spectrum row), stats_noise / stats_ela [n][(S/32)^2] (32x32 blocks at i, j in range(0, S - 31, 32)),
//   taps: spectrum / logmag [n][S][S] ([k1][k2], the layout of fft_tmp), edges [n][S*S].
#pragma once
#include "forensic_kernels.h"

namespace dfd {

constexpr int SIZED_MIN = 32, SIZED_MAX = 1024;
inline bool sized_ok(int S) { return S >= SIZED_MIN && S <= SIZED_MAX && S % 16 == 0; }
inline int sized_blocks(int S) { return (S / 32) * (S / 32); }

size_t forensic_sized_bytes_per_frame(int S);
void forensic_sized_carve(void* base, int S, int n, ForensicBuffers* out);
// table: S entries exp(-2 pi i j / S), computed in double (forensic_sized_table)
void forensic_sized_table(int S, float2* host_out);
hipError_t launch_forensics_sized(const ForensicBuffers& B, int S, int n, bool full, const ColorTables& T, const float2* table,
                                  hipStream_t s, ForensicStart start = FROM_RS, const ForensicTaps* taps = nullptr);
// sum |gray - prev| per image row: part [S]
void launch_absdiff_sized(const uint8_t* gray, const uint8_t* prev, double* part, int S, hipStream_t s);
// frames of many streams and edges (device table, one row per frame; max_S: the largest edge in it): frame `gray`
// against `prev` - an earlier frame of its stream in the call, the stream's stored plane, or null (sums 0) - into its S
// partial sums `part`, the doubles launch_absdiff_sized writes.  One launch.
struct SizedDiffRow { const uint8_t* gray; const uint8_t* prev; double* part; int S; int pad; };
void launch_absdiff_prev_sized(const SizedDiffRow* rows_dev, int n, int max_S, hipStream_t s);
// bytes = S * S of the plane; one launch for every entry
struct SizedPlaneCopy { const uint8_t* src; uint8_t* dst; size_t bytes; };
void launch_copy_planes_sized(const SizedPlaneCopy* copies_dev, int n, int max_S, hipStream_t s);

}  // namespace dfd

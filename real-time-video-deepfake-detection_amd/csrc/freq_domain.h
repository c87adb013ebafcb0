// Frequency-domain analysis at any size (freq_domain.hip): the rectangular, ragged, batched DFT / DCT-II on the fp32
// MFMA behind dfd_frequency_domain* and dfd_frequency_features_sized, and the pieces it shares with freq_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dfd_hip.h"

namespace dfd {

// cv2.cvtColor(BGR2GRAY) on uint8: the one copy of the integer formula (gray_resize_kernel, fd_gather_kernel)
__host__ __device__ __forceinline__ uint8_t bgr_to_gray_u8(int b, int g, int r) {
    return (uint8_t)((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14);
}

constexpr int kFdMaxSide = DFD_FREQ_MAX_SIDE;        // the 4096-entry table is 32 KB of LDS
constexpr int kFdMaxFeatureSize = DFD_FREQ_MAX_FEATURE_SIZE;

// one window of a call: its source rectangle and where its planes lie in the call's work arenas
struct FdWin {
    int x, y, w, h;         // rectangle of the source frame, true sizes
    int wp, hp;             // sides padded to multiples of 16: the gray plane is [hp][wp], the pass-1 output [wp][hp]
    long long gray_off;     // bytes into the gray arena
    long long rows_off;     // float2 elements into the pass-1 arena
    long long tap_off;      // elements into the compact [w][h] tap arrays (test entries only)
};

// freq_kernels.hip: the whole frame as a packed gray plane [sh][sw] (gray_resize_kernel; a gray frame is copied)
void launch_gray_full(const uint8_t* src, int sh, int sw, size_t sstride, int channels, uint8_t* gray_full, hipStream_t s);

struct FreqDomainState;
void freq_domain_destroy(dfd_handle* h);

}  // namespace dfd

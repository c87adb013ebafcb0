// Progressive JPEG scans ON THE DEVICE (option "jpeg_device_progressive").  The files' entropy-coded bytes
// cross PCIe; per (file, scan) they are de-stuffed into a flat byte array, then the scans run level by level:
//
//   * a scan depends only on earlier scans of its file that cover the same component and overlap its band, so the scans
//     of a batch fall into dependency LEVELS (libjpeg's default script: three levels for ten scans) and every ready
//     (file, scan, restart segment) job of a level runs in ONE launch;
//   * DC first, AC first and AC refinement scans are sequential walks - an AC refinement's parse depends on the
//     coefficients the block already holds, so a mis-placed speculative lane never resynchronises and the chunk
//     speculation of the baseline decoder does not carry over.  One job = one lane, running the functions of
//     jpeg_progressive.h as the host decoder runs them.  Throughput comes from the batch;
//   * a DC refinement scan is one bit per block at a position known from the block's index: one thread per unit, no walk.
//
// A job reports a defect into its file's status word; such a file is decoded again by the host path, which gives the
// authoritative status (jpeg_decode.hip).  Every index is bounded whatever the bytes say: the walkers by
// jpeg_progressive.h (coefficient index <= Se, unit < the scan's count, reads inside the scan's de-stuffed bytes), the
// de-stuffing kernel by the scan's raw length (it never writes more bytes than it read) and its segment table's size.
#pragma once
#include "jpeg_progressive.h"

namespace dfd_pjd {

using dfd_pj::PjHuff;
using dfd_pj::PjScan;

constexpr int PJD_DS_THREADS = 256;
constexpr int PJD_WALK_THREADS = 64;
constexpr uint32_t PJD_NONE = 0xffffffffu;

struct PjdScan {
    PjScan g;
    uint32_t file;                               // index into the status words
    uint32_t raw_off, raw_len;                   // the scan's entropy-coded bytes in the uploaded buffer
    uint32_t ds_off;                             // its de-stuffed bytes (capacity raw_len)
    uint32_t seg_off, nseg;                      // segment table: nseg + 1 entries (byte offset of segment k; [nseg]: a marker too many)
    uint32_t per;                                // units per restart segment
    uint32_t tab0;                               // first table of its set
    uint32_t coef_off;                           // the file's planes, int16 elements from the coefficient base
    uint32_t ds_len;                             // written by the de-stuffing kernel
};

struct PjdJob { uint32_t scan, seg; };

// ---- de-stuffing: one workgroup per scan walks its bytes 256 at a time.  FF 00 -> FF; FF D0..D7 removed, the byte
// offset behind marker k recorded as the start of segment k + 1; an FF in front of an FF (fill) and an FF as the last
// byte are dropped - the rules of dfd_jpeg::destuff.  (Every FF starts such a pair or stands alone: the second byte of
// a pair is never FF.)
__global__ __launch_bounds__(PJD_DS_THREADS) void pjd_destuff_kernel(const uint8_t* __restrict__ raw, uint8_t* __restrict__ ds,
                                                                    PjdScan* __restrict__ scans, uint32_t* __restrict__ segtab) {
    __shared__ uint32_t sums[PJD_DS_THREADS];
    PjdScan& S = scans[blockIdx.x];
    const uint32_t len = S.raw_len, nseg = S.nseg;
    const uint8_t* src = raw + S.raw_off;
    uint8_t* dst = ds + S.ds_off;
    uint32_t* seg = segtab + S.seg_off;
    const int tid = threadIdx.x;
    if (tid == 0) seg[0] = 0;
    uint32_t kept_base = 0, mark_base = 0;
    for (uint32_t base = 0; base < len; base += PJD_DS_THREADS) {
        const uint32_t i = base + (uint32_t)tid;
        uint32_t keep = 0, mark = 0;
        uint8_t cur = 0;
        if (i < len) {
            cur = src[i];
            const bool last = i + 1 == len;
            const uint8_t next = last ? (uint8_t)0 : src[i + 1];
            const uint8_t prev = i ? src[i - 1] : (uint8_t)0;
            if (cur == 0xFF) {
                if (!last && next == 0x00) keep = 1;
                else if (!last && (next & 0xF8u) == 0xD0u) mark = 1;
            } else {
                keep = !(prev == 0xFF && (cur == 0x00 || (cur & 0xF8u) == 0xD0u));
            }
        }
        // inclusive prefix sum of (kept | markers << 16): neither field passes 256 per tile
        uint32_t v = keep | (mark << 16);
        sums[tid] = v;
        __syncthreads();
        for (int d = 1; d < PJD_DS_THREADS; d <<= 1) {
            const uint32_t add = tid >= d ? sums[tid - d] : 0u;
            __syncthreads();
            v += add;
            sums[tid] = v;
            __syncthreads();
        }
        const uint32_t total = sums[PJD_DS_THREADS - 1];
        const uint32_t kept_before = kept_base + (v & 0xffffu) - keep, marks_before = mark_base + (v >> 16) - mark;
        if (keep && kept_before < len) dst[kept_before] = cur;
        if (mark && marks_before + 1 <= nseg) seg[marks_before + 1] = kept_before;     // behind the marker: nothing of it is kept
        kept_base += total & 0xffffu;
        mark_base += total >> 16;
        __syncthreads();
    }
    if (tid == 0) S.ds_len = kept_base;
}

// end of segment `k` of a scan: where the next one starts, or the end of the data
__device__ __forceinline__ uint32_t pjd_segment_end(const PjdScan& S, const uint32_t* seg, uint32_t k) {
    const uint32_t e = seg[k + 1];                                  // (the table holds nseg + 1 entries)
    return e == PJD_NONE || e > S.ds_len ? S.ds_len : e;
}

// ---- the walks of one level: one lane per (file, scan, restart segment)
__global__ __launch_bounds__(PJD_WALK_THREADS) void pjd_walk_kernel(const uint8_t* __restrict__ ds, const PjdScan* __restrict__ scans,
                                                                   const PjHuff* __restrict__ tabs, const uint32_t* __restrict__ segtab,
                                                                   const PjdJob* __restrict__ jobs, uint32_t njobs, int16_t* __restrict__ coef,
                                                                   int32_t* __restrict__ status) {
    const uint32_t j = blockIdx.x * PJD_WALK_THREADS + threadIdx.x;
    if (j >= njobs) return;
    const PjdScan& S = scans[jobs[j].scan];
    const uint32_t k = jobs[j].seg;
    if (k >= S.nseg) return;
    const uint32_t* seg = segtab + S.seg_off;
    const uint32_t start = seg[k];
    int st;
    if (start == PJD_NONE || start > S.ds_len) {
        st = dfd_pj::PJ_TRUNCATED;                                  // a restart marker is missing
    } else {
        const uint32_t u0 = k * S.per, u1 = u0 + S.per < S.g.units ? u0 + S.per : S.g.units;
        st = dfd_pj::pj_decode_segment(S.g, tabs + S.tab0, ds + S.ds_off, pjd_segment_end(S, seg, k), (uint64_t)start * 8, u0, u1,
                                       coef + S.coef_off);
    }
    if (st) atomicMax(&status[S.file], st);
}

// ---- DC refinement scans of one level: blockIdx.y = the scan (list[]), one thread per unit
__global__ __launch_bounds__(256) void pjd_dc_refine_kernel(const uint8_t* __restrict__ ds, const PjdScan* __restrict__ scans,
                                                           const uint32_t* __restrict__ segtab, const uint32_t* __restrict__ list,
                                                           int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    const PjdScan& S = scans[list[blockIdx.y]];
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= S.g.units) return;
    const PjScan& g = S.g;
    const uint32_t k = u / S.per, in_seg = u - k * S.per;
    const uint32_t* seg = segtab + S.seg_off;
    const uint32_t start = seg[k];
    if (start == PJD_NONE || start > S.ds_len) { atomicMax(&status[S.file], (int)dfd_pj::PJ_TRUNCATED); return; }
    uint32_t bpu = 0;                                                // blocks (= bits) per unit
    for (int ci = 0; ci < g.ncomp; ++ci) bpu += g.ncomp == 1 ? 1u : (uint32_t)(g.h[ci] * g.v[ci]);
    uint64_t bit = (uint64_t)start * 8 + (uint64_t)in_seg * bpu;
    const uint64_t end = (uint64_t)pjd_segment_end(S, seg, k) * 8;
    const uint8_t* bytes = ds + S.ds_off;
    const uint32_t uy = u / (uint32_t)g.units_x, ux = u - uy * (uint32_t)g.units_x;
    for (int ci = 0; ci < g.ncomp; ++ci) {
        const int hh = g.ncomp == 1 ? 1 : g.h[ci], vv = g.ncomp == 1 ? 1 : g.v[ci];
        for (int by = 0; by < vv; ++by)
            for (int bx = 0; bx < hh; ++bx, ++bit) {
                if (bit >= end) { atomicMax(&status[S.file], (int)dfd_pj::PJ_TRUNCATED); return; }
                const uint32_t b = (bytes[bit >> 3] >> (7u - (uint32_t)(bit & 7))) & 1u;
                dfd_pj::pj_dc_refine_block(dfd_pj::pj_block(g, coef + S.coef_off, ci, uy * (uint32_t)vv + (uint32_t)by, ux * (uint32_t)hh + (uint32_t)bx),
                                           b, g.Al);
            }
    }
}

}  // namespace dfd_pjd

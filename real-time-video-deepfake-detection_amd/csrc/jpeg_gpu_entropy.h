// Entropy decoding of baseline JPEG scans ON THE DEVICE (round 4; SURVEY 8(f) N2, reference backend_server.py:139-145:
// cv2.imdecode = libjpeg).  With the Huffman decoder on host threads a batch of frames had to cross PCIe as 16-bit
// coefficients - as many bytes as the raw frames (6.2 MB per 1080p frame) - and the host managed ~0.9 k frames/s per 16
// cores.  Here the JPEG BYTES cross (0.3-1.2 MB per frame) and the scan is decoded by one lane per 512-byte chunk:
//
//   1. de-stuffing (FF 00 -> FF) as a stream compaction: jg_count_kernel counts the stuffed zeros per 16-KB block and
//      finds the first marker (end of the entropy-coded data), jg_compact_kernel writes the flat byte array - after
//      that a bit position is one integer, as in the host decoder (jpeg_entropy.h);
//   2. the host decoder's speculative chunks as a fixed-point iteration.  A Huffman stream resynchronises after a few
//      symbols, so lane t > 0 decodes chunk t from its first byte AS IF a block of MCU slot 0 began there and records
//      where it ended: the first block boundary (bit position, slot of the next block) at or past the chunk's end
//      (round 0).  In round r every lane takes its predecessor's end state of round r - 1 as its start; a lane whose
//      start did not change keeps its result.  After round r the chunks 0 .. r hold the true decode whatever the data,
//      and on real scans everything is final after round 1 (round 2 .. only confirm, at no cost: whole waves skip).  The
//      rounds count blocks and sum DC differences per component, nothing is written;
//   3. jg_scan_kernel: per frame, prefix sums over the chunks give every chunk its first block index and its DC
//      predictions; it also CHECKS the fixed point (start of chunk t == end of chunk t - 1, slot == block index mod
//      blocks per MCU, block total >= the frame's: what the bits BEHIND the last block decode to is not looked at, and a
//      chunk whose lane met an invalid code / index / DC category IN FRONT of it fails the frame - the lane says in
//      which of its blocks) - a frame that fails any check gets ONE more pass with the round
//      kernel that also iterates inside a launch (RST = true below; jpeg_decode.hip JpegGpuJob::finish): a scan whose
//      codes nearly all have one length hardly resynchronises, and the true state then moves one chunk per launch.  A
//      frame that fails again is decoded by the host path instead;
//   4. jg_emit_kernel decodes every chunk once more from its true start and writes the coefficients (natural order,
//      DC integrated) where the IDCT kernel reads them; the buffer is zeroed first (most coefficients are zero).
//
// Decoding work: three passes over the scan instead of one, on ~2,400 lanes per 1080p frame.  The result does not depend
// on the chunk size or the number of rounds (tests: equal to the host decoder's coefficients, i.e. pinned to libjpeg
// through the oracle's IDCT, and the decoded frames equal Pillow's bit for bit).
//
// RESTART INTERVALS (option "jpeg_device_restart", kernels instantiated with RST = true; a batch without such a file runs
// the RST = false instantiations, which are the code above and nothing else).  An RSTn marker is byte aligned, resets the
// DC predictions and begins at a block index known from the header (segment k: block k * restart * blocks per MCU) - a
// start state that is CERTAIN where the chunk grid has to guess:
//   * de-stuffing removes FF D0..D7 like a stuffed zero (two bytes) and records marker k as seg[k] = (de-stuffed byte
//     offset of the byte behind it) << 3 | n: the bit position of segment k + 1, the marker's number in the low bits.
//     The table holds nseg - 1 entries (nseg from the header); a marker beyond that is counted, never written;
//   * a lane knows the next segment start behind its position (binary search at its start).  When a block completes
//     inside the last byte in front of it - or the decode of a mis-speculated lane has run past it - the lane continues AT
//     that position with slot 0 and DC predictions 0, and what it decodes from there is the true decode.  Chunk grid and
//     memory layout are unchanged.  The RST round kernel also iterates INSIDE a launch over the 256 consecutive chunks of
//     its block (jg_round_kernel): two launches reach the fixed point that took one launch per chunk of propagation.  Per chunk the counting pass also records the first crossing (blocks in front of it,
//     segment index) and sums the DC differences since the LAST crossing: the DC prefix of jg_scan_kernel is a segmented
//     scan, the block prefix a plain one (block indices run on across segments);
//   * checked besides the fixed point: every crossing happens at block k * restart * bpm (first crossing of a chunk:
//     against its block prefix; later ones: exactly restart * bpm blocks since the one before), nseg - 1 markers, marker
//     k numbered k mod 8.  A frame that fails is JG_RESTART and goes to the host decoder like any other.
// More than four distinct Huffman tables, a malformed restart structure and anything the header parser rejects stay on
// the host path; so do restart-interval files while the option is off (the default).  Included by jpeg_decode.hip
// (shares Parsed / ScanLayout / HuffTable with the host decoder).
#pragma once

namespace dfd_jpeg_gpu {

using dfd_jpeg::HuffTable;
using dfd_jpeg::Parsed;
using dfd_jpeg::ScanLayout;

constexpr int JG_LUT_BITS = 12, JG_LUT = 1 << JG_LUT_BITS;
constexpr int JG_TABLES = 4;                     // distinct Huffman tables of a frame (DC + AC)
constexpr int JG_MAX_ROUNDS = 32;                // rounds a call may ask for (option "jpeg_rounds"; the scan kernel verifies the result)
constexpr int JG_DS_THREADS = 256, JG_DS_PIECES = 4, JG_DS_BLOCK = JG_DS_THREADS * JG_DS_PIECES * 16;   // 16 KB per block
constexpr int JG_CB = 256;                       // chunks (lanes) per block of the decode kernels

struct JgTableSet {                              // device image of one frame's Huffman tables
    uint16_t lut[JG_TABLES][JG_LUT];             // (length << 8) | symbol for codes of <= 12 bits, 0 otherwise
    int32_t maxcode[JG_TABLES][4], mincode[JG_TABLES][4], valptr[JG_TABLES][4];   // lengths 13 .. 16
    uint8_t vals[JG_TABLES][256];
};

struct JgFrame {
    uint32_t raw_off, raw_len;                   // the scan's bytes in the uploaded buffer (any alignment: the de-stuffing kernels
                                                 // read whole 16-byte pieces from raw_off & ~15 and skip the bytes in front)
    uint32_t ds_off;                             // its de-stuffed bytes (% 16 == 0, capacity raw_len + 64)
    uint32_t chunk0, nchunks, cblk0;             // chunk range, first chunk block
    uint32_t dsblk0, ndsblk;                     // de-stuffing blocks
    uint32_t coef_off;                           // int16 elements from the coefficient base
    uint32_t tabset;
    int32_t bpm, total_blocks, mcux, chunk_bytes, cw_shift;   // cw_shift = log2(chunk_bytes / 4)
    uint8_t slot_comp[8], slot_bx[8], slot_by[8], slot_dc[8], slot_ac[8];
    int32_t comp_h[3], comp_v[3], comp_bw[3];
    uint32_t comp_off[3];
    uint32_t restart, nseg, seg_off;             // restart interval in MCUs (0: none), its segments, the frame's first entry in the segment table
    // written by the device
    uint32_t marker_pos;                         // raw offset of the first marker (0xffffffff before jg_count_kernel)
    uint32_t nbits;                              // payload bits of the de-stuffed scan
    int32_t status;                              // 0 = decoded; else why not (JgStatus)
    uint32_t blocks_found;
    uint32_t nmark;                              // RSTn markers in front of marker_pos (the table holds the first nseg - 1)
};
enum JgStatus { JG_OK = 0, JG_NOT_CONVERGED = 1, JG_BLOCK_COUNT = 2, JG_BAD_CODE = 3, JG_SLOT = 4, JG_RESTART = 5 };
inline const char* jg_status_name(int st) {
    static const char* const names[] = {"ok", "not converged", "block count", "bad code", "slot", "restart structure"};
    return st < 0 ? "huffman tables" : (st <= JG_RESTART ? names[st] : "?");
}

struct JgChunks {                                // per chunk, structure of arrays
    uint2* st;                                   // start state (bit position, slot)
    uint2* en[2];                                // end state of the last two rounds
    uint32_t* cnt;                               // complete blocks that start in the chunk
    int32_t* dcs;                                // [3] sum of their DC differences per component
    uint32_t* gfirst;                            // first block index (scan kernel)
    int32_t* dcb;                                // [3] DC prediction at the chunk's first block
    uint32_t* err;                               // complete blocks the chunk's decode had in front of its FIRST invalid code /
                                                 // coefficient index / DC category (0xffffffff: it met none)
    uint2* rs;                                   // RST: x = blocks in front of the chunk's first segment crossing | crossed << 31 | a whole
                                                 // segment of another length than restart * bpm << 30, y = index of the segment entered there
    uint32_t* redone;                            // [JG_MAX_ROUNDS] lanes that decoded in round r (diagnostics)
};

// Layout of a frame's de-stuffed scan in memory: CHUNK-INTERLEAVED dwords.  Lane t of a wave walks chunk t one dword at a
// time; stored flat, the 64 lanes of a wave streamed from 64 different cache lines per refill and every refill was an L2
// round trip (measured: 1.9 ms per pass over 64 x 1.2 MB, ~2,500 SIMD cycles per symbol step).  Here dword j of chunk c
// sits at ((c / 64) * CW + j) * 64 + c % 64 (CW = dwords per chunk, a power of two): the 64 lanes of a wave read
// neighbouring dwords of a few lines that stay in the L1 while the lanes drift apart by a few dwords.
__host__ __device__ __forceinline__ uint32_t jg_dword_at(uint32_t g, int cw_shift) {
    const uint32_t c = g >> cw_shift, j = g & ((1u << cw_shift) - 1u);
    return (((c >> 6) << cw_shift) + j) * 64u + (c & 63u);
}

// ---------------------------------------------------------------------------------------------- de-stuffing
// piece q of a block = its bytes [16 q, 16 q + 16): thread t takes the pieces t, t + 256, ... (coalesced 16-byte loads)
// (positions in [lead, raw_len) are the scan; a piece may start in front of it)
// RST (and the frame has a restart interval, `rst`): FF D0..D7 does not end the data - BOTH bytes are removed, each
// counted where it lies (the FF needs the byte behind it: `next` = the first byte of the following piece), and the
// marker is counted where its Dn lies.  A marker may straddle two pieces or two blocks: `prev` / `next` carry it.
__device__ __forceinline__ bool jg_is_rst(uint8_t v) { return (v & 0xF8u) == 0xD0u; }

template <bool RST>
__device__ __forceinline__ void jg_piece_scan(uint32_t lead, uint32_t raw_len, uint32_t pos0, const uint8_t (&b)[16], uint8_t prev,
                                              uint8_t next, bool rst, int* removed, int* markers, uint32_t* marker) {
    int rem = 0, nmk = 0;
    uint32_t mk = 0xffffffffu;
    uint8_t p = prev;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t pos = pos0 + i;
        if (pos == lead) p = 0;                                    // nothing in front of the first byte
        if (pos >= lead && pos < raw_len) {
            if (p == 0xFF) {
                if (b[i] == 0) ++rem;
                else if (RST && rst && jg_is_rst(b[i])) { ++rem; ++nmk; }
                else if (mk == 0xffffffffu) mk = pos - 1;
            }
            if constexpr (RST) {
                const uint8_t nb = i < 15 ? b[i < 15 ? i + 1 : 15] : next;
                if (rst && b[i] == 0xFF && pos + 1 < raw_len && jg_is_rst(nb)) ++rem;   // the FF of a marker
            }
            if (pos + 1 == raw_len && b[i] == 0xFF && mk == 0xffffffffu) mk = pos;   // an FF as the very last byte ends the data too
        }
        p = b[i];
    }
    *removed = rem;
    *markers = nmk;
    *marker = mk;
}

template <bool RST>
__global__ __launch_bounds__(JG_DS_THREADS) void jg_count_kernel(const uint8_t* __restrict__ raw, JgFrame* __restrict__ F,
                                                                 const uint16_t* __restrict__ blk_frame, uint32_t* __restrict__ blk_removed,
                                                                 uint32_t* __restrict__ blk_markers) {
    __shared__ int red[JG_DS_THREADS / 64];
    __shared__ int redm[JG_DS_THREADS / 64];
    const int f = blk_frame[blockIdx.x], tid = threadIdx.x;
    // positions count from the 16-byte boundary in front of the scan: its bytes are [lead, lead + raw_len)
    const uint32_t lead = F[f].raw_off & 15u, raw_len = F[f].raw_len + lead;
    const uint32_t base = (blockIdx.x - F[f].dsblk0) * (uint32_t)JG_DS_BLOCK;
    const uint8_t* scan = raw + (F[f].raw_off - lead);
    const bool rst = RST && F[f].restart != 0;
    int total = 0, totalm = 0;
    uint32_t mk = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < JG_DS_PIECES; ++i) {
        const uint32_t pos0 = base + (uint32_t)(i * JG_DS_THREADS + tid) * 16;
        uint8_t b[16];
        const uint4 v = pos0 < raw_len ? *reinterpret_cast<const uint4*>(scan + pos0) : make_uint4(0, 0, 0, 0);   // (capacity is padded)
        memcpy(b, &v, 16);
        const uint8_t prev = pos0 > lead && pos0 <= raw_len ? scan[pos0 - 1] : 0;
        uint8_t next = 0;
        if constexpr (RST) next = pos0 + 16 < raw_len ? scan[pos0 + 16] : 0;
        int rem, nmk;
        uint32_t m;
        jg_piece_scan<RST>(lead, raw_len, pos0, b, prev, next, rst, &rem, &nmk, &m);
        total += rem;
        totalm += nmk;
        mk = m < mk ? m : mk;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        total += __shfl_xor(total, off);
        if constexpr (RST) totalm += __shfl_xor(totalm, off);
        const uint32_t o = __shfl_xor(mk, off);
        mk = o < mk ? o : mk;
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = total;
        if constexpr (RST) redm[tid >> 6] = totalm;
        if (mk != 0xffffffffu) atomicMin(&F[f].marker_pos, mk);
    }
    __syncthreads();
    if (tid == 0) {
        int s = 0, sm = 0;
        for (int w = 0; w < JG_DS_THREADS / 64; ++w) {
            s += red[w];
            if constexpr (RST) sm += redm[w];
        }
        blk_removed[blockIdx.x] = (uint32_t)s;
        if constexpr (RST) blk_markers[blockIdx.x] = (uint32_t)sm;
    }
}

// (RST: the per-piece counts travel through the block's prefix as ONE integer, removed bytes | markers << 16 - at most
// 16,384 and 8,192 per block)
template <bool RST>
__global__ __launch_bounds__(JG_DS_THREADS) void jg_compact_kernel(const uint8_t* __restrict__ raw, uint8_t* __restrict__ ds,
                                                                   JgFrame* __restrict__ F, const uint16_t* __restrict__ blk_frame,
                                                                   const uint32_t* __restrict__ blk_removed,
                                                                   const uint32_t* __restrict__ blk_markers, uint32_t* __restrict__ segtab) {
    __shared__ int cnt[JG_DS_THREADS * JG_DS_PIECES];            // removed bytes per piece, then their exclusive prefix
    __shared__ int wsum[JG_DS_THREADS / 64 + 1];
    __shared__ int wsumm[JG_DS_THREADS / 64 + 1];
    __shared__ int before, mbefore;
    const int f = blk_frame[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t lead = F[f].raw_off & 15u, raw_len = F[f].raw_len + lead, b0 = F[f].dsblk0;
    const uint32_t base = (blockIdx.x - b0) * (uint32_t)JG_DS_BLOCK;
    const uint8_t* scan = raw + (F[f].raw_off - lead);
    uint8_t* out = ds + F[f].ds_off;
    const int cw_shift = F[f].cw_shift;
    const bool rst = RST && F[f].restart != 0;
    // removed bytes (and markers) in the frame's blocks before this one
    {
        int s = 0, sm = 0;
        for (uint32_t b = b0 + tid; b < blockIdx.x; b += JG_DS_THREADS) {
            s += (int)blk_removed[b];
            if constexpr (RST) sm += (int)blk_markers[b];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s += __shfl_xor(s, off);
            if constexpr (RST) sm += __shfl_xor(sm, off);
        }
        if (lane == 0) {
            wsum[wave] = s;
            if constexpr (RST) wsumm[wave] = sm;
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0, tm = 0;
            for (int w = 0; w < JG_DS_THREADS / 64; ++w) {
                t += wsum[w];
                if constexpr (RST) tm += wsumm[w];
            }
            before = t;
            if constexpr (RST) mbefore = tm;
        }
        __syncthreads();
    }
    uint8_t b[JG_DS_PIECES][16];
    uint8_t prev[JG_DS_PIECES], next[JG_DS_PIECES];
#pragma unroll
    for (int i = 0; i < JG_DS_PIECES; ++i) {
        const uint32_t pos0 = base + (uint32_t)(i * JG_DS_THREADS + tid) * 16;
        const uint4 v = pos0 < raw_len ? *reinterpret_cast<const uint4*>(scan + pos0) : make_uint4(0, 0, 0, 0);
        memcpy(b[i], &v, 16);
        prev[i] = pos0 > lead && pos0 <= raw_len ? scan[pos0 - 1] : 0;
        next[i] = 0;
        if constexpr (RST) next[i] = pos0 + 16 < raw_len ? scan[pos0 + 16] : 0;
        int rem, nmk;
        uint32_t m;
        jg_piece_scan<RST>(lead, raw_len, pos0, b[i], prev[i], next[i], rst, &rem, &nmk, &m);
        cnt[i * JG_DS_THREADS + tid] = RST ? rem | (nmk << 16) : rem;
    }
    __syncthreads();
    // exclusive prefix over the 1024 pieces in byte order: thread t scans the pieces 4 t .. 4 t + 3, then the block
    int mine[JG_DS_PIECES], tot = 0;
#pragma unroll
    for (int i = 0; i < JG_DS_PIECES; ++i) { mine[i] = tot; tot += cnt[JG_DS_PIECES * tid + i]; }
    int incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wsum[w];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < JG_DS_PIECES; ++i) cnt[JG_DS_PIECES * tid + i] = wbase + incl - tot + mine[i];
    __syncthreads();
    const uint32_t end = F[f].marker_pos < raw_len ? F[f].marker_pos : raw_len;   // one past the last payload byte
    const uint32_t cap = RST && rst ? F[f].nseg - 1u : 0u;       // entries of the frame's segment table (nseg >= 1)
    uint32_t* seg = RST ? segtab + F[f].seg_off : nullptr;
#pragma unroll
    for (int i = 0; i < JG_DS_PIECES; ++i) {
        const int q = i * JG_DS_THREADS + tid;
        const uint32_t pos0 = base + (uint32_t)q * 16;
        if (pos0 >= raw_len) continue;
        // output index of the piece's first scan byte: scan bytes in front of it minus the removed ones among them
        uint32_t o = (pos0 > lead ? pos0 - lead : 0u) - (uint32_t)before - (uint32_t)(RST ? cnt[q] & 0xffff : cnt[q]);
        uint32_t mi = RST ? (uint32_t)mbefore + ((uint32_t)cnt[q] >> 16) : 0u;   // index of the piece's first marker
        uint8_t p = prev[i];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t pos = pos0 + k;
            if (pos == lead) p = 0;
            if (pos >= lead && pos < raw_len) {
                bool gone = p == 0xFF && b[i][k] == 0;
                if constexpr (RST) {
                    if (rst) {
                        if (p == 0xFF && jg_is_rst(b[i][k])) {   // marker mi: the next segment begins at output byte o
                            gone = true;
                            if (pos < end && mi < cap) seg[mi] = (o << 3) | (uint32_t)(b[i][k] & 7u);
                            ++mi;
                        }
                        const uint8_t nb = k < 15 ? b[i][k < 15 ? k + 1 : 15] : next[i];
                        if (b[i][k] == 0xFF && pos + 1 < raw_len && jg_is_rst(nb)) gone = true;
                    }
                }
                if (!gone) { out[4u * jg_dword_at(o >> 2, cw_shift) + (o & 3u)] = b[i][k]; ++o; }
                if (pos + 1 == end) {
                    F[f].nbits = 8u * o;                           // (end == 0: set by the host to 0 beforehand)
                    if constexpr (RST) F[f].nmark = mi;
                }
            }
            p = b[i][k];
        }
    }
}

// ---------------------------------------------------------------------------------------------- the decoder
struct JgLds {
    JgTableSet tab;
    JgFrame fr;
    uint4 slot[8];                               // per MCU slot: coefficient offset of its block in MCU (0, 0), per MCU row, per MCU column
    uint8_t zigzag[64];
};

__device__ __forceinline__ int jg_extend(uint32_t v, int s) {
    return s == 0 ? 0 : ((int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v);
}

// Decodes blocks from bit position p0 (slot z0) of the de-stuffed scan `ds`: !EMIT - up to the first block boundary at
// or past `pend`; EMIT - exactly `want` blocks, written to coef.  Counts only COMPLETE blocks (every bit inside nbits).
// RST: `seg` = the frame's segment table (nvalid entries written), segblocks = restart * bpm.  The lane carries the bit
// position of the next segment start behind its own position; the test sits in the block-complete branch, the symbol
// path is the one of RST = false.  !EMIT: dsum comes back as the sums since the LAST crossing, *rs_out as JgChunks::rs.
// *bad_out: as JgChunks::err - WHERE the first defect lies, in blocks, so that the scan kernel can tell a defect inside a
// block of the frame from the bits behind its last block.  The symbol path only raises a flag, as it always did; the
// block-complete branch counts the blocks that end with the flag up - one add, no branch (with 64 lanes some lane
// completes a block in nearly every step: whatever stands there is paid per symbol) - and the first of them is block
// n - that count.  (A lane ends at a block boundary, or where the data ends - and a frame whose data ends inside a block
// fails on its block count.)
template <bool EMIT, bool RST>
__device__ __forceinline__ void jg_decode(const JgLds& L, const uint32_t* __restrict__ ds, uint32_t nbits, uint32_t p0, int z0,
                                          uint32_t pend, uint32_t want, uint32_t* p_out, int* z_out, uint32_t* n_out, int (&dsum)[3],
                                          uint32_t* bad_out, int16_t* __restrict__ coef, uint32_t g0, const int (&pred0)[3],
                                          const uint32_t* __restrict__ seg, uint32_t nvalid, uint32_t segblocks, uint2* rs_out) {
    const int bpm = L.fr.bpm, cws = L.fr.cw_shift;
    // slot -> DC table / AC table / component as nibbles of three registers: no LDS read on the symbol loop's critical path
    uint32_t dcmap = 0, acmap = 0, cmap = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        dcmap |= (uint32_t)L.fr.slot_dc[i] << (4 * i);
        acmap |= (uint32_t)L.fr.slot_ac[i] << (4 * i);
        cmap |= (uint32_t)L.fr.slot_comp[i] << (4 * i);
    }
    uint32_t idx = p0 >> 5;
    uint64_t buf = ((uint64_t)__builtin_bswap32(ds[jg_dword_at(idx, cws)]) << 32 | __builtin_bswap32(ds[jg_dword_at(idx + 1, cws)])) << (p0 & 31);
    int have = 64 - (int)(p0 & 31);
    // The next dword of the lane's stream is requested in EVERY step (all lanes, whether the last one was consumed or
    // not) and used one step later: a refill under `if (have < 32)` made the whole wave wait for the load of whichever lane
    // refilled last - a memory round trip in every step of every wave.
    uint32_t ridx = idx + 2;
    uint32_t wnext = ds[jg_dword_at(ridx, cws)];
    uint32_t p = p0, pb = p0, n = 0;                              // pb: position of the last block boundary
    int z = z0, k = 0;
    bool bad = false;
    uint32_t nbad = 0;                                             // blocks completed with `bad` up
    int pred[3] = {pred0[0], pred0[1], pred0[2]};
    // RST: entry sidx of the table is the first segment start behind p0 (0xffffffff: none, p + 7 never reaches it)
    uint32_t sidx = 0, nextseg = 0xffffffffu, rs_before = 0, rs_seg = 0, nlast = 0;
    if constexpr (RST) {
        uint32_t lo = 0, hi = nvalid;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((seg[mid] & ~7u) > p0) hi = mid; else lo = mid + 1;
        }
        sidx = lo;
        if (sidx < nvalid) nextseg = seg[sidx] & ~7u;
    }
    // EMIT: where the current block goes, and - computed while it is decoded, off the loop's critical path - the next one
    uint32_t mx = 0, my = 0, dst = 0, dstn = 0;
    int zn = z0;
    auto block_at = [&](int zz) {
        const uint4 sl = L.slot[zz];
        return sl.x + my * sl.y + mx * sl.z;
    };
    auto advance = [&]() {                                         // (zn, mx, my) -> the block after it
        if (++zn == bpm) {
            zn = 0;
            if (++mx == (uint32_t)L.fr.mcux) { mx = 0; ++my; }
        }
    };
    if constexpr (EMIT) {
        const uint32_t mcu = g0 / (uint32_t)bpm;
        my = mcu / (uint32_t)L.fr.mcux;
        mx = mcu - my * (uint32_t)L.fr.mcux;
        dst = block_at(zn);
        advance();
        dstn = block_at(zn);
    }
    // One symbol.  Returns false when the lane is done (block count / chunk end reached, or the data ended); a coefficient
    // to store comes back as (eo, ev) - eo = 0xffffffff: none.
    auto step = [&](uint32_t& eo, int& ev) -> bool {
        eo = 0xffffffffu;
        ev = 0;
        if (EMIT ? n >= want : (k == 0 && p >= pend)) return false;
        if (p >= nbits) return false;                              // data ended inside a block (or before the next one)
        if (have <= 32) {
            buf |= (uint64_t)__builtin_bswap32(wnext) << (32 - have);
            have += 32;
            ++ridx;
        }
        wnext = ds[jg_dword_at(ridx, cws)];
        const bool isdc = k == 0;
        const int tb = (int)(((isdc ? dcmap : acmap) >> (4 * z)) & 15u);
        const uint32_t code = (uint32_t)(buf >> 48);
        uint32_t e = L.tab.lut[tb][code >> (16 - JG_LUT_BITS)];
        if (e == 0) {                                              // a code of 13 .. 16 bits (rare), or none
            e = (16u << 8);
            bool found = false;
#pragma unroll
            for (int l = 13; l <= 16; ++l) {
                const int c = (int)(code >> (16 - l));
                if (!found && c <= L.tab.maxcode[tb][l - 13]) {
                    found = true;
                    e = ((uint32_t)l << 8) | L.tab.vals[tb][(L.tab.valptr[tb][l - 13] + c - L.tab.mincode[tb][l - 13]) & 255];
                }
            }
            bad |= !found;
        }
        const int len = (int)(e >> 8), rs = (int)(e & 255);
        int s = isdc ? rs : (rs & 15);
        const int r = isdc ? 0 : (rs >> 4);
        if (isdc && s > 11) { bad = true; s &= 7; }                // (an 8-bit file has no DC category above 11)
        const uint32_t v = s ? (uint32_t)((buf << len) >> (64 - s)) : 0u;
        const int used = len + s;
        buf <<= used;
        have -= used;
        p += (uint32_t)used;
        if (p > nbits) return false;                               // the symbol ran past the data: not a block
        if (isdc) {
            const int c = (int)((cmap >> (4 * z)) & 15u);
            const int d = jg_extend(v, s);
            dsum[c] += d;
            if constexpr (EMIT) {
                pred[c] += d;
                eo = dst;
                ev = pred[c];
            }
            k = 1;
        } else if (s == 0) {
            k = r == 15 ? k + 16 : 64;
        } else {
            k += r;
            if (k > 63) { bad = true; k = 64; }
            else {
                if constexpr (EMIT) {
                    eo = dst + L.zigzag[k];
                    ev = jg_extend(v, s);
                }
                ++k;
            }
        }
        if (k >= 64) {                                             // block complete
            nbad += bad ? 1u : 0u;
            k = 0;
            ++n;
            pb = p;
            if (++z == bpm) z = 0;
            if constexpr (EMIT) {
                dst = dstn;
                advance();
                dstn = block_at(zn);
            }
            if constexpr (RST) {
                // the block ended inside the last byte in front of the next segment and only padding follows (1-bits: no
                // Huffman code consists of ones alone, and a block of a flat area can be as short as 4 bits - the segment's
                // last blocks may all lie in that byte), or, mis-speculated, behind its start: on at that byte with slot 0
                // and predictions 0.  (EMIT runs on verified frames only: every crossing is at a whole number of MCUs, the
                // destination pipeline above is already where the segment begins.)
                bool cross = p + 7u >= nextseg;
                if (cross && p < nextseg) {
                    const uint32_t last = (nextseg >> 3) - 1u, pad = (1u << (nextseg - p)) - 1u;
                    cross = ((ds[jg_dword_at(last >> 2, cws)] >> (8u * (last & 3u))) & pad) == pad;
                }
                if (cross) {
                    if constexpr (!EMIT) {
                        if (!(rs_before >> 31)) { rs_before = n | 0x80000000u; rs_seg = sidx + 1u; }
                        else if (n - nlast != segblocks) rs_before |= 0x40000000u;
                        nlast = n;
                        dsum[0] = dsum[1] = dsum[2] = 0;
                    } else {
                        pred[0] = pred[1] = pred[2] = 0;
                    }
                    p = pb = nextseg;
                    z = 0;
                    ++sidx;
                    nextseg = sidx < nvalid ? seg[sidx] & ~7u : 0xffffffffu;
                    idx = p >> 5;
                    buf = ((uint64_t)__builtin_bswap32(ds[jg_dword_at(idx, cws)]) << 32 | __builtin_bswap32(ds[jg_dword_at(idx + 1, cws)])) << (p & 31);
                    have = 64 - (int)(p & 31);
                    ridx = idx + 2;
                    wnext = ds[jg_dword_at(ridx, cws)];
                }
            }
        }
        return true;
    };
    if constexpr (!EMIT) {
        uint32_t eo;
        int ev;
        while (step(eo, ev)) {}
    } else {
        // Stores count in vmcnt like loads and retire in order: with a 2-byte store in every step, the wait for the stream's
        // next dword at the top of the following step was a wait for that store's round trip (measured: the emit pass 3.5 x
        // a counting pass).  Sixteen steps keep their coefficients in registers and store them together: one such wait per
        // sixteen symbols.
        constexpr int G = 16;
        bool live = true;
        while (live) {
            uint32_t eo[G];
            int ev[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                eo[u] = 0xffffffffu;
                ev[u] = 0;
                if (live) live = step(eo[u], ev[u]);
            }
#pragma unroll
            for (int u = 0; u < G; ++u)
                if (eo[u] != 0xffffffffu) coef[eo[u]] = (int16_t)ev[u];
        }
    }
    *p_out = pb;
    *z_out = z;
    *n_out = n;
    *bad_out = nbad ? n - nbad : 0xffffffffu;
    if constexpr (RST && !EMIT) *rs_out = make_uint2(rs_before, rs_seg);
}

// entries of the frame's segment table that jg_compact_kernel has written (0 for a file without restart interval)
__device__ __forceinline__ uint32_t jg_seg_valid(const JgFrame& fr) {
    if (fr.restart == 0) return 0u;
    return fr.nmark < fr.nseg - 1u ? fr.nmark : fr.nseg - 1u;
}

__device__ __forceinline__ void jg_load_lds(JgLds& L, const JgFrame* F, const JgTableSet* T, int f) {
    const int tid = threadIdx.x;
    {
        const uint4* src = reinterpret_cast<const uint4*>(&T[F[f].tabset]);
        uint4* dst = reinterpret_cast<uint4*>(&L.tab);
        for (int i = tid; i < (int)(sizeof(JgTableSet) / 16); i += JG_CB) dst[i] = src[i];
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&F[f]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&L.fr);
        for (int i = tid; i < (int)(sizeof(JgFrame) / 4); i += JG_CB) dst[i] = src[i];
    }
    if (tid < 64) L.zigzag[tid] = dfd::kJpegZigzag[tid];
    __syncthreads();
    if (tid < 8) {
        const int z = tid < L.fr.bpm ? tid : 0, c = L.fr.slot_comp[z];
        L.slot[tid] = make_uint4(L.fr.coef_off + L.fr.comp_off[c] + ((uint32_t)L.fr.slot_by[z] * (uint32_t)L.fr.comp_bw[c] + L.fr.slot_bx[z]) * 64u,
                                 (uint32_t)L.fr.comp_v[c] * (uint32_t)L.fr.comp_bw[c] * 64u, (uint32_t)L.fr.comp_h[c] * 64u, 0u);
    }
    __syncthreads();
}

// One round.  RST = false: one decode per lane, as described at the top.
// RST = true: the 256 lanes of a block are 256 CONSECUTIVE chunks, so the iteration also runs INSIDE the launch - after
// its decode a lane looks at the end state its left neighbour has just written to LDS, and decodes again if that is not
// the state it started from; up to JG_INNER times, ending as soon as no lane of the block has anything to redo (a
// converged block: one look, no decode).  Only a block's first lane waits for the next launch.  Round 0 thus settles every
// block up to its first lane's guess, round 1 hands each first lane the true state: two launches reach the fixed point
// where lane-per-launch propagation needed one per chunk a guess takes to fall into step.  What is stored per chunk is
// what the last decode of the lane gave - the scan kernel checks exactly the same relations as before.
constexpr int JG_INNER = 16;

template <bool RST>
__global__ __launch_bounds__(JG_CB) void jg_round_kernel(const uint8_t* __restrict__ ds_base, const JgFrame* __restrict__ F,
                                                         const JgTableSet* __restrict__ T, const uint16_t* __restrict__ cblk_frame,
                                                         JgChunks S, int round, const uint32_t* __restrict__ segtab) {
    __shared__ __attribute__((aligned(16))) JgLds L;
    const int f = cblk_frame[blockIdx.x];
    jg_load_lds(L, F, T, f);
    const uint32_t t = (blockIdx.x - L.fr.cblk0) * JG_CB + threadIdx.x, gt = L.fr.chunk0 + t;
    const uint32_t nbits = L.fr.nbits, cbits = (uint32_t)L.fr.chunk_bytes * 8u;
    const uint32_t b0 = t * cbits;
    if constexpr (!RST) {
        if (t >= L.fr.nchunks || b0 >= nbits) return;                 // (chunks past the payload take no part)
        const uint32_t b1 = b0 + cbits < nbits ? b0 + cbits : nbits;
        uint2 start;
        if (t == 0) start = make_uint2(0u, 0u);
        else if (round == 0) start = make_uint2(b0, 0u);
        else start = S.en[(round - 1) & 1][gt - 1];
        if (round > 0) {
            const uint2 old = S.st[gt];
            if (old.x == start.x && old.y == start.y) { S.en[round & 1][gt] = S.en[(round - 1) & 1][gt]; return; }
        }
        S.st[gt] = start;
        {   // diagnostics: lanes that decode in this round (one atomic per wave)
            const unsigned long long m = __ballot(1);
            if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1u) atomicAdd(&S.redone[round], (uint32_t)__popcll(m));
        }
        uint32_t pe = start.x, n = 0;
        int ze = (int)start.y, dsum[3] = {0, 0, 0};
        uint32_t bad = 0xffffffffu;
        const int zero3[3] = {0, 0, 0};
        if (start.x < b1)
            jg_decode<false, false>(L, reinterpret_cast<const uint32_t*>(ds_base + L.fr.ds_off), nbits, start.x, (int)start.y, b1, 0u, &pe, &ze,
                                    &n, dsum, &bad, nullptr, 0u, zero3, nullptr, 0u, 0u, nullptr);
        S.en[round & 1][gt] = make_uint2(pe, (uint32_t)ze);
        S.cnt[gt] = n;
        S.dcs[3 * gt] = dsum[0];
        S.dcs[3 * gt + 1] = dsum[1];
        S.dcs[3 * gt + 2] = dsum[2];
        S.err[gt] = bad;
    } else {
        __shared__ uint2 ends[JG_CB];                                // the lanes' current end states
        const bool active = t < L.fr.nchunks && b0 < nbits;          // (the active chunks of a frame are its first ones)
        const uint32_t b1 = b0 + cbits < nbits ? b0 + cbits : nbits;
        uint2 start = make_uint2(0u, 0u), end = make_uint2(0u, 0u);
        bool need = false;
        if (active) {
            if (t == 0) start = make_uint2(0u, 0u);
            else if (round == 0) start = make_uint2(b0, 0u);
            else start = S.en[(round - 1) & 1][gt - 1];
            need = true;
            if (round > 0) {
                const uint2 old = S.st[gt];
                if (old.x == start.x && old.y == start.y) { need = false; end = S.en[(round - 1) & 1][gt]; }
            }
        }
        for (int it = 0; it < JG_INNER; ++it) {
            if (need) {
                S.st[gt] = start;
                const unsigned long long m = __ballot(1);              // diagnostics: decodes of this round, inner ones included
                if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1u) atomicAdd(&S.redone[round], (uint32_t)__popcll(m));
                uint32_t pe = start.x, n = 0;
                int ze = (int)start.y, dsum[3] = {0, 0, 0};
                uint32_t bad = 0xffffffffu;
                const int zero3[3] = {0, 0, 0};
                uint2 rs = make_uint2(0u, 0u);
                if (start.x < b1)
                    jg_decode<false, true>(L, reinterpret_cast<const uint32_t*>(ds_base + L.fr.ds_off), nbits, start.x, (int)start.y, b1, 0u, &pe,
                                           &ze, &n, dsum, &bad, nullptr, 0u, zero3, segtab + L.fr.seg_off, jg_seg_valid(L.fr),
                                           L.fr.restart * (uint32_t)L.fr.bpm, &rs);
                end = make_uint2(pe, (uint32_t)ze);
                S.cnt[gt] = n;
                S.dcs[3 * gt] = dsum[0];
                S.dcs[3 * gt + 1] = dsum[1];
                S.dcs[3 * gt + 2] = dsum[2];
                S.err[gt] = bad;
                S.rs[gt] = rs;
            }
            ends[threadIdx.x] = end;
            __syncthreads();
            need = false;
            if (active && threadIdx.x > 0 && t > 0) {                 // (t > 0 and not the block's first lane: the chunk in front is this block's)
                const uint2 pred = ends[threadIdx.x - 1];
                if (pred.x != start.x || pred.y != start.y) { start = pred; need = true; }
            }
            if (!__syncthreads_or(need ? 1 : 0)) break;
        }
        if (active) S.en[round & 1][gt] = end;
    }
}

// one 1024-thread block per frame: prefix sums over its chunks + the checks of the fixed point.
// A frame with a restart interval: the DC prefix is a SEGMENTED scan - element (crossed, sums since the last crossing),
// (f1, v1) + (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2) - so that a chunk's dcb is the sum since the last segment start; the
// block prefix stays plain.  Then the restart checks (header comment) per chunk and per table entry.
__global__ __launch_bounds__(1024) void jg_scan_kernel(JgFrame* __restrict__ F, JgChunks S, int last_round, const uint32_t* __restrict__ segtab) {
    __shared__ int wsum[16][4];
    __shared__ int wflag[16];
    __shared__ int carry[4];
    __shared__ int status, rstatus;                               // (a restart verdict counts only at the fixed point: reported after the others)
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const JgFrame fr = F[f];
    const bool rst = fr.restart != 0;
    const uint32_t segblocks = fr.restart * (uint32_t)fr.bpm;
    const uint32_t cbits = (uint32_t)fr.chunk_bytes * 8u;
    const uint32_t nvalid = fr.nbits ? (fr.nbits + cbits - 1) / cbits : 0u;
    if (tid < 4) carry[tid] = 0;
    if (tid == 0) { status = JG_OK; rstatus = JG_OK; }
    __syncthreads();
    const uint2* en = S.en[last_round & 1];
    for (uint32_t t0 = 0; t0 < nvalid; t0 += 1024) {
        const uint32_t t = t0 + tid, gt = fr.chunk0 + t;
        const bool live = t < nvalid;
        int v[4] = {0, 0, 0, 0};
        uint2 rs = make_uint2(0u, 0u);
        if (live) {
            v[0] = (int)S.cnt[gt];
            v[1] = S.dcs[3 * gt];
            v[2] = S.dcs[3 * gt + 1];
            v[3] = S.dcs[3 * gt + 2];
            if (rst) rs = S.rs[gt];
        }
        const int fl = (int)(rs.x >> 31);                          // the chunk crossed a segment start
        int incl[4], ifl = fl;
#pragma unroll
        for (int c = 0; c < 4; ++c) incl[c] = v[c];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int of = __shfl_up(ifl, off);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int o = __shfl_up(incl[c], off);
                if (lane >= off && (c == 0 || !ifl)) incl[c] += o;
            }
            if (lane >= off) ifl |= of;
        }
        if (lane == 63) {
#pragma unroll
            for (int c = 0; c < 4; ++c) wsum[wave][c] = incl[c];
            wflag[wave] = ifl;
        }
        __syncthreads();
        // exclusive: (carry + the waves before) + (the lanes before in this wave)
        int excl[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) excl[c] = carry[c];
        for (int w = 0; w < wave; ++w) {
            excl[0] += wsum[w][0];
#pragma unroll
            for (int c = 1; c < 4; ++c) excl[c] = wflag[w] ? wsum[w][c] : excl[c] + wsum[w][c];
        }
        {
            int ef = __shfl_up(ifl, 1);
            if (lane == 0) ef = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                int e = __shfl_up(incl[c], 1);
                if (lane == 0) e = 0;
                excl[c] = (c > 0 && ef) ? e : excl[c] + e;
            }
        }
        if (live) {
            S.gfirst[gt] = (uint32_t)excl[0];
            S.dcb[3 * gt] = excl[1];
            S.dcb[3 * gt + 1] = excl[2];
            S.dcb[3 * gt + 2] = excl[3];
            // the fixed point: this chunk started where its predecessor ended, in the slot its block index says
            const uint2 st = S.st[gt];
            const uint2 want = t == 0 ? make_uint2(0u, 0u) : en[gt - 1];
            int bad = JG_OK;
            if (st.x != want.x || st.y != want.y) bad = JG_NOT_CONVERGED;
            else if ((uint32_t)excl[0] % (uint32_t)fr.bpm != st.y) bad = JG_SLOT;
            // a defect inside one of the frame's blocks, wherever its chunk lies (what follows the LAST block - padding bits,
            // stray bytes in front of EOI - decodes to anything and is nobody's business: the host decoder does not look either)
            else if (S.err[gt] != 0xffffffffu && (uint32_t)excl[0] + S.err[gt] < (uint32_t)fr.total_blocks) bad = JG_BAD_CODE;
            // the chunk's first crossing lies at the first block of the segment entered there; its later ones a whole segment on
            else if (fl && ((rs.x & 0x40000000u) || (uint32_t)excl[0] + (rs.x & 0x3fffffffu) != rs.y * segblocks)) atomicMax(&rstatus, (int)JG_RESTART);
            if (bad) atomicMax(&status, bad);
        }
        __syncthreads();
        if (tid == 1023) {
            carry[0] = excl[0] + v[0];
#pragma unroll
            for (int c = 1; c < 4; ++c) carry[c] = fl ? v[c] : excl[c] + v[c];
        }
        __syncthreads();
    }
    if (rst) {
        // as many markers as the header says, numbered 0 .. 7 in turn (nmark == nseg - 1: every entry was written)
        int bad = fr.nmark != fr.nseg - 1u ? JG_RESTART : JG_OK;
        if (!bad)
            for (uint32_t k = tid; k < fr.nseg - 1u; k += 1024)
                if ((segtab[fr.seg_off + k] & 7u) != (k & 7u)) bad = JG_RESTART;
        if (bad) atomicMax(&rstatus, bad);
        __syncthreads();
    }
    if (tid == 0) {
        int st = status;
        if (st == JG_OK) st = rstatus;
        if (st == JG_OK && carry[0] < fr.total_blocks) st = JG_BLOCK_COUNT;   // (more: bits behind the last block made a block; emit stops at the total)
        F[f].status = st;
        F[f].blocks_found = (uint32_t)carry[0];
    }
}

template <bool RST>
__global__ __launch_bounds__(JG_CB) void jg_emit_kernel(const uint8_t* __restrict__ ds_base, const JgFrame* __restrict__ F,
                                                        const JgTableSet* __restrict__ T, const uint16_t* __restrict__ cblk_frame,
                                                        JgChunks S, int16_t* __restrict__ coef, const uint32_t* __restrict__ segtab) {
    __shared__ __attribute__((aligned(16))) JgLds L;
    const int f = cblk_frame[blockIdx.x];
    jg_load_lds(L, F, T, f);
    if (L.fr.status != JG_OK) return;
    const uint32_t t = (blockIdx.x - L.fr.cblk0) * JG_CB + threadIdx.x, gt = L.fr.chunk0 + t;
    const uint32_t nbits = L.fr.nbits, cbits = (uint32_t)L.fr.chunk_bytes * 8u;
    if (t >= L.fr.nchunks || t * cbits >= nbits) return;
    // (blocks at or behind the frame's total are what the bits behind its last block happened to decode to: never written)
    const uint32_t g0 = S.gfirst[gt], total = (uint32_t)L.fr.total_blocks;
    if (g0 >= total) return;
    const uint32_t want = S.cnt[gt] < total - g0 ? S.cnt[gt] : total - g0;
    if (want == 0) return;
    const uint2 start = S.st[gt];
    const int pred0[3] = {S.dcb[3 * gt], S.dcb[3 * gt + 1], S.dcb[3 * gt + 2]};
    uint32_t pe, n;
    int ze, dsum[3] = {0, 0, 0};
    uint32_t bad;
    jg_decode<true, RST>(L, reinterpret_cast<const uint32_t*>(ds_base + L.fr.ds_off), nbits, start.x, (int)start.y, 0u, want, &pe, &ze, &n, dsum,
                         &bad, coef, g0, pred0, RST ? segtab + L.fr.seg_off : nullptr, jg_seg_valid(L.fr),
                         L.fr.restart * (uint32_t)L.fr.bpm, nullptr);
}

// ---------------------------------------------------------------------------------------------- host side
// device image of a parsed file's tables; false: more than JG_TABLES distinct tables
inline bool jg_build_tables(const Parsed& P, JgTableSet* ts, uint8_t (&slot_dc)[8], uint8_t (&slot_ac)[8], const ScanLayout& L) {
    const HuffTable* used[JG_TABLES];
    int nused = 0;
    auto index_of = [&](const HuffTable* t) {
        for (int i = 0; i < nused; ++i)
            if (used[i] == t) return i;
        if (nused == JG_TABLES) return -1;
        used[nused] = t;
        return nused++;
    };
    for (int s = 0; s < L.bpm; ++s) {
        const dfd_jpeg::Component& C = P.comp[L.slot_comp[s]];
        const int d = index_of(&P.dc[C.td]), a = index_of(&P.ac[C.ta]);
        if (d < 0 || a < 0) return false;
        slot_dc[s] = (uint8_t)d;
        slot_ac[s] = (uint8_t)a;
    }
    memset(ts, 0, sizeof *ts);
    for (int i = 0; i < nused; ++i) {
        const HuffTable& H = *used[i];
        memcpy(ts->vals[i], H.vals, 256);
        for (int l = 1; l <= 16; ++l) {
            if (H.maxcode[l] < 0) { if (l >= 13) { ts->maxcode[i][l - 13] = -1; } continue; }
            if (l >= 13) {
                ts->maxcode[i][l - 13] = H.maxcode[l];
                ts->mincode[i][l - 13] = H.mincode[l];
                ts->valptr[i][l - 13] = H.valptr[l];
                continue;
            }
            for (int code = H.mincode[l]; code <= H.maxcode[l]; ++code) {
                const int sym = H.vals[(H.valptr[l] + code - H.mincode[l]) & 255];
                const int base = code << (JG_LUT_BITS - l);
                for (int fill = 0; fill < (1 << (JG_LUT_BITS - l)); ++fill) ts->lut[i][base + fill] = (uint16_t)((l << 8) | sym);
            }
        }
        for (int l = 13; l <= 16; ++l)
            if (H.maxcode[l] < 0) ts->maxcode[i][l - 13] = -1;
    }
    return true;
}

// can this parsed file take the device path?
// (restart-interval files only when the handle's option "jpeg_device_restart" allows them)
inline uint32_t jg_segments(const Parsed& P, const ScanLayout& L) {
    return P.restart ? (uint32_t)(((size_t)L.mcux * L.mcuy + P.restart - 1) / P.restart) : 1u;
}
inline bool jg_supported(const Parsed& P, const ScanLayout& L, bool restart_ok) {
    return (P.restart == 0 || restart_ok) && L.bpm <= 8 && (size_t)(P.end - P.scan) < ((size_t)1 << 30);
}

}  // namespace dfd_jpeg_gpu

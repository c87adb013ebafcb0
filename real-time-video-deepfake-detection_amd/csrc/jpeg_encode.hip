// Baseline JPEG encode on the device: pixels -> the bytes libjpeg(-turbo) writes for them with its defaults and the Annex K
// Huffman tables (include/dfd_hip.h "baseline JPEG encode"; the mirror image of jpeg_gpu_entropy.h, where
// de-stuffing was a stream compaction and stuffing is a stream expansion).  One chain of launches per batch of images of any
// sizes and modes; every index below runs over the whole batch and finds its image by a binary search over the per-image
// first-block / first-interval tables, so an image's bytes cannot depend on its neighbours or on the launch geometry.
//
//   enc_block_kernel     a lane per 8x8 block, in the order the scan codes them (MCU-interleaved): jccolor.c colour
//                        conversion, jcprepct.c / jcsample.c edge replication and h2v1 / h2v2 downsampling, jfdctint.c
//                        FDCT, jcdctmgr.c quantisation -> int16 coefficients in zig-zag order.  The blocks an interleaved
//                        MCU has beyond the component's real ones (jccoefct.c) carry the DC of the block before them.
//   enc_length_kernel    a lane per block: DC difference against the previous block of its component (0 at the start of a
//                        restart interval), then the exact number of bits the block codes to
//   scan (3 launches)    exclusive prefix sum u32 -> u64 over any number of workgroups: tile sums, one workgroup over the
//                        tile sums, tiles again with their offsets.  Used three times: bits per block, bytes per restart
//                        interval (each interval is byte-aligned), FF bytes per chunk.
//   enc_emit_kernel      a lane per block ORs its bits (vector atomicOr, MSB first) into the zeroed unstuffed buffer at its
//                        offset; the last block of an interval adds the 1-bit padding.  OR commutes: deterministic.
//   enc_ffcount_kernel   FF bytes per 64-byte chunk of the unstuffed buffer
//   enc_finalize_kernel  a lane per image: exact length of its stuffed scan.  The host reads these, refuses a capacity that
//                        is too small BEFORE anything is written, and places the files.
//   enc_scatter_kernel   a lane per chunk: every byte to its final place, 00 after each FF, RSTn between intervals
//
// Limit: an image holds at most 2^24 pixels.  A block codes to at most 20 + 63 * 26 = 1,658 bits and a 4:4:4 image of 2^24
// pixels has 3 * 2^18 blocks, about 1.3e9 bits: every bit offset inside one image fits 32 bits.  Offsets that run over the
// batch are 64-bit.  A batch holds fewer than 2^31 blocks.
#include <algorithm>

#include "dfd_common.h"
#include "jpeg_sample.h"
#include "kernel_util.h"

namespace dfd {
namespace {

constexpr int kEncScanTile = 1024;        // elements one workgroup of the scan covers in one pass: 256 lanes x 4
constexpr int kEncChunk = 64;             // bytes of the unstuffed buffer per lane of the stuffing passes
constexpr size_t kEncMaxPixels = (size_t)1 << 24;

// ITU-T T.81 Annex K.3: codes per length 1..16, then the symbols in code order
const unsigned char kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const unsigned char kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// jchuff.c jpeg_make_c_derived_tbl for the four tables: symbol -> code, length
struct EncTables {
    unsigned short ac_code[2][256];
    unsigned short dc_code[2][16];
    unsigned char ac_len[2][256];
    unsigned char dc_len[2][16];
};

struct EncImage {
    const uint8_t* src;
    int h, w, stride, mode, rgb;
    int hs, vs;                    // luma sampling factors (chroma is 1 x 1); gray: 1, 1
    int mcux, bpm, ri;             // MCUs per row, blocks per MCU, MCUs per restart interval (0: the scan is one interval)
    unsigned nmcu, nint;           // MCUs, restart intervals
    unsigned blk0, int0;           // first block / first interval of the image in the batch
    unsigned short div[2][64];     // quantisation divisors (table value << 3: the FDCT output is scaled by 8), natural order
};

// largest i in [0, n) with first[i] <= v  (first[0] = 0)
template <class T>
__device__ __forceinline__ int enc_find(const T* first, int n, T v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// component c (0 Y, 1 Cb, 2 Cr; gray: the sample) of the pixel at (y, x), both inside the image
__device__ __forceinline__ int enc_px(const EncImage& im, int y, int x, int c) {
    const uint8_t* row = im.src + (size_t)y * im.stride;
    if (im.mode == DFD_JPEG_GRAY) return row[x];
    const uint8_t* p = row + 3 * x;
    const int r = im.rgb ? p[0] : p[2], g = p[1], b = im.rgb ? p[2] : p[0];
    return c == 0 ? ycc_y(r, g, b) : c == 1 ? ycc_cb(r, g, b) : ycc_cr(r, g, b);
}

__device__ __forceinline__ unsigned enc_pack2(int a, int b) { return ((unsigned)a & 0xffffu) | ((unsigned)b << 16); }

__global__ __launch_bounds__(64) void enc_block_kernel(const EncImage* __restrict__ images, const unsigned* __restrict__ blk_first,
                                                       int n, unsigned nb, short* __restrict__ coef) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    const EncImage& im = images[enc_find(blk_first, n, b)];
    const unsigned j = b - im.blk0, mcu = j / (unsigned)im.bpm;
    const int k = (int)(j - mcu * im.bpm), my = (int)(mcu / (unsigned)im.mcux), mx = (int)(mcu - (unsigned)my * im.mcux);
    const int ny = im.hs * im.vs, H = im.h, W = im.w;
    int d[64];
    bool dummy = false;
    int tq = 0;
    if (k < ny) {
        int by = my * im.vs + k / im.hs, bx = mx * im.hs + k % im.hs;
        const int wb = (W + 7) >> 3, hb = (H + 7) >> 3;
        if (by >= hb) {                      // a dummy row: the DC of the last block of the row above in this MCU ...
            by -= 1;
            bx = mx * im.hs + im.hs - 1;
            dummy = true;
        }
        if (bx >= wb) {                      // ... and a block right of the real ones: the DC of the block left of it
            bx -= 1;
            dummy = true;
        }
#pragma unroll
        for (int i = 0; i < 64; ++i) d[i] = enc_px(im, min(by * 8 + (i >> 3), H - 1), min(bx * 8 + (i & 7), W - 1), 0) - 128;
    } else {
        tq = 1;
        const int c = 1 + k - ny, hs = im.hs, vs = im.vs;
        const int ch = (H + vs - 1) / vs;    // real rows of the downsampled plane: the rows below copy the last one
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const int cy = min(my * 8 + (i >> 3), ch - 1), cx = mx * 8 + (i & 7);
            int s = 0;
            for (int dy = 0; dy < vs; ++dy)
                for (int dx = 0; dx < hs; ++dx) s += enc_px(im, min(cy * vs + dy, H - 1), min(cx * hs + dx, W - 1), c);
            if (hs == 2) s = vs == 2 ? (s + ((cx & 1) ? 2 : 1)) >> 2 : (s + (cx & 1)) >> 1;     // bias 1,2,1,2 / 0,1,0,1
            d[i] = s - 128;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct8<true>(d + 8 * r, 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct8<false>(d + c, 8);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int qv = im.div[tq][i], a = (abs(d[i]) + (qv >> 1)) / qv;
        d[i] = (dummy && i) ? 0 : (d[i] < 0 ? -a : a);
    }
    u4* dst = reinterpret_cast<u4*>(coef + (size_t)b * 64);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        u4 v;
        v.x = enc_pack2(d[kJpegZigzag[8 * g]], d[kJpegZigzag[8 * g + 1]]);
        v.y = enc_pack2(d[kJpegZigzag[8 * g + 2]], d[kJpegZigzag[8 * g + 3]]);
        v.z = enc_pack2(d[kJpegZigzag[8 * g + 4]], d[kJpegZigzag[8 * g + 5]]);
        v.w = enc_pack2(d[kJpegZigzag[8 * g + 6]], d[kJpegZigzag[8 * g + 7]]);
        dst[g] = v;
    }
}

// where block b sits: its image, its MCU, its component's tables, the DC it is predicted from and its restart interval
struct EncWhere {
    const EncImage* im;
    int table, pred;
    unsigned interval, first, end;     // batch-wide interval index; first block and one past the last block of the interval
};

__device__ __forceinline__ EncWhere enc_where(const EncImage* images, const unsigned* blk_first, int n, unsigned b,
                                              const short* coef) {
    EncWhere w;
    const EncImage& im = images[enc_find(blk_first, n, b)];
    w.im = &im;
    const unsigned j = b - im.blk0, mcu = j / (unsigned)im.bpm;
    const int k = (int)(j - mcu * im.bpm), ny = im.hs * im.vs;
    w.table = k < ny ? 0 : 1;
    const unsigned li = im.ri ? mcu / (unsigned)im.ri : 0;
    const unsigned m0 = im.ri ? li * (unsigned)im.ri : 0, m1 = im.ri ? min(im.nmcu, m0 + (unsigned)im.ri) : im.nmcu;
    w.interval = im.int0 + li;
    w.first = im.blk0 + m0 * im.bpm;
    w.end = im.blk0 + m1 * im.bpm;
    if (k > 0 && k < ny) w.pred = coef[(size_t)(b - 1) * 64];                              // the luma block before it in the MCU
    else if (mcu == m0) w.pred = 0;                                                        // first MCU of an interval
    else w.pred = coef[(size_t)(im.blk0 + (mcu - 1) * im.bpm + (k == 0 ? ny - 1 : k)) * 64];   // the component's last block of the MCU before
    return w;
}

__device__ __forceinline__ int enc_nbits(int v) { return 32 - __clz(abs(v)); }      // __clz(0) = 32

// jchuff.c encode_one_block: every (code, length) of the block goes to sink.put, at most 27 bits at a time
template <class Sink>
__device__ __forceinline__ void enc_code_block(const EncTables* __restrict__ T, int t, const short* __restrict__ c, int pred,
                                               Sink& sink) {
    const int diff = c[0] - pred;
    int s = enc_nbits(diff);
    sink.put(((unsigned)T->dc_code[t][s] << s) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), T->dc_len[t][s] + s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        if (v == 0) { ++run; continue; }
        while (run > 15) { sink.put(T->ac_code[t][0xF0], T->ac_len[t][0xF0]); run -= 16; }
        s = enc_nbits(v);
        const int sym = ((run << 4) | s) & 255;
        sink.put(((unsigned)T->ac_code[t][sym] << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), T->ac_len[t][sym] + s);
        run = 0;
    }
    if (run) sink.put(T->ac_code[t][0], T->ac_len[t][0]);
}

struct EncLenSink {
    unsigned bits = 0;
    __device__ __forceinline__ void put(unsigned, int len) { bits += (unsigned)len; }
};

__global__ __launch_bounds__(256) void enc_length_kernel(const EncTables* __restrict__ T, const EncImage* __restrict__ images,
                                                         const unsigned* __restrict__ blk_first, int n, unsigned nb,
                                                         const short* __restrict__ coef, unsigned* __restrict__ bits) {
    const unsigned b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const EncWhere w = enc_where(images, blk_first, n, b, coef);
    EncLenSink sink;
    enc_code_block(T, w.table, coef + (size_t)b * 64, w.pred, sink);
    bits[b] = sink.bits;
}

// ---------------------------------------------------------------------------------- scan
// exclusive scan of 256 values, one per lane; *total = their sum
__device__ __forceinline__ unsigned long long enc_scan256(unsigned long long v, unsigned long long* sh, unsigned long long* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned long long x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const unsigned long long incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void enc_scan_reduce_kernel(const unsigned* __restrict__ in, unsigned n,
                                                              unsigned long long* __restrict__ tiles) {
    __shared__ unsigned long long sh[256];
    const unsigned i0 = blockIdx.x * kEncScanTile + threadIdx.x * 4;
    unsigned long long s = 0, total;
    for (int k = 0; k < 4; ++k)
        if (i0 + k < n) s += in[i0 + k];
    enc_scan256(s, sh, &total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void enc_scan_tiles_kernel(unsigned long long* __restrict__ tiles, unsigned nt) {
    __shared__ unsigned long long sh[256];
    unsigned long long carry = 0, total;
    for (unsigned base = 0; base < nt; base += 256) {
        const unsigned i = base + threadIdx.x;
        const unsigned long long ex = enc_scan256(i < nt ? tiles[i] : 0, sh, &total);
        if (i < nt) tiles[i] = carry + ex;
        carry += total;
    }
}

// out[0 .. n]: out[i] = sum of in[0 .. i), out[n] = the total
__global__ __launch_bounds__(256) void enc_scan_down_kernel(const unsigned* __restrict__ in, unsigned n,
                                                            const unsigned long long* __restrict__ tiles,
                                                            unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sh[256];
    const unsigned i0 = blockIdx.x * kEncScanTile + threadIdx.x * 4;
    unsigned a[4];
    unsigned long long s = 0, total;
    for (int k = 0; k < 4; ++k) {
        a[k] = i0 + k < n ? in[i0 + k] : 0;
        s += a[k];
    }
    unsigned long long run = tiles[blockIdx.x] + enc_scan256(s, sh, &total);
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run += a[k];
        if (i0 + k == n - 1) out[n] = run;
    }
}

// ---------------------------------------------------------------------------------- intervals, emit
__global__ __launch_bounds__(256) void enc_interval_kernel(const EncImage* __restrict__ images, const unsigned* __restrict__ int_first,
                                                           int n, unsigned ni, const unsigned long long* __restrict__ bit_off,
                                                           unsigned* __restrict__ ibytes) {
    const unsigned g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ni) return;
    const EncImage& im = images[enc_find(int_first, n, g)];
    const unsigned li = g - im.int0;
    const unsigned m0 = im.ri ? li * (unsigned)im.ri : 0, m1 = im.ri ? min(im.nmcu, m0 + (unsigned)im.ri) : im.nmcu;
    const unsigned long long bits = bit_off[im.blk0 + m1 * im.bpm] - bit_off[im.blk0 + m0 * im.bpm];
    ibytes[g] = (unsigned)((bits + 7) >> 3);
}

// MSB-first bit writer into 32-bit words; stream byte k of a word is (word >> (24 - 8 k)) & 255
struct EncBitSink {
    unsigned* word;
    unsigned long long acc = 0;
    int n;                               // bits held in acc (< 32 between puts); the first word starts with n zero bits
    __device__ __forceinline__ EncBitSink(unsigned* raw, unsigned long long bitpos) : word(raw + (bitpos >> 5)), n((int)(bitpos & 31)) {}
    __device__ __forceinline__ void put(unsigned code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            atomicOr(word++, (unsigned)(acc >> n));
            acc &= (1ull << n) - 1;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n) atomicOr(word, (unsigned)(acc << (32 - n)));
    }
};

__global__ __launch_bounds__(256) void enc_emit_kernel(const EncTables* __restrict__ T, const EncImage* __restrict__ images,
                                                       const unsigned* __restrict__ blk_first, int n, unsigned nb,
                                                       const short* __restrict__ coef, const unsigned long long* __restrict__ bit_off,
                                                       const unsigned long long* __restrict__ int_off, unsigned* __restrict__ raw) {
    const unsigned b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const EncWhere w = enc_where(images, blk_first, n, b, coef);
    EncBitSink sink(raw, int_off[w.interval] * 8 + (bit_off[b] - bit_off[w.first]));
    enc_code_block(T, w.table, coef + (size_t)b * 64, w.pred, sink);
    if (b + 1 == w.end) {                                            // the interval ends here: pad its last byte with 1-bits
        const int pad = (int)((8 - ((bit_off[w.end] - bit_off[w.first]) & 7)) & 7);
        if (pad) sink.put((1u << pad) - 1, pad);
    }
    sink.flush();
}

// ---------------------------------------------------------------------------------- stuffing
__device__ __forceinline__ unsigned enc_raw_byte(const unsigned* raw, unsigned long long p) {
    return (raw[p >> 2] >> (24 - 8 * (int)(p & 3))) & 255u;
}

__global__ __launch_bounds__(256) void enc_ffcount_kernel(const unsigned* __restrict__ raw, unsigned nc, unsigned* __restrict__ ffc) {
    const unsigned c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    unsigned cnt = 0;
    for (int k = 0; k < kEncChunk / 4; ++k) {
        const unsigned v = raw[(size_t)c * (kEncChunk / 4) + k];
        cnt += ((v >> 24) == 255u) + (((v >> 16) & 255u) == 255u) + (((v >> 8) & 255u) == 255u) + ((v & 255u) == 255u);
    }
    ffc[c] = cnt;
}

// FF bytes of the unstuffed buffer before byte p
__device__ __forceinline__ unsigned long long enc_ff_before(const unsigned* raw, const unsigned long long* ff_off, unsigned long long p) {
    unsigned long long cnt = ff_off[p / kEncChunk];
    for (unsigned long long q = p - p % kEncChunk; q < p; ++q) cnt += enc_raw_byte(raw, q) == 255u;
    return cnt;
}

// per image: bytes of its scan after stuffing, RSTn markers included; FF bytes before its first byte
__global__ __launch_bounds__(64) void enc_finalize_kernel(const EncImage* __restrict__ images, int n, const unsigned* __restrict__ raw,
                                                          const unsigned long long* __restrict__ int_off,
                                                          const unsigned long long* __restrict__ ff_off,
                                                          unsigned long long* __restrict__ scan_len, unsigned long long* __restrict__ ff_base) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const EncImage& im = images[i];
    const unsigned long long r0 = int_off[im.int0], r1 = int_off[im.int0 + im.nint];
    const unsigned long long f0 = enc_ff_before(raw, ff_off, r0), f1 = enc_ff_before(raw, ff_off, r1);
    ff_base[i] = f0;
    scan_len[i] = (r1 - r0) + (f1 - f0) + 2ull * (im.nint - 1);
}

// a lane per chunk of the unstuffed buffer: every byte to its place in its file
__global__ __launch_bounds__(256) void enc_scatter_kernel(const EncImage* __restrict__ images, const unsigned* __restrict__ int_first, int n,
                                                          unsigned ni, const unsigned* __restrict__ raw, unsigned long long raw_total,
                                                          const unsigned long long* __restrict__ int_off,
                                                          const unsigned long long* __restrict__ ff_off,
                                                          const unsigned long long* __restrict__ ff_base,
                                                          const unsigned long long* __restrict__ out0, uint8_t* __restrict__ out) {
    const unsigned long long c = (unsigned long long)blockIdx.x * 256 + threadIdx.x, p0 = c * kEncChunk;
    if (p0 >= raw_total) return;
    const unsigned long long p1 = min(p0 + kEncChunk, raw_total);
    unsigned g = (unsigned)enc_find(int_off, (int)ni, p0);           // intervals are never empty: the one that holds p0
    int i = enc_find(int_first, n, g);
    unsigned long long ff = ff_off[c];
    for (unsigned long long p = p0; p < p1; ++p) {
        while (p >= int_off[g + 1]) ++g;
        while (i + 1 < n && g >= int_first[i + 1]) ++i;
        const EncImage& im = images[i];
        const unsigned v = enc_raw_byte(raw, p);
        unsigned long long dst = out0[i] + (p - int_off[im.int0]) + (ff - ff_base[i]) + 2ull * (g - im.int0);
        out[dst++] = (uint8_t)v;
        if (v == 255u) {
            out[dst++] = 0;
            ++ff;
        }
        if (p + 1 == int_off[g + 1] && g + 1 < im.int0 + im.nint) {  // RSTn between this interval and the next of the image
            out[dst] = 0xFF;
            out[dst + 1] = (uint8_t)(0xD0 + ((g - im.int0) & 7));
        }
    }
}

// ---------------------------------------------------------------------------------- host
int enc_scan(dfd_handle* h, const unsigned* in, unsigned n, unsigned long long* tiles, unsigned long long* out) {
    const unsigned nt = (n + kEncScanTile - 1) / kEncScanTile;
    hipLaunchKernelGGL(enc_scan_reduce_kernel, dim3(nt), dim3(256), 0, h->stream, in, n, tiles);
    hipLaunchKernelGGL(enc_scan_tiles_kernel, dim3(1), dim3(256), 0, h->stream, tiles, nt);
    hipLaunchKernelGGL(enc_scan_down_kernel, dim3(nt), dim3(256), 0, h->stream, in, n, tiles, out);
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

void enc_derive(const unsigned char* bits, const unsigned char* vals, unsigned short* code_out, unsigned char* len_out) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code) {
            code_out[vals[k]] = (unsigned short)code;
            len_out[vals[k]] = (unsigned char)len;
        }
        code <<= 1;
    }
}

void enc_quant(int which, int quality, unsigned char* q) {
    for (int i = 0; i < 64; ++i) q[i] = (unsigned char)jpeg_quant_value(which, i, jpeg_quality_scale(quality));
}

struct EncGeom { int hs, vs, comps, bpm, mcux, mcuy; };

// DFD_OK and the geometry, or the code the header documents
int enc_geometry(int height, int width, int subsampling, EncGeom* g) {
    if (height < 1 || width < 1 || height > 65535 || width > 65535) return DFD_ERR_ARG;
    if (subsampling < DFD_JPEG_444 || subsampling > DFD_JPEG_GRAY) return DFD_ERR_ARG;
    if ((size_t)height * (size_t)width > kEncMaxPixels) return DFD_ERR_UNSUPPORTED;
    g->hs = subsampling == DFD_JPEG_422 || subsampling == DFD_JPEG_420 ? 2 : 1;
    g->vs = subsampling == DFD_JPEG_420 ? 2 : 1;
    g->comps = subsampling == DFD_JPEG_GRAY ? 1 : 3;
    g->bpm = subsampling == DFD_JPEG_GRAY ? 1 : g->hs * g->vs + 2;
    g->mcux = (width + 8 * g->hs - 1) / (8 * g->hs);
    g->mcuy = (height + 8 * g->vs - 1) / (8 * g->vs);
    return DFD_OK;
}

void enc_put16(std::vector<uint8_t>& o, unsigned v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); }

void enc_dht(std::vector<uint8_t>& o, int cls, int id, const unsigned char* bits, const unsigned char* vals, int nvals) {
    o.push_back(0xFF); o.push_back(0xC4);
    enc_put16(o, 19 + nvals);
    o.push_back((uint8_t)((cls << 4) | id));
    o.insert(o.end(), bits, bits + 16);
    o.insert(o.end(), vals, vals + nvals);
}

// jcmarker.c: SOI, APP0 (JFIF 1.01, no units, 1 x 1), DQT per table, SOF0, DHT DC0 AC0 [DC1 AC1], [DRI], SOS
void enc_header(const dfd_jpeg_source& s, const EncGeom& g, const unsigned char q[2][64], std::vector<uint8_t>& o) {
    static const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    o.assign(app0, app0 + sizeof app0);
    for (int t = 0; t < (g.comps == 1 ? 1 : 2); ++t) {
        o.push_back(0xFF); o.push_back(0xDB);
        enc_put16(o, 67);
        o.push_back((uint8_t)t);
        for (int i = 0; i < 64; ++i) o.push_back(q[t][kJpegZigzag[i]]);
    }
    o.push_back(0xFF); o.push_back(0xC0);
    enc_put16(o, 8 + 3 * g.comps);
    o.push_back(8);
    enc_put16(o, (unsigned)s.height);
    enc_put16(o, (unsigned)s.width);
    o.push_back((uint8_t)g.comps);
    for (int c = 0; c < g.comps; ++c) {
        o.push_back((uint8_t)(c + 1));
        o.push_back((uint8_t)(c == 0 ? (g.hs << 4) | g.vs : 0x11));
        o.push_back((uint8_t)(c ? 1 : 0));
    }
    for (int t = 0; t < (g.comps == 1 ? 1 : 2); ++t) {
        enc_dht(o, 0, t, kDcBits[t], kDcVals, 12);
        enc_dht(o, 1, t, kAcBits[t], kAcVals[t], 162);
    }
    if (s.restart_blocks) {
        o.push_back(0xFF); o.push_back(0xDD);
        enc_put16(o, 4);
        enc_put16(o, (unsigned)s.restart_blocks);
    }
    o.push_back(0xFF); o.push_back(0xDA);
    enc_put16(o, 6 + 2 * g.comps);
    o.push_back((uint8_t)g.comps);
    for (int c = 0; c < g.comps; ++c) {
        o.push_back((uint8_t)(c + 1));
        o.push_back((uint8_t)(c ? 0x11 : 0x00));
    }
    o.push_back(0); o.push_back(63); o.push_back(0);
}

size_t enc_align(size_t v, size_t a) { return (v + a - 1) / a * a; }

int enc_check_source(dfd_handle* h, const dfd_jpeg_source& s, int i, EncGeom* g) {
    const int rc = enc_geometry(s.height, s.width, s.subsampling, g);
    if (rc == DFD_ERR_UNSUPPORTED)
        return fail(h, rc, "encode_jpeg: image %d: %d x %d is above 2^24 pixels", i, s.width, s.height);
    if (rc) return fail(h, rc, "encode_jpeg: image %d: size %d x %d or subsampling %d", i, s.width, s.height, s.subsampling);
    if (!s.pixels || s.stride < s.width * (g->comps == 1 ? 1 : 3)) return fail(h, DFD_ERR_ARG, "encode_jpeg: image %d: null pixels or short stride", i);
    if (s.quality < 1 || s.quality > 100) return fail(h, DFD_ERR_ARG, "encode_jpeg: image %d: quality %d outside 1..100", i, s.quality);
    if (s.restart_blocks < 0 || s.restart_blocks > 65535) return fail(h, DFD_ERR_ARG, "encode_jpeg: image %d: restart_blocks %d outside 0..65535", i, s.restart_blocks);
    return DFD_OK;
}

// the chain on sources whose pixels are in HBM
int enc_run(dfd_handle* h, int n, const dfd_jpeg_source* src, uint8_t* out, size_t capacity, size_t* offsets, size_t* lens,
            size_t* total_out) {
    hipStream_t s = h->stream;
    std::vector<EncImage> images(n);
    std::vector<std::vector<uint8_t>> headers(n);
    std::vector<unsigned> blk_first(n + 1), int_first(n + 1);
    unsigned long long nb64 = 0, ni64 = 0;
    int rc;
    for (int i = 0; i < n; ++i) {
        EncGeom g;
        if ((rc = enc_check_source(h, src[i], i, &g))) return rc;
        EncImage& im = images[i];
        im.src = src[i].pixels;
        im.h = src[i].height; im.w = src[i].width; im.stride = src[i].stride;
        im.mode = src[i].subsampling; im.rgb = src[i].rgb ? 1 : 0;
        im.hs = g.hs; im.vs = g.vs; im.mcux = g.mcux; im.bpm = g.bpm;
        im.nmcu = (unsigned)g.mcux * (unsigned)g.mcuy;
        im.ri = (unsigned)src[i].restart_blocks >= im.nmcu ? 0 : src[i].restart_blocks;   // one interval either way
        im.nint = im.ri ? (im.nmcu + im.ri - 1) / im.ri : 1;
        if (nb64 + (unsigned long long)im.nmcu * im.bpm >= (1ull << 31))
            return fail(h, DFD_ERR_UNSUPPORTED, "encode_jpeg: more than 2^31 blocks in one call");
        im.blk0 = blk_first[i] = (unsigned)nb64;
        im.int0 = int_first[i] = (unsigned)ni64;
        nb64 += (unsigned long long)im.nmcu * im.bpm;
        ni64 += im.nint;
        unsigned char q[2][64];
        for (int t = 0; t < 2; ++t) {
            enc_quant(t, src[i].quality, q[t]);
            for (int k = 0; k < 64; ++k) im.div[t][k] = (unsigned short)(q[t][k] << 3);
        }
        enc_header(src[i], g, q, headers[i]);
    }
    const unsigned nb = (unsigned)nb64, ni = (unsigned)ni64;
    blk_first[n] = nb;
    int_first[n] = ni;

    // tables + descriptors in one upload; the per-image results and file positions behind them
    EncTables tab{};
    for (int t = 0; t < 2; ++t) {
        enc_derive(kDcBits[t], kDcVals, tab.dc_code[t], tab.dc_len[t]);
        enc_derive(kAcBits[t], kAcVals[t], tab.ac_code[t], tab.ac_len[t]);
    }
    const size_t o_img = enc_align(sizeof(EncTables), 16), o_bf = enc_align(o_img + (size_t)n * sizeof(EncImage), 16);
    const size_t o_if = o_bf + (size_t)(n + 1) * 4, o_res = enc_align(o_if + (size_t)(n + 1) * 4, 16), o_end = o_res + (size_t)n * 8 * 3;
    std::vector<uint8_t> blob(o_res, 0);
    memcpy(blob.data(), &tab, sizeof tab);
    memcpy(blob.data() + o_img, images.data(), (size_t)n * sizeof(EncImage));
    memcpy(blob.data() + o_bf, blk_first.data(), (size_t)(n + 1) * 4);
    memcpy(blob.data() + o_if, int_first.data(), (size_t)(n + 1) * 4);
    DevBuf* B = h->jpeg_enc;
    const unsigned nt_b = (nb + kEncScanTile - 1) / kEncScanTile, nt_i = (ni + kEncScanTile - 1) / kEncScanTile;
    const size_t s_bits = 0, s_boff = enc_align((size_t)nb * 4, 16), s_ib = s_boff + ((size_t)nb + 1) * 8;
    const size_t s_ioff = enc_align(s_ib + (size_t)ni * 4, 16), s_tiles = s_ioff + ((size_t)ni + 1) * 8;
    if ((rc = ensure(h, &B[1], o_end))) return rc;
    if ((rc = ensure(h, &B[2], (size_t)nb * 128))) return rc;
    if ((rc = ensure(h, &B[3], s_tiles + (size_t)std::max(nt_b, nt_i) * 8))) return rc;
    char* d1 = (char*)B[1].p;
    char* d3 = (char*)B[3].p;
    DFD_HIP_TRY(h, hipMemcpyAsync(d1, blob.data(), o_res, hipMemcpyHostToDevice, s));
    const EncTables* dT = (const EncTables*)d1;
    const EncImage* dI = (const EncImage*)(d1 + o_img);
    const unsigned *dBF = (const unsigned*)(d1 + o_bf), *dIF = (const unsigned*)(d1 + o_if);
    unsigned long long *dLen = (unsigned long long*)(d1 + o_res), *dFfBase = dLen + n, *dOut0 = dLen + 2 * (size_t)n;
    short* dCoef = (short*)B[2].p;
    unsigned* dBits = (unsigned*)(d3 + s_bits);
    unsigned long long* dBitOff = (unsigned long long*)(d3 + s_boff);
    unsigned* dIBytes = (unsigned*)(d3 + s_ib);
    unsigned long long* dIntOff = (unsigned long long*)(d3 + s_ioff);
    unsigned long long* dTiles = (unsigned long long*)(d3 + s_tiles);

    hipLaunchKernelGGL(enc_block_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, dI, dBF, n, nb, dCoef);
    hipLaunchKernelGGL(enc_length_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, dT, dI, dBF, n, nb, dCoef, dBits);
    if ((rc = enc_scan(h, dBits, nb, dTiles, dBitOff))) return rc;
    hipLaunchKernelGGL(enc_interval_kernel, dim3((ni + 255) / 256), dim3(256), 0, s, dI, dIF, n, ni, dBitOff, dIBytes);
    if ((rc = enc_scan(h, dIBytes, ni, dTiles, dIntOff))) return rc;
    unsigned long long raw_total = 0;
    DFD_HIP_TRY(h, hipMemcpyAsync(&raw_total, dIntOff + ni, 8, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));

    // the unstuffed buffer, zeroed, one spare chunk behind the last byte; FF counts and their scan behind it
    const size_t raw_cap = enc_align((size_t)raw_total, kEncChunk) + kEncChunk, nc = raw_cap / kEncChunk;
    const size_t r_ffc = raw_cap, r_ffoff = enc_align(r_ffc + nc * 4, 16), r_tiles = r_ffoff + (nc + 1) * 8;
    const unsigned nt_c = (unsigned)((nc + kEncScanTile - 1) / kEncScanTile);
    if (nc >= (1ull << 31)) return fail(h, DFD_ERR_UNSUPPORTED, "encode_jpeg: more than 2^37 bytes of scan data in one call");
    if ((rc = ensure(h, &B[4], r_tiles + (size_t)nt_c * 8))) return rc;
    char* d4 = (char*)B[4].p;
    unsigned* dRaw = (unsigned*)d4;
    unsigned* dFfc = (unsigned*)(d4 + r_ffc);
    unsigned long long* dFfOff = (unsigned long long*)(d4 + r_ffoff);
    unsigned long long* dTiles2 = (unsigned long long*)(d4 + r_tiles);
    DFD_HIP_TRY(h, hipMemsetAsync(dRaw, 0, raw_cap, s));
    hipLaunchKernelGGL(enc_emit_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, dT, dI, dBF, n, nb, dCoef, dBitOff, dIntOff, dRaw);
    hipLaunchKernelGGL(enc_ffcount_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, dRaw, (unsigned)nc, dFfc);
    if ((rc = enc_scan(h, dFfc, (unsigned)nc, dTiles2, dFfOff))) return rc;
    hipLaunchKernelGGL(enc_finalize_kernel, dim3((n + 63) / 64), dim3(64), 0, s, dI, n, dRaw, dIntOff, dFfOff, dLen, dFfBase);
    DFD_HIP_TRY(h, hipGetLastError());
    std::vector<unsigned long long> scan_len(n), out0(n);
    DFD_HIP_TRY(h, hipMemcpyAsync(scan_len.data(), dLen, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));

    // every length is exact now: place the files, refuse a short capacity before anything is written
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        const size_t len = headers[i].size() + (size_t)scan_len[i] + 2;
        if (offsets) offsets[i] = total;
        if (lens) lens[i] = len;
        out0[i] = total + headers[i].size();
        total += len;
    }
    if (total_out) *total_out = total;
    if (!out || capacity < total) return fail(h, DFD_ERR_ARG, "encode_jpeg: capacity %zu, the output needs %zu bytes", capacity, total);
    if ((rc = ensure(h, &B[5], total))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(dOut0, out0.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(enc_scatter_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, dI, dIF, n, ni, dRaw, raw_total, dIntOff,
                       dFfOff, dFfBase, dOut0, (uint8_t*)B[5].p);
    DFD_HIP_TRY(h, hipGetLastError());
    DFD_HIP_TRY(h, hipMemcpyAsync(out, B[5].p, total, hipMemcpyDeviceToHost, s));
    DFD_HIP_TRY(h, stream_sync(h));
    for (int i = 0; i < n; ++i) {                                    // header in front of each scan, EOI behind it
        uint8_t* f = out + out0[i] - headers[i].size();
        memcpy(f, headers[i].data(), headers[i].size());
        f[headers[i].size() + scan_len[i]] = 0xFF;
        f[headers[i].size() + scan_len[i] + 1] = 0xD9;
    }
    return DFD_OK;
}

int enc_call(dfd_handle* h, int n, const dfd_jpeg_source* images, uint8_t* out, size_t capacity, size_t* offsets, size_t* lens,
             size_t* total, bool on_device) {
    if (!h) return DFD_ERR_ARG;
    if (n < 1 || !images || !total) return fail(h, DFD_ERR_ARG, "encode_jpeg: no image or null argument");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    if (on_device) return enc_run(h, n, images, out, capacity, offsets, lens, total);
    std::vector<dfd_jpeg_source> dev(images, images + n);
    size_t bytes = 0;
    int rc;
    for (int i = 0; i < n; ++i) {
        EncGeom g;
        if ((rc = enc_check_source(h, images[i], i, &g))) return rc;
        bytes += enc_align((size_t)images[i].height * images[i].stride, 256);
    }
    if ((rc = ensure(h, &h->jpeg_enc[0], bytes))) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        uint8_t* dst = (uint8_t*)h->jpeg_enc[0].p + off;
        // the last row is read to its last pixel only
        const size_t used = (size_t)(images[i].height - 1) * images[i].stride + (size_t)images[i].width * (images[i].subsampling == DFD_JPEG_GRAY ? 1 : 3);
        DFD_HIP_TRY(h, hipMemcpyAsync(dst, images[i].pixels, used, hipMemcpyHostToDevice, h->stream));
        dev[i].pixels = dst;
        off += enc_align((size_t)images[i].height * images[i].stride, 256);
    }
    return enc_run(h, n, dev.data(), out, capacity, offsets, lens, total);
}

}  // namespace
}  // namespace dfd

using namespace dfd;

extern "C" {

size_t dfd_encode_jpeg_bound(int height, int width, int subsampling) {
    EncGeom g;
    if (enc_geometry(height, width, subsampling, &g) != DFD_OK) return 0;
    // header < 1 KiB; a block codes to at most 1,658 bits = 208 bytes, twice that if every byte were stuffed; an RSTn per MCU
    const size_t mcus = (size_t)g.mcux * g.mcuy;
    return 1024 + mcus * g.bpm * 416 + mcus * 2;
}

int dfd_encode_jpeg(dfd_handle* h, const uint8_t* pixels, int height, int width, int stride, int rgb, int quality, int subsampling,
                    int restart_blocks, uint8_t* out, size_t capacity, size_t* len) {
    const dfd_jpeg_source s{pixels, height, width, stride, rgb, quality, subsampling, restart_blocks};
    return enc_call(h, 1, &s, out, capacity, nullptr, nullptr, len, false);
}

int dfd_encode_jpeg_batch(dfd_handle* h, int n, const dfd_jpeg_source* images, uint8_t* out, size_t capacity, size_t* offsets,
                          size_t* lens, size_t* total) {
    return enc_call(h, n, images, out, capacity, offsets, lens, total, false);
}

int dfd_encode_jpeg_device(dfd_handle* h, int n, const dfd_jpeg_source* images, uint8_t* out, size_t capacity, size_t* offsets,
                           size_t* lens, size_t* total) {
    return enc_call(h, n, images, out, capacity, offsets, lens, total, true);
}

}  // extern "C"

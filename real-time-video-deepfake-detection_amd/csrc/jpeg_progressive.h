// The four scan decoders of progressive JPEG (T.81 G.2; libjpeg's jdphuff.c): DC first, DC refinement, AC first with
// end-of-band runs, AC refinement with correction bits - ONE copy of the arithmetic, written so that it compiles as
// plain C++ (jpeg_entropy.h, the sanitizer harness) and as __host__ __device__ under hipcc (the convention of
// jpeg_sample.h: the qualifiers exist only where the compiler knows them).
//
// pj_decode_segment decodes ONE segment of one scan - the whole scan, or what lies between two RSTn markers - from a
// known start state (bit position, first unit, EOBRUN = 0) out of a DE-STUFFED byte array into the coefficient planes
// (int16, natural order, 64 per block, blocks row-major with the MCU-padded row stride `bw`).
//
// Geometry.  An interleaved scan (more than one component; DC only) walks MCUs of the frame's MCU grid, each with h x v
// blocks per component.  A scan with ONE component walks that component's OWN grid of ceil(w_c / 8) x ceil(h_c / 8) blocks
// in raster order (T.81 A.2.3) - not the padded grid the planes are allocated at - and a restart interval counts blocks
// there.  A "unit" below is an MCU of the first kind and a block of the second.
//
// What holds whatever the bytes say:
//   * a coefficient index never passes Se, a unit index never passes the segment's last;
//   * no byte at or behind `nbytes` is read: bits behind the end read as zero, and a segment that consumed one ends with
//     PJ_TRUNCATED;
//   * an end-of-band run is local to the call: it starts at 0 and what is left of it at the end is dropped;
//   * arithmetic in 32 bits, the low 16 bits stored; no negative value is shifted.
// Defects (the caller rejects the file): a bit pattern that is no code, a coefficient index past Se, a DC category
// above 11, a refinement symbol whose size is not 1, data that ends before the segment's last unit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PJ_HD __host__ __device__ __forceinline__
#else
#define PJ_HD inline
#endif

namespace dfd_pj {

enum PjStatus { PJ_OK = 0, PJ_BAD_CODE = 1, PJ_INDEX = 2, PJ_DC_CATEGORY = 3, PJ_TRUNCATED = 4 };

struct PjHuff {                                  // canonical decoding arrays (T.81 F.2.2.3) + an 8-bit lookahead
    uint16_t look8[256];                         // (length << 8) | symbol for codes of <= 8 bits, 0 = longer / none
    int32_t maxcode[17], mincode[17], valptr[17];// per code length 1..16; maxcode = -1: no code of that length
    uint8_t vals[256];
};

struct PjScan {
    int32_t ncomp;                               // components in the scan, 1..3
    int32_t Ss, Se, Ah, Al;
    uint32_t comp_off[3];                        // int16 elements from the file's coefficient base
    int32_t bw[3], h[3], v[3];                   // padded row stride in blocks; sampling factors (interleaved scans)
    int32_t units_x;                             // MCUs per row (interleaved) / blocks per row of the component's own grid
    uint32_t units;                              // units of the whole scan
    int32_t dc_tab[3], ac_tab;                   // indices into the scan's table set (-1: not needed)
};

// zigzag position -> natural order (a copy of jpeg_tables.h's table that host and device code both see as a constant)
PJ_HD int pj_natural(int k) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

struct PjBits {
    const uint8_t* c;
    uint64_t nbytes;                             // bytes that may be read
    uint64_t bp;                                 // bit position
    PJ_HD uint32_t byte(uint64_t i) const { return i < nbytes ? c[i] : 0u; }
    PJ_HD uint32_t peek16() const {              // the 16 bits at bp
        const uint64_t i = bp >> 3;
        const uint32_t w = (byte(i) << 16) | (byte(i + 1) << 8) | byte(i + 2);
        return (w >> (8 - (uint32_t)(bp & 7))) & 0xffffu;
    }
    PJ_HD uint32_t get(int n) {                  // n in 0..16
        if (n == 0) return 0;
        const uint32_t v = peek16() >> (16 - n);
        bp += (uint64_t)n;
        return v;
    }
    PJ_HD bool past_end() const { return bp > nbytes * 8; }
};

// one Huffman symbol, or -1 for a bit pattern that is no code (the bits are consumed all the same)
PJ_HD int pj_symbol(const PjHuff& t, PjBits& b) {
    const uint32_t v = b.peek16();
    const uint32_t e = t.look8[v >> 8];
    if (e) { b.bp += e >> 8; return (int)(e & 0xffu); }
    for (int l = 9; l <= 16; ++l) {
        const int32_t code = (int32_t)(v >> (16 - l));
        if (code <= t.maxcode[l]) {
            const int32_t idx = t.valptr[l] + code - t.mincode[l];
            b.bp += (uint64_t)l;
            return (idx >= 0 && idx < 256) ? (int)t.vals[idx] : -1;
        }
    }
    b.bp += 16;
    return -1;
}

// T.81 F.2.2.1 EXTEND: `s` bits `v` -> the signed value
PJ_HD int32_t pj_extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int32_t)v - (int32_t)(1u << s) + 1 : (int32_t)v; }

// low 16 bits of x * 2^al, as the int16 the planes hold
PJ_HD int16_t pj_scaled(int32_t x, int al) { return (int16_t)(uint16_t)(((uint32_t)x << al) & 0xffffu); }

PJ_HD int16_t* pj_block(const PjScan& S, int16_t* coef, int ci, uint32_t row, uint32_t col) {
    return coef + S.comp_off[ci] + ((uint64_t)row * (uint32_t)S.bw[ci] + col) * 64u;
}

// ---- DC, first scan: units [u0, u1), predictions start at 0
PJ_HD int pj_dc_first(const PjScan& S, const PjHuff* tabs, PjBits& b, uint32_t u0, uint32_t u1, int16_t* coef) {
    uint32_t pred[3] = {0u, 0u, 0u};             // modulo 2^32: a damaged file cannot overflow it
    for (uint32_t u = u0; u < u1; ++u) {
        const uint32_t uy = u / (uint32_t)S.units_x, ux = u - uy * (uint32_t)S.units_x;
        for (int ci = 0; ci < S.ncomp; ++ci) {
            const int hh = S.ncomp == 1 ? 1 : S.h[ci], vv = S.ncomp == 1 ? 1 : S.v[ci];
            for (int by = 0; by < vv; ++by)
                for (int bx = 0; bx < hh; ++bx) {
                    const int s = pj_symbol(tabs[S.dc_tab[ci]], b);
                    if (s < 0) return PJ_BAD_CODE;
                    if (s > 11) return PJ_DC_CATEGORY;
                    if (s) pred[ci] += (uint32_t)pj_extend(b.get(s), s);
                    if (b.past_end()) return PJ_TRUNCATED;
                    pj_block(S, coef, ci, uy * (uint32_t)vv + (uint32_t)by, ux * (uint32_t)hh + (uint32_t)bx)[0] =
                        (int16_t)(uint16_t)((pred[ci] << S.Al) & 0xffffu);
                }
        }
    }
    return PJ_OK;
}

// ---- DC, refinement: one bit per block
PJ_HD void pj_dc_refine_block(int16_t* blk, uint32_t bit, int al) {
    if (bit) blk[0] = (int16_t)(uint16_t)((uint16_t)blk[0] | (uint16_t)(1u << al));
}

PJ_HD int pj_dc_refine(const PjScan& S, PjBits& b, uint32_t u0, uint32_t u1, int16_t* coef) {
    for (uint32_t u = u0; u < u1; ++u) {
        const uint32_t uy = u / (uint32_t)S.units_x, ux = u - uy * (uint32_t)S.units_x;
        for (int ci = 0; ci < S.ncomp; ++ci) {
            const int hh = S.ncomp == 1 ? 1 : S.h[ci], vv = S.ncomp == 1 ? 1 : S.v[ci];
            for (int by = 0; by < vv; ++by)
                for (int bx = 0; bx < hh; ++bx) {
                    const uint32_t bit = b.get(1);
                    if (b.past_end()) return PJ_TRUNCATED;
                    pj_dc_refine_block(pj_block(S, coef, ci, uy * (uint32_t)vv + (uint32_t)by, ux * (uint32_t)hh + (uint32_t)bx), bit, S.Al);
                }
        }
    }
    return PJ_OK;
}

// ---- AC, first scan of a band: blocks [u0, u1) of the component's own grid
PJ_HD int pj_ac_first(const PjScan& S, const PjHuff& T, PjBits& b, uint32_t u0, uint32_t u1, int16_t* coef) {
    uint32_t eobrun = 0;
    for (uint32_t u = u0; u < u1; ++u) {
        if (eobrun) { --eobrun; continue; }
        const uint32_t uy = u / (uint32_t)S.units_x, ux = u - uy * (uint32_t)S.units_x;
        int16_t* blk = pj_block(S, coef, 0, uy, ux);
        for (int k = S.Ss; k <= S.Se; ++k) {
            const int rs = pj_symbol(T, b);
            if (rs < 0) return PJ_BAD_CODE;
            const int r = rs >> 4, s = rs & 15;
            if (s) {
                k += r;
                if (k > S.Se) return PJ_INDEX;
                blk[pj_natural(k)] = pj_scaled(pj_extend(b.get(s), s), S.Al);
            } else if (r == 15) {
                k += 15;                         // ZRL: sixteen zeros (one more by the loop)
            } else {
                eobrun = (1u << r) + b.get(r) - 1u;   // this block ends here; eobrun more blocks are empty
                break;
            }
        }
        if (b.past_end()) return PJ_TRUNCATED;
    }
    return PJ_OK;
}

// the correction bit of a coefficient that is already non-zero (jdphuff.c decode_mcu_AC_refine)
PJ_HD void pj_correct(int16_t* c, uint32_t bit, int32_t p1) {
    if (!bit) return;
    const int32_t v = *c;
    if ((v & p1) == 0) *c = (int16_t)(uint16_t)((uint32_t)(v >= 0 ? v + p1 : v - p1) & 0xffffu);
}

// ---- AC, refinement of a band
PJ_HD int pj_ac_refine(const PjScan& S, const PjHuff& T, PjBits& b, uint32_t u0, uint32_t u1, int16_t* coef) {
    const int32_t p1 = (int32_t)(1u << S.Al);
    uint32_t eobrun = 0;
    for (uint32_t u = u0; u < u1; ++u) {
        const uint32_t uy = u / (uint32_t)S.units_x, ux = u - uy * (uint32_t)S.units_x;
        int16_t* blk = pj_block(S, coef, 0, uy, ux);
        int k = S.Ss;
        if (eobrun == 0) {
            for (; k <= S.Se; ++k) {
                const int rs = pj_symbol(T, b);
                if (rs < 0) return PJ_BAD_CODE;
                int r = rs >> 4;
                const int s = rs & 15;
                int32_t val = 0;
                if (s) {
                    if (s != 1) return PJ_BAD_CODE;
                    val = b.get(1) ? p1 : -p1;
                } else if (r != 15) {
                    eobrun = (1u << r) + b.get(r);    // this block included
                    break;
                }
                // over the coefficients that are already non-zero (a correction bit each) and r that are still zero
                for (; k <= S.Se; ++k) {
                    int16_t* c = blk + pj_natural(k);
                    if (*c) pj_correct(c, b.get(1), p1);
                    else if (--r < 0) break;
                }
                if (s) {
                    if (k > S.Se) return PJ_INDEX;
                    blk[pj_natural(k)] = (int16_t)val;
                }
                if (b.past_end()) return PJ_TRUNCATED;
            }
        }
        if (eobrun) {
            for (; k <= S.Se; ++k) {
                int16_t* c = blk + pj_natural(k);
                if (*c) pj_correct(c, b.get(1), p1);
            }
            --eobrun;
        }
        if (b.past_end()) return PJ_TRUNCATED;
    }
    return PJ_OK;
}

// One segment of a scan: units [u0, u1) from bit position bp0 of bytes[0, nbytes).  tabs: the scan's table set.
PJ_HD int pj_decode_segment(const PjScan& S, const PjHuff* tabs, const uint8_t* bytes, uint64_t nbytes, uint64_t bp0, uint32_t u0,
                            uint32_t u1, int16_t* coef) {
    PjBits b{bytes, nbytes, bp0};
    if (u1 > S.units) u1 = S.units;
    if (S.Ss == 0) return S.Ah == 0 ? pj_dc_first(S, tabs, b, u0, u1, coef) : pj_dc_refine(S, b, u0, u1, coef);
    return S.Ah == 0 ? pj_ac_first(S, tabs[S.ac_tab], b, u0, u1, coef) : pj_ac_refine(S, tabs[S.ac_tab], b, u0, u1, coef);
}

}  // namespace dfd_pj

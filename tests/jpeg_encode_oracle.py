"""ORACLE (test infrastructure only): a baseline JPEG encoder in numpy whose FILE equals what Pillow (libjpeg-turbo) writes
with ``optimize=False``.  The forward steps up to the quantised coefficients come from oracle/jpeg_ref.py; this adds what
that file leaves out, restated from libjpeg's sources:

  jcprepct.c / jcsample.c   edge handling: the right column is replicated out to the width the blocks cover BEFORE the
                            downsample, the last row to a multiple of the vertical factor; AFTER the downsample the last
                            row of every component is replicated down to the block rows (so for an even height that is no
                            multiple of 16 the padding chroma rows are copies of the last real chroma row, which mixes two
                            image rows, not a downsample of replicated image rows); h2v1 with bias 0,1,0,1
  jccoefct.c                blocks an interleaved MCU has beyond the component's real blocks: AC zero, DC copied from the
                            block before them in the MCU, so their DC difference is zero
  jcparam.c                 both base tables at any quality
  jchuff.c                  DC prediction per component (reset at restarts), run/size coding with ZRL and EOB in zig-zag
                            order, MSB-first packing, FF -> FF 00, padding with 1-bits, RSTn
  jcmarker.c                SOI, APP0 JFIF 1.01, DQT per table, SOF0, DHT (DC0 AC0 DC1 AC1), DRI, one interleaved SOS, EOI

PINNED: tests/test_jpeg_encode_oracle.py requires `encode` to equal Pillow's bytes over the corpus of jpeg_encode_cases.py.
"""
from __future__ import annotations

import struct

import numpy as np

from oracle import jpeg_ref as J

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.3: (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
    0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
    0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])

# (horizontal, vertical) factor of the luma component; chroma is always 1x1
MODES = {"gray": None, 0: (1, 1), 1: (2, 1), 2: (2, 2)}


def _derive(table):
    """jchuff.c jpeg_make_c_derived_tbl: symbol -> (code, length)."""
    bits, vals = table
    code, k = 0, 0
    ehufco, ehufsi = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            ehufco[vals[k]], ehufsi[vals[k]] = code, length
            code += 1
            k += 1
        code <<= 1
    return ehufco, ehufsi


def quant_table(base: np.ndarray, quality: int) -> np.ndarray:
    return J.quant_table(base, quality)


def _pad_right(p, cols):
    return p if p.shape[1] >= cols else np.concatenate([p, np.repeat(p[:, -1:], cols - p.shape[1], 1)], 1)


def _pad_bottom(p, rows):
    return p if p.shape[0] >= rows else np.concatenate([p, np.repeat(p[-1:], rows - p.shape[0], 0)], 0)


def h2v1_downsample(p: np.ndarray) -> np.ndarray:
    s = p[:, 0::2] + p[:, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2 == 0, 0, 1)[None, :]
    return (s + bias) >> 1


def component_planes(img: np.ndarray, subsampling):
    """-> [(plane padded to whole blocks, blocks wide, blocks high, h factor, v factor)] per component, and the MCU grid.
    img: (H, W) gray or (H, W, 3) BGR."""
    H, W = img.shape[:2]
    if img.ndim == 2:
        wb, hb = -(-W // 8), -(-H // 8)
        p = _pad_bottom(_pad_right(img.astype(np.int64), wb * 8), hb * 8)
        return [(p, wb, hb, 1, 1)], (wb, hb)
    hs, vs = MODES[subsampling]
    y, cb, cr = J.rgb_to_ycc(img[..., ::-1])
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    out = []
    for c, p in enumerate((y, cb, cr)):
        h, v = (hs, vs) if c == 0 else (1, 1)
        cw, ch = -(-W * h // hs), -(-H * v // vs)                       # the component's real size in samples
        wb, hb = -(-cw // 8), -(-ch // 8)
        if c and (hs, vs) != (1, 1):
            p = _pad_bottom(_pad_right(p, wb * 8 * hs), -(-H // vs) * vs)
            p = J.h2v2_downsample(p) if vs == 2 else h2v1_downsample(p)
        else:
            p = _pad_right(p, wb * 8)
        out.append((_pad_bottom(p, hb * 8), wb, hb, h, v))
    return out, (mx, my)


def scan_blocks(img: np.ndarray, quality: int, subsampling, qtabs=None):
    """The quantised blocks in the order the scan codes them: (coef (n, 64) in zig-zag order, comp (n,) component of each
    block, blocks per MCU, MCU count).  qtabs: one 8x8 table per component instead of the two that `quality` scales."""
    planes, (mx, my) = component_planes(img, subsampling)
    tabs = [quant_table(J._LUMA, quality), quant_table(J._CHROMA, quality)]
    if qtabs is None:
        qtabs = [tabs[0 if c == 0 else 1] for c in range(len(planes))]
    per_comp = []
    for c, (p, wb, hb, h, v) in enumerate(planes):
        q = J.quantize(J.fdct_islow(J._blocks(p - 128)), qtabs[c]).reshape(hb, wb, 64)[..., ZIGZAG]
        full = np.zeros((my * v, mx * h, 64), np.int64)
        full[:hb, :wb] = q
        # dummy blocks (jccoefct.c compress_data): right of the real ones first, then whole dummy rows from the block
        # that precedes them in the MCU (the last block of the row above)
        for bx in range(wb, mx * h):
            full[:hb, bx, 0] = full[:hb, bx - 1, 0]
        for by in range(hb, my * v):
            full[by, :, 0] = np.repeat(full[by - 1, h - 1::h, 0], h)
        per_comp.append(full.reshape(my, v, mx, h, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, v * h, 64))
    coef = np.concatenate(per_comp, 1)
    comp = np.concatenate([np.full(pc.shape[1], c) for c, pc in enumerate(per_comp)])
    bpm = coef.shape[1]
    return coef.reshape(-1, 64), np.tile(comp, mx * my), bpm, mx * my


def _nbits(a):
    a = np.abs(a)
    n = np.zeros(a.shape, np.int64)
    for k in range(12):
        n += (a >> k) > 0
    return n


_TABLES = [(_derive(DC_LUMA), _derive(AC_LUMA)), (_derive(DC_CHROMA), _derive(AC_CHROMA))]


def block_symbols(coef, comp, bpm, restart_blocks, tables=None, comp_table=None):
    """Per block 65 slots (DC, 63 AC positions, EOB) of (bits, length <= 59): the exact bit string of the block is the
    slots' bits in order.  Also the statistics the corpus asserts on.
    tables: [((DC bits, symbols), (AC bits, symbols))] and comp_table: component -> index into it, instead of Annex K's
    luma pair for component 0 and chroma pair for the others.  A slot is built in 62 bits: where three ZRLs, a code and
    its value bits of some other table need more, the call fails; so it does where a block needs a symbol its table lacks."""
    derived = _TABLES if tables is None else [(_derive(d), _derive(a)) for d, a in tables]
    n = coef.shape[0]
    mcu = np.arange(n) // bpm
    pred = np.zeros(n, np.int64)
    for c in np.unique(comp):
        idx = np.nonzero(comp == c)[0]
        dc = coef[idx, 0]
        prev = np.concatenate([[0], dc[:-1]])
        if restart_blocks:
            first = np.concatenate([[True], (mcu[idx][1:] // restart_blocks) != (mcu[idx][:-1] // restart_blocks)])
            prev[first] = 0
        pred[idx] = prev
    t = (comp > 0).astype(np.int64) if comp_table is None else np.asarray(comp_table, np.int64)[comp]
    val = np.zeros((n, 65), np.uint64)
    ln = np.zeros((n, 65), np.int64)
    # DC
    diff = coef[:, 0] - pred
    s = _nbits(diff)
    dco = np.stack([tab[0][0] for tab in derived])
    dsi = np.stack([tab[0][1] for tab in derived])
    assert (dsi[t, s] > 0).all(), "a DC category without a code"
    extra = np.where(diff < 0, diff - 1, diff) & ((1 << s) - 1)
    val[:, 0] = ((dco[t, s] << s) | extra).astype(np.uint64)
    ln[:, 0] = dsi[t, s] + s
    # AC
    aco = np.stack([tab[1][0] for tab in derived])
    asi = np.stack([tab[1][1] for tab in derived])
    ac = coef[:, 1:]
    nz = ac != 0
    pos = np.arange(1, 64)[None, :]
    lastnz = np.maximum.accumulate(np.where(nz, pos, 0), 1)
    prevnz = np.concatenate([np.zeros((n, 1), np.int64), lastnz[:, :-1]], 1)
    run = pos - prevnz - 1
    sz = _nbits(ac)
    tt = t[:, None]
    sym = ((run & 15) << 4) | sz
    zrl = run >> 4
    v = np.zeros((n, 63), np.int64)
    l = np.zeros((n, 63), np.int64)
    for k in range(3):
        m = zrl > k
        v = np.where(m, (v << asi[tt, 0xF0]) | aco[tt, 0xF0], v)
        l = l + m * asi[tt, 0xF0]
    v = (v << asi[tt, sym]) | aco[tt, sym]
    l = l + asi[tt, sym]
    extra = np.where(ac < 0, ac - 1, ac) & ((1 << sz) - 1)
    v = (v << sz) | extra
    l = l + sz
    val[:, 1:64] = np.where(nz, v, 0).astype(np.uint64)
    ln[:, 1:64] = np.where(nz, l, 0)
    eob = lastnz[:, -1] < 63
    assert (asi[tt, sym][nz] > 0).all() and (np.broadcast_to(asi[tt, 0xF0], nz.shape)[nz & (zrl > 0)] > 0).all() and (asi[t, 0][eob] > 0).all(), \
        "a run/size symbol without a code"
    assert int(np.where(nz, l, 0).max(initial=0)) <= 62, "a slot longer than 62 bits"
    val[:, 64] = np.where(eob, aco[t, 0], 0).astype(np.uint64)
    ln[:, 64] = np.where(eob, asi[t, 0], 0)
    stats = dict(zrl=int((zrl * nz).sum()), max_ac_size=int((sz * nz).max(initial=0)),
                 eob_only=int((~nz.any(1)).sum()), max_block_bits=int(ln.sum(1).max()))
    return val, ln, stats


def _pack(val, ln):
    """Slots of one restart interval -> its bytes before stuffing, padded with 1-bits."""
    val, ln = val.ravel(), ln.ravel()
    keep = ln > 0
    val, ln = val[keep], ln[keep]
    start = np.cumsum(ln) - ln
    total = int(ln.sum())
    owner = np.repeat(np.arange(len(ln)), ln)
    j = np.arange(total) - start[owner]
    bits = ((val[owner] >> (ln[owner] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
    return np.packbits(bits)


def _stuff(raw):
    ff = raw == 0xFF
    out = np.zeros(len(raw) + int(ff.sum()), np.uint8)
    out[np.arange(len(raw)) + np.cumsum(ff) - ff] = raw
    return out.tobytes(), int(ff.sum())


def _dht(cls, ident, table):
    bits, vals = table
    return b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), (cls << 4) | ident) + bytes(bits) + bytes(vals)


def header(H, W, quality, subsampling, restart_blocks):
    gray = subsampling == "gray"
    out = b"\xff\xd8\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i, base in enumerate((J._LUMA,) if gray else (J._LUMA, J._CHROMA)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(quant_table(base, quality).reshape(64)[ZIGZAG].astype(np.uint8))
    nc = 1 if gray else 3
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * nc, 8, H, W, nc)
    hs, vs = (1, 1) if gray else MODES[subsampling]
    for c in range(nc):
        out += bytes([c + 1, (hs << 4) | vs if c == 0 else 0x11, 0 if c == 0 else 1])
    out += _dht(0, 0, DC_LUMA) + _dht(1, 0, AC_LUMA)
    if not gray:
        out += _dht(0, 1, DC_CHROMA) + _dht(1, 1, AC_CHROMA)
    if restart_blocks:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart_blocks)
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * nc, nc)
    for c in range(nc):
        out += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return out + b"\x00\x3f\x00"


def encode_with_stats(img: np.ndarray, quality: int, subsampling, restart_blocks: int = 0):
    """img: (H, W) gray u8 or (H, W, 3) BGR u8; subsampling 0 (4:4:4), 1 (4:2:2), 2 (4:2:0), ignored for gray."""
    img = np.asarray(img)
    if img.ndim == 2:
        subsampling = "gray"
    coef, comp, bpm, nmcu = scan_blocks(img, quality, subsampling)
    val, ln, stats = block_symbols(coef, comp, bpm, restart_blocks)
    per = (restart_blocks or nmcu) * bpm
    out, stuffed = header(img.shape[0], img.shape[1], quality, subsampling, restart_blocks), 0
    for i, b0 in enumerate(range(0, nmcu * bpm, per)):
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        data, n_ff = _stuff(_pack(val[b0:b0 + per], ln[b0:b0 + per]))
        out += data
        stuffed += n_ff
    stats["stuffed"] = stuffed
    return out + b"\xff\xd9", stats


def encode(bgr_or_gray: np.ndarray, quality: int, subsampling=2, restart_blocks: int = 0) -> bytes:
    return encode_with_stats(bgr_or_gray, quality, subsampling, restart_blocks)[0]


def pillow_bytes(bgr_or_gray: np.ndarray, quality: int, subsampling=2, restart_blocks: int = 0) -> bytes:
    """The pin: Pillow's non-optimised save of the same pixels."""
    import io

    from PIL import Image

    a = np.asarray(bgr_or_gray)
    im = Image.fromarray(a if a.ndim == 2 else np.ascontiguousarray(a[..., ::-1]))
    buf = io.BytesIO()
    kw = dict(restart_marker_blocks=restart_blocks) if restart_blocks else {}
    if a.ndim == 3:
        kw["subsampling"] = subsampling
    im.save(buf, format="JPEG", quality=quality, optimize=False, **kw)
    return buf.getvalue()

"""TEST INFRASTRUCTURE: a baseline JPEG written from explicit parts, for the dialects that are valid but that Pillow never
writes (other Huffman tables and table ids, 16-bit quantisation tables, component ids, APP14, fill bytes, one DHT for all
tables, DRI 0, coefficient blocks chosen by hand).  The forward path, the symbol coding, the packing and the stuffing are
jpeg_encode_oracle's; this file adds the choice of every table and id and the marker layout.

PINNED: with libjpeg's defaults (`defaults(...)`) the bytes equal jpeg_encode_oracle.encode, which is itself pinned to
Pillow's bytes (tests/test_jpeg_streams.py::test_writer_with_defaults_equals_the_encode_oracle).
"""
from __future__ import annotations

import itertools
import struct
from dataclasses import dataclass, field

import numpy as np

import jpeg_encode_oracle as O
from oracle import jpeg_ref as J


# ------------------------------------------------------------------------------------------------ Huffman tables
def reversed_table(t):
    """the same code lengths, the symbols in reverse order: the common symbols get the long codes"""
    bits, vals = t
    return (list(bits), list(vals)[::-1])


def table_of(symbols):
    """A table that holds exactly `symbols`: all codes of one length, the shortest at which the all-ones code stays free
    (one symbol: a single 1-bit code, "0")."""
    vals = sorted(set(int(s) for s in symbols))
    length = 1
    while (1 << length) < len(vals) + 1:
        length += 1
    bits = [0] * 16
    bits[length - 1] = len(vals)
    return (bits, vals)


def check_table(t):
    """the lengths satisfy Kraft (jdhuff.c refuses other tables), no code is all ones (T.81 C.2), no symbol twice"""
    bits, vals = t
    assert len(bits) == 16 and sum(bits) == len(vals) and len(set(vals)) == len(vals) and 1 <= len(vals) <= 256
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        assert code <= (1 << length), f"over-subscribed at length {length}"
        assert not (bits[length - 1] and code == (1 << length)), f"the last code of length {length} is all ones"
        code <<= 1


def used_symbols(coef, comp, bpm, restart_mcus=0):
    """{component: (DC categories, AC run/size symbols incl. ZRL 0xF0 and EOB 0x00)} of a scan's blocks (n, 64) in zig-zag
    order, the DC prediction reset every `restart_mcus` MCUs"""
    out = {}
    mcu = np.arange(len(coef)) // bpm
    for c in np.unique(comp):
        idx = np.nonzero(comp == c)[0]
        dc = coef[idx, 0]
        prev = np.concatenate([[0], dc[:-1]])
        if restart_mcus:
            seg = mcu[idx] // restart_mcus
            prev[np.concatenate([[True], seg[1:] != seg[:-1]])] = 0
        dcs = set(O._nbits(dc - prev).tolist())
        acs = set()
        ac = coef[idx, 1:]
        busy = (ac != 0).any(1)
        if not busy.all():
            acs.add(0x00)
        for row in ac[busy]:
            run = 0
            for v in row:
                if v == 0:
                    run += 1
                    continue
                if run >= 16:
                    acs.add(0xF0)
                acs.add(((run & 15) << 4) | int(O._nbits(np.array([v]))[0]))
                run = 0
            if run:
                acs.add(0x00)
        out[int(c)] = (dcs, acs)
    return out


# ------------------------------------------------------------------------------------------------ the stream
@dataclass
class Comp:
    id: int                                      # component id of SOF / SOS
    h: int
    v: int
    tq: int                                      # table ids
    td: int
    ta: int


@dataclass
class Stream:
    """Everything a file is written from.  qtables: {id: (8x8 natural order, 16-bit?)}; dc / ac: {id: (bits, symbols)}."""
    height: int
    width: int
    comps: list
    qtables: dict
    dc: dict
    ac: dict
    jfif: bool = True
    adobe: int | None = None                     # APP14 "Adobe" with this transform byte
    one_dht: bool = False                        # all Huffman tables in one DHT segment
    one_dqt: bool = False
    between: list = field(default_factory=list)  # segments (whole, marker included) put in turn between the header segments
    fill: list = field(default_factory=list)     # FF fill bytes in front of the markers after SOI, in turn (empty: none)
    dri: int | None = None                       # None: no DRI segment; any value is written as it is
    after_eoi: bytes = b""
    precision: int = 8
    sof: int = 0xC0


def segment(marker, body):
    assert len(body) + 2 <= 65535
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def com(text=b"written by tests/jpeg_stream_writer.py"):
    return segment(0xFE, text)


def appn(n, size):
    """an APPn segment of `size` payload bytes (65,533 is the most a segment holds)"""
    return segment(0xE0 + n, bytes((7 * i + 1) & 0xFF for i in range(size)))


def _header_segments(S: Stream):
    segs = []
    if S.jfif:
        segs.append(segment(0xE0, struct.pack(">5sBBBHHBB", b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)))
    if S.adobe is not None:
        segs.append(segment(0xEE, struct.pack(">5sHHHB", b"Adobe", 100, 0, 0, S.adobe)))
    dqt = []
    for tq in dict.fromkeys(c.tq for c in S.comps):                # jcmarker.c: per component, each table once
        q, wide = S.qtables[tq]
        zz = np.asarray(q).reshape(64)[O.ZIGZAG]
        assert zz.min() >= 1 and zz.max() <= (65535 if wide else 255)
        dqt.append(bytes([(16 if wide else 0) | tq]) + (zz.astype(">u2").tobytes() if wide else bytes(zz.astype(np.uint8))))
    segs += [segment(0xDB, b"".join(dqt))] if S.one_dqt else [segment(0xDB, d) for d in dqt]
    nc = len(S.comps)
    sof = struct.pack(">BHHB", S.precision, S.height, S.width, nc)
    for c in S.comps:
        sof += bytes([c.id, (c.h << 4) | c.v, c.tq])
    segs.append(segment(S.sof, sof))
    dht, sent = [], set()
    for c in S.comps:                                              # DC then AC of each component, each table once
        for cls, ident, table in ((0, c.td, S.dc[c.td]), (1, c.ta, S.ac[c.ta])):
            if (cls, ident) not in sent:
                sent.add((cls, ident))
                check_table(table)
                dht.append(bytes([(cls << 4) | ident]) + bytes(table[0]) + bytes(table[1]))
    segs += [segment(0xC4, b"".join(dht))] if S.one_dht else [segment(0xC4, d) for d in dht]
    if S.dri is not None:
        segs.append(segment(0xDD, struct.pack(">H", S.dri)))
    sos = bytes([nc])
    for c in S.comps:
        sos += bytes([c.id, (c.td << 4) | c.ta])
    segs.append(segment(0xDA, sos + b"\x00\x3f\x00"))
    return segs


def interleave(fulls, comps):
    """per component (blocks high, blocks wide, 64) with MCU padding -> the scan's order: (coef (n, 64), comp (n,), blocks
    per MCU, MCUs)"""
    my, mx = fulls[0].shape[0] // comps[0].v, fulls[0].shape[1] // comps[0].h
    per = []
    for f, c in zip(fulls, comps):
        assert f.shape == (my * c.v, mx * c.h, 64)
        per.append(f.reshape(my, c.v, mx, c.h, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, c.v * c.h, 64))
    coef = np.concatenate(per, 1)
    comp = np.concatenate([np.full(p.shape[1], i) for i, p in enumerate(per)])
    return coef.reshape(-1, 64).astype(np.int64), np.tile(comp, mx * my), coef.shape[1], mx * my


def write(S: Stream, coef, comp, bpm, nmcu) -> bytes:
    """the file of stream S around the scan of blocks `coef` (n, 64) in zig-zag order, `comp` the component of each"""
    restart = S.dri if S.dri and S.dri < nmcu else 0                # (a DRI of 0 or past the last MCU: one segment, no RSTn)
    pairs = list(dict.fromkeys((c.td, c.ta) for c in S.comps))
    val, ln, _ = O.block_symbols(coef, comp, bpm, restart, tables=[(S.dc[d], S.ac[a]) for d, a in pairs],
                                 comp_table=[pairs.index((c.td, c.ta)) for c in S.comps])
    fills = itertools.cycle(S.fill or [0])

    def marked(b):                                                  # b starts with its marker
        return b"\xff" * next(fills) + b

    out = b"\xff\xd8"
    segs = _header_segments(S)
    for i, s in enumerate(segs):
        out += marked(s)
        if S.between and i + 1 < len(segs):
            out += marked(S.between[i % len(S.between)])
    per = (restart or nmcu) * bpm
    for i, b0 in enumerate(range(0, nmcu * bpm, per)):
        if i:
            out += marked(bytes([0xFF, 0xD0 + (i - 1) % 8]))
        out += O._stuff(O._pack(val[b0:b0 + per], ln[b0:b0 + per]))[0]           # padded with 1-bits, as libjpeg pads
    return out + marked(b"\xff\xd9") + S.after_eoi


# ------------------------------------------------------------------------------------------------ libjpeg's defaults
def defaults(height, width, subsampling, quality) -> Stream:
    """the stream Pillow writes with optimize=False: JFIF, DQT 0 / 1, components 1, 2, 3, the Annex K tables 0 / 1"""
    ql, qc = O.quant_table(J._LUMA, quality), O.quant_table(J._CHROMA, quality)
    if subsampling == "gray":
        return Stream(height, width, [Comp(1, 1, 1, 0, 0, 0)], {0: (ql, False)}, {0: O.DC_LUMA}, {0: O.AC_LUMA})
    hs, vs = O.MODES[subsampling]
    comps = [Comp(1, hs, vs, 0, 0, 0), Comp(2, 1, 1, 1, 1, 1), Comp(3, 1, 1, 1, 1, 1)]
    return Stream(height, width, comps, {0: (ql, False), 1: (qc, False)}, {0: O.DC_LUMA, 1: O.DC_CHROMA},
                  {0: O.AC_LUMA, 1: O.AC_CHROMA})


def from_pixels(S: Stream, img, subsampling) -> bytes:
    """img (H, W) gray or (H, W, 3) BGR through the oracle's forward path with S's quantisation tables and sampling"""
    img = np.asarray(img)
    if img.ndim == 2:
        subsampling = "gray"
    assert img.shape[:2] == (S.height, S.width)
    assert [(c.h, c.v) for c in S.comps] == ([(1, 1)] if subsampling == "gray" else [O.MODES[subsampling], (1, 1), (1, 1)])
    coef, comp, bpm, nmcu = O.scan_blocks(img, 0, subsampling, qtabs=[np.asarray(S.qtables[c.tq][0]) for c in S.comps])
    return write(S, coef, comp, bpm, nmcu)


def from_blocks(S: Stream, fulls) -> bytes:
    """fulls: per component the quantised blocks (blocks high, blocks wide, 64) in zig-zag order, MCU padding included"""
    return write(S, *interleave(fulls, S.comps))

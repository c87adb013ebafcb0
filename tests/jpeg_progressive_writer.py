"""TEST INFRASTRUCTURE: a progressive JPEG (SOF2) written from given quantised coefficients under a given scan script, for
the scripts Pillow never writes (spectral selection only, DC per component, other bands, two refinement levels, scripts
that are out of order or incomplete).  The coding is T.81 annex G as libjpeg's jcphuff.c does it: point transform by
arithmetic shift for DC and by division towards zero for AC, end-of-band runs flushed at 32767, correction bits buffered
behind the symbol they follow.  Every scan gets fresh Huffman tables in a DHT of its own in front of its SOS, under
alternating table ids: all codes of one length (jpeg_stream_writer.table_of), DC categories 0..11, AC every run/size up
to size 10 plus ZRL and the EOBn symbols.

PINNED (tests/test_jpeg_progressive.py): Pillow decodes these files to the same pixels as the baseline file that
tests/jpeg_stream_writer.py makes of the same coefficients.

A script is a list of scans (components, Ss, Se, Ah, Al), components as indices into the stream's."""
import struct

import numpy as np

import jpeg_stream_writer as W

DC_SYMBOLS = list(range(12))
AC_SYMBOLS = [(r << 4) | s for r in range(16) for s in range(11)]


def libjpeg_script(ncomp):
    """jcparam.c jpeg_simple_progression"""
    if ncomp == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
            ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


class _Out:
    def __init__(self, table):
        length = next((l + 1 for l, n in enumerate(table[0]) if n), 0) if table else 0
        self.code = {s: (i, length) for i, s in enumerate(table[1])} if table else {}
        self.bits = []

    def put(self, value, n):
        if n:
            self.bits.append(format(value & ((1 << n) - 1), "0%db" % n))

    def symbol(self, s):
        code, n = self.code[s]
        self.put(code, n)

    def bytes(self):
        text = "".join(self.bits)
        text += "1" * (-len(text) % 8)
        raw = int(text, 2).to_bytes(len(text) // 8, "big") if text else b""
        return raw.replace(b"\xff", b"\xff\x00")


def _size(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, n):
    v = int(v)
    return v if v >= 0 else v + (1 << n) - 1


def _scan_bytes(S, fulls, scan, tables):
    comps, Ss, Se, Ah, Al = scan
    hmax, vmax = S.comps[0].h, S.comps[0].v
    if Ss == 0:
        out = _Out(tables)
        if len(comps) == 1:
            c = S.comps[comps[0]]
            wc, hc = -(-S.width * c.h // hmax), -(-S.height * c.v // vmax)
            order = [(comps[0], r, x) for r in range(-(-hc // 8)) for x in range(-(-wc // 8))]
        else:
            my, mx = fulls[0].shape[0] // vmax, fulls[0].shape[1] // hmax
            order = [(ci, y * S.comps[ci].v + by, x * S.comps[ci].h + bx) for y in range(my) for x in range(mx) for ci in comps
                     for by in range(S.comps[ci].v) for bx in range(S.comps[ci].h)]
        pred = {ci: 0 for ci in comps}
        for ci, r, x in order:
            v = int(fulls[ci][r, x, 0])
            if Ah:
                out.put((v >> Al) & 1, 1)
                continue
            t = v >> Al                                             # arithmetic shift (jcphuff.c encode_mcu_DC_first)
            d = t - pred[ci]
            pred[ci] = t
            n = _size(d)
            out.symbol(n)
            out.put(_value_bits(d, n), n)
        return out.bytes()
    (ci,) = comps
    c = S.comps[ci]
    wc, hc = -(-S.width * c.h // hmax), -(-S.height * c.v // vmax)
    out = _Out(tables)
    eobrun, pending = 0, []                                         # pending: correction bits behind the end-of-band run

    def flush():
        nonlocal eobrun, pending
        if eobrun:
            n = eobrun.bit_length() - 1
            out.symbol(n << 4)
            out.put(eobrun, n)
            eobrun = 0
        for b in pending:
            out.put(b, 1)
        pending = []

    for r in range(-(-hc // 8)):
        for x in range(-(-wc // 8)):
            blk = [int(v) for v in fulls[ci][r, x]]
            mag = [abs(v) >> Al for v in blk]
            if Ah == 0:
                run = 0
                for k in range(Ss, Se + 1):
                    if mag[k] == 0:
                        run += 1
                        continue
                    flush()
                    while run > 15:
                        out.symbol(0xF0)
                        run -= 16
                    n = mag[k].bit_length()
                    out.symbol((run << 4) | n)
                    out.put(mag[k] if blk[k] >= 0 else (~mag[k]), n)
                    run = 0
                if run:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        flush()
                continue
            eob = max([k for k in range(Ss, Se + 1) if mag[k] == 1], default=-1)
            run, local = 0, []
            for k in range(Ss, Se + 1):
                if mag[k] == 0:
                    run += 1
                    continue
                while run > 15 and k <= eob:
                    flush()
                    out.symbol(0xF0)
                    run -= 16
                    for b in local:
                        out.put(b, 1)
                    local = []
                if mag[k] > 1:
                    local.append(mag[k] & 1)
                    continue
                flush()
                out.symbol((run << 4) | 1)
                out.put(0 if blk[k] < 0 else 1, 1)
                for b in local:
                    out.put(b, 1)
                local = []
                run = 0
            if run or local:
                eobrun += 1
                pending += local
                if eobrun == 0x7FFF or len(pending) > 1000 - 64 + 1:
                    flush()
    flush()
    return out.bytes()


def write(S: W.Stream, fulls, script, eoi=True) -> bytes:
    """S: a jpeg_stream_writer.Stream (its size, components, quantisation tables, JFIF); fulls: per component the quantised
    blocks (blocks high, blocks wide, 64) in zig-zag order with MCU padding, as jpeg_stream_writer.from_blocks takes them"""
    out = b"\xff\xd8"
    if S.jfif:
        out += W.segment(0xE0, struct.pack(">5sBBBHHBB", b"JFIF\0", 1, 1, 0, 1, 1, 0, 0))
    for tq in dict.fromkeys(c.tq for c in S.comps):
        q, wide = S.qtables[tq]
        assert not wide
        out += W.segment(0xDB, bytes([tq]) + bytes(np.asarray(q).reshape(64)[W.O.ZIGZAG].astype(np.uint8)))
    sof = struct.pack(">BHHB", 8, S.height, S.width, len(S.comps))
    for c in S.comps:
        sof += bytes([c.id, (c.h << 4) | c.v, c.tq])
    out += W.segment(0xC2, sof)
    dc_table, ac_table = W.table_of(DC_SYMBOLS), W.table_of(AC_SYMBOLS)
    for i, scan in enumerate(script):
        comps, Ss, Se, Ah, Al = scan
        tid = i & 1                                                 # alternating ids: the table in force at each SOS is that scan's
        table = None
        if Ss == 0 and Ah == 0:
            table = dc_table
            out += W.segment(0xC4, bytes([tid]) + bytes(table[0]) + bytes(table[1]))
        elif Ss > 0:
            table = ac_table
            out += W.segment(0xC4, bytes([0x10 | tid]) + bytes(table[0]) + bytes(table[1]))
        sos = bytes([len(comps)])
        for ci in comps:
            sos += bytes([S.comps[ci].id, (tid << 4) | tid])
        out += W.segment(0xDA, sos + bytes([Ss, Se, (Ah << 4) | Al]))
        out += _scan_bytes(S, fulls, scan, table)
    return out + (b"\xff\xd9" if eoi else b"")

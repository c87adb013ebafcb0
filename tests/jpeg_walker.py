"""TEST INFRASTRUCTURE: the verdict on a baseline JPEG's entropy-coded data, by a plain sequential walk after ITU-T T.81
F.2.2 (one bit position, block after block, no chunks, no threads).  It shares no code with csrc/jpeg_entropy.h or
csrc/jpeg_gpu_entropy.h and is the reference for "accept or reject" in tests/test_jpeg_damage_cases.py and
tests/test_jpeg_damage_gpu.py.

walk(data) ->
    Ok(blocks, frame)           all `total` blocks of the scan: (total, 64) in scan order, zig-zag positions, DC integrated
    Defect(kind, block, bit)    the first "code" (a bit pattern that is no code of the table in force), "index" (a run that
                                carries the coefficient index past 63) or "dccat" (a DC category above 11: an 8-bit file has
                                none) inside one of the `total` blocks; bit = de-stuffed position of the offending symbol
    Short(blocks)               the data ended after `blocks` complete blocks
tally(data) -> (block of the first defect or None, complete blocks up to the END of the data) for a file without restart
interval, walking on behind a defect the way both decoders of the library define it (an unassigned code: 16 bits, symbol
0; an index past 63: the block ends; a DC category s > 11: s & 7 value bits) and behind the last block: what the seeded
bit flips of tests/jpeg_damage_cases.py are sorted by (does the block total survive the flip?), never a verdict.
Bits behind the last block are not examined by walk().  A run of ZRLs that carries the index from 49 .. 63 past 63 ends the block, as
in libjpeg (jdhuff.c) and both decoders of the library.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Ok = namedtuple("Ok", "blocks frame")
Defect = namedtuple("Defect", "kind block bit")
Short = namedtuple("Short", "blocks")
Frame = namedtuple("Frame", "height width comps restart scan mcux mcuy bpm total slots")   # comps: [(h, v, dc table, ac table)]

_NATURAL = np.array([[0, 1, 5, 6, 14, 15, 27, 28], [2, 4, 7, 13, 16, 26, 29, 42], [3, 8, 12, 17, 25, 30, 41, 43],
                     [9, 11, 18, 24, 31, 40, 44, 53], [10, 19, 23, 32, 39, 45, 52, 54], [20, 22, 33, 38, 46, 51, 55, 60],
                     [21, 34, 37, 47, 50, 56, 59, 61], [35, 36, 48, 49, 57, 58, 62, 63]]).reshape(64)   # T.81 figure A.6
_luts = {}


def _lut(bits, vals):
    """16 bits of the stream -> (code length, symbol); length 0: no code of this table begins so (T.81 C.2, F.2.2.3)"""
    key = (tuple(bits), tuple(vals))
    if key not in _luts:
        ln, sy = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                ln[code << (16 - length):(code + 1) << (16 - length)] = length
                sy[code << (16 - length):(code + 1) << (16 - length)] = vals[k]
                code, k = code + 1, k + 1
            code <<= 1
        _luts[key] = (ln.tolist(), sy.tolist())
    return _luts[key]


def parse(data: bytes) -> Frame:
    assert data[:2] == b"\xff\xd8"
    pos, tables, comps, restart, size = 2, {}, None, 0, None
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m, n = data[pos], int.from_bytes(data[pos + 1:pos + 3], "big")
        s = data[pos + 3:pos + 1 + n]
        pos += 1 + n
        if m == 0xC4:
            i = 0
            while i < len(s):
                bits = list(s[i + 1:i + 17])
                tables[s[i] >> 4, s[i] & 15] = (bits, list(s[i + 17:i + 17 + sum(bits)]))
                i += 17 + sum(bits)
        elif m in (0xC0, 0xC1):
            size = (int.from_bytes(s[1:3], "big"), int.from_bytes(s[3:5], "big"))
            comps = [[s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15] for c in range(s[5])]
        elif m == 0xDD:
            restart = int.from_bytes(s[:2], "big")
        elif m == 0xDA:
            assert s[0] == len(comps) and all(s[1 + 2 * c] == comps[c][0] for c in range(s[0]))
            sel = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]
            break
    if len(comps) == 1:
        comps[0][1:] = [1, 1]
    cs = [(h, v, _lut(*tables[0, td]), _lut(*tables[1, ta])) for (_, h, v), (td, ta) in zip(comps, sel)]
    hmax, vmax = max(c[0] for c in cs), max(c[1] for c in cs)
    mcux, mcuy = -(-size[1] // (8 * hmax)), -(-size[0] // (8 * vmax))
    slots = [(c, bx, by) for c, (h, v, _, _) in enumerate(cs) for by in range(v) for bx in range(h)]
    return Frame(size[0], size[1], cs, restart, pos, mcux, mcuy, len(slots), mcux * mcuy * len(slots), slots)


def destuff(scan: bytes, restart: int):
    """the payload per restart segment: FF 00 -> FF, FF FF: a fill byte, RSTn: the next segment (with a restart interval),
    any other marker or a final FF: the end"""
    segs, cur, i = [], bytearray(), 0
    while i < len(scan):
        b = scan[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif i + 1 >= len(scan):
            break
        elif scan[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif scan[i + 1] == 0xFF:
            i += 1
        elif restart and 0xD0 <= scan[i + 1] <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            break
    return segs + [bytes(cur)]


def walk(data: bytes):
    fr = parse(data)
    segs = destuff(data[fr.scan:], fr.restart)
    per = (fr.restart if fr.restart else fr.mcux * fr.mcuy) * fr.bpm
    blocks = np.zeros((fr.total, 64), np.int64)
    b, base = 0, 0
    for seg in segs:
        nbits, buf, p, pred = 8 * len(seg), seg + bytes(4), 0, [0, 0, 0]
        for _ in range(min(per, fr.total - b)):
            c = fr.slots[b % fr.bpm][0]
            k = 0
            while k < 64:
                (ln, sy) = fr.comps[c][2 if k == 0 else 3]
                w = (int.from_bytes(buf[p >> 3:(p >> 3) + 3], "big") >> (8 - (p & 7))) & 0xFFFF
                length = ln[w]
                if p + (length or 16) > nbits:
                    return Short(b)
                if length == 0:
                    return Defect("code", b, base + p)
                rs = sy[w]
                r, s = (0, rs) if k == 0 else (rs >> 4, rs & 15)
                if k == 0 and s > 11:
                    return Defect("dccat", b, base + p)
                if k and s == 0:
                    p += length
                    k = k + 16 if r == 15 else 64
                    continue
                if k + r > 63:
                    return Defect("index", b, base + p)
                if p + length + s > nbits:
                    return Short(b)
                q = p + length
                v = (int.from_bytes(buf[q >> 3:(q >> 3) + 4], "big") >> (32 - (q & 7) - s)) & ((1 << s) - 1) if s else 0
                if s and v < (1 << (s - 1)):
                    v -= (1 << s) - 1
                p = q + s
                if k == 0:
                    pred[c] += v
                    v = pred[c]
                blocks[b, k + r] = v
                k += r + 1
            b += 1
        base += nbits
        if b == fr.total:
            return Ok(blocks, fr)
    return Short(b)


def tally(data: bytes, p0=0, n0=0):
    """(p0, n0): begin at a known block boundary (bit position, blocks in front of it)"""
    fr = parse(data)
    assert not fr.restart
    seg = destuff(data[fr.scan:], 0)[0]
    nbits, buf, p, n, k, first = 8 * len(seg), seg + bytes(8), p0, n0, 0, None
    while p < nbits:
        ln, sy = fr.comps[fr.slots[n % fr.bpm][0]][2 if k == 0 else 3]
        w = (int.from_bytes(buf[p >> 3:(p >> 3) + 3], "big") >> (8 - (p & 7))) & 0xFFFF
        length, rs, bad = (ln[w], sy[w], False) if ln[w] else (16, 0, True)
        r, s = (0, rs) if k == 0 else (rs >> 4, rs & 15)
        if k == 0 and s > 11:
            bad, s = True, s & 7
        p += length + s
        if p > nbits:
            break
        if k == 0:
            k = 1
        elif s == 0:
            k = k + 16 if r == 15 else 64
        elif k + r > 63:
            bad, k = True, 64
        else:
            k += r + 1
        if bad and first is None:
            first = n
        if k >= 64:
            k, n = 0, n + 1
    return first, n


def library_order(res: Ok):
    """the blocks as dfd_jpeg_coefficients lays them out: per component its block grid (MCU padding included) row-major,
    64 coefficients in natural order, int16"""
    fr, out = res.frame, []
    grids = [np.zeros((fr.mcuy * v, fr.mcux * h, 64), np.int64) for h, v, _, _ in fr.comps]
    for g, blk in enumerate(res.blocks):
        c, bx, by = fr.slots[g % fr.bpm]
        my, mx = divmod(g // fr.bpm, fr.mcux)
        grids[c][my * fr.comps[c][1] + by, mx * fr.comps[c][0] + bx] = blk[_NATURAL]
    for g in grids:
        out.append(g.reshape(-1))
    return np.concatenate(out).astype(np.int16)

"""TEST INFRASTRUCTURE: a plain sequential decoder of progressive JPEG (T.81 G.2 with the procedures of annex F), one
symbol at a time, in Python.  It shares no code with csrc/: its own marker walk, its own Huffman decoding (a dictionary of
(length, code)), its own bit reader, its own block addressing.  tests/test_jpeg_progressive.py pins it first - on every
Pillow-written file of the corpus `oracle.jpeg_ref.decode_from_coefficients(decode(file))` equals Pillow's pixels - and then
holds the library's coefficients to it.

decode(data) -> the dict `_lib.jpeg_coefficients` returns (coefficients int16 in natural order, 64 per block, blocks
row-major per component on the MCU-padded grid, components concatenated), or raises
    Defect    the first thing wrong with the bytes (no code, an index past Se, a DC category above 11, data that ends
              before a scan's last block, a malformed segment), or
    Refused   a file that is sound but that the decoder under test does not take (script out of order or incomplete, 12
              bits, ...).
It decodes what the bytes say and nothing else: bits behind the end of a segment read as zero and make the segment a
Defect once a block has used one; an end-of-band run never crosses a restart marker."""
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Defect(Exception):
    pass


class Refused(Exception):
    pass


def _huffman(bits, vals):
    """{(length, code): symbol} by T.81 C.2; None when the lengths over-subscribe the code space"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        if code + bits[length - 1] > (1 << length):
            return None
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self, data, start, end):
        self.d = data                           # zero bytes follow the payload
        self.pos = start * 8
        self.end = end * 8

    def bit(self):
        p = self.pos
        self.pos = p + 1
        if p >= self.end:
            return 0
        return (self.d[p >> 3] >> (7 - (p & 7))) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise Defect("a bit pattern that is no code")

    def check(self):
        if self.pos > self.end:
            raise Defect("the data ends inside a block")


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _i16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def _destuff(data, pos):
    """entropy-coded bytes from pos -> (payload without stuffing and RSTn, segment starts, position of the marker that ends it)"""
    out, starts, n = bytearray(), [0], len(data)
    while pos < n:
        f = data.find(b"\xff", pos)
        if f < 0:
            out += data[pos:]
            pos = n
            break
        out += data[pos:f]
        if f + 1 >= n:
            pos = n
            break
        m = data[f + 1]
        if m == 0:
            out.append(0xFF)
            pos = f + 2
        elif 0xD0 <= m <= 0xD7:
            starts.append(len(out))
            pos = f + 2
        elif m == 0xFF:
            pos = f + 1
        else:
            pos = f
            break
    return bytes(out), starts, pos


def decode(data: bytes) -> dict:
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Defect("no SOI")
    pos, n = 2, len(data)
    q = np.zeros((4, 64), np.uint16)
    qseen = [False] * 4
    dc, ac = {}, {}
    frame = None
    restart = 0
    coef = None
    prec = None
    nscans = 0
    jfif = adobe = False
    adobe_transform = 0
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            raise Defect("marker expected")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            break
        m = data[pos]
        pos += 1
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m == 0xD9:
            break
        if pos + 2 > n:
            break
        seg = struct.unpack(">H", data[pos:pos + 2])[0]
        if seg < 2 or pos + seg > n:
            raise Defect("truncated segment")
        s = data[pos + 2:pos + seg]
        if m == 0xDB:
            i = 0
            while i < len(s):
                pq, tq = s[i] >> 4, s[i] & 15
                i += 1
                size = 128 if pq else 64
                if tq > 3 or i + size > len(s):
                    raise Defect("bad DQT")
                if nscans and qseen[tq]:
                    raise Refused("quantisation table redefined between scans")
                for k in range(64):
                    q[tq, ZIGZAG[k]] = struct.unpack(">H", s[i + 2 * k:i + 2 * k + 2])[0] if pq else s[i + k]
                qseen[tq] = True
                i += size
        elif m == 0xC4:
            i = 0
            while i + 17 <= len(s):
                tc, th = s[i] >> 4, s[i] & 15
                bits = list(s[i + 1:i + 17])
                total = sum(bits)
                if tc > 1 or th > 3 or total > 256 or i + 17 + total > len(s):
                    raise Defect("bad DHT")
                t = _huffman(bits, list(s[i + 17:i + 17 + total]))
                if t is None:
                    raise Defect("bad DHT: over-subscribed")
                (ac if tc else dc)[th] = t
                i += 17 + total
        elif m == 0xC2 and frame is None:
            if len(s) < 6 or s[0] != 8:
                raise Refused("sample precision")
            H, W, nc = struct.unpack(">HHB", s[1:6])
            if nc not in (1, 3):
                raise Refused("components")
            if len(s) < 6 + 3 * nc or W <= 0 or H <= 0:
                raise Defect("bad SOF")
            comps = []
            for c in range(nc):
                ident, hv, tq = s[6 + 3 * c:9 + 3 * c]
                if tq > 3:
                    raise Defect("bad quantisation table index")
                comps.append([ident, hv >> 4, hv & 15, tq])
            frame = (W, H, comps)
            prec = [[-1] * 64 for _ in range(nc)]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if frame is not None:
                raise Defect("second SOF")
            raise Refused("not a progressive Huffman file")
        elif m == 0xE0:
            if len(s) >= 14 and s[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe":
                adobe, adobe_transform = True, s[11]
        elif m == 0xDD:
            if len(s) >= 2:
                restart = struct.unpack(">H", s[:2])[0]
        elif m == 0xDA:
            if frame is None:
                raise Defect("SOS before SOF")
            W, H, comps = frame
            if coef is None:
                # geometry, once: the first scan needs it
                if len(comps) == 1:
                    comps[0][1] = comps[0][2] = 1
                else:
                    (y, b, r) = comps
                    if (b[1], b[2], r[1], r[2]) != (1, 1, 1, 1) or (y[1], y[2]) not in ((1, 1), (2, 1), (2, 2)):
                        raise Refused("sampling")
                hmax, vmax = comps[0][1], comps[0][2]
                mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
                offs, total = [], 0
                for c in comps:
                    offs.append(total)
                    total += mcux * c[1] * mcuy * c[2] * 64
                coef = np.zeros(total, np.int64)
            ns = s[0] if len(s) else 0
            if ns < 1 or ns > len(comps) or len(s) != 1 + 2 * ns + 3:
                raise Defect("bad SOS")
            cis, tds, tas = [], [], []
            for j in range(ns):
                ids = [c[0] for c in comps]
                if s[1 + 2 * j] not in ids:
                    raise Defect("scan component")
                ci = ids.index(s[1 + 2 * j])
                if cis and ci <= cis[-1]:
                    raise Defect("scan component order")
                cis.append(ci)
                tds.append(s[2 + 2 * j] >> 4)
                tas.append(s[2 + 2 * j] & 15)
                if tds[-1] > 3 or tas[-1] > 3:
                    raise Defect("table selector")
            Ss, Se, Ah, Al = s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns] >> 4, s[3 + 2 * ns] & 15
            ok = (Se == 0) if Ss == 0 else (ns == 1 and Ss <= Se <= 63)
            ok = ok and (Ah == 0 or Al == Ah - 1) and Al <= 13
            if ok:
                for ci in cis:
                    if Ss > 0 and prec[ci][0] < 0:
                        ok = False
                    for k in range(Ss, Se + 1):
                        if prec[ci][k] != (-1 if Ah == 0 else Ah):
                            ok = False
                        prec[ci][k] = Al
            if not ok:
                raise Refused("scan script out of order")
            payload, starts, nxt = _destuff(data, pos + seg)
            padded = payload + bytes(8)
            # units of the scan
            if ns == 1:
                c = comps[cis[0]]
                wc, hc = -(-W * c[1] // hmax), -(-H * c[2] // vmax)
                ux, uy = -(-wc // 8), -(-hc // 8)
            else:
                ux, uy = mcux, mcuy
            units = ux * uy
            per = restart if restart else units
            nseg = -(-units // per)
            if len(starts) < nseg:
                raise Defect("restart marker missing")
            if Ss == 0 and Ah == 0:
                tables = []
                for td in tds:
                    if td not in dc:
                        raise Defect("Huffman table missing")
                    tables.append(dc[td])
            elif Ss > 0:
                if tas[0] not in ac:
                    raise Defect("Huffman table missing")
                tables = [ac[tas[0]]]

            def block(ci, row, col):
                c = comps[ci]
                return offs[ci] + (row * mcux * c[1] + col) * 64

            for sidx in range(nseg):
                u0, u1 = sidx * per, min(units, sidx * per + per)
                rd = _Bits(padded, starts[sidx], starts[sidx + 1] if sidx + 1 < len(starts) else len(payload))
                if Ss == 0:
                    pred = [0] * ns
                    for u in range(u0, u1):
                        my, mx = divmod(u, ux)
                        for j, ci in enumerate(cis):
                            hh, vv = (1, 1) if ns == 1 else (comps[ci][1], comps[ci][2])
                            for by in range(vv):
                                for bx in range(hh):
                                    at = block(ci, my * vv + by, mx * hh + bx)
                                    if Ah == 0:
                                        t = rd.symbol(tables[j])
                                        if t > 11:
                                            raise Defect("DC category above 11")
                                        if t:
                                            pred[j] += _extend(rd.bits(t), t)
                                        rd.check()
                                        coef[at] = _i16(pred[j] << Al)
                                    else:
                                        b = rd.bit()
                                        rd.check()
                                        if b:
                                            coef[at] = _i16(int(coef[at]) | (1 << Al))
                    continue
                table = tables[0]
                ci = cis[0]
                eobrun = 0
                p1 = 1 << Al
                for u in range(u0, u1):
                    row, col = divmod(u, ux)
                    at = block(ci, row, col)
                    if Ah == 0:
                        if eobrun:
                            eobrun -= 1
                            continue
                        k = Ss
                        while k <= Se:
                            rs = rd.symbol(table)
                            r, sz = rs >> 4, rs & 15
                            if sz:
                                k += r
                                if k > Se:
                                    raise Defect("coefficient index past Se")
                                coef[at + ZIGZAG[k]] = _i16(_extend(rd.bits(sz), sz) << Al)
                                k += 1
                            elif r == 15:
                                k += 16
                            else:
                                eobrun = (1 << r) + rd.bits(r) - 1
                                break
                        rd.check()
                        continue
                    # refinement (G.1.2.3, figure G.7)
                    k = Ss
                    if eobrun == 0:
                        while k <= Se:
                            rs = rd.symbol(table)
                            r, sz = rs >> 4, rs & 15
                            val = 0
                            if sz:
                                if sz != 1:
                                    raise Defect("refinement symbol of size %d" % sz)
                                val = p1 if rd.bit() else -p1
                            elif r != 15:
                                eobrun = (1 << r) + rd.bits(r)
                                break
                            while k <= Se:
                                i = at + ZIGZAG[k]
                                v = int(coef[i])
                                if v:
                                    if rd.bit() and not (v & p1):
                                        coef[i] = _i16(v + p1 if v >= 0 else v - p1)
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            if sz:
                                if k > Se:
                                    raise Defect("coefficient index past Se")
                                coef[at + ZIGZAG[k]] = val
                            rd.check()
                            k += 1
                    if eobrun:
                        if k <= Se:
                            band = [at + ZIGZAG[j] for j in range(k, Se + 1)]
                            for i in (band[j] for j in np.flatnonzero(coef[band])):
                                v = int(coef[i])
                                if rd.bit() and not (v & p1):
                                    coef[i] = _i16(v + p1 if v >= 0 else v - p1)
                        eobrun -= 1
                    rd.check()
            nscans += 1
            pos = nxt
            continue
        pos += seg
    if frame is None or coef is None:
        raise Defect("no frame or scan")
    W, H, comps = frame
    if len(comps) == 3:
        ids = [c[0] for c in comps]
        if not jfif and ((adobe and adobe_transform == 0) or (not adobe and ids == [ord("R"), ord("G"), ord("B")])):
            raise Refused("RGB samples")
    for c in comps:
        if not qseen[c[3]]:
            raise Defect("quantisation table missing")
    if any(p != 0 for row in prec for p in row):
        raise Refused("incomplete: not every coefficient was sent and refined to its last bit")
    return {"width": W, "height": H, "components": len(comps), "hmax": hmax, "vmax": vmax,
            "comps": [(mcux * c[1], mcuy * c[2], c[3]) for c in comps], "qtables": q, "coef": coef.astype(np.int16), "scans": nscans}


def scan_ranges(data: bytes):
    """[(Ss, Se, Ah, Al, first byte, byte behind the last)] of the entropy-coded data of every scan of a sound file"""
    out, pos = [], 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        m = data[pos + 1]
        if m == 0xD9:
            break
        seg = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if m != 0xDA:
            pos += 2 + seg
            continue
        s = data[pos + 4:pos + 2 + seg]
        ns = s[0]
        first = pos + 2 + seg
        _, _, nxt = _destuff(data, first)
        out.append((s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns] >> 4, s[3 + 2 * ns] & 15, first, nxt))
        pos = nxt
    return out

"""The corpus of baseline JPEGs whose entropy-coded data is damaged BY CONSTRUCTION, shared by
tests/test_jpeg_damage_cases.py (walker, host decoder, sanitizer driver) and tests/test_jpeg_damage_gpu.py (device decoder).

A case = base file x damage kind x position.  jpeg_encode_oracle.block_symbols gives every block's bit string, so the bit
position of every block boundary in the de-stuffed scan is known, and with it the chunk of the device decoder's grid
(csrc/jpeg_gpu_entropy.h: lane t decodes the blocks that START in bits [t * 8 * chunk, (t + 1) * 8 * chunk)) a block belongs
to - nothing is decoded to know it.  A kind replaces the symbols of ONE block so that every block behind it stays bit
aligned under the recovery both decoders of the library share (an unassigned code consumes 16 bits and counts as symbol 0,
an index past 63 closes the block, a DC category s > 11 consumes s & 7 value bits): the block total still matches, which is
the condition under which a chunk-level error flag can be forgiven.

kind        what the chosen block holds                                                     verdict (tests/jpeg_walker.py)
index       its DC symbol, (15, 1) three times (index 49), (15, 1) once more (index 64)    Defect("index")
code-dc     sixteen 1-bits where the DC code belongs, then its AC symbols                   Defect("code")
code-ac     its DC symbol, then sixteen 1-bits                                              Defect("code")
dccat       DC symbol 12 of a table that holds it, 4 value bits, then its AC symbols        Defect("dccat")
zrl         its DC symbol, (15, 1) three times, ZRL (index 49 -> 65), no EOB                Ok: libjpeg accepts it
pad0        the padding bits of the final byte 0 instead of 1                               Ok: behind the last block
extra1..3   one to three bytes (not FF) between the final byte and EOI                      Ok: behind the last block
cut-*       the scan cut at a chunk boundary / in the middle of a block / one byte short,   Short
            with and without EOI behind the cut; cut-ff: a lone FF as the file's last byte
flip        one bit of the scan (before stuffing: no marker appears) flipped                whatever the walker says

The flips (FLIPS) were chosen by a seeded search over the bits of each class's blocks, sorted by jpeg_walker.tally: per
base and class one flip that leaves a defect in a real block and the block total intact ("defect"), one that leaves a
valid other stream ("ok") and one after which the total differs ("total").  tests/test_jpeg_damage_cases.py asserts that
spread on the walker; where NO bit of a class's blocks gives a defect with the total intact (the smooth chroma blocks at
the end of the 4:2:0 file) it asserts that by trying them all.

Position classes of a block, for a chunk size (the module states the class in the case id):
single      the whole scan is one chunk
first       it starts in chunk 0
interior    it starts in a chunk between
straddle    it starts in the second-to-last chunk and ends in the last one
lastchunk   it starts in the chunk in which the last block starts, and is not the last block
lastblock   the last block
"""
from __future__ import annotations

import io
from dataclasses import dataclass, field

import numpy as np

import jpeg_encode_oracle as O
import jpeg_stream_writer as Wr

OPTIONS = (256, 4096)                            # values of "jpeg_chunk_bytes" the GPU tests run


def effective_chunk(option):
    """dfd_decode_jpeg_batch halves a chunk size above 256 for a call with less than 8 MiB of scan (jpeg_decode.hip)"""
    return option // 2 if option > 256 else option


def _img(h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(xx / (7.0 + c) + c) * np.cos(yy / (11.0 - c)) for c in range(3)], -1)
    return np.clip(base + rs.randn(h, w, 3) * 12, 0, 255).astype(np.uint8)


def _noise(h, w, seed):
    return np.random.RandomState(seed).randint(50, 200, (h, w, 3)).astype(np.uint8)


def _with12(table):
    """Annex K's DC table + symbol 12 with a code one bit longer than its longest (Kraft holds, no code is all ones)"""
    bits, vals = list(table[0]), list(table[1])
    bits[max(i for i in range(16) if bits[i]) + 1] = 1
    return (bits, vals + [12])


@dataclass
class Base:
    name: str
    S: Wr.Stream
    coef: np.ndarray
    comp: np.ndarray
    bpm: int
    nmcu: int
    own_tables: bool                             # table_of(...) tables (a miss at <= 12 bits) / Annex K (the 13 .. 16-bit branch)
    restart: int = 0
    val: np.ndarray = field(default=None, repr=False)
    ln: np.ndarray = field(default=None, repr=False)

    @property
    def total(self):
        return len(self.coef)

    def symbols(self, S=None):
        S = S or self.S
        pairs = list(dict.fromkeys((c.td, c.ta) for c in S.comps))
        val, ln, _ = O.block_symbols(self.coef, self.comp, self.bpm, self.restart, tables=[(S.dc[d], S.ac[a]) for d, a in pairs],
                                     comp_table=[pairs.index((c.td, c.ta)) for c in S.comps])
        return val, ln

    def tables_of_block(self, b, S=None):
        c = (S or self.S).comps[int(self.comp[b])]
        return (S or self.S).dc[c.td], (S or self.S).ac[c.ta]


def _segments(base, val, ln):
    """the scan's bytes per restart segment, before stuffing, padded with 1-bits"""
    per = (base.restart or base.nmcu) * base.bpm
    return [O._pack(val[b0:b0 + per], ln[b0:b0 + per]) for b0 in range(0, base.total, per)]


def assemble(base, segs, S=None, tail=b"", eoi=True):
    """the file of stream S (the base's own by default) around the scan `segs` (bytes per restart segment, not yet stuffed)"""
    out = b"\xff\xd8" + b"".join(Wr._header_segments(S or base.S))
    for i, seg in enumerate(segs):
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        out += O._stuff(np.asarray(seg, np.uint8))[0]
    return out + tail + (b"\xff\xd9" if eoi else b"")


def _make_base(name, h, w, mode, quality, seed, source=_img, own_tables=False, dri=None):
    img = source(h, w, seed)
    if mode == "gray":
        img = img[..., 1]
    S = Wr.defaults(h, w, mode, quality)
    S.dri = dri
    coef, comp, bpm, nmcu = O.scan_blocks(img, 0, mode, qtabs=[np.asarray(S.qtables[c.tq][0]) for c in S.comps])
    restart = dri if dri and dri < nmcu else 0
    if own_tables:
        used = Wr.used_symbols(coef, comp, bpm, restart)
        for i, c in enumerate(S.comps):
            dcs = set().union(*[used[j][0] for j, cc in enumerate(S.comps) if cc.td == c.td])
            acs = set().union(*[used[j][1] for j, cc in enumerate(S.comps) if cc.ta == c.ta])
            S.dc[c.td], S.ac[c.ta] = Wr.table_of(dcs | {12}), Wr.table_of(acs | {0x00, 0xF0, 0xF1})
    base = Base(name, S, coef, comp, bpm, nmcu, own_tables, restart)
    base.val, base.ln = base.symbols()
    assert assemble(base, _segments(base, base.val, base.ln)) == Wr.write(S, coef, comp, bpm, nmcu), name
    return base


_BASES = {
    # name: (h, w, mode, quality, seed, source, own tables, DRI)
    "gray": (45, 77, "gray", 90, 11, _img, False, None),                # bpm 1
    "444": (33, 17, 0, 85, 12, _img, True, None),                       # bpm 3, table_of tables
    "420": (64, 96, 2, 90, 13, _img, False, None),                      # bpm 6, about ten 256-byte chunks
    "tiny": (16, 16, 2, 30, 14, _img, True, None),                      # the whole scan in one 256-byte chunk
    "noise": (240, 320, 2, 95, 15, _noise, False, None),                # ~280 chunks: the last behind the wave and block borders
    "restart": (64, 96, 2, 90, 16, _img, False, 5),                     # five segments, for the RST = true kernels
}
_bases = {}


def base(name):
    if name not in _bases:
        h, w, mode, q, seed, src, own, dri = _BASES[name]
        _bases[name] = _make_base(name, h, w, mode, q, seed, src, own, dri)
    return _bases[name]


# ------------------------------------------------------------------------------------------------ geometry
def block_bits(b: Base, ln=None):
    """(start, end) of every block in bits of the de-stuffed scan, and the scan's payload bits"""
    ln = b.ln if ln is None else ln
    size = ln.sum(1)
    per = (b.restart or b.nmcu) * b.bpm
    start = np.zeros(b.total, np.int64)
    at = 0
    for b0 in range(0, b.total, per):
        s = size[b0:b0 + per]
        start[b0:b0 + per] = at + np.cumsum(s) - s
        at += -(-int(s.sum()) // 8) * 8
    return start, start + size, at


def classes(b: Base, chunk_bytes, ln=None):
    """class of every block under a chunk size, and the number of chunks"""
    start, end, nbits = block_bits(b, ln)
    cb = 8 * chunk_bytes
    nch = -(-nbits // cb)
    sc, ec = start // cb, (end - 1) // cb
    out = np.where(sc == 0, "first", "interior").astype(object)
    out[(sc == nch - 2) & (ec == nch - 1)] = "straddle"
    out[sc == sc[-1]] = "lastchunk"
    out[-1] = "lastblock"
    if nch == 1:
        out[:] = "single"
    return list(out), nch


def chunk_counts(b: Base, chunk_bytes, block, ln=None):
    """for the forgiveness rules: (chunk in which `block` starts, blocks in front of that chunk, blocks that start in it, total)"""
    start, _, _ = block_bits(b, ln)
    sc = start // (8 * chunk_bytes)
    c = int(sc[block])
    return c, int((sc < c).sum()), int((sc == c).sum()), b.total


# ------------------------------------------------------------------------------------------------ damage in a block
def _sym(table, symbol, extra=0, nextra=0):
    code, size = O._derive(table)
    assert size[symbol] > 0, f"symbol {symbol:#x} has no code"
    return (int(code[symbol]) << nextra) | extra, int(size[symbol]) + nextra


ONES16 = (0xFFFF, 16)


def _damage(b: Base, kind, block):
    """-> (the stream to write with, the block's new slots)"""
    S = b.S
    if kind == "dccat" and not b.own_tables:
        S = Wr.Stream(**{**b.S.__dict__, "dc": {k: _with12(t) for k, t in b.S.dc.items()}})   # (codes of 0 .. 11 stay)
    dc, ac = b.tables_of_block(block, S)
    keep = [(int(b.val[block, i]), int(b.ln[block, i])) for i in range(65)]
    run1 = _sym(ac, 0xF1, 1, 1)
    new = {
        "index": lambda: [keep[0]] + [run1] * 4,
        "zrl": lambda: [keep[0]] + [run1] * 3 + [_sym(ac, 0xF0)],
        "code-dc": lambda: [ONES16] + keep[1:],
        "code-ac": lambda: [keep[0], ONES16],
        "dccat": lambda: [_sym(dc, 12, 0b1010, 4)] + keep[1:],
    }[kind]()
    return S, new


def damaged_lengths(b: Base, kind, block):
    ln = b.ln.copy()
    ln[block] = 0
    for i, (_, l) in enumerate(_damage(b, kind, block)[1]):
        ln[block, i] = l
    return ln


def damaged(b: Base, kind, block):
    """-> (file, the stream it was written with, its lengths table)"""
    S, new = _damage(b, kind, block)
    val, ln = (b.val.copy(), b.ln.copy()) if S is b.S else b.symbols(S)
    val[block], ln[block] = 0, 0
    for i, (v, l) in enumerate(new):
        val[block, i], ln[block, i] = v, l
    assert np.array_equal(ln, damaged_lengths(b, kind, block))
    return assemble(b, _segments(b, val, ln), S), S, ln


# ------------------------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    id: str
    base: str
    kind: str
    data: bytes
    verdict: str                                 # "ok" | "defect" | "short"; a flip: "ok" | "defect" | "total", what it was chosen for
    defect: str | None = None                    # the walker's kind
    block: int | None = None                     # defect: the block; short: blocks in front of the cut
    classes: dict = field(default_factory=dict)  # option -> class of the damaged block
    counts: dict = field(default_factory=dict)   # option -> chunk_counts(...)
    span: tuple | None = None                    # the damaged block's bits [start, end) in the de-stuffed scan
    healthy: str = ""                            # key of healthy(...): same size, sampling


BLOCK_KINDS = {"index": "index", "code-dc": "code", "code-ac": "code", "dccat": "dccat", "zrl": None}
WANTED = ("single", "first", "interior", "straddle", "lastchunk", "lastblock")


def _candidates(cls, want, lo):
    """blocks to try for a class: those the undamaged file has in it, from the middle one outwards; for the (unique)
    straddling block also its neighbours, since the damage changes the block's own length"""
    idx = [i for i, c in enumerate(cls) if c == want and i >= lo]
    if want == "straddle":
        idx = sorted({j for i in [i for i, c in enumerate(cls) if c == want] for j in range(i - 3, i + 4) if lo <= j < len(cls)})
    mid = idx[len(idx) // 2] if idx else 0
    return sorted(idx, key=lambda i: abs(i - mid))[:12]


def _block_cases(name, kinds, only_last_segment=False):
    b = base(name)
    lo = ((b.nmcu - 1) // b.restart) * b.restart * b.bpm if only_last_segment else 0
    out = []
    for kind in kinds:
        blocks = {}
        for opt in OPTIONS:
            cls, _ = classes(b, effective_chunk(opt))
            for want in WANTED:
                for blk in _candidates(cls, want, lo):
                    # the class must hold on the DAMAGED file (the block's own length has changed)
                    if classes(b, effective_chunk(opt), damaged_lengths(b, kind, blk))[0][blk] == want:
                        blocks.setdefault(blk, set()).add(opt)
                        break
        for blk in sorted(blocks):
            data, S, ln = damaged(b, kind, blk)
            cl = {opt: classes(b, effective_chunk(opt), ln)[0][blk] for opt in OPTIONS}
            cn = {opt: chunk_counts(b, effective_chunk(opt), blk, ln) for opt in OPTIONS}
            tag = "+".join(f"{cl[o]}@{o}" for o in OPTIONS)
            dk = BLOCK_KINDS[kind]
            start, end, _ = block_bits(b, ln)
            out.append(Case(f"{name}-{kind}-b{blk}-{tag}", name, kind, data, "defect" if dk else "ok", dk, blk, cl, cn,
                            (int(start[blk]), int(end[blk])), name + ("+dc12" if S is not b.S else "")))
    return out


def _tail_cases(name):
    b = base(name)
    segs = _segments(b, b.val, b.ln)
    _, end, _ = block_bits(b)
    out = []
    npad = (-int(end[-1])) % 8
    assert npad > 0, (name, "no padding bits: take another seed")
    last = segs[:-1] + [np.frombuffer(bytes(segs[-1][:-1]) + bytes([int(segs[-1][-1]) & (0xFF << npad) & 0xFF]), np.uint8)]
    out.append(Case(f"{name}-pad0-{npad}bits", name, "pad0", assemble(b, last), "ok", healthy=name))
    for n, extra in ((1, b"\x00"), (2, b"\x5a\xa5"), (3, b"\x12\x34\x56")):
        out.append(Case(f"{name}-extra{n}", name, f"extra{n}", assemble(b, segs, tail=extra), "ok", healthy=name))
    return out


def _cut_cases(name):
    b = base(name)
    raw = _segments(b, b.val, b.ln)[0]
    start, end, nbits = block_bits(b)
    mid = int(np.searchsorted(start, nbits // 2))
    cuts = {"chunk": 256 if len(raw) > 256 else len(raw) // 2, "midblock": int(start[mid] + end[mid]) // 16, "lastbyte": len(raw) - 1}
    out = []
    for what, nbytes in cuts.items():
        assert 0 < nbytes < len(raw)
        found = int((end <= 8 * nbytes).sum())
        for eoi in (True, False):
            out.append(Case(f"{name}-cut-{what}{'-eoi' if eoi else ''}", name, "cut", assemble(b, [raw[:nbytes]], eoi=eoi), "short",
                            block=found, healthy=name))
    nbytes = cuts["midblock"]
    out.append(Case(f"{name}-cut-ff", name, "cut", assemble(b, [raw[:nbytes]], tail=b"\xff", eoi=False), "short",
                    block=int((end <= 8 * nbytes).sum()), healthy=name))
    return out


def damaged_frame(img, quality, kind, want, chunk_bytes, mode=2):
    """For the tests of whole routes: the frame `img` (H, W, 3 BGR) written with libjpeg's defaults and damaged `kind` in a
    block of class `want` under `chunk_bytes` -> (the damaged file, the healthy file)"""
    h, w = img.shape[:2]
    b = _make_base(f"{h}x{w}", h, w, mode, quality, 0, lambda *_: img)
    cls, _ = classes(b, chunk_bytes)
    for blk in _candidates(cls, want, 0):
        if classes(b, chunk_bytes, damaged_lengths(b, kind, blk))[0][blk] == want:
            return damaged(b, kind, blk)[0], assemble(b, _segments(b, b.val, b.ln))
    raise AssertionError((kind, want))


# (base, class at 256-byte chunks) -> bit of the de-stuffed scan to flip, per outcome
FLIPS = {
    ("gray", "first"): dict(total=2117, ok=1584, defect=2043), ("gray", "interior"): dict(total=8711, ok=11184, defect=4273),
    ("gray", "straddle"): dict(total=12454, ok=12325, defect=12469), ("gray", "lastchunk"): dict(ok=12720, total=12733, defect=12603),
    ("gray", "lastblock"): dict(total=12944, ok=13019, defect=12957),
    ("444", "first"): dict(total=261, ok=1003, defect=1958), ("444", "straddle"): dict(total=2058, ok=2052, defect=2024),
    ("444", "lastchunk"): dict(total=3820, ok=2471, defect=3115), ("444", "lastblock"): dict(ok=3864, total=3865, defect=3858),
    ("420", "first"): dict(defect=1230, ok=1946, total=1805), ("420", "interior"): dict(total=13064, ok=12399, defect=14504),
    ("420", "straddle"): dict(ok=20346, total=20351), ("420", "lastchunk"): dict(ok=21093, total=20938, defect=20747),
    ("420", "lastblock"): dict(ok=21167, total=21207),
    ("tiny", "single"): dict(ok=107, defect=101, total=184),
    ("noise", "first"): dict(ok=1599, total=1028, defect=1396), ("noise", "interior"): dict(ok=245209, total=455056, defect=219238),
    ("noise", "straddle"): dict(total=585583, ok=585505, defect=585816), ("noise", "lastchunk"): dict(total=586010, ok=586888, defect=586884),
    ("noise", "lastblock"): dict(total=587279, ok=587144, defect=587168),
}
NO_DEFECT_FLIP = (("420", "straddle"), ("420", "lastblock"))


def flipped(b: Base, bit):
    raw = bytearray(_segments(b, b.val, b.ln)[0].tobytes())
    raw[bit >> 3] ^= 0x80 >> (bit & 7)
    return assemble(b, [np.frombuffer(bytes(raw), np.uint8)])


def _flip_cases():
    out = []
    for (name, cls), bits in FLIPS.items():
        b = base(name)
        start, end, _ = block_bits(b)
        for outcome, bit in bits.items():
            blk = int(np.searchsorted(start, bit, "right")) - 1
            cl = {opt: classes(b, effective_chunk(opt))[0][blk] for opt in OPTIONS}
            assert cl[256] == cls and start[blk] <= bit < end[blk], (name, cls, bit)
            tag = "+".join(f"{cl[o]}@{o}" for o in OPTIONS)
            out.append(Case(f"{name}-flip-{outcome}-bit{bit}-b{blk}-{tag}", name, "flip", flipped(b, bit), outcome, block=blk, classes=cl,
                            span=(int(start[blk]), int(end[blk])), healthy=name))
    return out


PLAIN = ("gray", "444", "420", "tiny", "noise")
_cases = None


def cases():
    """every constructed case - made once, shared, never modified"""
    global _cases
    if _cases is None:
        out = []
        for name in PLAIN:
            out += _block_cases(name, tuple(BLOCK_KINDS)) + _tail_cases(name) + _cut_cases(name)
        out += _block_cases("restart", ("index", "code-dc", "code-ac"), only_last_segment=True)
        out += _flip_cases()
        assert len({c.id for c in out}) == len(out)
        _cases = out
    return _cases


_healthy, _pillow = {}, {}


def healthy(key):
    """three healthy files of the base's size and sampling (the base's own first; the others from seeds + 1, + 2, with the
    tables of `key`: "+dc12" = Annex K's DC tables with symbol 12 added)"""
    if key not in _healthy:
        name = key.split("+")[0]
        h, w, mode, q, seed, src, own, dri = _BASES[name]
        files = []
        for i in range(3):
            b = base(name) if i == 0 else _make_base(name, h, w, mode, q, seed + 100 * i, src, own, dri)
            S = b.S
            if key.endswith("+dc12"):
                S = Wr.Stream(**{**b.S.__dict__, "dc": {k: _with12(t) for k, t in b.S.dc.items()}})
            val, ln = b.symbols(S)
            files.append(assemble(b, _segments(b, val, ln), S))
        _healthy[key] = files
    return _healthy[key]


def pillow(data: bytes):
    """Pillow's decode (BGR) - the reference for every file that is accepted; computed once per file"""
    from PIL import Image

    if data not in _pillow:
        a = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])
        a.setflags(write=False)
        _pillow[data] = a
    return _pillow[data]


# ------------------------------------------------------------------------------------------------ the forgiveness rules
def parent_rule_forgives(chunk, in_front, in_chunk, total, first_bad=None):
    """the rule of jg_scan_kernel before this corpus existed, per chunk: an error flag is forgiven in any chunk that
    reaches the last block"""
    return in_front + in_chunk >= total


def intended_rule_forgives(chunk, in_front, in_chunk, total, first_bad):
    """forgiven only when the first defect lies at or behind block `total`; first_bad = complete blocks the chunk's lane
    decoded in front of its first defect"""
    return in_front + first_bad >= total

"""Baseline JPEGs whose entropy-coded data is damaged inside a block (tests/jpeg_damage_cases.py), CPU side: the
sequential walker (tests/jpeg_walker.py, after T.81 F.2.2) is the verdict; the host decoder (csrc/jpeg_entropy.h) must
reject exactly what the walker rejects and return the walker's coefficients otherwise (tests/test_host_asan.py runs the
same files through the sanitizer driver); and the two rules by which the device decoder's scan kernel may forgive a
chunk's error flag are stated and compared on the corpus.  tests/test_jpeg_damage_gpu.py holds the device decoder to the same verdicts."""
import numpy as np
import pytest

import jpeg_damage_cases as D
import jpeg_stream_cases as C
import jpeg_walker as W
from oracle import jpeg_ref

_walked = {}


def walked(data):
    """the walker's verdict - once per file, shared"""
    if data not in _walked:
        _walked[data] = W.walk(data)
    return _walked[data]


def _verdict(res):
    return {W.Ok: "ok", W.Defect: "defect", W.Short: "short"}[type(res)]


HEALTHY = sorted({c.healthy for c in D.cases()})


# ------------------------------------------------------------------------------------------------ the walker
@pytest.mark.parametrize("name", HEALTHY + [r.name for r in C.ROWS if r.kind == "decode"])
def test_walker_on_valid_files_equals_the_host_decoder(pkg, name):
    files = D.healthy(name) if name in HEALTHY else [f.data for f in C.files(name)]
    for i, data in enumerate(files):
        res = walked(data)
        assert isinstance(res, W.Ok), (name, i, res)
        info = pkg._lib.jpeg_coefficients(data)
        assert (info["height"], info["width"]) == (res.frame.height, res.frame.width)
        assert np.array_equal(W.library_order(res), info["coef"]), (name, i)


def test_corpus_covers_every_kind_in_every_class():
    got = {(c.kind, c.classes[256]) for c in D.cases() if c.classes}
    for kind in D.BLOCK_KINDS:
        for cls in D.WANTED:
            assert (kind, cls) in got, (kind, cls)
    # at 4096 the small files are one chunk and the classes move; the noise file keeps its last chunk behind lane 255
    assert {c.classes[4096] for c in D.cases() if c.base in ("gray", "444", "tiny") and c.classes} == {"single"}
    assert {"first", "straddle", "lastchunk", "lastblock"} <= {c.classes[4096] for c in D.cases() if c.base == "420" and c.classes}
    assert D.classes(D.base("noise"), 256)[1] > 256 and D.classes(D.base("tiny"), 256)[1] == 1
    assert {c.base for c in D.cases()} == set(D.PLAIN) | {"restart"}
    # both table kinds: a lookup miss at <= 12 bits (table_of) and the 13 .. 16-bit branch (Annex K)
    assert {D.base(n).own_tables for n in D.PLAIN} == {True, False}
    for n in D.PLAIN:
        longest = max(max(i + 1 for i in range(16) if t[0][i]) for t in list(D.base(n).S.dc.values()) + list(D.base(n).S.ac.values()))
        assert (longest <= 12) == D.base(n).own_tables, (n, longest)


CONSTRUCTED = [c for c in D.cases() if c.kind != "flip"]


@pytest.mark.parametrize("case", CONSTRUCTED, ids=lambda c: c.id)
def test_walker_reports_what_the_case_declares(case):
    res = walked(case.data)
    assert _verdict(res) == case.verdict, (case.id, res)
    if case.verdict == "defect":
        assert (res.kind, res.block) == (case.defect, case.block), (case.id, res)
        assert case.span[0] <= res.bit < case.span[1], (case.id, res, case.span)
        b = D.base(case.base)
        for opt in D.OPTIONS:                                       # the chunk the defect's block starts in, as the case id says
            chunk, in_front, in_chunk, total = case.counts[opt]
            assert chunk == case.span[0] // (8 * D.effective_chunk(opt)) and in_front <= case.block < in_front + in_chunk
            assert total == b.total
    elif case.verdict == "short":
        assert res.blocks == case.block, (case.id, res)


def _sorted_flip(b, data, blk, start):
    """how a flip in block `blk` ends: ("defect" | "ok" | "total"), by the tally from that block on"""
    first, n = W.tally(data, int(start[blk]), blk)
    return "total" if n != b.total else ("defect" if first is not None and first < b.total else "ok")


def test_flips_spread_over_every_class_of_every_base():
    """a condition on the inputs, checked on the walker alone: every position class of every restart-less base holds a flip
    the walker calls Defect with the block total preserved, one it calls Ok (a valid other stream) and one after which the
    total differs - except where no bit of the class's blocks gives the first, which is shown by trying every bit"""
    flips = [c for c in D.cases() if c.kind == "flip"]
    for name in D.PLAIN:
        b = D.base(name)
        start, end, _ = D.block_bits(b)
        cls = D.classes(b, 256)[0]
        for want in sorted(set(cls)):
            mine = {c.verdict: c for c in flips if c.base == name and c.classes[256] == want}
            need = {"ok", "total"} | (set() if (name, want) in D.NO_DEFECT_FLIP else {"defect"})
            assert set(mine) == need, (name, want, set(mine))
            for outcome, c in mine.items():
                res = walked(c.data)
                assert _sorted_flip(b, c.data, c.block, start) == outcome, c.id
                if outcome == "defect":
                    assert isinstance(res, W.Defect) and res.block >= c.block, (c.id, res)
                elif outcome == "ok":
                    assert isinstance(res, W.Ok), (c.id, res)
                    assert not np.array_equal(res.blocks, walked(D.healthy(name)[0]).blocks), c.id
                else:
                    assert W.tally(c.data)[1] != b.total, c.id
            if (name, want) in D.NO_DEFECT_FLIP:
                for blk in [i for i, x in enumerate(cls) if x == want]:
                    for bit in range(int(start[blk]), int(end[blk])):
                        assert _sorted_flip(b, D.flipped(b, bit), blk, start) != "defect", (name, want, bit)


# ------------------------------------------------------------------------------------------------ the host decoder
@pytest.mark.parametrize("case", D.cases(), ids=lambda c: c.id)
def test_host_decoder_agrees_with_the_walker(pkg, monkeypatch, case):
    """code -1 exactly where the walker says defect or short; the walker's coefficients where it says ok, and through the
    oracle's IDCT the pixels of libjpeg (Pillow) for the same bytes; at 1, 3 and 61 speculative chunks"""
    res = walked(case.data)
    for chunks in (None, 1, 3, 61):
        if chunks is None:
            monkeypatch.delenv("DFD_JPEG_CHUNKS", raising=False)
        else:
            monkeypatch.setenv("DFD_JPEG_CHUNKS", str(chunks))
        try:
            info = pkg._lib.jpeg_coefficients(case.data)
        except pkg._lib.DfdError as e:
            assert e.code == -1, (case.id, e.code, str(e))
            assert not isinstance(res, W.Ok), f"{case.id}: the host decoder is stricter than the walker: {e}"
            continue
        assert isinstance(res, W.Ok), f"{case.id}: the host decoder accepts what the walker rejects: {res}"
        assert np.array_equal(info["coef"], W.library_order(res)), (case.id, chunks)
        if chunks is None:
            assert np.array_equal(jpeg_ref.decode_from_coefficients(info), D.pillow(case.data)), case.id


# ------------------------------------------------------------------------------------------------ the forgiveness rules
def _rule_rows():
    """(case, option, class, (chunk of the first defect, blocks in front, blocks in that chunk, total), first_bad)"""
    rows = []
    for c in CONSTRUCTED:
        b = D.base(c.base)
        for opt in D.OPTIONS:
            if c.verdict == "defect":
                counts = c.counts[opt]
                rows.append((c, opt, c.classes[opt], counts, c.block - counts[1]))
            elif c.kind.startswith(("pad", "extra")):
                # whatever the bits behind the last block decode to, the lane has all its blocks in front of it
                counts = D.chunk_counts(b, D.effective_chunk(opt), b.total - 1)
                rows.append((c, opt, "behind", counts, counts[2]))
    return rows


def test_forgiveness_rules_on_the_corpus():
    """jg_scan_kernel keeps one error flag per chunk and used to forgive it in every chunk that reaches the last block
    (`err && blocks in front + blocks in the chunk < total -> bad code`).  The intended rule forgives only a defect at or
    behind block `total`.  The rows the old rule forgives although they hold a defect in a real block are what
    tests/test_jpeg_damage_gpu.py is expected to catch on the old kernels: printed here.

    A block that starts in the second-to-last chunk belongs to THAT chunk's lane (a lane decodes the blocks that start in
    its chunk, up to the first boundary at or past the chunk's end), so the old rule rejected a straddling block unless no
    block starts in the last chunk."""
    rows = _rule_rows()
    forgiven = []
    for c, opt, cls, counts, first_bad in rows:
        new, old = D.intended_rule_forgives(*counts, first_bad), D.parent_rule_forgives(*counts)
        if c.verdict == "defect":
            assert not new, (c.id, opt)
            if cls in ("single", "lastchunk", "lastblock"):
                assert old, (c.id, opt)
            else:
                assert not old, (c.id, opt, cls)
            if old:
                forgiven.append((c.kind, cls, f"{c.id} @ jpeg_chunk_bytes {opt}"))
        else:
            assert new and old, (c.id, opt)
    for kind in ("index", "code-dc", "code-ac", "dccat"):
        for cls in ("single", "lastchunk", "lastblock"):
            assert any(f[:2] == (kind, cls) for f in forgiven), (kind, cls)
    print(f"{len(forgiven)} rows with a defect in a real block that the old rule forgives:")
    print("\n".join(f[2] for f in forgiven))

"""CPU: the host half of the JPEG path (csrc/jpeg_entropy.h: markers, tables, entropy decoder) and the oracle's pixel half
(oracle/jpeg_ref.py decode_from_coefficients) against libjpeg itself (Pillow's decode) on valid files that Pillow never
writes - the corpus of tests/jpeg_stream_cases.py.  Every comparison is exact.

One rule holds for every file of the corpus, decodable or not: the library returns Pillow's pixels or raises DfdError
with DFD_ERR_UNSUPPORTED (-7) or DFD_ERR_ARG (-1).  It never returns other pixels.

Before this corpus existed two dialects decoded silently wrong.  RGB samples (Adobe transform 0, or component ids R, G, B,
without JFIF) were converted as YCbCr: 155 to 165 levels off Pillow on `adobe0` and `rgb_ids`.  Chroma planes one or two
samples wide were blended where jdsample.c replicates them: 12 to 66 levels off on the geometry rows 17x3, 17x4, 1x3 and 4x4
at 4:2:2 and 4:2:0 and on 17x1 and 17x2 at 4:2:0 (this corpus through the parent commit's library and oracle; every other
row was equal there)."""
import numpy as np
import pytest

import jpeg_encode_cases as EC
import jpeg_encode_oracle as O
import jpeg_stream_cases as C
import jpeg_stream_writer as Wr
from oracle import jpeg_ref


pillow = C.pillow


# ------------------------------------------------------------------------------------------------ the writer itself
PIN = ["noise-1x1-gray-q1", "noise-37x53-444-q100", "noise-37x53-422-q100", "noise-37x53-420-q100", "cosine-160x160-gray-q90",
       "flat128-17x13-420-q75", "natural-160x160-444-q90-r1", "noise-160x160-422-q100-r2", "natural-160x160-420-q90-r7",
       "gradient-17x13-420-q75-r1"]


@pytest.mark.parametrize("name", PIN)
def test_writer_with_defaults_equals_the_encode_oracle(name):
    """the pin: with libjpeg's defaults the writer's bytes are jpeg_encode_oracle.encode's, which are Pillow's"""
    _, img, quality, sub, rb = next(c for c in EC.CASES if c[0] == name)
    mode = "gray" if img.ndim == 2 else sub
    S = Wr.defaults(img.shape[0], img.shape[1], mode, quality)
    S.dri = rb or None
    assert Wr.from_pixels(S, img, mode) == O.encode(img, quality, sub, rb)


def test_table_helpers():
    for t in (O.DC_LUMA, O.AC_LUMA, O.DC_CHROMA, O.AC_CHROMA):
        r = Wr.reversed_table(t)
        Wr.check_table(t)
        Wr.check_table(r)
        assert r[0] == list(t[0]) and r[1] == list(t[1])[::-1] and Wr.reversed_table(r) == (list(t[0]), list(t[1]))
    assert Wr.table_of({0}) == ([1] + [0] * 15, [0])               # one symbol: the 1-bit code "0"
    assert Wr.table_of({5, 0, 4}) == ([0, 3] + [0] * 14, [0, 4, 5])
    for n in (1, 2, 3, 4, 7, 8, 255, 256):
        Wr.check_table(Wr.table_of(range(n)))
    with pytest.raises(AssertionError):
        Wr.check_table(([2] + [0] * 15, [0, 1]))                   # "1" is all ones
    with pytest.raises(AssertionError):
        Wr.check_table(([1, 3] + [0] * 14, [0, 1, 2, 3]))          # over-subscribed
    with pytest.raises(AssertionError):
        Wr.check_table(([0, 2] + [0] * 14, [7, 7]))
    # a block that needs a symbol its table lacks is refused, not written with a code of no bits
    S = Wr.defaults(8, 8, "gray", 75)
    S.dc = {0: Wr.table_of({0})}
    with pytest.raises(AssertionError):
        Wr.from_pixels(S, np.full((8, 8), 200, np.uint8), "gray")


def test_corpus_rows_are_what_their_names_say():
    """the conditions of the rows that jpeg_stream_cases does not assert while it builds them, read off the bytes"""
    for name in C.BY_NAME:
        assert len(C.files(name)) == 3
    f = C.files("fill_com")[0].data
    assert b"\xff\xff\xff\xff\xe0" not in f and f[2:5] == b"\xff\xff\xe0" and len(f) > 65533 + 1000 and f.endswith(b"\xff\xff\xd9")
    assert C.files("one_dht")[0].data.count(b"\xff\xc4") == 1 and C.files("one_dht")[0].data.count(b"\xff\xdb") == 1
    assert b"\xff\xdd\x00\x04\x00\x00" in C.files("dri_zero")[0].data
    assert b"\xff\xdd\x00\x04\x03\xe8" in C.files("dri_beyond")[0].data       # 1000 > the 36 MCUs
    assert not C.files("after_eoi")[0].data.endswith(b"\xff\xd9") and len(C.scan_of(C.files("two_bit_blocks-flat")[0].data)) == 4096
    d = C.files("dqt16")[0].data
    at = d.index(b"\xff\xdb")
    assert d[at + 4] == 0x10 and d[at + 2:at + 4] == b"\x00\x83" and max(d[at + 5:at + 133:2]) >= 1     # Pq = 1, entries above 255
    assert b"Adobe" in C.files("adobe0")[0].data and b"JFIF" not in C.files("adobe0")[0].data
    assert b"Adobe" in C.files("adobe0_jfif")[0].data and b"JFIF" in C.files("adobe0_jfif")[0].data
    assert b"Adobe" not in C.files("rgb_ids")[0].data and b"JFIF" not in C.files("rgb_ids")[0].data


@pytest.mark.parametrize("name", [r.name for r in C.ROWS if r.pillow])
def test_pillow_decodes_every_row(name):
    for want, f in zip(pillow(name), C.files(name)):
        assert want.shape[2] == 3 and want.size > 0


# ------------------------------------------------------------------------------------------------ the host decoder
def _natural(blocks):
    """(blocks high, blocks wide, 64) zig-zag -> natural order, flat"""
    nat = np.zeros(blocks.shape, np.int64)
    nat[..., O.ZIGZAG] = blocks
    return nat.reshape(-1)


@pytest.mark.parametrize("name", C.DECODABLE)
def test_host_decoder_and_oracle_equal_libjpeg(pkg, monkeypatch, name):
    """coefficients -> oracle == Pillow bit for bit; the coefficients equal the written blocks where the row has them
    (errors that cancel in the pixels); the same coefficients at 1, 3 and 61 speculative chunks"""
    for i, (f, want) in enumerate(zip(C.files(name), pillow(name))):
        monkeypatch.delenv("DFD_JPEG_CHUNKS", raising=False)
        info = pkg._lib.jpeg_coefficients(f.data)
        assert (info["height"], info["width"]) == want.shape[:2]
        got = jpeg_ref.decode_from_coefficients(info)
        d = int(np.abs(got.astype(int) - want.astype(int)).max())
        print(f"{name}[{i}]: max |host decoder + oracle - Pillow| = {d}")
        assert np.array_equal(got, want), (name, i, d)
        if f.blocks is not None:
            assert np.array_equal(info["coef"], np.concatenate([_natural(b) for b in f.blocks])), (name, i)
        if i == 0:
            for chunks in (1, 3, 61):
                monkeypatch.setenv("DFD_JPEG_CHUNKS", str(chunks))
                assert np.array_equal(pkg._lib.jpeg_coefficients(f.data)["coef"], info["coef"]), (name, chunks)


@pytest.mark.parametrize("name", [r.name for r in C.ROWS])
def test_pillows_pixels_or_a_loud_refusal(pkg, name):
    """the rule for every file: Pillow's pixels, or DfdError -7 / -1; the colour-space and loud-only rows as the issue sets
    them (RGB samples and the layouts the device half does not have are refused with -7)"""
    row = C.BY_NAME[name]
    for i, f in enumerate(C.files(name)):
        try:
            got = jpeg_ref.decode_from_coefficients(pkg._lib.jpeg_coefficients(f.data))
        except pkg._lib.DfdError as e:
            assert e.code in (-7, -1), (name, e.code)
            assert row.kind != "decode", (name, str(e))
            assert e.code == -7, (name, e.code, str(e))
            if row.kind == "rgb":
                assert "RGB" in str(e), str(e)                      # the message names the reason
            continue
        assert row.kind == "decode", f"{name}: decoded a file whose samples the device half does not convert"
        assert np.array_equal(got, pillow(name)[i]), (name, i)

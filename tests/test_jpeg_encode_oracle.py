"""CPU: the numpy JPEG encoder (tests/jpeg_encode_oracle.py) writes Pillow's file, byte for byte, over the whole corpus
the device encoder is held to, and that corpus exercises every coder path it claims to."""
import pytest

import jpeg_encode_cases as C
import jpeg_encode_oracle as O


@pytest.fixture(scope="module")
def encoded():
    return {c[0]: O.encode_with_stats(*c[1:]) for c in C.CASES}


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_oracle_equals_pillow(case, encoded):
    assert encoded[case[0]][0] == O.pillow_bytes(*case[1:])


def test_corpus_covers_every_coder_path(encoded):
    C.assert_coverage([encoded[c[0]][1] for c in C.CASES])


def test_corpus_holds_every_size_mode_quality_and_content():
    names = [c[0] for c in C.CASES]
    for mode in ("gray", "444", "422", "420"):
        mine = [n for n in names if f"-{mode}-" in n]
        for h, w in C.SIZES:
            assert any(f"-{w}x{h}-" in n for n in mine), (mode, h, w)
        for q in C.QUALITIES:
            assert any(n.endswith(f"-q{q}") or f"-q{q}-" in n for n in mine), (mode, q)
        for kind in C.CONTENTS:
            assert any(n.startswith(kind + "-") for n in mine), (mode, kind)
    assert any("512x512-444" in n for n in names)
    assert any(n.startswith("noise-") and "-q100" in n for n in names)


def test_marker_layout():
    """SOI, APP0 JFIF 1.01, DQT x2, SOF0, DHT x4 (DC0 AC0 DC1 AC1), [DRI], SOS; gray: one DQT, two DHT."""
    def markers(b):
        out, i = [], 2
        while b[i + 1] != 0xDA:
            out.append(b[i + 1])
            i += 2 + int.from_bytes(b[i + 2:i + 4], "big")
        return out

    assert markers(O.header(16, 16, 75, 2, 0)) == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4]
    assert markers(O.header(16, 16, 75, 2, 3)) == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD]
    assert markers(O.header(16, 16, 75, "gray", 0)) == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4]

"""CPU: progressive JPEG through the host half of the library (`_lib.jpeg_coefficients(data, progressive=True)` =
dfd_jpeg_coefficients_ex with DFD_JPEG_ALLOW_PROGRESSIVE; csrc/jpeg_entropy.h parses, csrc/jpeg_progressive.h decodes
the scans) against two oracles that share no code with it:

  * tests/jpeg_progressive_walker.py, a sequential T.81 G.2 decoder in Python - pinned here first: on every Pillow-written
    file its coefficients, put through `oracle.jpeg_ref.decode_from_coefficients`, give Pillow's pixels;
  * the library's own decode of the BASELINE file of the same pixels / quality / subsampling: libjpeg quantises once and a
    complete progressive file carries the same coefficients, bit for bit.

Scripts Pillow never writes come from tests/jpeg_progressive_writer.py - pinned here too: Pillow decodes its files to the
pixels of the baseline file tests/jpeg_stream_writer.py makes of the same coefficients.  With the flag off every one of
these files is DFD_ERR_UNSUPPORTED (-7), as before."""
import numpy as np
import pytest

import jpeg_progressive_cases as PC
import jpeg_progressive_history  # noqa: F401  (registers the export and the case with the call-history table)
from oracle import jpeg_ref as J
from rtdfd_amd import _lib as L

CORPUS = [p.name for p in PC.corpus()]
SCRIPTED = [p.name for p in PC.scripted()]


def _lib_coefficients(data):
    """(dict, 0) or (None, status)"""
    try:
        return L.jpeg_coefficients(data, progressive=True), 0
    except L.DfdError as e:
        return None, e.code


def _same(a, b):
    """geometry, the quantisation tables the components use, every coefficient"""
    used = sorted({tq for _, _, tq in a["comps"]})
    return (all(a[k] == b[k] for k in ("width", "height", "components", "hmax", "vmax")) and list(map(tuple, a["comps"])) == list(map(tuple, b["comps"]))
            and np.array_equal(a["qtables"][used], b["qtables"][used]) and np.array_equal(a["coef"], b["coef"]))


# ------------------------------------------------------------------------------------------------ the oracles, pinned
@pytest.mark.parametrize("name", CORPUS)
def test_walker_gives_pillows_pixels(name):
    p = PC.by_name(name)
    w = PC.K.decode(p.progressive)
    assert np.array_equal(J.decode_from_coefficients(w), PC.pillow_bgr(p.progressive))
    assert w["scans"] == (6 if w["components"] == 1 else 10)          # libjpeg's default script


def test_the_corpus_is_what_the_issue_names():
    names = set(CORPUS)
    for h, w in PC.SIZES:
        for mode in PC.MODES:
            assert {f"{h}x{w}.{mode}.q{q}" for q in PC.QUALITIES} <= names
    for p in PC.corpus():
        assert b"\xff\xc2" in p.progressive and b"\xff\xc2" not in p.baseline[:700] and b"\xff\xc0" in p.baseline
        if "restart3" in p.name:
            assert b"\xff\xdd\x00\x04" in p.progressive and b"\xff\xd0" in p.progressive
    # fresh tables before most scans: one DHT marker per table
    assert PC.by_name("96x128.420.optimize").progressive.count(b"\xff\xc4") >= 8
    big = PC.by_name("1464x1464.gray.flat")
    assert PC.K.decode(big.progressive)["comps"][0][0] * PC.K.decode(big.progressive)["comps"][0][1] > 32767    # blocks: past the EOBRUN cap


@pytest.mark.parametrize("name", SCRIPTED)
def test_writer_files_decode_in_pillow_to_the_baseline_files_pixels(name):
    p = next(q for q in PC.scripted() if q.name == name)
    assert np.array_equal(PC.pillow_bgr(p.progressive), PC.pillow_bgr(p.baseline))


# ------------------------------------------------------------------------------------------------ the library
@pytest.mark.parametrize("name", CORPUS)
def test_library_equals_walker_and_the_baseline_file(name):
    p = PC.by_name(name)
    got, rc = _lib_coefficients(p.progressive)
    assert rc == 0
    assert _same(got, PC.K.decode(p.progressive))
    assert _same(got, L.jpeg_coefficients(p.baseline))
    assert _same(got, L.jpeg_coefficients(p.baseline, progressive=True))       # the flag changes nothing for a baseline file


@pytest.mark.parametrize("name", SCRIPTED)
def test_library_on_scripts_pillow_never_writes(name):
    p = next(q for q in PC.scripted() if q.name == name)
    got, rc = _lib_coefficients(p.progressive)
    assert rc == 0
    assert _same(got, PC.K.decode(p.progressive))
    assert _same(got, L.jpeg_coefficients(p.baseline))


def test_scripts_cover_what_the_issue_names():
    for kind, n in (("gray8", 1), ("420", 3)):
        s = PC.scripts(n)
        assert all(Ah == 0 and Al == 0 for _, _, _, Ah, Al in s["spectral_selection_only"])
        assert all(len(c) == 1 for c, *_ in s["dc_per_component"])
        assert {(Ss, Se) for _, Ss, Se, _, _ in s["bands_1_2__3_9__10_63"]} == {(0, 0), (1, 2), (3, 9), (10, 63)}
        assert [(Ah, Al) for _, Ss, _, Ah, Al in s["two_refinement_levels"] if Ss == 0] == [(0, 2), (2, 1), (1, 0)]
        assert {(Ah, Al) for _, Ss, _, Ah, Al in s["two_refinement_levels"] if Ss} == {(0, 2), (2, 1), (1, 0)}
    assert [c for c, Ss, *_ in PC.scripts(3)["dc_two_interleaved_one_alone"] if Ss == 0] == [(0, 1), (2,), (0, 2), (1,)]


@pytest.mark.parametrize("name", [n for n, _ in PC.refused()])
def test_incomplete_and_out_of_order_scripts_are_unsupported(name):
    data = dict(PC.refused())[name]
    got, rc = _lib_coefficients(data)
    assert got is None and rc == -7
    with pytest.raises(PC.K.Refused):
        PC.K.decode(data)


@pytest.mark.parametrize("name", [n for n, _, _ in PC.crafted()])
def test_a_second_frame_header_or_a_table_redefined_between_scans_is_rejected(name):
    """a trailing gray SOF0 once laid the recorded three-component scans over one gray plane: a write past the planes"""
    _, data, status = next(c for c in PC.crafted() if c[0] == name)
    got, rc = _lib_coefficients(data)
    assert got is None and rc == status
    assert PC.walker_verdict(data)[0] is None
    with pytest.raises(L.DfdError) as e:
        L.jpeg_coefficients(data)
    assert e.value.code == -7                                        # and with the flag off it is a progressive file like any other


def test_other_flavours_stay_unsupported():
    p = PC.by_name("17x33.420.q85").progressive
    at = p.index(b"\xff\xc2")
    twelve = bytearray(p)
    twelve[at + 4] = 12
    assert _lib_coefficients(bytes(twelve))[1] == -7
    for marker in (0xC9, 0xCA, 0xC3):                                 # arithmetic sequential / progressive, lossless
        m = bytearray(p)
        m[at + 1] = marker
        assert _lib_coefficients(bytes(m))[1] == -7
    four = bytearray(PC.by_name("8x8.gray.q85").progressive)          # a component count the decoder does not take
    at = bytes(four).index(b"\xff\xc2")
    four[at + 9] = 4
    assert _lib_coefficients(bytes(four))[1] == -7


def test_with_the_flag_off_every_file_is_still_unsupported():
    files = [p.progressive for p in PC.corpus()] + [p.progressive for p in PC.scripted()] + [f for _, f in PC.refused()]
    for f in files:
        with pytest.raises(L.DfdError) as e:
            L.jpeg_coefficients(f)
        assert e.value.code == -7
        with pytest.raises(L.DfdError) as e:
            L.jpeg_coefficients(f, progressive=False)
        assert e.value.code == -7


# ------------------------------------------------------------------------------------------------ damaged files
def test_damaged_files_get_the_walkers_verdict():
    cases = PC.damaged()
    kinds = {n.split(".")[-2] for n, _ in cases}
    assert kinds == set(PC.KINDS) and len(cases) == 72
    accepted = 0
    for name, data in cases:
        w, why = PC.walker_verdict(data)
        got, rc = _lib_coefficients(data)
        print(f"{name}: walker {'ok' if w else why}; library {rc}")
        assert (got is not None) == (w is not None), (name, why, rc)
        if w is not None:
            accepted += 1
            assert _same(got, w), name                               # another sound file: the same coefficients too
        else:
            assert rc in (-1, -7), (name, rc)
    print(f"the walker accepts {accepted} of {len(cases)}")
    assert 4 * accepted <= len(cases)

"""The files of the progressive-JPEG tests (tests/test_jpeg_progressive.py, _asan.py, _gpu.py), made once per process.

corpus()        Pillow-written pairs (progressive, baseline) of the same pixels / quality / subsampling: noise images (ZRLs
                and many correction bits) at 1x1, 8x8, 17x33, 37x53, 96x128, gray / 4:4:4 / 4:2:2 / 4:2:0, quality 30 / 85 /
                100; `optimize` and restart_marker_blocks=3 variants; one 1464 x 1464 gray image that is flat but for a
                textured corner: 33,489 blocks, so its end-of-band runs reach the 32,767 cap and go past it.
scripted()      files by tests/jpeg_progressive_writer.py under scripts Pillow never writes, with the baseline file of the
                same coefficients (tests/jpeg_stream_writer.py).
refused()       sound files whose script the library does not take.
damaged()       seeded bit flips and cuts inside each kind of scan of two files."""
import functools
import io
from dataclasses import dataclass

import numpy as np
from PIL import Image

import jpeg_progressive_walker as K
import jpeg_progressive_writer as PW
import jpeg_stream_writer as W

SIZES = ((1, 1), (8, 8), (17, 33), (37, 53), (96, 128))          # (height, width)
MODES = ("gray", "444", "422", "420")
QUALITIES = (30, 85, 100)
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


@dataclass(frozen=True)
class Pair:
    name: str
    progressive: bytes
    baseline: bytes


def noise(h, w, seed, gray=False):
    a = np.random.RandomState(seed).randint(0, 256, (h, w) if gray else (h, w, 3)).astype(np.uint8)
    return a


def pillow(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow_bgr(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def _pair(name, img, mode, **kw):
    if mode != "gray":
        kw["subsampling"] = SUBSAMPLING[mode]
    return Pair(name, pillow(img, progressive=True, **kw), pillow(img, **kw))


def flat_with_a_textured_corner():
    img = np.full((1464, 1464), 117, np.uint8)
    img[:96, :160] = noise(96, 160, 5, gray=True)
    return img


@functools.lru_cache(maxsize=None)
def corpus():
    out = []
    for i, (h, w) in enumerate(SIZES):
        for j, mode in enumerate(MODES):
            img = noise(h, w, 100 + 10 * i + j, mode == "gray")
            for q in QUALITIES:
                out.append(_pair(f"{h}x{w}.{mode}.q{q}", img, mode, quality=q))
            if (h, w) in ((17, 33), (37, 53), (96, 128)):
                out.append(_pair(f"{h}x{w}.{mode}.optimize", img, mode, quality=85, optimize=True))
                out.append(_pair(f"{h}x{w}.{mode}.restart3", img, mode, quality=85, restart_marker_blocks=3))
                out.append(_pair(f"{h}x{w}.{mode}.restart3.q100", img, mode, quality=100, restart_marker_blocks=3))
    out.append(_pair("1464x1464.gray.flat", flat_with_a_textured_corner(), "gray", quality=85))
    return tuple(out)


def by_name(name):
    return next(p for p in corpus() if p.name == name)


# ------------------------------------------------------------------------------------------------ scripts Pillow never writes
def _blocks_of(name, quality, own):
    """the quantised blocks of a corpus file, per component (blocks high, blocks wide, 64) in zig-zag order, by the walker
    (which is pinned to Pillow).  The blocks of the MCU padding are zeroed: a scan of one component never sends them, so
    only then does every script carry what the baseline file of the same blocks carries (the Pillow-written files of
    corpus() keep libjpeg's dummy blocks there, with their DC terms)."""
    w = K.decode(by_name(name).progressive)
    fulls, off = [], 0
    for (bw, bh, _), (own_h, own_w) in zip(w["comps"], own):
        f = w["coef"][off:off + bw * bh * 64].astype(np.int64).reshape(bh, bw, 64)[..., K.ZIGZAG]
        off += bw * bh * 64
        f[own_h:] = 0
        f[:, own_w:] = 0
        fulls.append(f)
    return fulls


def stream_and_blocks(kind):
    """"gray8": 8 x 8 gray; "420": 17 x 33 4:2:0, both noise at quality 100 -> (Stream, fulls)"""
    if kind == "gray8":
        return W.defaults(8, 8, "gray", 100), _blocks_of("8x8.gray.q100", 100, [(1, 1)])
    # 33 wide, 17 high: 3 x 2 MCUs of 16 x 16; luma 4 x 6 blocks of which 3 x 5 are its own; chroma 17 x 9 samples: all 2 x 3
    return W.defaults(17, 33, 2, 100), _blocks_of("17x33.420.q100", 100, [(3, 5), (2, 3), (2, 3)])


def scripts(ncomp):
    cs = tuple(range(ncomp))
    every = lambda Ss, Se, Ah, Al: [((c,), Ss, Se, Ah, Al) for c in cs]
    out = {
        "spectral_selection_only": [(cs, 0, 0, 0, 0)] + every(1, 5, 0, 0) + every(6, 63, 0, 0),
        "dc_per_component": every(0, 0, 0, 0) + every(1, 63, 0, 0),
        "bands_1_2__3_9__10_63": [(cs, 0, 0, 0, 0)] + every(1, 2, 0, 0) + every(3, 9, 0, 0) + every(10, 63, 0, 0),
        "two_refinement_levels": [(cs, 0, 0, 0, 2)] + every(1, 63, 0, 2) + [(cs, 0, 0, 2, 1)] + every(1, 63, 2, 1) + [(cs, 0, 0, 1, 0)]
        + every(1, 63, 1, 0),
        "libjpeg": PW.libjpeg_script(ncomp),
    }
    if ncomp == 3:
        out["dc_two_interleaved_one_alone"] = [((0, 1), 0, 0, 0, 1), ((2,), 0, 0, 0, 1)] + every(1, 63, 0, 1) + [((0, 2), 0, 0, 1, 0), ((1,), 0, 0, 1, 0)] \
            + every(1, 63, 1, 0)
    return out


@functools.lru_cache(maxsize=None)
def scripted():
    out = []
    for kind in ("gray8", "420"):
        S, fulls = stream_and_blocks(kind)
        base = W.from_blocks(S, fulls)
        for name, script in scripts(len(S.comps)).items():
            out.append(Pair(f"{kind}.{name}", PW.write(S, fulls, script), base))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def refused():
    """(name, file): each is -7 with the flag on"""
    out = []
    for kind in ("gray8", "420"):
        S, fulls = stream_and_blocks(kind)
        n = len(S.comps)
        cs = tuple(range(n))
        every = lambda Ss, Se, Ah, Al: [((c,), Ss, Se, Ah, Al) for c in cs]
        last = n - 1
        bad = {
            "last_component_6_63_never_sent": [(cs, 0, 0, 0, 0)] + every(1, 5, 0, 0) + [((c,), 6, 63, 0, 0) for c in cs[:last]],
            "missing_last_refinement": [(cs, 0, 0, 0, 1)] + every(1, 63, 0, 1) + [(cs, 0, 0, 1, 0)] + [((c,), 1, 63, 1, 0) for c in cs[:last]],
            "missing_last_dc_refinement": [(cs, 0, 0, 0, 1)] + every(1, 63, 0, 0),
            "ac_before_dc": every(1, 63, 0, 0) + [(cs, 0, 0, 0, 0)],
            "ah_al_do_not_continue": [(cs, 0, 0, 0, 0)] + every(1, 63, 0, 2) + every(1, 63, 1, 0),
            "refinement_skips_a_level": [(cs, 0, 0, 0, 0)] + every(1, 63, 0, 2) + every(1, 63, 2, 0),
            "band_sent_twice": [(cs, 0, 0, 0, 0)] + every(1, 63, 0, 0) + every(5, 9, 0, 0),
        }
        if kind == "gray8":                  # (one component: "the last component" is the only one)
            bad["last_component_6_63_never_sent"] = [(cs, 0, 0, 0, 0)] + every(1, 5, 0, 0)
            bad["missing_last_refinement"] = [(cs, 0, 0, 0, 1)] + every(1, 63, 0, 1) + [(cs, 0, 0, 1, 0)]
        for name, script in bad.items():
            out.append((f"{kind}.{name}", PW.write(S, fulls, script)))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ crafted structure
def _segment_at(data, marker):
    at = data.index(bytes([0xFF, marker]))
    return at, at + 2 + int.from_bytes(data[at + 2:at + 4], "big")


@functools.lru_cache(maxsize=None)
def crafted():
    """(name, file, status): files whose STRUCTURE would move the geometry under scans already parsed, or the tables under
    coefficients already sent - each must be rejected before a coefficient is written"""
    src = by_name("8x8.444.q85").progressive
    eoi = src.rindex(b"\xff\xd9")
    gray_sof0 = W.segment(0xC0, bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0]))
    a, b = _segment_at(src, 0xC2)
    wide = bytearray(src)
    wide[a + 4 + 6 + 3 + 1] = 0x22                                   # component 1 of the SOF2: sampling 2 x 2
    out = [
        # a second frame header behind the scans: one gray component, so that three-component scans would be laid over its planes
        ("sof0_behind_the_scans", src[:eoi] + gray_sof0 + src[eoi:], -1),
        ("chroma_2x2_and_sof0_behind_the_scans", bytes(wide[:eoi]) + gray_sof0 + bytes(wide[eoi:]), -7),
        ("second_sof2_behind_the_scans", src[:eoi] + src[a:b] + src[eoi:], -1),
        ("chroma_2x2", bytes(wide), -7),                             # refused at the first SOS, before a scan is recorded
    ]
    # a quantisation table redefined between two scans (libjpeg latches a component's table at its first scan)
    qa, qb = _segment_at(src, 0xDB)
    second_sos = src.index(b"\xff\xda", src.index(b"\xff\xda") + 2)
    dht_before = src.rindex(b"\xff\xc4", 0, second_sos)
    other = bytearray(src[qa:qb])
    other[5] ^= 3
    out.append(("dqt_redefined_between_scans", src[:dht_before] + bytes(other) + src[dht_before:], -7))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ damage
DAMAGE_SOURCES = ("37x53.420.restart3", "96x128.gray.q85")
DAMAGE_SEED = 3          # of the seeds 1..8 the walker accepts 16 to 22 of the 72 cases; the cap of the test is a quarter
KINDS = {"dc_first": lambda s: s[0] == 0 and s[2] == 0, "dc_refine": lambda s: s[0] == 0 and s[2] > 0,
         "ac_first": lambda s: s[0] > 0 and s[2] == 0, "ac_refine": lambda s: s[0] > 0 and s[2] > 0}


@functools.lru_cache(maxsize=None)
def damaged(seed=DAMAGE_SEED):
    """(name, file): per source and scan kind 3 single-bit flips, 3 excisions of 1..6 bytes and 3 cuts of the file, all at
    seeded places inside the entropy-coded data of a scan of that kind.  (A flipped bit of a DC refinement scan, of a
    value or of a correction bit is another sound file: those are the cases the walker accepts.)"""
    out = []
    for src in DAMAGE_SOURCES:
        data = by_name(src).progressive
        ranges = K.scan_ranges(data)
        for kind, pick in KINDS.items():
            rs = np.random.RandomState(seed * 1000 + len(out))
            mine = [r for r in ranges if pick(r) and r[5] - r[4] >= 2]
            assert mine, (src, kind)
            for i in range(9):
                _, _, _, _, a, b = mine[rs.randint(len(mine))]
                at = int(rs.randint(a, b))
                m = bytearray(data)
                if i < 3:
                    m[at] ^= 1 << int(rs.randint(8))
                    what = "flip"
                elif i < 6:
                    del m[at:min(b, at + int(rs.randint(1, 7)))]
                    what = "excise"
                else:
                    del m[at:]
                    what = "cut"
                out.append((f"{src}.{kind}.{what}{i}", bytes(m)))
    return tuple(out)


def walker_verdict(data):
    """(coefficient dict or None, why not)"""
    try:
        return K.decode(data), ""
    except (K.Defect, K.Refused) as e:
        return None, f"{type(e).__name__}: {e}"

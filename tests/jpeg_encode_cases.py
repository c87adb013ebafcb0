"""The corpus the JPEG encoder is held to Pillow on, shared by the CPU oracle test and the GPU test.

A case is (id, image, quality, subsampling, restart_blocks): image (H, W) gray or (H, W, 3) BGR u8; subsampling 0 = 4:4:4,
1 = 4:2:2, 2 = 4:2:0 (ignored for gray).  Every size meets every mode; content and quality rotate over them so that every
quality and every content meets every mode, and the pairs that hit a coder path on purpose are added by name:
uniform noise at q100 (long codes, the top size categories, many FF bytes), flat fields (EOB-only blocks, zero DC
differences), one isolated high-frequency cosine per block on a flat field (zero runs >= 16, hence ZRL).
`assert_coverage` checks on the oracle's own symbol statistics that those paths are really in the corpus.
"""
import numpy as np

import frames

# (H, W): 13 x 17 and 53 x 37 are ragged in both directions, 360 is no multiple of 16
SIZES = [(1, 1), (8, 8), (16, 16), (13, 17), (53, 37), (160, 160), (256, 256), (360, 640)]
BIG = (512, 512)                      # at 4:4:4: 12,288 blocks, more than one workgroup of the device scan covers
BIG_BLOCKS = 3 * (512 // 8) ** 2
MODES = ["gray", 0, 1, 2]
QUALITIES = [1, 25, 75, 90, 95, 100]
CONTENTS = ["noise", "flat0", "flat255", "flat128", "gradient", "cosine", "natural"]


def _content(kind, h, w, seed):
    if kind == "noise":
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind.startswith("flat"):
        return np.full((h, w, 3), int(kind[4:]), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "gradient":
        g = (255 * (xx + 2 * yy) // max(1, w + 2 * h - 3)).astype(np.uint8)
        return np.stack([g, 255 - g, (g // 2 + 60).astype(np.uint8)], -1)
    if kind == "cosine":
        # block (by, bx) carries the single frequency (v, u) = (7 - by % 4, 7 - bx % 4) on a flat field: after the DC the
        # first non-zero coefficient sits late in zig-zag order
        u, v = 7 - (xx // 8) % 4, 7 - (yy // 8) % 4
        c = np.cos((2 * (xx % 8) + 1) * u * np.pi / 16) * np.cos((2 * (yy % 8) + 1) * v * np.pi / 16)
        g = np.clip(128 + 100 * c, 0, 255).astype(np.uint8)
        return np.stack([g, g, g], -1)
    if kind == "natural":
        return frames.natural_like(h, w, seed=seed)
    raise ValueError(kind)


def _image(kind, h, w, mode, seed):
    img = _content(kind, h, w, seed)
    return np.ascontiguousarray(img[..., 1]) if mode == "gray" else img


def _mode_name(mode):
    return {"gray": "gray", 0: "444", 1: "422", 2: "420"}[mode]


def _case(kind, size, mode, q, rb=0, seed=7):
    h, w = size
    name = f"{kind}-{w}x{h}-{_mode_name(mode)}-q{q}" + (f"-r{rb}" if rb else "")
    return (name, _image(kind, h, w, mode, seed), q, 2 if mode == "gray" else mode, rb)


def _build():
    cases, k = [], 0
    for si, size in enumerate(SIZES):
        for mi, mode in enumerate(MODES):
            # 7 contents and 6 qualities against 8 x 4 (size, mode) pairs: the strides walk every content and quality
            # through every mode
            cases.append(_case(CONTENTS[(k + mi) % 7], size, mode, QUALITIES[(k // 4 + mi) % 6], seed=k))
            k += 1
    for mode in MODES:
        cases.append(_case("noise", (53, 37), mode, 100))
        cases.append(_case("noise", (256, 256), mode, 100))
        cases.append(_case("cosine", (160, 160), mode, 90))
        cases.append(_case("natural", (360, 640), mode, 75))
        cases.append(_case("flat128", (13, 17), mode, 75))
    cases.append(_case("natural", BIG, 0, 95))
    # restart intervals: 100 / 200 / 400 MCUs at 160 x 160, so more than 8 intervals at every interval length (RSTn wraps)
    for mode in MODES:
        for rb in (1, 2, 7):
            cases.append(_case("natural" if rb != 2 else "noise", (160, 160), mode, 90 if rb != 2 else 100, rb))
    cases.append(_case("gradient", (13, 17), 2, 75, 1))
    cases.append(_case("natural", (360, 640), 2, 90, 7))
    assert len({c[0] for c in cases}) == len(cases)
    return cases


CASES = _build()
PLAIN = [c for c in CASES if c[4] == 0]
RESTART = [c for c in CASES if c[4] != 0]


def assert_coverage(stats):
    """stats: the oracle's `encode_with_stats` statistics of every case of CASES."""
    assert len(stats) == len(CASES)
    assert sum(s["zrl"] for s in stats) >= 1, "no ZRL in the corpus"
    assert sum(s["stuffed"] for s in stats) >= 1, "no stuffed FF in the corpus"
    assert max(s["max_ac_size"] for s in stats) >= 9, "no AC size category >= 9 in the corpus"
    assert sum(s["eob_only"] for s in stats) >= 1, "no EOB-only block in the corpus"
    assert max(s["max_block_bits"] for s in stats) > 64, "no block coded to more than 64 bits in the corpus"
    for rb in (1, 2, 7):
        assert any(c[4] == rb and _mcus(c) > 8 * rb for c in CASES), f"no case with more than 8 intervals of {rb} MCUs"


def _mcus(case):
    img, sub = case[1], case[3]
    hs, vs = (1, 1) if img.ndim == 2 else {0: (1, 1), 1: (2, 1), 2: (2, 2)}[sub]
    return -(-img.shape[0] // (8 * vs)) * -(-img.shape[1] // (8 * hs))

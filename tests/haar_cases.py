"""Test material of the Haar fallback (tests/test_haar.py, test_haar_oracle.py, test_haar_stages_gpu.py): cascades and
frames, plain numpy, seeded.

Cascades (arrays as haar.load_cascade_xml returns them; `cascade_xml` renders any of them in OpenCV's layout):
  toy         the hand-written 24 x 24 cascade of test_haar.py (TOY_XML)
  wide        generated: window 20 wide x 28 high, 8 stages / 44 stumps over 26 two- and three-rectangle features that touch
              every window border, some 1 pixel thin, weights -1, 2, 3 and non-dyadic ones (1.5, 2.25, 1/3 in float32), stump
              and stage thresholds taken from what the oracle computes on the calibration frames, so that every stage
              rejects a share of what reaches it
  ties        window 24 wide x 20 high: leaves +-1 against stage threshold 1.0 with odd stump counts (stage sums land ON the
              threshold), balanced features against stump threshold 0.0 (flat windows land ON it)
  accept_all  24 x 24, one stage, one stump, both leaves 1: every window is a candidate

Frames: `frames(cascade name)` -> [Case(name, frame, scale_factor)], geometry relative to that cascade's window."""
import functools
from collections import namedtuple

import numpy as np

from oracle import haar_ref
from oracle import imgproc_ref as I

TOY_XML = """<?xml version="1.0"?>
<opencv_storage>
<cascade>
  <stageType>BOOST</stageType>
  <featureType>HAAR</featureType>
  <height>24</height>
  <width>24</width>
  <stageParams><boostType>GAB</boostType><maxWeakCount>3</maxWeakCount></stageParams>
  <featureParams><maxCatCount>0</maxCatCount><featSize>1</featSize><mode>BASIC</mode></featureParams>
  <stageNum>3</stageNum>
  <stages>
    <_><maxWeakCount>1</maxWeakCount><stageThreshold>0.5</stageThreshold>
      <weakClassifiers>
        <_><internalNodes>0 -1 0 0.7</internalNodes><leafValues>-1. 1.</leafValues></_>
      </weakClassifiers></_>
    <_><maxWeakCount>2</maxWeakCount><stageThreshold>1.5</stageThreshold>
      <weakClassifiers>
        <_><internalNodes>0 -1 1 -0.2</internalNodes><leafValues>-1. 1.</leafValues></_>
        <_><internalNodes>0 -1 1 0.2</internalNodes><leafValues>1. -1.</leafValues></_>
      </weakClassifiers></_>
    <_><maxWeakCount>3</maxWeakCount><stageThreshold>2.5</stageThreshold>
      <weakClassifiers>
        <_><internalNodes>0 -1 2 -0.2</internalNodes><leafValues>-1. 1.</leafValues></_>
        <_><internalNodes>0 -1 2 0.2</internalNodes><leafValues>1. -1.</leafValues></_>
        <_><internalNodes>0 -1 3 0.4</internalNodes><leafValues>-1. 1.</leafValues></_>
      </weakClassifiers></_>
  </stages>
  <features>
    <_><rects><_>0 0 24 24 -1.</_><_>6 6 12 12 4.</_></rects><tilted>0</tilted></_>
    <_><rects><_>0 0 24 24 -1.</_><_>0 0 12 24 2.</_></rects><tilted>0</tilted></_>
    <_><rects><_>0 0 24 24 -1.</_><_>0 0 24 12 2.</_></rects><tilted>0</tilted></_>
    <_><rects><_>2 2 20 20 -1.</_><_>8 8 8 8 6.25</_><_>0 0 1 1 0.5</_></rects><tilted>0</tilted></_>
  </features>
</cascade>
</opencv_storage>
"""

Case = namedtuple("Case", "name frame scale_factor")


# ------------------------------------------------------------------------------------------------------------ frames
def noise_frame(h, w, blobs, seed):
    """noise 30..69 with bright Gaussian blobs (cx, cy, radius) planted in it"""
    rs = np.random.RandomState(seed)
    f = rs.randint(30, 70, (h, w, 3)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for cx, cy, r in blobs:
        f += 150.0 * np.exp(-(((xx - cx) / r) ** 2 + ((yy - cy) / r) ** 2))[..., None]
    return np.clip(f, 0, 255).astype(np.uint8)


def flat_frame(h, w, value=97):
    return np.full((h, w, 3), value, np.uint8)


def half_flat_frame(h, w, seed):
    """left half one value (every window inside it has zero variance), right half full-range noise"""
    f = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    f[:, : w // 2] = 140
    return f


def checker_frame(h, w, cell=1):
    """0 / 255 checkerboard: the largest variance a window can have"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy // cell + xx // cell) % 2) * 255).astype(np.uint8)[..., None], 3, 2)


def padded_view(frame, pad):
    """the same pixels as a view whose rows are `pad` bytes apart beyond 3 * width (the padding holds 0xA5)"""
    h, w = frame.shape[:2]
    buf = np.full((h, 3 * w + pad), 0xA5, np.uint8)
    buf[:, : 3 * w] = frame.reshape(h, 3 * w)
    v = buf[:, : 3 * w].reshape(h, w, 3)
    assert v.base is buf and v.strides == (3 * w + pad, 3, 1)
    return v


FACTOR_BLOBS = [(100, 60, 14), (300, 60, 22), (440, 50, 18)]      # the 120 x 521 frame on which 1.1 and 1.1f part ways


def factor_frame(transposed=False):
    f = noise_frame(120, 521, FACTOR_BLOBS, 1)
    return np.ascontiguousarray(f.transpose(1, 0, 2)) if transposed else f


WINDOWS = {"toy": (24, 24), "wide": (20, 28), "ties": (24, 20), "accept_all": (24, 24)}      # (width, height)


@functools.lru_cache(maxsize=None)
def frames(name):
    ww, wh = WINDOWS[name]
    out = [Case("blobs", noise_frame(120, 150, [(40, 50, 12), (105, 70, 20)], 31), 1.1),
           Case("flat", flat_frame(60, 80), 1.1),
           Case("half-flat", half_flat_frame(90, 110, 32), 1.1),
           Case("checker", checker_frame(64, 72), 1.1),
           Case("one-position", noise_frame(wh + 1, ww + 1, [], 34), 1.1),
           Case("one-column", noise_frame(wh + 30, ww + 1, [(10, 20, 6)], 35), 1.1),
           Case("step1-scale", noise_frame(70, 90, [(45, 35, 14)], 37), 1.5),               # factors 1, 1.5, 2.25 (> 2: step 1)
           Case("row-padded", padded_view(noise_frame(100, 130, [(60, 50, 15)], 38), 17), 1.25)]
    if name == "accept_all":
        return out[:1] + out[4:7]
    out += [Case("checker2", checker_frame(75, 66, 2), 1.25),
            Case("one-row", noise_frame(wh + 1, ww + 40, [(20, 12, 6)], 36), 1.1)]
    # the integral image has one row and one column more than the image: 64 rows per block of the row scan, 256 columns
    # per block of the column scan.  Unscaled (scale 0) and as the result of the resize (scale 1 at 1.1)
    out += [Case(f"edge-{h}x{w}", noise_frame(h, w, [(w // 3, h // 2, 9)], 40 + h), 1.1)
            for h, w in ((62, 254), (63, 255), (64, 256), (65, 257))]
    out += [Case("edge-scaled-64x256", noise_frame(70, 282, [(90, 30, 12)], 51), 1.1),
            Case("edge-scaled-65x257", noise_frame(72, 283, [(200, 40, 14)], 52), 1.1),
            Case("edge-scaled-62x254", noise_frame(68, 279, [(60, 30, 10)], 53), 1.1),
            Case("edge-scaled-63x255", noise_frame(69, 281, [(150, 35, 11)], 54), 1.1)]
    out += [Case("factor-120x521", factor_frame(), 1.1), Case("factor-521x120", factor_frame(True), 1.1)]
    return out


def gray_of(frame):
    return I.bgr2gray_u8(np.ascontiguousarray(frame))


def all_scales(gray, cas, scale_factor):
    """haar_ref.scale_stages for index 0, 1, ... up to the last scale"""
    k = 0
    while True:
        t = haar_ref.scale_stages(gray, cas, scale_factor, k)
        if t is None:
            return
        yield k, t
        k += 1


def no_scale_frames(name):
    """exactly the window, and smaller: no scale fits, the result is []"""
    ww, wh = WINDOWS[name]
    return [noise_frame(wh, ww, [], 60), noise_frame(wh, ww + 50, [], 61), noise_frame(wh + 50, ww, [], 62),
            noise_frame(wh - 5, ww + 50, [], 63), noise_frame(3, 2, [], 64)]


# ---------------------------------------------------------------------------------------------------------- cascades
def _cas(win, stages, stumps, rects):
    return {"haar.win": np.asarray(win, np.float32), "haar.stages": np.asarray(stages, np.float32).reshape(-1, 3),
            "haar.stumps": np.asarray(stumps, np.float32).reshape(-1, 4), "haar.rects": np.asarray(rects, np.float32).reshape(-1, 15)}


def _num(v):
    return repr(float(v))                                     # the shortest text that reads back as the same float


def _idx(v):
    return str(int(v)) if np.isfinite(v) and v == int(v) else _num(v)      # an integer as OpenCV writes it; anything else as it is


def cascade_xml(cas):
    """the arrays in OpenCV's new cascade layout; load_cascade_xml(cascade_xml(c)) returns c bit for bit"""
    ww, wh = (int(v) for v in cas["haar.win"])
    st = ""
    for first, cnt, thr in cas["haar.stages"]:
        weak = "".join(f"<_><internalNodes>0 -1 {_idx(fi)} {_num(th)}</internalNodes><leafValues>{_num(le)} {_num(ri)}</leafValues></_>\n"
                       for fi, th, le, ri in cas["haar.stumps"][int(first):int(first + cnt)])
        st += f"<_><maxWeakCount>{int(cnt)}</maxWeakCount><stageThreshold>{_num(thr)}</stageThreshold>\n<weakClassifiers>\n{weak}</weakClassifiers></_>\n"
    ft = ""
    for r in cas["haar.rects"].reshape(-1, 3, 5):
        rs = "".join(f"<_>{_idx(x)} {_idx(y)} {_idx(w)} {_idx(h)} {_num(wt)}</_>" for j, (x, y, w, h, wt) in enumerate(r) if j < 2 or wt != 0)
        ft += f"<_><rects>{rs}</rects><tilted>0</tilted></_>\n"
    return (f'<?xml version="1.0"?>\n<opencv_storage>\n<cascade>\n<stageType>BOOST</stageType>\n<featureType>HAAR</featureType>\n'
            f"<height>{wh}</height>\n<width>{ww}</width>\n<stageNum>{len(cas['haar.stages'])}</stageNum>\n<stages>\n{st}</stages>\n"
            f"<features>\n{ft}</features>\n</cascade>\n</opencv_storage>\n")


@functools.lru_cache(maxsize=None)
def toy():
    from rtdfd_amd import haar

    return haar.load_cascade_xml(TOY_XML)


@functools.lru_cache(maxsize=None)
def accept_all():
    return _cas((24, 24), [(0, 1, 0.5)], [(0, 0.0, 1.0, 1.0)], [[0, 0, 24, 24, -1, 0, 0, 12, 24, 2, 0, 0, 0, 0, 0]])


@functools.lru_cache(maxsize=None)
def ties():
    W, H = WINDOWS["ties"]
    rects = [[0, 0, W, H, -1, 0, 0, W // 2, H, 2, 0, 0, 0, 0, 0],                    # left half against the whole: 0 on a flat window
             [0, 0, W, H, -1, 0, 0, W, H // 2, 2, 0, 0, 0, 0, 0],                    # top half
             [0, 0, W, H, -1, 6, 5, 12, 10, 4, 0, 0, 0, 0, 0],                       # centre quarter
             [0, 0, W // 2, H // 2, 1, W // 2, 0, W // 2, H // 2, -1, 0, 0, 0, 0, 0],   # top-left against top-right quadrant
             [0, 0, 8, H, 1, 8, 0, 8, H, -2, 16, 0, 8, H, 1]]                        # three vertical bands
    stumps = [(0, 0.0, -1, 1), (1, 0.0, 1, -1), (2, 0.0, -1, 1),                     # a flat window: +1 -1 +1 = 1.0, ON the threshold
              (3, 0.0, -1, 1),                                                       # one stump: +-1 against 1.0
              (4, 0.0, -1, 1), (0, 0.004, 1, -1), (1, -0.004, -1, 1),
              (2, 0.01, -1, 1), (3, -0.002, 1, -1), (4, 0.003, -1, 1), (0, -0.01, -1, 1), (1, 0.006, -1, 1)]
    return _cas((W, H), [(0, 3, 1.0), (3, 1, 1.0), (4, 3, 1.0), (7, 5, 1.0)], stumps, rects)


WIDE_WEIGHTS = [-1.0, 2.0, 3.0, 1.5, 2.25, float(np.float32(1.0 / 3.0)), -2.25, float(np.float32(-1.0 / 3.0)), -1.5]
WIDE_LEAVES = [-1.0, 1.0, 0.75, -0.5, float(np.float32(0.3)), float(np.float32(-0.7)), float(np.float32(0.9)), -0.25]


def _window_values(img, rects, win_w, win_h, step):
    """float32 norm [ny][nx] and feature values [n_feats][ny][nx] of every window of `img`, as the oracle computes them"""
    s, q = haar_ref._integral(img), haar_ref._integral(img.astype(np.int64) ** 2)
    ys, xs = np.arange(0, img.shape[0] - win_h, step), np.arange(0, img.shape[1] - win_w, step)
    nw, nh = win_w - 2, win_h - 2
    vs = haar_ref._rect(s, 1, 1, nw, nh, ys, xs).astype(np.float64)
    vq = haar_ref._rect(q, 1, 1, nw, nh, ys, xs).astype(np.float64)
    nf = float(nw * nh) * vq - vs * vs
    norm = np.where(nf > 0, 1.0 / np.sqrt(np.where(nf > 0, nf, 1.0)), 1.0).astype(np.float32)
    vals, sums = [], []
    for r in rects.reshape(-1, 3, 5):
        rs = [haar_ref._rect(s, *(int(t) for t in r[j, :4]), ys, xs) for j in range(3)]
        v = np.float32(r[0, 4]) * rs[0].astype(np.float32) + np.float32(r[1, 4]) * rs[1].astype(np.float32)
        if r[2, 4] != 0:
            v = v + np.float32(r[2, 4]) * rs[2].astype(np.float32)
        vals.append(v)
        sums.append(rs)
    return norm, np.stack(vals), sums


def window_pool(name, cas_rects, cases):
    """(norm [N], values [n_feats][N]) over every window of every scale of `cases`"""
    ww, wh = WINDOWS[name]
    probe = _cas((ww, wh), [(0, 1, 0.5)], [(0, 0.0, 1.0, 1.0)], [[0, 0, ww, wh, -1, 0, 0, 1, 1, 2, 0, 0, 0, 0, 0]])
    norms, vals = [], []
    for c in cases:
        gray = I.bgr2gray_u8(np.ascontiguousarray(c.frame))
        k = 0
        while True:
            t = haar_ref.scale_stages(gray, probe, c.scale_factor, k)
            if t is None:
                break
            n, v, _ = _window_values(t["scaled"], cas_rects, ww, wh, t["step"])
            norms.append(n.ravel())
            vals.append(v.reshape(v.shape[0], -1))
            k += 1
    return np.concatenate(norms), np.concatenate(vals, 1)


@functools.lru_cache(maxsize=None)
def wide():
    W, H = WINDOWS["wide"]
    rs = np.random.RandomState(2024)
    pick = lambda seq: seq[rs.randint(len(seq))]                  # noqa: E731
    # rectangles on every border of the window, and 1-pixel-thin ones
    rects = [[0, 0, W, 1, 3, 0, 1, W, 1, -1, 0, 0, 0, 0, 0],                            # top row against the second row
             [0, H - 1, W, 1, 2.25, 0, H - 3, W, 2, -1, 0, 0, 0, 0, 0],                 # bottom row
             [0, 0, 1, H, 1.5, 1, 0, 1, H, -1, 0, 0, 0, 0, 0],                          # left column
             [W - 1, 0, 1, H, 2, W - 3, 0, 2, H, -1, 0, 0, 0, 0, 0],                    # right column
             [0, 0, W, H, -1, 0, 0, W, H // 2, 2, W - 1, H - 1, 1, 1, WIDE_WEIGHTS[5]],  # whole window, top half, the last pixel
             [0, 0, W, H, WIDE_WEIGHTS[5], 5, 7, 10, 14, -1, 0, 0, 0, 0, 0]]
    while len(rects) < 26:
        f = []
        for j in range(3):
            if j == 2 and rs.randint(2):
                f += [0, 0, 0, 0, 0]
                continue
            w, h = 1 + rs.randint(W), 1 + rs.randint(H)
            f += [rs.randint(W - w + 1), rs.randint(H - h + 1), w, h, pick(WIDE_WEIGHTS)]
        rects.append(f)
    rects = np.asarray(rects, np.float32)
    norm, vals = window_pool("wide", rects, [c for c in frames("wide") if c.name in ("blobs", "half-flat", "checker", "step1-scale", "edge-64x256", "factor-120x521")])
    prod = vals * norm[None, :]                                   # float32, the number a stump compares
    alive = np.ones(norm.shape, bool)
    stages, stumps = [], []
    for count in (3, 4, 5, 5, 6, 6, 7, 8):
        first = len(stumps)
        acc = np.zeros(norm.shape, np.float64)
        for _ in range(count):
            fi = rs.randint(len(rects))
            reach = np.sort(prod[fi][alive])
            thr = reach[int(len(reach) * (0.3 + 0.4 * rs.rand()))]      # a value some window produces: met exactly there
            left = pick(WIDE_LEAVES)
            right = pick([v for v in WIDE_LEAVES if v != left])
            stumps.append((fi, thr, left, right))
            acc += np.where(prod[fi] < thr, np.float32(left), np.float32(right)).astype(np.float64)
        levels = np.unique(acc[alive])
        share = np.array([(acc[alive] < t).mean() for t in levels])
        thr = np.float32(levels[np.argmax(share >= 0.4)])          # the lowest level that rejects two fifths of what arrives
        stages.append((first, count, thr))
        alive &= acc >= np.float64(thr)
    return _cas((W, H), stages, stumps, rects)


CASCADES = {"toy": toy, "wide": wide, "ties": ties, "accept_all": accept_all}


# ------------------------------------------------------------------------------------------------- malformed cascades
def malformed(base=None):
    """[(what is wrong, cascade arrays)]: one per condition dfd_create and the XML reader refuse"""
    base = base or ties()

    def edit(key, index, value):
        c = {k: v.copy() for k, v in base.items()}
        c[key][index] = value
        return c

    n_stumps, n_feats = len(base["haar.stumps"]), len(base["haar.rects"])
    W, H = (float(v) for v in base["haar.win"])
    skipped = {k: v.copy() for k, v in base.items()}
    skipped["haar.stages"][1:, 0] += 1                             # stage 1 starts one stump late: a gap
    skipped["haar.stumps"] = np.concatenate([skipped["haar.stumps"], skipped["haar.stumps"][-1:]])
    # (what is wrong, arrays, whether OpenCV's XML layout can express it: the stage table is implied there)
    return [("feature index == feature count", edit("haar.stumps", (2, 0), n_feats), True),
            ("feature index negative", edit("haar.stumps", (0, 0), -1), True),
            ("feature index fractional", edit("haar.stumps", (1, 0), 0.5), True),
            ("feature index NaN", edit("haar.stumps", (0, 0), np.nan), True),
            ("rectangle reaches past the right border", edit("haar.rects", (1, 2), W + 1), True),
            ("rectangle reaches past the bottom border", edit("haar.rects", (3, 6), H - 1), True),
            ("rectangle x negative", edit("haar.rects", (0, 5), -1), True),
            ("rectangle width 0", edit("haar.rects", (2, 7), 0), True),
            ("rectangle y fractional", edit("haar.rects", (2, 6), 5.5), True),
            ("third rectangle past the window", edit("haar.rects", (4, 12), 9), True),
            ("unused third rectangle with geometry", edit("haar.rects", (0, 12), 3), False),
            ("last stage runs past the stump table", edit("haar.stages", (-1, 1), base["haar.stages"][-1, 1] + 1), False),
            ("first stage claims more stumps than there are", edit("haar.stages", (0, 1), n_stumps + 1), False),
            ("stage count 0", edit("haar.stages", (1, 1), 0), True),
            ("stage first negative", edit("haar.stages", (0, 0), -1), False),
            ("stages not contiguous", skipped, False),
            ("stage threshold NaN", edit("haar.stages", (0, 2), np.nan), True),
            ("stump threshold infinite", edit("haar.stumps", (3, 1), np.inf), True),
            ("leaf NaN", edit("haar.stumps", (3, 3), np.nan), True),
            ("rectangle weight infinite", edit("haar.rects", (1, 4), -np.inf), True)]

"""Inputs and the exact float32 reference for the tests of the 8-bit face path (test_imgproc.py, test_imgproc_gpu.py).
No GPU and no product code here: numpy only.

  lattice(order)           512 x 512 x 3 image of all 64^3 (b, g, r) triples over LEVELS: sRGB levels 0..12 (the gamma knee
                           and the cube-root table's linear branch), then 51 levels up to 255 - black, white, every
                           saturated primary and 64 grays among them
  PATTERNS / crop(...)     constant, checkerboard, ramp and full-range noise crops at any (h, w)
  GEOMETRIES               the (h, w) at which CLAHE's kernels change path (see each list)
  crop_norm_f32            crop_norm_kernel restated in numpy float32, one rounding per kernel operation
"""
import numpy as np

# ------------------------------------------------------------------------------------------------ full-gamut lattice
LEVELS = np.unique(np.concatenate([np.arange(0, 13), np.linspace(13, 255, 51).astype(int)]))
assert LEVELS.size == 64 and LEVELS[0] == 0 and LEVELS[-1] == 255
LATTICE_ORDERS = ("meshgrid", "permuted")


def lattice(order: str = "meshgrid") -> np.ndarray:
    """All 64^3 (b, g, r) triples as a 512 x 512 x 3 image: meshgrid order (b slowest; long constant runs, tiles of few
    levels) or one seeded permutation of the same pixels (every tile sees the whole gamut)."""
    b, g, r = np.meshgrid(LEVELS, LEVELS, LEVELS, indexing="ij")
    px = np.stack([b.ravel(), g.ravel(), r.ravel()], axis=-1).astype(np.uint8)
    if order == "permuted":
        px = px[np.random.RandomState(20240).permutation(px.shape[0])]
    elif order != "meshgrid":
        raise ValueError(order)
    return np.ascontiguousarray(px.reshape(512, 512, 3))


# ------------------------------------------------------------------------------------------------ structured crops
MID_COLOUR = (37, 150, 201)                      # b, g, r


def _const(v):
    return lambda h, w: np.broadcast_to(np.asarray(v, np.uint8), (h, w, 3)).copy()


def _checker(lo, hi):
    def make(h, w):
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat(np.where((yy + xx) & 1, hi, lo).astype(np.uint8)[:, :, None], 3, axis=2)
    return make


def _hramp(h, w):
    x = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)            # 0 .. 255 across the row (0 when w == 1)
    row = np.stack([x, 255 - x, x // 2], axis=-1)
    return np.ascontiguousarray(np.broadcast_to(row[None], (h, w, 3)))


def _noise(h, w):
    return np.random.RandomState(1000 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)


PATTERNS = {
    "const0": _const(0),
    "const255": _const(255),
    "const_mid": _const(MID_COLOUR),
    "checker_0_255": _checker(0, 255),
    "checker_127_128": _checker(127, 128),
    "hramp": _hramp,
    "noise": _noise,
}


def crop(pattern: str, h: int, w: int) -> np.ndarray:
    out = PATTERNS[pattern](h, w)
    assert out.shape == (h, w, 3) and out.dtype == np.uint8
    return out


# ------------------------------------------------------------------------------------------------ geometries (h, w)
# CLAHE pads both sides by a full 8 - n % 8 once either is ragged: for n in {1, 2, 3, 4, 8} the pad passes one reflection
REFLECT_GEOMS = [(8, 13), (13, 8), (4, 16), (16, 4), (3, 3), (2, 40), (1, 1), (1, 9), (8, 8)]
# tile areas 1, 4, 4, 9: below 128 the clip limit int(2 * area / 256) is 0 and becomes 1
SMALL_TILE_GEOMS = [(5, 5), (9, 9), (16, 16), (15, 17)]
# every w % 4 and w % 8: the four-pixel path, the one-pixel border path, groups of the apply kernel that wrap a row
WIDTH_GEOMS = [(33, w) for w in range(61, 69)]
# One crop alone gets min(64, ceil(h*w / 4 / 1024)) apply blocks of ceil(groups / blocks) four-pixel groups each.
# 257 x 1023 = 65728 groups is exactly 64 blocks of 1027; 257 x 1025 = 263425 pixels = 65857 groups (the last holds one
# pixel) is 63 blocks of 1030 and a last block of 967 (apply_grid_facts, asserted below).
BIG_GEOMS = [(257, 1023), (257, 1025)]
GEOMETRIES = REFLECT_GEOMS + SMALL_TILE_GEOMS + WIDTH_GEOMS + BIG_GEOMS


def apply_grid_facts(h: int, w: int, n: int = 1, max_pixels: int = None):
    """(blocks, groups, groups per block, groups of the last non-empty block) of the CLAHE apply launch for an h x w
    crop in a call of n crops whose largest has max_pixels: the arithmetic documented for launch_clahe, restated so that
    the cases can be chosen by it."""
    mp = h * w if max_pixels is None else max_pixels
    cap = 8 if n >= 256 else 16 if n >= 64 else 64
    gx = max(1, min(cap, (mp // 4 + 1023) // 1024))
    groups = (h * w + 3) // 4
    per = (groups + gx - 1) // gx
    last = groups - ((groups - 1) // per) * per
    return gx, groups, per, last


assert apply_grid_facts(257, 1023) == (64, 65728, 1027, 1027) and apply_grid_facts(257, 1025) == (64, 65857, 1030, 967)


# ------------------------------------------------------------------------------------------------ crop -> network input
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# (h, w) of the crops crop_norm is held to: one pixel, one row, one column, just below / at / just above the output
# size (down-, identity and up-sampling weights), a large ragged one
NORM_GEOMS = [(1, 1), (1, 50), (50, 1), (223, 223), (224, 224), (225, 225), (300, 500)]


def _crop_norm(face_bgr: np.ndarray, dt) -> np.ndarray:
    h, w = face_bgr.shape[:2]
    f = dt
    o = np.arange(224, dtype=dt)

    def taps(n):
        s = f(n) / f(224.0)
        c = s * (o + f(0.5)) - f(0.5)
        c = np.where(c < 0, f(0), c).astype(dt)
        i0 = c.astype(np.int64)                                   # truncation; c >= 0
        i1 = i0 + (i0 < n - 1)
        lo = (c - i0.astype(dt)).astype(dt)
        return i0, i1, lo, (f(1.0) - lo).astype(dt)

    y0, y1, ly, hy = taps(h)
    x0, x1, lx, hx = taps(w)
    ly, hy, lx, hx = ly[:, None], hy[:, None], lx[None, :], hx[None, :]
    out = np.empty((3, 224, 224), dt)
    for c in range(3):                                            # output channel c = R, G, B = source byte 2 - c
        p = face_bgr[:, :, 2 - c].astype(dt)
        p00, p01 = p[y0][:, x0], p[y0][:, x1]
        p10, p11 = p[y1][:, x0], p[y1][:, x1]
        v = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11)
        out[c] = (v / f(255.0) - f(MEAN[c])) / f(STD[c])
    assert out.dtype == dt
    return out


def crop_norm_f32(face_bgr: np.ndarray) -> np.ndarray:
    """crop_norm_kernel in its own operation order, every operation rounded to float32 once (numpy float32 arrays and
    scalars; the kernel's file is compiled without contraction): scale = n / 224, source coordinate scale * (o + 0.5) -
    0.5 clamped at 0, truncated to the first tap, second tap + 1 unless at the edge, weights l = c - i0 and 1 - l,
    hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11), then (v / 255 - mean) / std.  -> (3, 224, 224) float32"""
    return _crop_norm(face_bgr, np.float32)


def crop_norm_f64(face_bgr: np.ndarray) -> np.ndarray:
    """the same formula evaluated in float64 (constants 0.485 ... as doubles)"""
    return _crop_norm(face_bgr, np.float64)


NORM_CASE_NAMES = [f"{h}x{w}" for h, w in NORM_GEOMS] + ["corner"]


def norm_cases():
    """[(name, frame, (x, y, w, h))]: every NORM_GEOMS crop inside a full-range noise frame at x = 5, y = 3 (row stride
    above 3 w), and one 120 x 97 crop that ends on the frame's last row and column"""
    out = []
    for h, w in NORM_GEOMS:
        out.append((f"{h}x{w}", _noise(h + 7, w + 8), (5, 3, w, h)))
    out.append(("corner", _noise(160, 190), (190 - 97, 160 - 120, 97, 120)))
    return out


def cut(frame: np.ndarray, box) -> np.ndarray:
    x, y, w, h = box
    return frame[y:y + h, x:x + w]


# ------------------------------------------------------------------------------------------------ batched launch shapes
BATCH_FRAME_HW = (400, 400)
BATCH_SIZES = (17, 64, 256)
BIG_BOX_WH = (300, 300)


def batch_frame() -> np.ndarray:
    return np.random.RandomState(77).randint(0, 256, BATCH_FRAME_HW + (3,)).astype(np.uint8)


def _small_boxes(count: int):
    """`count` boxes (x, y, w, h) of at most 224 x 224 inside the batch frame: the reflection and small-tile geometries
    first, then seeded sizes - mostly small (every crop is a 64-block hist launch and a host reference), every 16th up to
    224, widths and heights over all residues of 8"""
    H, W = BATCH_FRAME_HW
    rs = np.random.RandomState(78)
    sizes = [(h, w) for h, w in REFLECT_GEOMS + SMALL_TILE_GEOMS + WIDTH_GEOMS[:4]]
    while len(sizes) < count:
        hi = 225 if len(sizes) % 16 == 0 else 49
        sizes.append((int(rs.randint(1, hi)), int(rs.randint(1, hi))))
    return [(int(rs.randint(0, W - w + 1)), int(rs.randint(0, H - h + 1)), w, h) for h, w in sizes[:count]]


def batch_boxes(n: int):
    """n boxes for one preprocess_crops call: the first n - 3 of one fixed list of small boxes (so the calls of different
    n share references), and one 300 x 300 box placed first, in the middle and last - it alone sets the launch's
    max_pixels (90000 px -> 22 apply blocks per crop, capped to 16 at n >= 64 and 8 at n >= 256)."""
    small = _small_boxes(n - 3)
    big = (50, 60) + BIG_BOX_WH
    mid = (n - 3) // 2
    boxes = [big] + small[:mid] + [big] + small[mid:] + [big]
    assert len(boxes) == n
    return boxes

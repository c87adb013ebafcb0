"""CPU: product colour tables vs the oracle's independent construction, and sanity of the
image-processing oracle itself (properties that hold for any correct implementation)."""
import numpy as np

import imgproc_cases as IC
from oracle import imgproc_ref as R


def test_product_tables_equal_oracle_tables(pkg):
    mine = pkg.luts.build()
    ref = R.lab_tables()
    pairs = {"lut.gamma": "gamma", "lut.cbrt": "cbrt", "lut.fwd_coef": "fwd_coef", "lut.L_fy": "L_fy",
             "lut.L_y": "L_y", "lut.a_div": "a_div", "lut.b_div": "b_div", "lut.ab_xz": "ab_xz",
             "lut.inv_coef": "inv_coef", "lut.inv_gamma": "inv_gamma"}
    for a, b in pairs.items():
        assert np.array_equal(mine[a], ref[b].astype(np.int64)), a
    sdiv, hdiv = R._hsv_tables()
    assert np.array_equal(mine["lut.hsv_sdiv"], sdiv) and np.array_equal(mine["lut.hsv_hdiv"], hdiv)


def test_resize_identity_constant_and_shapes():
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    assert np.array_equal(R.resize_linear_u8(img, 53, 37), img)
    flat = np.full((1080, 1920, 3), 77, np.uint8)
    assert np.all(R.resize_linear_u8(flat, 256, 256) == 77)
    up = R.resize_linear_u8(img, 300, 300)
    assert up.shape == (300, 300, 3) and up.min() >= img.min() and up.max() <= img.max()
    # 2x upsample of a horizontal ramp stays monotone
    ramp = np.tile(np.arange(0, 200, 4, dtype=np.uint8)[None, :, None], (8, 1, 3))
    r2 = R.resize_linear_u8(ramp, 100, 8).astype(int)
    assert np.all(np.diff(r2[0, :, 0]) >= 0)


def test_gray_hsv_known_values():
    px = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 100]]], np.uint8)
    g = R.bgr2gray_u8(px)[0]
    assert list(g[:5]) == [0, 255, 29, 150, 76]              # ITU-R 601 weights, fixed point
    hsv = R.bgr2hsv_u8(px)[0]
    assert list(hsv[0]) == [0, 0, 0] and list(hsv[1]) == [0, 0, 255]
    assert list(hsv[2]) == [120, 255, 255] and list(hsv[3]) == [60, 255, 255] and list(hsv[4]) == [0, 255, 255]
    assert hsv[:, 0].max() < 180


def test_lab_roundtrip_and_anchors():
    t = R.lab_tables()
    px = np.array([[[0, 0, 0], [255, 255, 255], [128, 128, 128]]], np.uint8)
    lab = R.bgr2lab_u8(px, t)[0]
    assert list(lab[0]) == [0, 128, 128] and list(lab[1]) == [255, 128, 128] and abs(int(lab[2][0]) - 137) <= 1
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    back = R.lab2bgr_u8(R.bgr2lab_u8(img, t), t)
    d = np.abs(back.astype(int) - img.astype(int))
    # 8-bit Lab quantisation only: sub-level on average, a few levels in the dark saturated corner
    assert d.mean() < 1.0 and np.percentile(d, 99) <= 8 and d.max() <= 32


def test_lab2rgb_integer_table_anchors():
    """Facts OpenCV's color_lab.cpp states about its own Lab2RGBinteger tables (source comments and constants): the a/b
    offsets reach down to exactly minABvalue = -8145 over the 8-bit cube, abToXZ_b spans [-1335, 88231] over
    LAB_BASE*9/4 entries, f(y) starts at BASE*16/116, the inverse gamma table has 2^12 entries ending at 255."""
    t = R.lab_tables()
    fx = t["L_fy"][:, None].astype(int) + t["a_div"][None, :]
    fz = t["L_fy"][:, None].astype(int) - t["b_div"][None, :]
    assert min(fx.min(), fz.min()) == -8145 and max(fx.max(), fz.max()) < 36864 - 8145
    assert len(t["ab_xz"]) == 36864 and t["ab_xz"].min() == -1335 and t["ab_xz"].max() == 88231
    assert t["L_fy"][0] == 2260 and t["L_fy"][255] == 16384 and t["L_y"][0] == 0 and t["L_y"][255] == 16384
    assert np.all(np.diff(t["L_y"]) > 0) and np.all(np.diff(t["ab_xz"]) >= 0)
    assert len(t["inv_gamma"]) == 4096 and t["inv_gamma"][0] == 0 and t["inv_gamma"][-1] == 255
    assert t["a_div"][128] == 0 and t["b_div"][128] == 1          # the "+1" of bdiv is OpenCV's, "not a typo" there
    # greys survive the 8-bit round trip within one level
    g = np.arange(256, dtype=np.uint8)
    grey = np.stack([g, g, g], -1)[None]
    assert np.abs(R.lab2bgr_u8(R.bgr2lab_u8(grey, t), t).astype(int) - grey).max() <= 1


def test_clahe_properties():
    rs = np.random.RandomState(2)
    flat = np.full((64, 64), 90, np.uint8)
    out = R.clahe_u8(flat)
    assert out.shape == flat.shape and len(np.unique(out)) == 1
    low = (rs.rand(80, 104) * 40 + 100).astype(np.uint8)      # low-contrast, ragged size (pads)
    eq = R.clahe_u8(low)
    assert eq.shape == low.shape and int(eq.max()) - int(eq.min()) > int(low.max()) - int(low.min())
    # monotone within a single tile-LUT region: equalisation never reorders grey levels of a flat-LUT image
    g = np.tile(np.arange(256, dtype=np.uint8), (256, 1))
    e = R.clahe_u8(g).astype(int)
    assert np.all(np.diff(e[128]) >= -1)


def test_gaussian_laplacian_canny_properties():
    rs = np.random.RandomState(3)
    const = np.full((32, 32), 50, np.uint8)
    assert np.allclose(R.gaussian5_f32(const), 50.0) and np.all(R.laplacian_i32(const) == 0)
    assert R.canny_u8(const).max() == 0
    sq = np.zeros((64, 64), np.uint8)
    sq[16:48, 16:48] = 255
    e = R.canny_u8(sq)
    assert e[16, 30] == 255 or e[15, 30] == 255                # an edge along the square's border
    assert e[32, 32] == 0 and e[2, 2] == 0
    assert set(np.unique(e)) <= {0, 255}
    imp = np.zeros((9, 9), np.float32)
    imp[4, 4] = 256.0
    k = np.array([1, 4, 6, 4, 1], np.float32) / 16
    assert np.allclose(R.gaussian5_f32(imp)[2:7, 2:7], 256 * np.outer(k, k))


def test_crop_resize_normalize_shape_and_range():
    rs = np.random.RandomState(4)
    face = rs.randint(0, 256, (90, 70, 3)).astype(np.uint8)
    x = R.crop_resize_normalize(face)
    assert x.shape == (3, 224, 224) and x.dtype == np.float32
    assert x.min() >= (0 - 0.485) / 0.229 - 1e-5 and x.max() <= (1 - 0.406) / 0.225 + 1e-5
    same = R.crop_resize_normalize(np.full((224, 224, 3), 128, np.uint8))
    assert np.allclose(same[0], (128 / 255 - 0.485) / 0.229, atol=1e-6)


# ------------------------------------------------------------------------------------------------ edges of the face path
def _border_interpolate_101(p, n):
    """OpenCV's borderInterpolate for BORDER_REFLECT_101, as its source states it, one index at a time"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def test_reflect101_stays_in_range_under_clahe_pad():
    """CLAHE pads a ragged side n to n + (8 - n % 8): for n in {1, 2, 3, 4, 8} that passes one reflection.  The helper
    must land in [0, n) for every n and equal borderInterpolate; a single reflection goes negative exactly at those n."""
    one_pass_negative = []
    for n in range(1, 21):
        i = np.arange(n + 8 - n % 8)
        got = R._reflect101(i, n)
        assert got.shape == i.shape and got.min() >= 0 and got.max() < n, n
        assert list(got) == [_border_interpolate_101(int(p), n) for p in i], n
        assert np.array_equal(got[:n], i[:n])
        once = np.where(i >= n, 2 * (n - 1) - i, i)
        if once.min() < 0:
            one_pass_negative.append(n)
    assert one_pass_negative == [1, 2, 3, 4, 8]


def test_reflect101_filter_offsets_unchanged():
    """The Gaussian and Laplacian oracles call the helper with offsets of at most 2: for n >= 3 one reflection was
    already enough, and the indices are what it gave."""
    for n in range(3, 21):
        for d in (-2, -1, 0, 1, 2):
            i = np.arange(n) + d
            a = np.abs(i)
            assert np.array_equal(R._reflect101(i, n), np.where(a >= n, 2 * (n - 1) - a, a)), (n, d)
            assert list(R._reflect101(i, n)) == [_border_interpolate_101(int(p), n) for p in i]


def test_clahe_accepts_every_small_geometry():
    """clahe_u8 of the parent raised IndexError at sides 1 and 2; every geometry of the cases runs and a constant
    crop stays constant."""
    for h, w in IC.REFLECT_GEOMS + IC.SMALL_TILE_GEOMS:
        out = R.clahe_u8(np.full((h, w), 93, np.uint8))
        assert out.shape == (h, w) and len(np.unique(out)) == 1, (h, w)


def _constant_tile_lut(v, area):
    """OpenCV's clip / redistribute rule on a tile whose `area` pixels all hold v, in closed form: the one bin keeps
    `clip`, the other area - clip counts go back as `batch` to every bin and one more to bins 0, step, 2 step, ...
    (`residual` of them); the LUT entry is the rounded cdf at v times 255 / area."""
    clip = max(int(2.0 * area / 256), 1)
    clipped = area - clip
    batch, residual = clipped // 256, clipped % 256
    cdf = clip + batch * (v + 1)
    if residual:
        step = max(256 // residual, 1)
        cdf += min(residual, v // step + 1)
    return int(np.clip(np.rint(np.float32(cdf) * (np.float32(255.0) / np.float32(area))), 0, 255))


def test_clahe_constant_tile_closed_form():
    """A constant crop: every tile has the same LUT, so the blend returns LUT[v] whatever the weights.
    Tile area 25 (40 x 40 crop, below 256): clip = max(int(50 / 256), 1) = 1, 24 counts to hand back, batch 0, residual 24,
      step 256 // 24 = 10 -> bins 0, 10, ..., 230 get one.  v = 100: cdf = 1 + 11 = 12 -> rint(12 * 255 / 25 = 122.4) = 122;
      v = 5: cdf = 1 + 1 = 2 -> rint(20.4) = 20;  v = 255: cdf = 1 + 24 = 25 -> 255;  v = 0: cdf = 1 + 1 -> 20.
    Tile area 1024 (256 x 256 crop, above 256): clip = int(2048 / 256) = 8, 1016 back, batch 3, residual 248, step 1 ->
      bins 0..247 get one.  v = 100: cdf = 8 + 3 * 101 + 101 = 412 -> rint(412 * 255 / 1024 = 102.6) = 103;
      v = 250: cdf = 8 + 3 * 251 + 248 = 1009 -> rint(251.26) = 251;  v = 255: cdf = 1024 -> 255;  v = 0: 8 + 3 + 1 = 12 -> 3.
    A ragged 37 x 43 crop pads to 40 x 48: tile 5 x 6 = 30, clip 1, residual 29, step 8: v = 100: 1 + 13 = 14 -> 119."""
    by_hand = {(40, 40, 100): 122, (40, 40, 5): 20, (40, 40, 255): 255, (40, 40, 0): 20,
               (256, 256, 100): 103, (256, 256, 250): 251, (256, 256, 255): 255, (256, 256, 0): 3,
               (37, 43, 100): 119}
    for (h, w, v), want in by_hand.items():
        eh, ew = (h, w) if h % 8 == 0 and w % 8 == 0 else (h + 8 - h % 8, w + 8 - w % 8)
        area = (eh // 8) * (ew // 8)
        assert _constant_tile_lut(v, area) == want, (h, w, v)
        out = R.clahe_u8(np.full((h, w), v, np.uint8))
        assert np.all(out == want), (h, w, v, np.unique(out))


def _lab_float64(bgr):
    """CIE L*a*b* of sRGB pixels from the definition, in float64, on the 8-bit scale (L * 255 / 100, a + 128, b + 128),
    unrounded; matrix and white point are the oracle's D65 constants"""
    x = bgr.astype(np.float64) / 255
    lin = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    b, g, r = lin[..., 0], lin[..., 1], lin[..., 2]
    m = R._RGB2XYZ
    xyz = [(m[3 * i] * r + m[3 * i + 1] * g + m[3 * i + 2] * b) / R._D65[i] for i in range(3)]
    fx, fy, fz = [np.where(u > 216 / 24389, np.cbrt(u), u * (841 / 108) + 16 / 116) for u in xyz]
    return np.stack([(116 * fy - 16) * 255 / 100, 500 * (fx - fy) + 128, 200 * (fy - fz) + 128], axis=-1)


def test_bgr2lab_lattice_near_cie_definition():
    """The integer BGR->Lab oracle over the full-gamut lattice (all 64^3 triples: the gamma knee, the cube-root table's
    linear branch, black, white, saturated primaries, grays) stays within 2 / 3 / 2 levels of the float64 definition;
    measured 1.443 / 2.358 / 1.593.  A guard against a gross table or coefficient error, not a claim of cv2 parity."""
    img = IC.lattice("meshgrid")
    assert len(np.unique(img.reshape(-1, 3), axis=0)) == 64 ** 3
    perm = IC.lattice("permuted")
    assert not np.array_equal(perm, img)
    assert np.array_equal(np.unique(perm.reshape(-1, 3), axis=0), np.unique(img.reshape(-1, 3), axis=0))
    t = R.lab_tables()
    d = np.abs(R.bgr2lab_u8(img, t).astype(np.float64) - _lab_float64(img)).reshape(-1, 3).max(axis=0)
    print("bgr2lab_u8 vs float64 CIE, max |d| (L, a, b):", d)
    assert d[0] <= 2 and d[1] <= 3 and d[2] <= 2, d
    for im in (img, perm):                       # lab2bgr_u8 asserts that every index stays inside OpenCV's table
        out = R.preprocess_face_quality(im, t)
        assert out.shape == im.shape and out.dtype == np.uint8


# measured maxima of test_crop_norm_f32_against_torch_and_float64, asserted at twice their value
CROP_NORM_VS_TORCH = 6.628e-5
CROP_NORM_VS_F64 = 1.649e-4


def test_crop_norm_f32_against_torch_and_float64():
    """imgproc_cases.crop_norm_f32 restates crop_norm_kernel in float32, operation by operation; the GPU tests hold the
    kernel to it bit for bit.  Here it is placed between two independent evaluations over the same crops (1x1, 1x50,
    50x1, 223^2, 224^2, 225^2, 300x500, a frame-corner crop; each raw and after the CLAHE oracle):
      max |crop_norm_f32 - R.crop_resize_normalize| (torch float32)  = 6.628e-5
      max |crop_norm_f32 - the same formula in float64|              = 1.649e-4
    (both at the CLAHE'd 300x500 crop; 224^2 is 0 against torch and 3.7e-7 against float64)
    on outputs of magnitude up to 2.64.  Each is asserted at twice the measured value: torch's vectorised kernel orders
    the weights differently from build to build, and the float64 distance is a few ulps of the blend weight (the source
    coordinate near 500 carries 3e-5 of float32 rounding, times a step of up to 255 / 255 / 0.224 between neighbours)."""
    t = R.lab_tables()
    worst_torch = worst_f64 = 0.0
    for name, frame, box in IC.norm_cases():
        raw = np.ascontiguousarray(IC.cut(frame, box))
        for face in (raw, R.preprocess_face_quality(raw, t)):
            a = IC.crop_norm_f32(face)
            assert a.dtype == np.float32 and a.shape == (3, 224, 224)
            d_torch = float(np.abs(a - R.crop_resize_normalize(face)).max())
            d_f64 = float(np.abs(a.astype(np.float64) - IC.crop_norm_f64(face)).max())
            print(f"crop_norm_f32 {name}: vs torch {d_torch:.4e}  vs float64 {d_f64:.4e}")
            worst_torch, worst_f64 = max(worst_torch, d_torch), max(worst_f64, d_f64)
    print(f"crop_norm_f32 maxima: vs torch {worst_torch:.4e}  vs float64 {worst_f64:.4e}")
    assert worst_torch <= 2 * CROP_NORM_VS_TORCH, worst_torch
    assert worst_f64 <= 2 * CROP_NORM_VS_F64, worst_f64
    # a 224 x 224 crop is sampled at integer coordinates: weights 1 and 0, the bytes themselves
    face = np.ascontiguousarray(IC.cut(*[c for c in IC.norm_cases() if c[0] == "224x224"][0][1:]))
    want = (face[..., ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
            - np.array(IC.MEAN, np.float32)[:, None, None]) / np.array(IC.STD, np.float32)[:, None, None]
    assert np.array_equal(IC.crop_norm_f32(face), want)


def test_imgproc_cases_cover_what_they_claim():
    """The inputs reach the paths they are chosen for (so a later edit of the cases cannot quietly stop covering them)."""
    t = R.lab_tables()
    lab = R.bgr2lab_u8(IC.lattice(), t)
    assert lab[..., 0].min() == 0 and lab[..., 0].max() == 255                      # black and white
    assert lab[..., 1].min() < 60 and lab[..., 1].max() > 200 and lab[..., 2].min() < 30 and lab[..., 2].max() > 220
    assert set(IC.PATTERNS) == {"const0", "const255", "const_mid", "checker_0_255", "checker_127_128", "hramp", "noise"}
    for h, w in IC.GEOMETRIES:
        for p in IC.PATTERNS:
            assert IC.crop(p, h, w).shape == (h, w, 3)
    assert {w % 8 for _, w in IC.WIDTH_GEOMS} == set(range(8))
    assert IC.apply_grid_facts(*IC.BIG_GEOMS[1])[3] != IC.apply_grid_facts(*IC.BIG_GEOMS[1])[2]
    H, W = IC.BATCH_FRAME_HW
    for n in IC.BATCH_SIZES:
        boxes = IC.batch_boxes(n)
        big = [i for i, b in enumerate(boxes) if b[2:] == IC.BIG_BOX_WH]
        assert len(boxes) == n and big == [0, (n - 3) // 2 + 1, n - 1]
        assert all(0 <= x and 0 <= y and x + w <= W and y + h <= H and w >= 1 and h >= 1 for x, y, w, h in boxes)
        assert all(w <= 224 and h <= 224 for i, (x, y, w, h) in enumerate(boxes) if i not in big)
        assert {(h, w) for x, y, w, h in boxes} >= set(IC.REFLECT_GEOMS)
        gx = IC.apply_grid_facts(300, 300, n)[0]
        assert gx == {17: 22, 64: 16, 256: 8}[n]                                    # all three rows of the cap table


def test_binding_passes_a_real_row_stride_for_one_row_images(pkg):
    """numpy calls a one-row view C-contiguous whatever its row stride (0 after broadcast_to); the binding hands
    strides[0] to the library, which refuses a stride below 3 w.  _as_bgr normalises it and keeps the pixels."""
    as_bgr = pkg._lib.Handle._as_bgr
    row = np.arange(27, dtype=np.uint8).reshape(9, 3)
    view = np.broadcast_to(row[None], (1, 9, 3))
    assert view.flags["C_CONTIGUOUS"] and view.strides[0] == 0
    for a in (view, IC.crop("hramp", 1, 9), IC.crop("hramp", 1, 1), np.zeros((40, 50, 3), np.uint8)[3:4, 5:20],
              np.zeros((40, 50, 3), np.uint8)[3:9, 5:20], np.zeros((6, 7, 3), np.uint8)):
        got = as_bgr(a)
        assert got.strides == (a.shape[1] * 3, 3, 1) and np.array_equal(got, a)

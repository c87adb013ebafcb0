"""GPU parity for the 8-bit image path through the C ABI: bit-exact against the integer oracle (resize, BGR<->Lab + CLAHE)
over the full gamut and at the geometries where the CLAHE kernels change path (imgproc_cases), the normalised network input
bit for bit against its float32 restatement (and 5e-4 against torch), all three rows of the batched CLAHE launch table,
1e-3 on crop logits."""
import numpy as np
import pytest
import torch

import imgproc_cases as IC
from oracle import b0_ref
from oracle import imgproc_ref as R

pytestmark = pytest.mark.gpu


def _frame(h, w, seed):
    rs = np.random.RandomState(seed)
    base = rs.randint(50, 200, (h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ell = ((xx - w // 2) / (w / 6.0)) ** 2 + ((yy - h // 2) / (h / 4.0)) ** 2 <= 1.0     # a flat "face"
    base[ell] = (180, 160, 140)
    return base


def _full_range(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _same_u8(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} bytes differ, max "
                             f"{np.abs(got.astype(int) - want).max()}, first at {bad[0].tolist()}")


def _same_f32(got, want, what=""):
    """equal as float32 words (np.array_equal on the values; neither side holds a NaN or a signed zero to confuse it)"""
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} floats differ, max |d| {np.abs(got - want).max():.3e}, "
                             f"first at {bad[0].tolist()}")


@pytest.fixture(scope="module")
def tables():
    return R.lab_tables()


# ---------------------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("h,w,dh,dw", [(1080, 1920, 256, 256), (480, 640, 300, 300), (120, 160, 256, 256),
                                         (300, 500, 300, 300), (256, 256, 256, 256), (31, 47, 64, 80),
                                         (37, 1, 64, 80), (1, 53, 64, 80), (2, 2, 64, 80)])
def test_resize_bit_exact(b0_handle, h, w, dh, dw):
    f = _frame(h, w, h + w)
    got = b0_handle.resize_bgr(f, dw, dh)
    want = R.resize_linear_u8(f, dw, dh)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{(got != want).sum()} differing bytes"


@pytest.mark.parametrize("h,w,dh,dw", [(480, 640, 300, 300), (31, 47, 64, 80)])
@pytest.mark.parametrize("kind", ["noise", "checker_0_255"])
def test_resize_full_range_bit_exact(b0_handle, kind, h, w, dh, dw):
    """0 and 255 next to each other: the largest horizontal sums and the clamp of the vertical pass"""
    f = _full_range(h, w, 5 * h + w) if kind == "noise" else IC.crop(kind, h, w)
    _same_u8(b0_handle.resize_bgr(f, dw, dh), R.resize_linear_u8(f, dw, dh), f"{kind} {h}x{w}->{dh}x{dw}")


def test_resize_strided_view(b0_handle):
    f = _frame(200, 300, 9)
    view = f[10:150, 20:260]                       # row stride != width*3
    assert np.array_equal(b0_handle.resize_bgr(np.ascontiguousarray(view), 64, 64),
                          R.resize_linear_u8(np.ascontiguousarray(view), 64, 64))


# ------------------------------------------------------------------------------------------------- BGR -> Lab -> CLAHE -> BGR
@pytest.mark.parametrize("h,w", [(224, 224), (160, 128), (83, 101), (37, 64), (480, 640)])
def test_preprocess_face_quality_bit_exact(b0_handle, h, w):
    f = _frame(h, w, 3 * h + w)
    got = b0_handle.preprocess_face_quality(f)
    want = R.preprocess_face_quality(f)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {got.size} bytes differ; max {np.abs(got.astype(int) - want).max()}"


@pytest.mark.parametrize("order", IC.LATTICE_ORDERS)
def test_face_quality_full_gamut_bit_exact(b0_handle, tables, order):
    """All 64^3 colours over the gamma knee, the cube-root table's linear branch, black, white, saturated primaries and
    grays: the kernels' 32-bit matrices, the clamp of the index into the inverse gamma table on both sides (82 k and
    41 k pixels of the lattice) and ab_to_xz evaluated on both of its branches (27 k on the linear one), against the
    oracle's 64-bit gathers.  (a and b stay within 42..226 and 20..223: no 8-bit colour reaches their clamps.)"""
    img = IC.lattice(order)
    _same_u8(b0_handle.preprocess_face_quality(img), R.preprocess_face_quality(img, tables), order)


@pytest.mark.parametrize("pattern", list(IC.PATTERNS))
@pytest.mark.parametrize("h,w", IC.GEOMETRIES)
def test_face_quality_structured_bit_exact(b0_handle, tables, h, w, pattern):
    """Constant crops (one bin clipped, the whole area redistributed by the residual / step rule), two-level
    checkerboards, a ramp and full-range noise at: sides whose CLAHE pad passes one reflection; tile areas below 128
    (clip limit 1); every w % 8; and crops of 64 apply blocks with and without a short last block."""
    f = IC.crop(pattern, h, w)
    _same_u8(b0_handle.preprocess_face_quality(f), R.preprocess_face_quality(f, tables), f"{pattern} {h}x{w}")


@pytest.mark.parametrize("h,w", IC.GEOMETRIES)
def test_structured_crops_inside_a_frame(b0_handle, tables, h, w):
    """The same crops as the interior of a larger noise frame (x = 7, y > 0, row stride 3 (w + 16)), all patterns of a
    geometry in one preprocess_crops call: the 224 x 224 network input equals crop_norm_f32 of the oracle's CLAHE'd crop
    bit for bit, so nothing outside a box reaches its histogram and the packed crops do not touch each other."""
    names = list(IC.PATTERNS)
    frame = _full_range(5 + len(names) * (h + 3), w + 16, 7 * h + w)
    boxes = []
    for k, p in enumerate(names):
        x, y = 7, 5 + k * (h + 3)
        frame[y:y + h, x:x + w] = IC.crop(p, h, w)
        boxes.append((x, y, w, h))
    got = b0_handle.preprocess_crops(frame, boxes, apply_clahe=True)
    for k, p in enumerate(names):
        want = IC.crop_norm_f32(R.preprocess_face_quality(IC.crop(p, h, w), tables))
        _same_f32(got[k], want, f"{p} {h}x{w}")


# ------------------------------------------------------------------------------------------------- crop -> network input
def test_preprocess_crops_matches_oracle(b0_handle):
    f = _frame(1080, 1920, 7)
    boxes = [(800, 300, 320, 440), (10, 20, 64, 64), (1700, 900, 220, 180), (0, 0, 1920, 1080), (500, 500, 79, 233)]
    for clahe in (False, True):
        got = b0_handle.preprocess_crops(f, boxes, apply_clahe=clahe)
        for i, (x, y, w, h) in enumerate(boxes):
            face = f[y:y + h, x:x + w]
            if clahe:
                face = R.preprocess_face_quality(face)
            want = R.crop_resize_normalize(face)
            err = np.abs(got[i] - want).max()
            # the kernel works in crop coordinates: a float32 source coordinate of up to 1920 (the full-frame box)
            # carries ~1e-4 of rounding, which the blend weight inherits and torch orders differently; values are
            # u8/255/std, so 5e-4 is a few ulps of that weight.  The exact statement is test_crop_norm_exact below.
            assert err <= 5e-4, (clahe, i, err)


@pytest.mark.parametrize("clahe", [False, True], ids=["from_frame", "from_clahe_scratch"])
@pytest.mark.parametrize("name", IC.NORM_CASE_NAMES)
def test_crop_norm_exact(b0_handle, tables, name, clahe):
    """crop_norm_kernel against its float32 restatement, bit for bit: one pixel, one row, one column, just below / at /
    just above the output size, a large ragged crop, and a crop ending on the frame's last row and column - read from the
    frame through its stride, and from the packed CLAHE scratch."""
    _, frame, box = [c for c in IC.norm_cases() if c[0] == name][0]
    face = np.ascontiguousarray(IC.cut(frame, box))
    if clahe:
        face = R.preprocess_face_quality(face, tables)
    got = b0_handle.preprocess_crops(frame, [box], apply_clahe=clahe)
    _same_f32(got[0], IC.crop_norm_f32(face), name)


# ------------------------------------------------------------------------------------------------- batched CLAHE launch shapes
@pytest.fixture(scope="module")
def big_handle(pkg, seeded_sd, ssd_sd):
    h = pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, ssd_sd), device=0, max_batch=256)
    yield h
    h.close()


@pytest.fixture(scope="module")
def batch_refs(tables):
    """box -> expected network input; the three batch sizes share most of their boxes"""
    frame = IC.batch_frame()
    cache = {}

    def ref(box):
        if box not in cache:
            cache[box] = IC.crop_norm_f32(R.preprocess_face_quality(np.ascontiguousarray(IC.cut(frame, box)), tables))
        return cache[box]
    return frame, ref


@pytest.mark.parametrize("n", IC.BATCH_SIZES)
def test_batched_clahe_launch_shapes(big_handle, batch_refs, n):
    """launch_clahe sizes the apply grid by the call's largest crop and caps it by n: 22 blocks per crop at n = 17, 16 at
    n = 64, 8 at n = 256 (a 300 x 300 crop first, in the middle and last sets the size; the other crops, at most
    224 x 224 and many of a few pixels, then own fewer pixel groups than blocks).  Every crop's network input equals
    crop_norm_f32 of the oracle's CLAHE'd crop bit for bit: at up-scaling every source byte has weight >= 1/4 in some
    output, so one wrong level cannot hide; the down-scaled 300 x 300 crop is also checked byte by byte on its own."""
    frame, ref = batch_refs
    boxes = IC.batch_boxes(n)
    got = big_handle.preprocess_crops(frame, boxes, apply_clahe=True)
    assert got.shape == (n, 3, 224, 224)
    bad = [(i, boxes[i]) for i in range(n) if not np.array_equal(got[i], ref(boxes[i]))]
    assert not bad, f"{len(bad)} of {n} crops differ: {bad[:8]}"


def test_batched_big_crop_alone(big_handle, tables):
    big = np.ascontiguousarray(IC.cut(IC.batch_frame(), IC.batch_boxes(17)[0]))
    assert big.shape[:2] == IC.BIG_BOX_WH[::-1]
    _same_u8(big_handle.preprocess_face_quality(big), R.preprocess_face_quality(big, tables), "300x300")


# ------------------------------------------------------------------------------------------------- logits, arguments
def test_classify_crops_matches_oracle(pkg, b0_handle, seeded_sd):
    f = _frame(720, 1280, 11)
    boxes = [(500, 200, 300, 380), (30, 40, 120, 90), (900, 400, 224, 224)]
    got = b0_handle.classify_crops(f, boxes, apply_clahe=True)
    x = np.stack([R.crop_resize_normalize(R.preprocess_face_quality(f[y:y + h, x:x + w])) for (x, y, w, h) in boxes])
    want = b0_ref.forward(pkg.weights.to_torch(seeded_sd), torch.from_numpy(x)).numpy()
    assert np.abs(got - want).max() <= 1e-3, (got.ravel(), want.ravel())


def test_bad_boxes_fail_loudly(pkg, b0_handle):
    f = _frame(100, 100, 1)
    with pytest.raises(pkg._lib.DfdError):
        b0_handle.preprocess_crops(f, [(90, 90, 20, 20)])           # leaves the frame
    with pytest.raises(pkg._lib.DfdError):
        b0_handle.preprocess_crops(f, [(0, 0, 0, 10)])


def test_bad_arguments_fail_loudly(pkg, b0_handle):
    """negative x, negative y, more boxes than the handle holds (the capacity status) and no boxes at all (the binding
    refuses an empty list itself, so that call goes to the C entry directly): each a DfdError, none a launch"""
    E = pkg._lib.DfdError
    f = _frame(100, 100, 2)
    for clahe in (False, True):
        with pytest.raises(E) as e:
            b0_handle.preprocess_crops(f, [(-1, 10, 20, 20)], apply_clahe=clahe)
        assert e.value.code == -1
        with pytest.raises(E) as e:
            b0_handle.preprocess_crops(f, [(10, -1, 20, 20)], apply_clahe=clahe)
        assert e.value.code == -1
        with pytest.raises(E) as e:
            b0_handle.preprocess_crops(f, [(1, 1, 8, 8)] * (b0_handle.max_batch + 1), apply_clahe=clahe)
        assert e.value.code == -6                                     # DFD_ERR_CAPACITY
        boxes = np.zeros((1, 4), np.int32)
        out = np.empty((1, 3, 224, 224), np.float32)
        ptr = pkg._lib._ptr
        with pytest.raises(E) as e:
            b0_handle._check(b0_handle._lib.dfd_preprocess_crops(b0_handle._p, ptr(f), 100, 100, 300, ptr(boxes), 0,
                                                                 int(clahe), ptr(out)))
        assert e.value.code == -1
    # the handle still works
    good = b0_handle.preprocess_crops(f, [(10, 10, 20, 20)], apply_clahe=False)
    _same_f32(good[0], IC.crop_norm_f32(np.ascontiguousarray(f[10:30, 10:30])), "after the refused calls")

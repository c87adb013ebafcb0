"""GPU: the any-size frequency-domain kernels (csrc/freq_domain.hip) - the window DFT launch by launch against float64
at the project's bars, the two sums against the device's own magnitudes and against the reference, the verdict of
DeepfakeDetector.analyze_frequency_domain, one call with every window as a box, and the features at sizes other than 224.

Measured on an MI355X (worst over the cases, as printed by the tests): window rows 1.61x rms / 2.13x
maximum of the yardstick's error, window spectrum 1.63x / 2.17x, feature spectrum 1.88x / 3.19x, feature dct 1.39x / 3.05x
(bars 4x / 8x); sums equal to the float64 sums of the device's magnitudes to the last bit; high / total at most 0.07 of
their bar against the reference; features at most 1.1e-4 maximum and 7.4e-6 mean from float64 (size 1024; bars 2e-3, 1e-4).

The issue asks for one call with all windows as boxes of one 4200 x 320 frame.  No frame of that size holds both the
2 x 4096 window (w = 4096) and the 4095 x 3 window (h = 4095): the test runs the frame in both orientations, 320 x 4200
with every window that fits it (all but 4095 x 3) and 4200 x 320 (all but 2 x 4096)."""
import numpy as np
import pytest

import freq_domain_oracle as O

pytestmark = pytest.mark.gpu

CASES = list(O.cases())
_TAPS = {}


def taps(handle, name):
    """the device's buffers of a case, fetched once: rows, spectrum, mag, sums"""
    if name not in _TAPS:
        g = O.cases()[name]
        _TAPS[name] = {k: handle.frequency_domain_tap(g, k) for k in ("rows", "spectrum", "mag", "sums")}
    return _TAPS[name]


@pytest.mark.parametrize("name", CASES)
def test_rows_and_spectrum_meet_the_yardstick_bars(b0_handle, name):
    g = O.cases()[name]
    h, w = g.shape
    t, r = taps(b0_handle, name), O.case_reference(name)
    assert t["rows"].shape == t["spectrum"].shape == t["mag"].shape == (w, h)
    rr = O.fft_ratios(t["rows"], r["rows64"], r["rows_yard"])
    rs = O.fft_ratios(t["spectrum"], r["spec64"], r["spec_yard"])
    print(f"{name}: rows rms x{rr[0]:.3f} max x{rr[1]:.3f} | spectrum rms x{rs[0]:.3f} max x{rs[1]:.3f} "
          f"(yardstick rms {O.fft_error(r['spec_yard'], r['spec64'])[0]:.3e})")
    assert O.meets_bar(rr), ("rows", rr)
    assert O.meets_bar(rs), ("spectrum", rs)
    mag = np.hypot(t["spectrum"].real.astype(np.float64), t["spectrum"].imag.astype(np.float64))
    assert np.abs(t["mag"] - mag).max() <= 2.0 ** -22 * max(float(mag.max()), 1e-30)      # the magnitudes are those of the stored spectrum


@pytest.mark.parametrize("name", CASES)
def test_sums_are_the_float64_sums_of_the_magnitudes(b0_handle, name):
    g = O.cases()[name]
    h, w = g.shape
    t = taps(b0_handle, name)
    high, total = O.sums_of_mag(t["mag"], h, w)
    rtol = 4 * h * w * O.EPS64
    print(f"{name}: high {t['sums'][0]!r} vs {high!r}, total {t['sums'][1]!r} vs {total!r}")
    assert abs(t["sums"][0] - high) <= rtol * high and abs(t["sums"][1] - total) <= rtol * total
    if name.startswith("constant"):
        assert t["sums"][0] == 0.0                                # all energy in bin 0: exact through the centring
    assert np.array_equal(b0_handle.frequency_domain(g)[0], t["sums"])      # the product call: the same launches


@pytest.mark.parametrize("name", CASES)
def test_sums_against_the_reference(b0_handle, name):
    """sum ||X'| - |X|| <= h w rms(X' - X), which the tap test bounds by 4 e_rms, plus hypotf's rounding"""
    g = O.cases()[name]
    h, w = g.shape
    t, r = taps(b0_handle, name), O.case_reference(name)
    e_rms = O.fft_error(r["spec_yard"], r["spec64"])[0]
    bar = h * w * 4 * e_rms + 2.0 ** -22 * r["ref"]["total"]
    dh, dt = abs(t["sums"][0] - r["ref"]["high"]), abs(t["sums"][1] - r["ref"]["total"])
    print(f"{name}: |high - ref| {dh:.3e} |total - ref| {dt:.3e} bar {bar:.3e}")
    assert dh <= bar and dt <= bar


@pytest.fixture(scope="module")
def detector(pkg, b0_handle):
    return pkg.deepfake_detection.DeepfakeDetector(use_tta=False, num_tta_augmentations=1, handle=b0_handle)


@pytest.mark.parametrize("name", CASES)
def test_verdict_is_the_references(detector, name):
    g = O.cases()[name]
    want = O.case_reference(name)["ref"]["verdict"]
    assert detector.analyze_frequency_domain(O.bgr_of(g)) == want
    assert detector.analyze_frequency_domain_boxes(O.bgr_of(g), [(0, 0, g.shape[1], g.shape[0])]) == [want]


def test_verdict_edges(detector):
    assert detector.analyze_frequency_domain(O.cases()["gaussian_120x100"]) == 0.0        # 2-D input: the reference's except
    assert detector.analyze_frequency_domain(np.zeros((0, 5, 3), np.uint8)) == 0.0
    assert detector.analyze_frequency_domain(np.zeros((5, 0, 3), np.uint8)) == 0.0
    assert detector.analyze_frequency_domain(np.zeros((4, 4, 4), np.uint8)) == 0.0
    with pytest.raises(ValueError):
        detector.analyze_frequency_domain(np.zeros((2, 4097, 3), np.uint8))
    with pytest.raises(ValueError):
        detector.analyze_frequency_domain(np.zeros((8, 8, 3), np.float32))
    assert detector.analyze_frequency_domain_boxes(np.zeros((8, 8, 3), np.uint8), []) == []
    assert detector.analyze_frequency_domain(np.zeros((8, 8, 3), np.uint8)) == 0.15       # 0 / 1e-10 < 0.15, as the reference


def test_library_refusals(pkg, b0_handle):
    E = pkg._lib.DfdError
    with pytest.raises(E) as e:
        b0_handle.frequency_domain(np.zeros((2, 4097), np.uint8))
    assert e.value.code == -7 and "4096" in str(e.value)
    with pytest.raises(E) as e:
        b0_handle.frequency_domain_tap(np.zeros((4097, 2), np.uint8), "sums")
    assert e.value.code == -7
    img = np.zeros((20, 30, 3), np.uint8)
    for box in ((0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (26, 0, 5, 5), (0, 16, 5, 5), (0, 0, 31, 20), (0, 0, 30, 21)):
        with pytest.raises(E) as e:
            b0_handle.frequency_domain(img, [(0, 0, 30, 20), box])
        assert e.value.code == -1, box
    for size in (0, 1, 127, 1026, -2):
        with pytest.raises(E) as e:
            b0_handle.frequency_features(img, size)
        assert e.value.code == -1, size
    with pytest.raises(E) as e:
        b0_handle.frequency_features_tap(img, 16, "nothing")
    assert e.value.code == -1


def _boxes(H, W, rs):
    """(x, y, w, h) of every window shape that fits an H x W frame: the first four in the frame's corners (every edge
    touched), one overlapping its predecessor by all but a pixel, the rest anywhere"""
    shapes = [(h, w) for h, w in O.SHAPES if h <= H and w <= W] + [(120, 100), (256, 256), (48, 64)]
    out = []
    for i, (h, w) in enumerate(shapes):
        x, y = [(0, 0), (W - w, 0), (0, H - h), (W - w, H - h)][i] if i < 4 else (rs.randint(0, W - w + 1), rs.randint(0, H - h + 1))
        out.append((x, y, w, h))
    x, y, w, h = out[-1]
    out.append((min(x + 1, W - w), min(y + 1, H - h), w, h))
    big = max(out, key=lambda b: b[2] * b[3])
    out += [(0, 0, W, 1), (0, H - 1, W, 1), (0, 0, 1, H), (W - 1, 0, 1, H)] if max(H, W) <= O.MAX_SIDE else \
           [(0, 0, min(W, 4096), 1), (max(W - 4096, 0), H - 1, min(W, 4096), 1), (0, 0, 1, min(H, 4096)), (W - 1, max(H - 4096, 0), 1, min(H, 4096))]
    return out + [big]


@pytest.mark.parametrize("H,W", [(320, 4200), (4200, 320)])
def test_one_call_with_every_window_as_a_box(pkg, b0_handle, H, W):
    rs = np.random.RandomState(H)
    frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    boxes = _boxes(H, W, rs)
    assert {(b[3], b[2]) for b in boxes} >= {s for s in O.SHAPES if s[0] <= H and s[1] <= W} and len(boxes) >= 20
    got = b0_handle.frequency_domain(frame, boxes)
    assert got.shape == (len(boxes), 2) and got.dtype == np.float64
    for (x, y, w, h), row in zip(boxes, got):
        alone = b0_handle.frequency_domain(frame[y:y + h, x:x + w])
        assert np.array_equal(alone[0], row), (x, y, w, h, alone, row)
    assert np.array_equal(b0_handle.frequency_domain(frame, boxes), got)            # the same call again: the same bits
    buf = pkg._lib.DeviceBuffer(b0_handle, frame.nbytes).upload(frame)
    try:
        dev = b0_handle.frequency_domain_device(buf.ptr, H, W, frame.strides[0], 3, boxes)
        assert np.array_equal(dev, got)
        assert np.array_equal(b0_handle.frequency_domain_device(buf.ptr, H, W, frame.strides[0], 3, boxes[:3]), got[:3])
        for bad in ((W - 15, 0, 16, 16), (0, H - 15, 16, 16), (-1, 0, 16, 16), (0, -1, 16, 16)):      # one pixel outside
            for call in (lambda b: b0_handle.frequency_domain(frame, boxes[:2] + [b]),
                         lambda b: b0_handle.frequency_domain_device(buf.ptr, H, W, frame.strides[0], 3, boxes[:2] + [b])):
                with pytest.raises(pkg._lib.DfdError) as e:
                    call(bad)
                assert e.value.code == -1, bad
    finally:
        buf.free()
    # a gray frame gives the bits of its BGR source
    gray = np.ascontiguousarray(frame[..., 1])
    want = b0_handle.frequency_domain(O.bgr_of(gray), boxes[:6])
    assert np.array_equal(b0_handle.frequency_domain(gray, boxes[:6]), want)
    # launch sets of one window each (a work budget of one byte), and of a few: the same bits
    for budget in (1, 300000):
        b0_handle.set_option("forensic_chunk_bytes", budget)
        try:
            assert np.array_equal(b0_handle.frequency_domain(frame, boxes), got), budget
        finally:
            b0_handle.set_option("forensic_chunk_bytes", 0)               # the default


# ------------------------------------------------------------------------------------------------ features
def _feature_check(handle, img, size, tag):
    f64, spec64, dct64 = O.features_float64(img, size)
    fy, specy, dcty = O.features_yardstick(img, size)
    gray = handle.frequency_features_tap(img, size, "gray")
    assert np.array_equal(gray, O.feature_gray(img, size)), "gray"
    rs = O.fft_ratios(handle.frequency_features_tap(img, size, "spectrum"), spec64, specy)
    rd = O.fft_ratios(handle.frequency_features_tap(img, size, "dct"), dct64, dcty)
    got = handle.frequency_features(img, size, sized=True)
    assert got.shape == (2, size, size) and got.dtype == np.float32
    d = np.abs(got.astype(np.float64) - f64)
    dy = np.abs(fy.astype(np.float64) - f64)
    print(f"size {size} {tag}: spectrum rms x{rs[0]:.3f} max x{rs[1]:.3f} | dct rms x{rd[0]:.3f} max x{rd[1]:.3f} | "
          f"features max {d.max():.3e} mean {d.mean():.3e} (yardstick max {dy.max():.3e} mean {dy.mean():.3e})")
    assert O.meets_bar(rs), ("spectrum", rs)
    assert O.meets_bar(rd), ("dct", rd)
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert d.max() <= O.FEATURE_MAX and d.mean() <= O.FEATURE_MEAN, (float(d.max()), float(d.mean()))
    return got


@pytest.mark.parametrize("size", O.FEATURE_SIZES)
def test_features_at_other_sizes(b0_handle, size):
    for tag, img in O.feature_images().items():
        _feature_check(b0_handle, img, size, tag)


def test_features_at_the_largest_size(b0_handle):
    _feature_check(b0_handle, O.feature_images()["face"], O.FEATURE_SIZE_MAX, "face")


def test_features_224_through_the_sized_entry(pkg, b0_handle):
    for tag, img in O.feature_images().items():
        got = _feature_check(b0_handle, img, 224, tag)
        old = b0_handle.frequency_features(img)                                       # the 224 kernels: same bars, not the same bits
        assert np.abs(got - old).max() <= 2 * O.FEATURE_MAX


def test_features_properties(pkg, b0_handle, monkeypatch):
    img = O.feature_images()["rand300"]
    f = pkg.model.compute_frequency_features
    for size in (30, 258):
        z = f(np.zeros((200, 200, 3), np.uint8), size=size, any_size=True, handle=b0_handle)
        assert z.shape == (2, size, size) and not z.any()                             # the flat image: zeros in both channels
        a = f(img, size=size, any_size=True, handle=b0_handle)
        assert np.array_equal(a, f(img, size=size, any_size=True, handle=b0_handle))  # deterministic
        from oracle import imgproc_ref as I
        assert np.array_equal(f(I.bgr2gray_u8(img), size=size, any_size=True, handle=b0_handle), a)    # a gray input: its BGR source's bits
    monkeypatch.delenv("DFD_FREQ_ANY_SIZE", raising=False)
    with pytest.raises(ValueError):
        f(img, size=30, handle=b0_handle)
    monkeypatch.setenv("DFD_FREQ_ANY_SIZE", "1")
    assert np.array_equal(f(img, size=30, handle=b0_handle), f(img, size=30, any_size=True, handle=b0_handle))
    assert np.array_equal(f(img, size=224, handle=b0_handle), b0_handle.frequency_features(img))       # 224 stays on its kernels

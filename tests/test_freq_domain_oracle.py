"""CPU: the helper of the frequency-domain GPU tests (tests/freq_domain_oracle.py) against closed forms, the mask in
unshifted signed indices against the reference's slice, and the condition the verdict test rests on: no case of the
table has a float64 ratio within 1 % of the 0.15 threshold."""
import numpy as np
import pytest

import freq_domain_oracle as O


@pytest.mark.parametrize("h,w", [(4, 4), (8, 12), (48, 64), (31, 33), (120, 100), (17, 4)])
def test_constant_window_has_all_energy_in_bin_0(h, w):
    r = O.reference(O.constant_window(h, w, 137))
    assert O.mask_size(h, w) > 0
    assert r["total"] == pytest.approx(137.0 * h * w, rel=1e-12)
    assert r["high"] <= 1e-9 * r["total"]                         # numpy's FFT of a constant: zero up to its rounding
    assert r["verdict"] == 0.15


@pytest.mark.parametrize("h,w,y,x", [(31, 33, 5, 7), (16, 16, 0, 0), (48, 64, 47, 63), (9, 40, 3, 11)])
def test_lit_pixel_ratio(h, w, y, x):
    r = O.reference(O.lit_pixel(h, w, y, x))
    m = O.mask_size(h, w)
    assert r["total"] == pytest.approx(255.0 * h * w, rel=1e-12)   # |X| is 255 on every bin
    assert r["ratio"] == pytest.approx(1.0 - (2 * m) ** 2 / (h * w), rel=1e-12)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (2, 2), (3, 5), (3, 300), (200, 2)])
def test_sides_below_4_mask_nothing(h, w):
    g = O.random_window(h, w)
    g[0, 0] = 200                                                 # total > 0
    r = O.reference(g)
    assert O.mask_size(h, w) == 0 and not O.mask_unshifted(h, w).any()
    assert r["high"] == r["total"] and r["ratio"] == pytest.approx(1.0, rel=1e-12) and r["verdict"] == 0.0


@pytest.mark.parametrize("h,w", [(4, 4), (5, 5), (8, 9), (9, 8), (15, 17), (16, 16), (17, 16), (31, 33), (97, 113), (12, 300),
                                 (257, 255), (300, 20), (4, 4096), (4095, 5)] + list(O.SHAPES))
def test_mask_in_signed_indices_is_the_reference_slice(h, w):
    a, b = O.mask_unshifted(h, w), O.mask_reference(h, w)
    assert a.shape == b.shape == (h, w) and np.array_equal(a, b)
    m = O.mask_size(h, w)
    assert a.sum() == (2 * m) ** 2                                # half-open: -m is masked, +m is not
    if m > 0:
        sy, sx = O.signed(h), O.signed(w)
        assert a[sy == -m][:, sx == -m].all() and not a[sy == m].any() and not a[:, sx == m].any()


def test_sums_of_mag_uses_the_same_mask():
    g = O.natural_window(40, 28)
    spec = np.fft.fft2(g.astype(np.float64))
    high, total = O.sums_of_mag(np.abs(spec).T, 40, 28)
    r = O.reference(g)
    assert high == pytest.approx(r["high"], rel=1e-12) and total == pytest.approx(r["total"], rel=1e-12)


def test_float64_layouts():
    g = O.random_window(6, 10)
    rows, spec = O.fft_float64(g)
    assert rows.shape == spec.shape == (10, 6)
    k, row = 3, 4
    want = sum(g[row, n] * np.exp(-2j * np.pi * k * n / 10) for n in range(10))
    assert abs(rows[k, row] - want) < 1e-9
    ry, sy = O.fft_yardstick(g)
    assert O.fft_ratios(ry, rows, ry) == (1.0, 1.0) and O.fft_error(sy, spec)[1] < 1e-2
    assert O.fft_ratios(rows, rows, ry) == (0.0, 0.0)
    c = O.constant_window(4, 4, 9)
    assert O.fft_ratios(O.fft_yardstick(c)[1] + 1e-3, O.fft_float64(c)[1], O.fft_yardstick(c)[1])[0] == np.inf   # zero demands zero


def test_feature_reference_is_float64_and_close_to_the_oracle():
    from oracle import imgproc_ref as I

    img = O.feature_images()["natural224"]
    f, spec, d = O.features_float64(img, 64)
    assert f.dtype == np.float64 and spec.dtype == np.complex128 and d.dtype == np.float64
    assert f.shape == (2, 64, 64) and spec.shape == (64, 64)
    assert np.abs(f - I.compute_frequency_features(img, 64)).max() < 2e-3
    fy, sy, dy = O.features_yardstick(img, 64)
    assert np.abs(fy - f).max() < 2e-3 and O.fft_error(sy, spec)[0] > 0
    z, _, _ = O.features_float64(np.zeros((50, 50, 3), np.uint8), 16)
    assert not z.any()


def test_every_case_is_away_from_the_threshold():
    seen = set()
    for name, g in O.cases().items():
        r = O.case_reference(name)["ref"]
        assert abs(r["ratio"] / O.THRESHOLD - 1.0) > 0.01, (name, r["ratio"])
        seen.add(r["verdict"])
    assert seen == {0.0, 0.15}                                    # both verdicts occur
    assert {g.shape for n, g in O.cases().items() if n.startswith("random_")} == set(O.SHAPES)
    ref = lambda n: O.case_reference(n)["ref"]
    assert ref("gaussian_120x100")["verdict"] == 0.15 and ref("constant_48x64")["verdict"] == 0.15
    assert ref("gradient_256x256")["verdict"] == 0.0 and 0.4 < ref("natural_160x120")["ratio"] < 0.6

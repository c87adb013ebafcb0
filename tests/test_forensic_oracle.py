"""CPU: the per-stage forensic references (tests/forensic_oracle.py) agree with oracle/forensics_ref.py, the FFT bit
mirror meets the bar the device is held to, and each bar rejects the mutant it is meant to catch."""
from fractions import Fraction

import numpy as np
import pytest

import forensic_oracle as O
from oracle.forensics_ref import ForensicsRef


@pytest.fixture(scope="module")
def fixtures():
    return O.fixture_frames()


@pytest.fixture(scope="module")
def fft_in():
    return O.fft_inputs()


@pytest.fixture(scope="module")
def hyst_maps():
    return O.hysteresis_maps()


def test_stage_references_chain_to_forensics_ref(fixtures):
    """statistics assembled from the stage references = ForensicsRef's on the 8 fixtures (ForensicsRef keeps some of
    them in float32, hence 1e-5 there; the integer-derived ones and the float64 band means to 1e-12)"""
    low, mid, high = O.band_masks()
    for name, bgr in fixtures.items():
        ref = ForensicsRef()
        ref.analyze(bgr)
        st = ref.stats
        g = O.gray(bgr)
        gr = O.grad(g)
        assert O.edges(O.labels(gr)).sum() / 65536 == st["edge_density"], name
        lp = O.lap_part(g).sum(0)
        lap_var = float(Fraction(int(lp[1]), 65536) - Fraction(int(lp[0]), 65536) ** 2)
        assert lap_var == pytest.approx(st["lap_var"], rel=1e-12, abs=1e-12), name
        ela = O.ela_block_sums(bgr) / 1024.0
        assert ela.mean() == pytest.approx(st["ela_mean"], rel=1e-6), name
        assert ela.std() / (ela.mean() + 1e-10) == pytest.approx(st["ela_cv"], rel=1e-5), name
        ns = O.noise_stds(g)
        assert ns.mean() == pytest.approx(st["noise_mean"], rel=1e-5, abs=1e-12), name
        part, bits = O.hsv_part(bgr)
        s1, s2, v1, v2 = (int(x) for x in part.sum(0))
        assert np.sqrt(float(Fraction(s2, 65536) - Fraction(s1, 65536) ** 2)) == pytest.approx(st["sat_std"], rel=1e-5, abs=1e-9), name
        assert np.sqrt(float(Fraction(v2, 65536) - Fraction(v1, 65536) ** 2)) == pytest.approx(st["val_std"], rel=1e-5, abs=1e-9), name
        assert sum(bin(int(b)).count("1") for b in bits) == st["unique_hues"], name
        mag = np.log1p(np.abs(O.fft_float64(g)[1].T))
        for k, m in (("freq_low", low), ("freq_mid", mid), ("freq_high", high)):
            assert mag[m].mean() == pytest.approx(st[k], rel=1e-12), (name, k)


def test_band_masks_are_the_kernels_integer_test():
    """the sqrt-distance masks of the reference = the kernel's d2 <= r^2 on signed bin indices"""
    s = np.where(np.arange(256) < 128, np.arange(256), np.arange(256) - 256)
    d2 = s[:, None] ** 2 + s[None, :] ** 2
    low, mid, high = O.band_masks()
    assert (low == (d2 <= 32 * 32)).all() and (mid == ((d2 > 32 * 32) & (d2 <= 64 * 64))).all()
    assert (high == ((d2 > 64 * 64) & (d2 <= 128 * 128))).all()


def test_fft_mirror_meets_the_device_bar(fft_in):
    """On every FFT input of the GPU test the mirror is within 4x rms / 8x max of the fp32 yardstick's error against
    float64, and exact on the constant, origin-impulse and checkerboard frames."""
    worst = [0.0, 0.0]
    for name, g in fft_in.items():
        mir, ref, yard = O.fft_mirror(g), O.fft_float64(g), O.fft_yardstick(g)
        for which in (0, 1):
            r, m = O.fft_ratios(mir[which], ref[which], yard[which])
            assert r <= O.FFT_RMS_X and m <= O.FFT_MAX_X, (name, which, r, m)
            worst = [max(worst[0], r), max(worst[1], m)]
            if name in O.FFT_EXACT:
                assert O.fft_error(mir[which], ref[which]) == (0.0, 0.0), (name, which)
    print(f"mirror vs yardstick, worst over {len(fft_in)} inputs: rms {worst[0]:.2f}x, max {worst[1]:.2f}x")


NATURAL = ("determinism", "noisy", "face_vga", "natural_720p", "gray_random")


def test_fft_mutant_twiddles_by_recurrence(fft_in):
    """It passes the rms bar on every frame (2.4-2.8x) and the max bar on most (2.2-5.1x); the max bar rejects it on the
    smooth natural frame (10.8x), the bit mirror on every frame."""
    tw = O.twiddles_recurrence()
    over_max = set()
    for name in NATURAL:
        g = fft_in[name]
        mut, mir, ref, yard = O.fft_mirror(g, tw)[1], O.fft_mirror(g)[1], O.fft_float64(g)[1], O.fft_yardstick(g)[1]
        assert not O.bits_equal(mut, mir), name
        r, m = O.fft_ratios(mut, ref, yard)
        print(f"recurrence twiddles on {name}: rms {r:.1f}x, max {m:.1f}x")
        assert r <= O.FFT_RMS_X, name
        if m > O.FFT_MAX_X:
            over_max.add(name)
    assert "natural_720p" in over_max


def test_fft_mutant_one_twiddle_off_by_1e_6(fft_in):
    """within the float64 bars: only the bit mirror catches it"""
    tw = O.twiddles()
    tw[37] = np.complex64(tw[37] * (1 + 1e-6))
    assert tw[37] != O.twiddles()[37]
    for name in NATURAL:
        g = fft_in[name]
        mut, mir = O.fft_mirror(g, tw), O.fft_mirror(g)
        assert not O.bits_equal(mut[0], mir[0]) and not O.bits_equal(mut[1], mir[1]), name
        assert O.fft_meets_bar(mut[1], O.fft_float64(g)[1], O.fft_yardstick(g)[1]), name     # the reason the mirror exists


def test_fft_mutant_swapped_bins(fft_in):
    for name in NATURAL:
        g = fft_in[name]
        mir = O.fft_mirror(g)[1]
        mut = mir.copy()
        mut[11, 5], mut[11, 251] = mir[11, 251], mir[11, 5]
        assert not O.bits_equal(mut, mir)
        assert not O.fft_meets_bar(mut, O.fft_float64(g)[1], O.fft_yardstick(g)[1]), name


def test_bitboard_restatement_equals_flood_fill_and_needs_its_carries(hyst_maps):
    """The kernel's sweep scheme, restated on numpy words, reaches the stack flood fill's set on every adversarial map
    and on random maps; without the carry bits between words it fails every map whose chain crosses a word border."""
    crossing = 0
    word = lambda lab, v: set(np.nonzero(lab == v)[1] // 64)
    for name, lab in hyst_maps.items():
        want = O.edges(lab)
        assert (O.hysteresis_bitboard(lab) == want).all(), name
        wrong = not (O.hysteresis_bitboard(lab, carry=False) == want).all()
        if name.startswith(("row_", "diag_", "anti_", "spiral", "serpentine", "border_ring")):
            assert wrong, name
        if name.startswith("touch_"):
            assert wrong == (word(lab, 0) != word(lab, 2)), name     # exactly the maps whose weak pixels lie across the border
            crossing += wrong
    assert crossing >= 4 * 3 * 5 - 6, crossing                         # 3 directions per side, less those off the image
    for lab in O.random_maps(6, seed=1):
        assert (O.hysteresis_bitboard(lab) == O.edges(lab)).all()


def test_touch_maps_cross_the_border_in_all_eight_directions(hyst_maps):
    """(d): for each border and row, the strong pixel's weak neighbour lies in the other word in 3 directions per side"""
    across = 0
    for name, lab in hyst_maps.items():
        if not name.startswith("touch_"):
            continue
        (sy,), (sx,) = np.nonzero(lab == 2)
        wy, wx = np.nonzero(lab == 0)
        across += any(x // 64 != sx // 64 for x in wx)
        assert O.edges(lab).sum() == 1 + len(wy), name          # the whole chain is reached
    assert across >= 4 * 3 * 5


def test_nms_fields_take_every_branch_and_reject_the_tie_mutant():
    total = dict.fromkeys(O.NMS_BRANCHES, 0)
    differ = 0
    mags = set()
    for f in O.nms_fields():
        br = {}
        lab = O.labels(f, branches=br)
        assert br["at_tg22"] == 0 and br["at_tg67"] == 0        # unreachable above `low` (see NMS_BRANCHES)
        for k in total:
            total[k] += br[k]
        differ += int((O.labels(f, ties_pass=True) != lab).sum())
        assert set(np.unique(lab)) <= {0, 1, 2}
        mags |= set(np.unique(np.abs(f.astype(np.int64)).sum(-1)))
    print(total, differ)
    assert all(v >= 100 for v in total.values()), total
    assert {50, 51, 150, 151, 2040} <= mags
    assert differ >= 1000


def test_sobel_ramp_sits_on_the_thresholds():
    m = np.abs(O.grad(O.sobel_ramp()).astype(np.int64)).sum(-1)
    for v in (50, 52, 150, 152):
        assert (m == v).sum() >= 100, v
    assert (m % 2 == 0).all()
    rs = np.random.RandomState(0)
    assert (np.abs(O.grad(rs.randint(0, 256, (256, 256)).astype(np.uint8)).astype(np.int64)).sum(-1) % 2 == 0).all()


def test_noise_bar_rejects_reflect_borders(fixtures):
    for name in ("determinism", "face_vga", "natural_720p"):
        g = O.gray(fixtures[name])
        want, mut = O.noise_stds(g), O.noise_stds(g, O.blur_reflect)
        rel = np.abs(mut - want) / want
        border = np.array([(b // 8 in (0, 7)) or (b % 8 in (0, 7)) for b in range(64)])
        assert (rel[border] > 1e6 * O.NOISE_RTOL).all() and (rel[~border] == 0).all(), name


def test_jpeg_planes_reject_a_wrong_downsample_bias(fixtures):
    for name in ("determinism", "natural_720p"):
        bgr = fixtures[name]
        want, mut = O.jpeg_planes(bgr), O.jpeg_planes(bgr, bias=(2, 2))
        assert (want[0] == mut[0]).all()
        assert (want[1] != mut[1]).any() and (want[2] != mut[2]).any(), name
    bgr = fixtures["natural_720p"]
    assert (O.ela_block_sums(bgr, O.jpeg_planes(bgr)) == O.ela_block_sums(bgr)).all()


def test_logmag_yardstick_is_about_an_ulp(fft_in):
    spec = O.fft_mirror(fft_in["natural_720p"])[1]
    got, yard = O.logmag_ulps(np.log1p(np.hypot(spec.real, spec.imag)), spec)
    assert got == yard and 0.4 < yard < 4.0, yard

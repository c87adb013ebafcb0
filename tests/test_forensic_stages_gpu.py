"""GPU: every buffer of the forensic kernel chain (dfd_forensic_tap) against the per-stage references of
tests/forensic_oracle.py - exact where the stage is integer arithmetic, bit-equal to the fp32 mirror for the FFT, derived
bars elsewhere - on the 8 fixture frames, edge frames and injected gradients / label maps that no image produces."""
import numpy as np
import pytest

import forensic_oracle as O

pytestmark = pytest.mark.gpu

FAST_TAPS = ("rs", "gray", "fft_tmp", "spectrum", "logmag", "fft_part", "grad", "lap_part", "map", "edges", "edge_count", "stats")
FULL_TAPS = FAST_TAPS + ("jy", "jcb", "jcr", "stats_ela", "stats_noise", "hsv_part", "hue_bits")
ST_LOW, ST_MID, ST_HIGH, ST_MID_STD, ST_LAP_VAR, ST_EDGES, ST_SAT, ST_VAL, ST_HUES = range(9)


@pytest.fixture(scope="module")
def frames():
    return {**O.fixture_frames(), **O.edge_frames()}


@pytest.fixture(scope="module")
def taps(b0_handle, frames):
    """every tap of every frame, from one 26-frame batch per tap"""
    stack = np.stack(list(frames.values()))
    got = {t: b0_handle.forensic_tap(stack, t) for t in FULL_TAPS}
    return {name: {t: got[t][i] for t in FULL_TAPS} for i, name in enumerate(frames)}


@pytest.fixture(scope="module")
def twiddle(b0_handle):
    return b0_handle.forensic_tap(np.zeros((1, 256, 256, 3), np.uint8), "twiddle")


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


def _integers(got, want, what):
    assert (got == np.rint(got)).all(), what
    _same(got.astype(np.int64), want, what)


def test_integer_stages_equal_the_references(frames, taps):
    low, mid, high = O.band_masks()
    counts = np.stack([m.T.sum(1) for m in (low, mid, high)], -1)          # per device row k1 = kx
    for name, bgr in frames.items():
        t = taps[name]
        _same(t["rs"], bgr, (name, "rs"))
        g = O.gray(bgr)
        _same(t["gray"], g, (name, "gray"))
        gr = O.grad(g)
        _same(t["grad"], gr, (name, "grad"))
        lab = O.labels(gr)
        _same(t["map"], lab, (name, "map"))
        e = O.edges(lab)
        _same(t["edges"], e, (name, "edges"))
        assert t["edge_count"][0] == e.sum() and t["stats"][ST_EDGES] == e.sum(), name
        for k, want in zip(("jy", "jcb", "jcr"), O.jpeg_planes(bgr)):
            _same(t[k], want, (name, k))
        part, bits = O.hsv_part(bgr)
        _same(t["hue_bits"], bits, (name, "hue_bits"))
        assert t["stats"][ST_HUES] == sum(bin(int(b)).count("1") for b in bits), name
        _integers(t["hsv_part"], part, (name, "hsv_part"))
        _integers(t["lap_part"], O.lap_part(g), (name, "lap_part"))
        _integers(t["stats_ela"] * 1024, O.ela_block_sums(bgr), (name, "stats_ela"))
        _integers(t["fft_part"][:, [1, 4, 6]], counts, (name, "fft_part counts"))


def test_noise_block_stds(frames, taps):
    """Per 32x32 block against the float64 population std of the oracle's fp32 residual (the kernel restates the blur's
    operation order, so its residual is the same fp32 values).  Bar 4 * 1024 * 2^-53 relative: the mean and the sum of
    squared deviations are 1024-term double sums (relative error at most 1024 * 2^-53 each in the worst order), the
    factor 4 covers the two passes, the division and the sqrt; exactly 0 where the reference is 0.
    Measured on MI355X: worst relative error 0 on all 26 frames (the residual is a multiple of 2^-8 below 2^8, so the
    1024-term double sums are exact and both sides round the same quotient and root); bar 4.5e-13."""
    worst = 0.0
    for name, bgr in frames.items():
        want, got = O.noise_stds(O.gray(bgr)), taps[name]["stats_noise"]
        zero = want == 0
        assert (got[zero] == 0).all(), name
        rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
        if rel.size:
            worst = max(worst, float(rel.max()))
            assert rel.max() <= O.NOISE_RTOL, (name, float(rel.max()))
    print(f"stats_noise: worst relative error {worst:.3e} (bar {O.NOISE_RTOL:.3e})")


def _var_check(got, s1, s2, n, root, what):
    """got against the exact variance (or its root) of integer sums, within 8 * 2^-53 * E[x^2] / var"""
    from fractions import Fraction

    rtol = O.cancel_rtol(s1, s2, n)
    if rtol is None:
        assert got == 0.0, what
        return 0.0
    want = float(Fraction(s2, n) - Fraction(s1, n) ** 2)
    want = np.sqrt(want) if root else want
    rel = abs(got - want) / want
    assert rel <= rtol, (what, got, want, rel, rtol)
    return rel / rtol


def test_derived_statistics(frames, taps):
    """lap_var, sat_std, val_std from exact integer sums (rational arithmetic), the mid-band std and the three band
    means teacher-forced from the device's own logmag values in float64.  Variances are E[x^2] - mean^2 in doubles:
    bar 8 * 2^-53 * E[x^2] / var relative, exactly 0 where the variance is 0.  Band means: 65536 non-negative terms at
    most, bar 4 * 65536 * 2^-53.
    Measured on MI355X: at worst 0.144 of the variance bar; band means equal to the float64 means (error 0)."""
    low, mid, high = (m.T for m in O.band_masks())
    worst, worst_mean = 0.0, 0.0
    for name, bgr in frames.items():
        t = taps[name]
        st = t["stats"]
        lp = O.lap_part(O.gray(bgr)).sum(0)
        worst = max(worst, _var_check(st[ST_LAP_VAR], int(lp[0]), int(lp[1]), 65536, False, (name, "lap_var")))
        s1, s2, v1, v2 = (int(x) for x in O.hsv_part(bgr)[0].sum(0))
        worst = max(worst, _var_check(st[ST_SAT], s1, s2, 65536, True, (name, "sat_std")))
        worst = max(worst, _var_check(st[ST_VAL], v1, v2, 65536, True, (name, "val_std")))
        lm = t["logmag"].astype(np.float64)
        for idx, m in ((ST_LOW, low), (ST_MID, mid), (ST_HIGH, high)):
            want = lm[m].mean()
            if want == 0:
                assert st[idx] == 0, (name, idx)
            else:
                rel = abs(st[idx] - want) / want
                worst_mean = max(worst_mean, rel)
                assert rel <= 4 * 65536 * O.EPS64, (name, idx, rel)
        x = lm[mid]
        var = x.var()
        if var == 0:
            assert st[ST_MID_STD] == 0, name
        else:
            rtol = 8 * O.EPS64 * float((x * x).mean() / var)
            rel = abs(st[ST_MID_STD] - x.std()) / x.std()
            worst = max(worst, rel / rtol)
            assert rel <= rtol, (name, "mid std", rel, rtol)
    print(f"derived statistics: worst use of the variance bar {worst:.3f}, worst band mean error {worst_mean:.3e}")


def _fft_check(name, g, dev_tmp, dev_spec, tw, state):
    mir, ref, yard = O.fft_mirror(g, tw), O.fft_float64(g), O.fft_yardstick(g)
    for which, dev in ((0, dev_tmp), (1, dev_spec)):
        if not O.bits_equal(dev, mir[which]):
            state["unequal"].append((name, which, int((dev != mir[which]).sum())))
        r, m = O.fft_ratios(dev, ref[which], yard[which])
        state["rms"], state["max"] = max(state["rms"], r), max(state["max"], m)
        assert r <= O.FFT_RMS_X and m <= O.FFT_MAX_X, (name, which, r, m)
        if name in O.FFT_EXACT:
            assert O.fft_error(dev, ref[which]) == (0.0, 0.0), (name, which)


def test_fft_is_the_bit_mirror(frames, taps, twiddle):
    """fft_tmp and spectrum are bit-equal to the numpy float32 restatement of the kernels' butterflies (run with the
    table the device holds), on every frame; independently, against float64 the rms error stays within 4x and the
    maximum within 8x the fp32 yardstick's (scipy complex64 on the same frame), and the constant, origin-impulse and
    checkerboard frames are exact.
    Measured on MI355X: bit-equal on all 26 frames (and on the injected gray planes of test_chain_from_injected_gray);
    worst ratios to the yardstick rms 1.53x, max 2.77x (the gradient frame) - the mirror's own figures."""
    state = {"unequal": [], "rms": 0.0, "max": 0.0}
    for name, bgr in frames.items():
        _fft_check(name, O.gray(bgr), taps[name]["fft_tmp"], taps[name]["spectrum"], twiddle, state)
    print(f"fft: worst ratios to the yardstick rms {state['rms']:.2f}x max {state['max']:.2f}x; not bit-equal: {state['unequal']}")
    assert not state["unequal"], state["unequal"]


def test_logmag_and_band_sums(frames, taps):
    """logmag against float64 log1p(hypot) of the device's own spectrum, in fp32 ulps of the result; the yardstick is
    numpy's float32 log1p(hypot) on the same values, the bar 4x its maximum and no less than 1 ulp.  The band sums of
    fft_part against float64 sums of the device's logmag values, 4 * 128 * 2^-53 relative per row partial.
    Measured on MI355X: device 1.13 ulp, yardstick 1.26 ulp (bar 5.0 ulp); band sums worst 1.9e-16 relative (bar 5.7e-14)."""
    low, mid, high = (m.T for m in O.band_masks())
    worst_dev, worst_yard, worst_sum = 0.0, 0.0, 0.0
    per_frame = []
    for name in frames:
        t = taps[name]
        got, yard = O.logmag_ulps(t["logmag"], t["spectrum"])
        per_frame.append((name, got, yard))
        worst_dev, worst_yard = max(worst_dev, got), max(worst_yard, yard)
        lm = t["logmag"].astype(np.float64)
        for col, m, sq in ((0, low, False), (2, mid, False), (3, mid, True), (5, high, False)):
            want = np.where(m, lm * lm if sq else lm, 0.0).sum(1)
            got_s = t["fft_part"][:, col]
            assert (got_s[want == 0] == 0).all(), (name, col)
            nz = want != 0
            if nz.any():
                rel = np.abs(got_s[nz] - want[nz]) / want[nz]
                worst_sum = max(worst_sum, float(rel.max()))
                assert rel.max() <= O.BAND_RTOL, (name, col, float(rel.max()))
    print(f"logmag: device {worst_dev:.2f} ulp, yardstick {worst_yard:.2f} ulp; band sums worst {worst_sum:.3e}")
    bar = max(1.0, 4 * worst_yard)
    for name, got, yard in per_frame:
        assert got <= bar, (name, got, yard)


# ------------------------------------------------------------------------------------------------ injected inputs
def _hysteresis_batch(h, maps, names):
    for i in range(0, len(maps), 32):
        stack = np.stack(maps[i:i + 32])
        got, cnt = h.forensic_tap(stack, "edges", start="map"), h.forensic_tap(stack, "edge_count", start="map")
        for j, lab in enumerate(stack):
            want = O.edges(lab)
            _same(got[j], want, ("edges", names[i + j]))
            assert cnt[j, 0] == want.sum(), names[i + j]


def test_hysteresis_on_adversarial_maps(b0_handle):
    """label maps injected in place of `map`: chains along a row through all four words in both directions, diagonals
    through the word borders, weak pixels touching a strong one only across a word border in all 8 directions at rows
    0, 1, 254, 255, chains along the image borders (no wrap between rows), all weak / all strong / all none"""
    maps = {k: v for k, v in O.hysteresis_maps().items() if not k.startswith(("spiral", "serpentine"))}
    _hysteresis_batch(b0_handle, list(maps.values()), list(maps))


def test_hysteresis_needing_many_sweeps():
    """one-pixel spirals and serpentines over the whole plane: up to ~32,000 sweeps inside one launch.  Run once, in a
    process of its own under a time limit, so a sweep loop that never ends cannot hold the suite's handle."""
    import os
    import subprocess
    import sys

    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import rtdfd_amd as pkg, forensic_oracle as O
W = pkg.weights
h = pkg._lib.Handle(W.pack_all(W.seeded_state_dict(0), W.seeded_ssd_state_dict(0)), device=0, max_batch=1)
maps = {k: v for k, v in O.hysteresis_maps().items() if k.startswith(("spiral", "serpentine"))}
assert len(maps) == 4
stack = np.stack(list(maps.values()))
got, cnt = h.forensic_tap(stack, "edges", start="map"), h.forensic_tap(stack, "edge_count", start="map")
for j, (name, lab) in enumerate(maps.items()):
    want = O.edges(lab)
    assert (got[j] == want).all() and cnt[j, 0] == want.sum() == (lab != 1).sum(), name
print("many sweeps ok")
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "many sweeps ok" in r.stdout, r.stdout


def test_hysteresis_on_200_random_maps(b0_handle):
    maps = O.random_maps(200)
    _hysteresis_batch(b0_handle, maps, [f"random{i}" for i in range(len(maps))])


def test_nms_on_injected_gradients(b0_handle):
    """gradient fields over the whole Sobel range injected in place of `grad`; the reference takes every branch
    (direction classes, both diagonal signs, one step either side of tg22 and tg67, ties towards every neighbour, the
    image border) at least 100 times, counted here so the fields cannot silently degrade"""
    fields = O.nms_fields()
    got = b0_handle.forensic_tap(fields, "map", start="grad")
    got_e = b0_handle.forensic_tap(fields, "edges", start="grad")
    total = dict.fromkeys(O.NMS_BRANCHES, 0)
    for i, f in enumerate(fields):
        br = {}
        want = O.labels(f, branches=br)
        for k in total:
            total[k] += br[k]
        _same(got[i], want, ("map", i))
        _same(got_e[i], O.edges(want), ("edges", i))
    assert all(v >= 100 for v in total.values()), total
    with pytest.raises(Exception):
        b0_handle.forensic_tap(fields, "gray", start="grad")     # not downstream: refused, not stale data


def test_chain_from_injected_gray(b0_handle, twiddle):
    """gray planes that are the gray of no BGR frame, injected in place of `gray`: every kernel downstream"""
    planes = O.gray_only_frames()
    stack = np.stack(list(planes.values()))
    got = {t: b0_handle.forensic_tap(stack, t, start="gray")
           for t in ("gray", "grad", "lap_part", "map", "edges", "edge_count", "fft_tmp", "spectrum", "stats_noise", "stats")}
    state = {"unequal": [], "rms": 0.0, "max": 0.0}
    for i, (name, g) in enumerate(planes.items()):
        gr = O.grad(g)
        lab = O.labels(gr)
        _same(got["gray"][i], g, (name, "gray"))
        _same(got["grad"][i], gr, (name, "grad"))
        _integers(got["lap_part"][i], O.lap_part(g), (name, "lap_part"))
        _same(got["map"][i], lab, (name, "map"))
        _same(got["edges"][i], O.edges(lab), (name, "edges"))
        assert got["edge_count"][i, 0] == O.edges(lab).sum() == got["stats"][i, ST_EDGES], name
        want = O.noise_stds(g)
        assert (np.abs(got["stats_noise"][i] - want) <= O.NOISE_RTOL * want).all(), name
        _fft_check(name, g, got["fft_tmp"][i], got["spectrum"][i], twiddle, state)
    assert np.abs(got["grad"]).max() == 1020                      # the Sobel maximum is reached
    assert not state["unequal"], state["unequal"]
    with pytest.raises(Exception):
        b0_handle.forensic_tap(stack, "jy", start="gray")         # needs rs


@pytest.mark.parametrize("n", [1, 3, 16])
def test_batch_slots_equal_single_frame_calls(b0_handle, frames, n):
    """a different frame in every slot: every tap of frame f of an n-frame call equals, byte for byte, the tap of a
    single-frame call on that frame - full and fast mode (fast mode reads no full-only buffer)"""
    pick = [k for k in frames if k not in ("all0", "smooth", "blank")][:n]
    stack = np.stack([frames[k] for k in pick])
    for full, names in ((True, FULL_TAPS), (False, FAST_TAPS)):
        for t in names:
            batch = b0_handle.forensic_tap(stack, t, full=full)
            assert batch.shape[0] == n
            for f in range(n):
                single = b0_handle.forensic_tap(stack[f:f + 1], t, full=full)[0]
                assert batch[f].tobytes() == single.tobytes(), (t, full, pick[f])
                assert b0_handle.forensic_tap(stack, t, full=full, frame=f).tobytes() == single.tobytes(), (t, full, pick[f])
    with pytest.raises(Exception):
        b0_handle.forensic_tap(stack, "jy", full=False)


def test_production_path_is_untouched_by_the_taps(b0_handle, frames):
    """dfd_forensics on a 256x256 frame (its resize is the identity) reports the statistics the tapped chain holds"""
    bgr = frames["natural_720p"]
    st = b0_handle.forensic_tap(bgr[None], "stats")[0]
    b0_handle.forensics_reset(930)
    _, _, stats = b0_handle.forensics(bgr, True, 930)
    assert (stats["freq_low"], stats["freq_mid"], stats["freq_high"]) == (st[ST_LOW], st[ST_MID], st[ST_HIGH])
    assert stats["lap_var"] == st[ST_LAP_VAR] and stats["edge_density"] == st[ST_EDGES] / 65536.0
    assert (stats["sat_std"], stats["val_std"], stats["unique_hues"]) == (st[ST_SAT], st[ST_VAL], st[ST_HUES])

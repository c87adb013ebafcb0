"""GPU: the any-size frequency-domain entries are held to a fresh handle's bits after other calls on the same handle, in
the harness of tests/test_call_history_gpu.py (tests/history_cases.py; the case and its histories are in
tests/freq_domain_history.py).  The case - six boxes of a 90 x 110 frame through the host and the device entry, a 33 x 31
gray window through every tap, the features and their taps at 30 and 250 - runs on a handle of its own and again after

  repeat  the case itself
  large   eight boxes up to 1900 x 1000 of 1080p noise, white and checkerboard frames, features and taps at 1024
  grow    an 8 x 8 call, then one that makes ensure() re-allocate
  cross   the largest call of every family of the table, then `large` (four of the case's calls recorded)

with the history repeated in front of every recorded call.  Every output must be equal bit for bit.  The padded planes
of these kernels are what a larger earlier call leaves full of other windows' values."""
import pytest

import freq_domain_history as FH
import history_cases as H

pytestmark = pytest.mark.gpu

_FRESH = {}


def fresh():
    if "out" not in _FRESH:
        h = H.new_handle(FH.CASE.blob)
        try:
            _FRESH["out"] = FH.run(h)
        finally:
            h.close()
    return _FRESH["out"]


@pytest.mark.parametrize("hname", ["repeat", "large", "grow", "cross"])
def test_bits_of_a_fresh_handle(hname):
    want = fresh()
    h = H.new_handle(FH.CASE.blob)
    try:
        if hname == "repeat":
            FH.run(h)
            got = FH.run(h)
        else:
            got = FH.run(h, lambda: FH.HISTORIES[hname](h), thin=hname == "cross")
    finally:
        h.close()
    if hname == "cross":
        assert set(got) == set(FH.THIN)
        want = {k: want[k] for k in got}
    else:
        assert len(got) == 15
    diffs = H.compare(want, got)
    print(f"[call_history] frequency_domain after {hname}: {H.report(diffs)}")
    assert not diffs, H.report(diffs)


def test_the_fresh_results_are_right(pkg):
    """the baseline of the comparison against the float64 reference, so that it is not only self-consistent"""
    import numpy as np

    import freq_domain_oracle as O

    out = fresh()
    frame, gray, img = FH.case_inputs()
    from oracle import imgproc_ref as I

    g = I.bgr2gray_u8(frame)
    for (x, y, w, b), row, dev in zip(FH.BOXES, out["boxes"], out["device"]):
        win = g[y:y + b, x:x + w]
        r = O.reference(win)
        e_rms = O.fft_error(O.fft_yardstick(win)[1], O.fft_float64(win)[1])[0]
        bar = b * w * 4 * e_rms + 2.0 ** -22 * r["total"]        # the bar of test_freq_domain_gpu.py
        assert abs(row[0] - r["high"]) <= bar and abs(row[1] - r["total"]) <= bar
        assert np.array_equal(row, dev)
    assert np.array_equal(out["whole_gray"][0], out["tap.sums"])
    for size in FH.FEATURE_SIZES:
        f64 = O.features_float64(img, size)[0]
        assert np.abs(out[f"features{size}"] - f64).max() <= O.FEATURE_MAX

"""CPU: the frequency-domain case of the call-history table (tests/freq_domain_history.py) is in the table, reaches the
five new entry points, and its histories' inputs differ from its case inputs in every position they share."""
import numpy as np

import freq_domain_history as FH
import history_cases as H
from rtdfd_amd import _lib as L


def test_the_case_is_in_the_table_and_reaches_the_new_entries():
    assert H.BY_NAME["frequency_domain"] is FH.CASE and FH.CASE in H.CASES
    assert set(FH.REACHES) <= set(L.SIGNATURES) and len(FH.REACHES) == 5
    missing, unknown, both = H.coverage()
    assert not missing and not unknown and not both
    assert FH.CASE.histories[0] == "repeat" and set(FH.HISTORIES) == {"large", "grow", "cross"}
    assert set(FH.THIN) <= {"boxes", "whole_gray", "device"} | {f"tap.{n}" for n in FH.TAPS} | \
        {f"features{s}{t}" for s in FH.FEATURE_SIZES for t in [""] + ["." + n for n in FH.FEATURE_TAPS]}


def test_history_inputs_differ_from_the_case_inputs_in_every_shared_position():
    hists = [FH.history_frame()] + FH.grow_frames() + [FH.history_gray()]
    for hist in hists:
        for case in FH.case_inputs():
            a, b = (case, hist) if hist.ndim < case.ndim else (hist, case)    # the history's gray tap window against a colour case frame
            hv, cv = H.shared(a, b)
            assert hv.size and not (hv == cv).any(), (hist.shape, case.shape, int((hv == cv).sum()))


def test_the_boxes_lie_in_their_frames():
    frame = FH.case_inputs()[0]
    for boxes, (hh, ww) in ((FH.BOXES, frame.shape[:2]), (FH.history_boxes(), (1080, 1920))):
        assert all(x >= 0 and y >= 0 and w >= 1 and h >= 1 and x + w <= ww and y + h <= hh for x, y, w, h in boxes)
    xs = [b for b in FH.BOXES]
    assert any(x == 0 for x, *_ in xs) and any(x + w == 110 for x, _, w, _ in xs) and any(y + h == 90 for _, y, _, h in xs)

"""GPU: a depth-11 trainer session and the block-rows extraction are held to a fresh handle's bits after other calls on the
same handle, in the harness of tests/test_call_history_gpu.py (tests/history_cases.py; the case is in
tests/block11_history.py).  The case - a trainer with blocks 15 down to 11 unfrozen, the skip blocks at the reference's
drop-connect rates: two accumulates with every tap, gradient and export of the five blocks, one apply, eval on the live and
the EMA parameters, then `extract_block_rows` at blocks 11..15 and `train_augment_block_rows` at block 11 - runs on a handle
of its own and again after

  repeat     the case itself
  large      a whole block-15 session at max_n = 64
  nonfinite  the same with NaN and both infinities in every float the caller hands over

with the history repeated in front of every recorded call.  Every output must be equal bit for bit."""
import numpy as np
import pytest

import block11_history as BH
import history_cases as H

pytestmark = pytest.mark.gpu

_FRESH = {}


def fresh():
    if "out" not in _FRESH:
        h = H.new_handle(BH.CASE.blob)
        try:
            _FRESH["out"] = BH.run(h)
        finally:
            h.close()
    return _FRESH["out"]


@pytest.mark.parametrize("hname", BH.CASE.histories)
def test_bits_of_a_fresh_handle(hname):
    want = fresh()
    h = H.new_handle(BH.CASE.blob)
    try:
        if hname == "repeat":
            BH.run(h)
            got = BH.run(h)
        else:
            hist = H.history(BH.CASE, hname)
            got = BH.run(h, lambda: hist(h))
    finally:
        h.close()
    diffs = H.compare(want, got)
    print(f"[call_history] trainer_block11 after {hname}: {H.report(diffs)}")
    assert not diffs, H.report(diffs)


def test_the_fresh_results_are_a_depth_11_session():
    """the baseline is not only self-consistent: the session trained all five blocks, and the extraction at 12..15 is the
    older entry's"""
    out = fresh()
    for k in range(len(H.TRAIN_N)):
        step = out[f"accumulate{k}"]
        assert np.isfinite(step["loss"]) and np.isfinite(step["logits"]).all()
        for b in BH.BLOCKS:
            assert all(np.isfinite(v).all() and v.any() for v in step[f"b{b}.grads"].values()), (k, b)
        assert step["tap.b11.dae"].shape[1:] == (196, 672) and step["tap.b11.out"].shape[1:] == (49, 192)
    assert np.isfinite(out["grad_norm"]) and out["grad_norm"] > 0
    for b in BH.BLOCKS:
        assert not np.array_equal(out["after_apply"][f"b{b}.export"]["exp_w"], out["accumulate0"][f"b{b}.export"]["exp_w"]), b
    h = H.new_handle(BH.CASE.blob)
    try:
        for block in (12, 13, 14, 15):
            assert np.array_equal(out[f"rows{block}"], h.extract_block_input(BH.crops(), block)), block
    finally:
        h.close()
    assert out["rows11"].shape == (2, 14, 14, 112) and out["augment11"].shape == (1, 14, 14, 112)
    assert np.abs(out["rows11"]).max() > 0 and np.abs(out["augment11"]).max() > 0

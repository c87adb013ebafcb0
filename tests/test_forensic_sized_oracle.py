"""CPU: the size-generic stage references of tests/forensic_sized_oracle.py reproduce ForensicsRef((S, S))'s statistics,
and every fixture of the sized GPU tests sits away from every threshold at every size it is run at - so the GPU tests
compare scores exactly on every case, none left out."""
import numpy as np
import pytest

import forensic_sized_oracle as Z
from oracle.forensics_ref import ForensicsRef

CPU_SIZES = tuple(s for s in Z.SIZES if s <= 272)     # the 512 cases of the condition run in the module fixture below


def _close(a, b):
    return a == b or abs(a - b) <= 1e-9 * max(1.0, abs(b))


@pytest.mark.parametrize("S", CPU_SIZES)
def test_stage_references_reproduce_the_analyzer(S):
    for name, frame in Z.fixture_frames(S).items():
        ref = ForensicsRef((S, S))
        ref.analyze(frame)
        got, _ = Z.stats_from_stages(frame, S)
        assert set(ref.stats) <= set(got) | {"temporal_cv"}, (name, set(ref.stats) - set(got))
        for k, want in ref.stats.items():
            tol = 1e-6 if k in ("sat_std", "val_std", "noise_mean", "noise_cv", "ela_cv") else 1e-9   # float32 std in the reference
            assert abs(got[k] - want) <= tol * max(1.0, abs(want)), (S, name, k, got[k], want)
        if S < 64:
            assert "noise_mean" not in ref.stats and "ela_mean" not in ref.stats


def test_temporal_reference():
    S = 80
    ref, prev = ForensicsRef((S, S)), None
    for frame in Z.moving_sequence():
        ref.analyze(frame)
        got, prev = Z.stats_from_stages(frame, S, prev)
        assert _close(got["mean_diff"], ref.stats["mean_diff"])


def _assert_margin(stats, what):
    rel, cnt = Z.margin(stats)
    assert rel >= 10 * Z.STAT_RTOL and cnt >= 1, (what, rel, cnt, stats)


@pytest.mark.parametrize("S", Z.SIZES)
def test_fixtures_sit_away_from_every_threshold(S):
    for name, frame in Z.fixture_frames(S).items():
        ref = ForensicsRef((S, S))
        ref.analyze(frame)
        _assert_margin(ref.stats, (S, name))
    ref = ForensicsRef((S, S))
    for i, frame in enumerate(Z.moving_sequence()):
        ref.analyze(frame)
        _assert_margin(ref.stats, (S, "moving", i))
    if S in (48, 80, 272):
        ref = ForensicsRef((S, S))
        for i, (frame, full) in enumerate(Z.schedule_frames()):
            (ref.analyze if full else ref.analyze_fast)(frame)
            _assert_margin(ref.stats, (S, "schedule", i))


def test_largest_fixture_sits_away_from_every_threshold():
    ref = ForensicsRef((Z.LARGEST, Z.LARGEST))
    ref.analyze(Z.largest_frame())
    _assert_margin(ref.stats, "largest")


def test_band_masks_and_blocks():
    for S in (48, 80, 272):
        low, mid, high = Z.band_masks(S)
        assert low[0, 0] and not (low & mid).any() and not (mid & high).any()
        k = np.fft.fftfreq(S, 1.0 / S).astype(int)
        d2 = k[:, None] ** 2 + k[None, :] ** 2
        assert (low == (d2 <= (S // 8) ** 2)).all() and (high == ((d2 > (S // 4) ** 2) & (d2 <= (S // 2) ** 2))).all()
        assert Z.blocks(np.zeros((S, S))).shape[0] == (S // 32) ** 2


def test_hysteresis_maps_exercise_the_row_end():
    for S in (80, 272):
        maps = Z.hysteresis_maps(S)
        assert any(f"_b{S - 1}_" in k for k in maps) and "serpentine_columns" in maps
        e = Z.edges(maps["serpentine_rows"])
        assert e.sum() == (maps["serpentine_rows"] != 1).sum()          # the whole chain is reached
        assert Z.edges(maps["no_wrap_right"]).sum() == 1


def test_constant_plane_transforms_exactly():
    """the references of the spectrum test are exact on a constant plane, so the yardstick demands exact zeros there"""
    for S in Z.TAP_SIZES:
        g = np.full((S, S), 128, np.uint8)
        for ref, yard in zip(Z.fft_float64(g), Z.fft_yardstick(g)):
            print(S, Z.fft_error(yard, ref), np.abs(ref).max())

"""GPU: the general forensic chain (dfd_forensics_sized / dfd_forensic_tap_sized: csrc/forensic_kernels.hip, run-time edge) against
oracle/forensics_ref.ForensicsRef((S, S)) and the size-generic stage references of tests/forensic_sized_oracle.py.
Bars are those of tests/test_forensics_gpu.py and tests/test_forensic_stages_gpu.py."""
import numpy as np
import pytest

import forensic_oracle as O256
import forensic_sized_oracle as Z
import frames as F
from oracle.forensics_ref import ForensicsRef

pytestmark = pytest.mark.gpu

STATE_ERR = -5          # DFD_ERR_STATE


def _compare(got_scores, got_prob, got_stats, ref, res):
    """statistics within the bars, and - every fixture sits away from every threshold (asserted on the CPU by
    tests/test_forensic_sized_oracle.py) - scores and probability equal, always"""
    for k, want in ref.stats.items():
        have = got_stats[k]
        if k in Z.EXACT:
            assert have == want, (k, have, want)
        else:
            assert abs(have - want) <= Z.STAT_RTOL * max(1.0, abs(want)), (k, have, want)
    assert set(got_scores) == set(res["scores"])
    for k in res["scores"]:
        assert abs(got_scores[k] - res["scores"][k]) <= 1e-6, (k, got_scores[k], res["scores"][k], ref.stats)
    assert abs(got_prob - res["fake_probability"]) <= 1e-6


def _fresh(h, sid):
    h.forensics_release(sid)
    return sid


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ 1: statistics, scores
@pytest.mark.parametrize("S", Z.SIZES)
def test_statistics_and_scores_match_the_oracle(b0_handle, S):
    for name, frame in Z.fixture_frames(S).items():
        ref = ForensicsRef((S, S))
        res = ref.analyze(frame)
        sid = _fresh(b0_handle, 940)
        scores, prob, stats = b0_handle.forensics_sized(frame, S, full=True, stream_id=sid)
        _compare(scores, prob, stats, ref, res)
        if S < 64:                                                # one block: score exactly 0.0, statistics not computed
            assert scores["noise"] == 0.0 and scores["ela"] == 0.0
            assert all(np.isnan(stats[k]) for k in ("noise_mean", "noise_cv", "ela_mean", "ela_cv")), (name, stats)
    ref = ForensicsRef((S, S))
    sid = _fresh(b0_handle, 941)
    for frame in Z.moving_sequence():
        res = ref.analyze(frame)
        _compare(*b0_handle.forensics_sized(frame, S, full=True, stream_id=sid), ref, res)


@pytest.mark.parametrize("S", (48, 80, 272))
def test_stream_schedule_and_temporal_state(b0_handle, S):
    """13 frames with the reference's full / fast mix on one stream: temporal deque, frame counter (`frame_count > 10`)
    and every per-frame result follow the oracle"""
    ref = ForensicsRef((S, S))
    sid = _fresh(b0_handle, 942)
    for cur, full in Z.schedule_frames():
        res = ref.analyze(cur) if full else ref.analyze_fast(cur)
        scores, prob, stats = b0_handle.forensics_sized(cur, S, full=full, stream_id=sid)
        _compare(scores, prob, stats, ref, res)
        assert b0_handle.forensics_state(sid) == (ref.frame_count, len(ref.temporal_diffs), ref.prev_frame_gray is not None)
    assert ref.frame_count > 10 and "temporal_cv" in ref.stats
    b0_handle.forensics_reset(sid)
    assert b0_handle.forensics_state(sid) == (0, 0, False)


def test_largest_size_full_chain(b0_handle):
    S = Z.LARGEST
    frame = Z.largest_frame()
    ref = ForensicsRef((S, S))
    res = ref.analyze(frame)
    _compare(*b0_handle.forensics_sized(frame, S, full=True, stream_id=_fresh(b0_handle, 943)), ref, res)
    b0_handle.forensics_release(943)


# ------------------------------------------------------------------------------------------------ 2: stages
@pytest.fixture(scope="module", params=Z.TAP_SIZES)
def staged(request, b0_handle):
    S = request.param
    frames = {k: Z.resized(f, S) for k, f in Z.fixture_frames(S).items()}
    stack = np.stack(list(frames.values()))
    names = ("rs", "gray", "fft_tmp", "spectrum", "logmag", "fft_part", "grad", "lap_part", "map", "edges", "edge_count", "stats",
             "jy", "jcb", "jcr", "stats_ela", "stats_noise", "hsv_part", "hue_bits")
    got = {t: b0_handle.forensic_tap_sized(stack, S, t) for t in names}
    return S, frames, {name: {t: got[t][i] for t in names} for i, name in enumerate(frames)}


def test_integer_stages_equal_the_references(staged):
    S, frames, taps = staged
    counts = np.stack([m.T.sum(1) for m in Z.band_masks(S)], -1)
    for name, bgr in frames.items():
        t = taps[name]
        _same(t["rs"], bgr, (name, "rs"))
        g = Z.gray(bgr)
        _same(t["gray"], g, (name, "gray"))
        gr = Z.grad(g)
        _same(t["grad"], gr, (name, "grad"))
        lab = Z.labels(gr)
        _same(t["map"], lab, (name, "map"))
        e = Z.edges(lab)
        _same(t["edges"], e, (name, "edges"))
        assert t["edge_count"][0] == e.sum() and t["stats"][5] == e.sum(), name
        for k, want in zip(("jy", "jcb", "jcr"), Z.jpeg_planes(bgr)):
            _same(t[k], want, (name, k))
        part, bits = Z.hsv_part(bgr)
        _same(t["hue_bits"], bits, (name, "hue_bits"))
        _same(t["hsv_part"], part.astype(np.float64), (name, "hsv_part"))
        _same(t["lap_part"], Z.lap_part(g).astype(np.float64), (name, "lap_part"))
        _same(t["stats_ela"] * 1024, Z.ela_block_sums(bgr).astype(np.float64), (name, "stats_ela"))
        _same(t["fft_part"][:, [1, 4, 6]], counts.astype(np.float64), (name, "band counts"))
        want, got = Z.noise_stds(g), t["stats_noise"]
        assert got.shape == want.shape == ((S // 32) ** 2,)
        zero = want == 0
        assert (got[zero] == 0).all(), name
        assert (np.abs(got[~zero] - want[~zero]) <= O256.NOISE_RTOL * want[~zero]).all(), (name, "stats_noise")


def test_spectrum_against_float64(staged):
    """fft_tmp and spectrum against numpy float64, in units of the error of the fp32 yardstick (scipy complex64 on the
    same plane): rms within 4x, maximum within 8x - tests/forensic_oracle.py's fft_meets_bar, at size S.  The band sums
    against float64 sums of the device's own logmag values, per row partial.
    Measured on MI355X: worst ratios 1.77x rms (faint, 272, row pass), 2.66x max (gradient, 64, row pass); exact on the
    constant frame."""
    S, frames, taps = staged
    low, mid, high = (m.T for m in Z.band_masks(S))
    for name, bgr in frames.items():
        g = Z.gray(bgr)
        ref, yard = Z.fft_float64(g), Z.fft_yardstick(g)
        for which, tap in ((0, "fft_tmp"), (1, "spectrum")):
            r, m = Z.fft_ratios(taps[name][tap], ref[which], yard[which])
            print(f"S={S} {name} {tap}: {r:.2f}x rms, {m:.2f}x max of the yardstick's error")
            assert r <= Z.FFT_RMS_X and m <= Z.FFT_MAX_X, (S, name, tap, r, m)
        lm = taps[name]["logmag"].astype(np.float64)
        for col, msk, sq in ((0, low, False), (2, mid, False), (3, mid, True), (5, high, False)):
            want = np.where(msk, lm * lm if sq else lm, 0.0).sum(1)
            got = taps[name]["fft_part"][:, col]
            assert (got[want == 0] == 0).all(), (name, col)
            nz = want != 0
            if nz.any():
                # a row partial adds at most S doubles: 4 * S * 2^-53 (BAND_RTOL of the 256 chain, restated for S)
                assert (np.abs(got[nz] - want[nz]) / want[nz]).max() <= 4 * S * Z.EPS64, (name, col)


# ------------------------------------------------------------------------------------------------ 3: hysteresis
@pytest.mark.parametrize("S", (80, 272))
def test_hysteresis_on_injected_maps(b0_handle, S):
    named = Z.hysteresis_maps(S)
    maps = list(named.values()) + Z.random_maps(S, 50)
    names = list(named) + [f"random{i}" for i in range(50)]
    for i in range(0, len(maps), 16):
        stack = np.stack(maps[i:i + 16])
        got = b0_handle.forensic_tap_sized(stack, S, "edges", start="map")
        cnt = b0_handle.forensic_tap_sized(stack, S, "edge_count", start="map")
        for j, lab in enumerate(stack):
            want = Z.edges(lab)
            _same(got[j], want, ("edges", S, names[i + j]))
            assert cnt[j, 0] == want.sum(), names[i + j]


# ------------------------------------------------------------------------------------------------ 4: 256 through both
def test_size_256_equals_the_specialised_chain(b0_handle):
    for name, bgr in O256.fixture_frames().items():
        a = b0_handle.forensics(bgr, True, _fresh(b0_handle, 944))
        b = b0_handle.forensics_sized(bgr, 256, True, _fresh(b0_handle, 945))
        assert a[0] == b[0] and a[1] == b[1], (name, a[0], b[0])
        for k, want in a[2].items():
            have = b[2][k]
            if k in Z.EXACT or k == "frame_count":
                assert have == want, (name, k, have, want)
            else:
                assert (np.isnan(want) and np.isnan(have)) or abs(have - want) <= Z.STAT_RTOL * max(1.0, abs(want)), (name, k, have, want)
    b0_handle.forensics_release(944)
    b0_handle.forensics_release(945)


def test_the_two_instantiations_are_one_function_outside_the_spectrum(b0_handle):
    """The 256x256 chain and the general chain are two instantiations of one set of kernel bodies (compile-time edge
    256 / run-time edge): at S = 256 every buffer that does not pass through the spectrum - a radix-2 FFT on one, a
    dense DFT on the other - is the same bytes, frame slot by frame slot."""
    frames = O256.fixture_frames()
    stack = np.stack([frames[k] for k in ("noisy", "face_vga", "gradient")])
    assert stack.shape == (3, 256, 256, 3)
    for t in ("gray", "grad", "lap_part", "map", "edges", "edge_count", "jy", "jcb", "jcr", "stats_ela", "stats_noise", "hsv_part",
              "hue_bits"):
        a = b0_handle.forensic_tap(stack, t)
        b = b0_handle.forensic_tap_sized(stack, 256, t)
        assert a.dtype == b.dtype and a.shape == b.shape, (t, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), t
    a = b0_handle.forensic_tap(stack, "stats")
    b = b0_handle.forensic_tap_sized(stack, 256, "stats")
    assert a.shape == b.shape == (3, 9)
    assert a[:, 4:].tobytes() == b[:, 4:].tobytes()               # lap_var, edge count, sat / val std, hues
    for f in range(3):
        for j in range(4):                                           # freq low, mid, high, mid std: through the spectrum
            assert abs(b[f, j] - a[f, j]) <= Z.STAT_RTOL * max(1.0, abs(a[f, j])), (f, j, a[f, j], b[f, j])


# ------------------------------------------------------------------------------------------------ 5: batch slots
def test_batch_slots_equal_single_frame_calls(b0_handle):
    S = 80
    frames = [Z.resized(f, S) for f in Z.fixture_frames(S).values()]
    stack = np.stack(frames[:5])
    assert stack.shape[0] == 5
    for t in ("gray", "fft_tmp", "spectrum", "fft_part", "grad", "lap_part", "map", "edges", "edge_count", "stats", "jy", "jcb",
              "jcr", "stats_ela", "stats_noise", "hsv_part", "hue_bits"):
        batch = b0_handle.forensic_tap_sized(stack, S, t)
        for f in range(5):
            single = b0_handle.forensic_tap_sized(stack[f:f + 1], S, t)[0]
            assert batch[f].tobytes() == single.tobytes(), (t, f)


# ------------------------------------------------------------------------------------------------ 6: stream state
def test_stream_size_is_fixed_by_the_first_frame(pkg, b0_handle):
    frame = Z.wave_frame()
    sid = _fresh(b0_handle, 946)
    b0_handle.forensics_sized(frame, 80, True, sid)
    state = b0_handle.forensics_state(sid)
    for call in (lambda: b0_handle.forensics_sized(frame, 96, True, sid), lambda: b0_handle.forensics(frame, True, sid)):
        with pytest.raises(pkg._lib.DfdError) as e:
            call()
        assert e.value.code == STATE_ERR
        assert b0_handle.forensics_state(sid) == state
    b0_handle.forensics_reset(sid)
    with pytest.raises(pkg._lib.DfdError):
        b0_handle.forensics_sized(frame, 96, True, sid)          # reset keeps the size
    b0_handle.forensics_sized(frame, 80, True, sid)
    b0_handle.forensics_release(sid)
    b0_handle.forensics_sized(frame, 96, True, sid)              # after release: any size
    b0_handle.forensics_release(sid)
    sid256 = _fresh(b0_handle, 947)
    b0_handle.forensics(frame, True, sid256)
    with pytest.raises(pkg._lib.DfdError) as e:
        b0_handle.forensics_sized(frame, 80, True, sid256)
    assert e.value.code == STATE_ERR
    b0_handle.forensics_release(sid256)
    for bad in (100, 16, 1040):
        with pytest.raises(pkg._lib.DfdError):
            b0_handle.forensics_sized(frame, bad, True, _fresh(b0_handle, 948))


def test_released_plane_goes_to_streams_of_its_size_only(b0_handle):
    """an 80 x 80 plane released to the free list, then a 512 x 512 stream and an 80 x 80 stream run three frames each:
    a 6400-byte plane under the 512 stream would be overrun by its 262144-byte gray copy and corrupt the neighbour"""
    seq = Z.moving_sequence()
    b0_handle.forensics_sized(seq[0], 80, True, _fresh(b0_handle, 949))
    b0_handle.forensics_release(949)
    refs = {950: ForensicsRef((512, 512)), 951: ForensicsRef((80, 80))}
    sizes = {950: 512, 951: 80}
    for sid in refs:
        _fresh(b0_handle, sid)
    for frame in seq:
        for sid, ref in refs.items():
            res = ref.analyze(frame)
            _compare(*b0_handle.forensics_sized(frame, sizes[sid], True, sid), ref, res)
    for sid in refs:
        b0_handle.forensics_release(sid)


# ------------------------------------------------------------------------------------------------ 7: class surface
def test_analyzer_class_surface_at_128(pkg, b0_handle):
    A = pkg.frame_analysis.FrameForensicAnalyzer
    an = A(analysis_size=(128, 128), any_size=True, handle=b0_handle)
    frame = F.face_frame()
    r = an.analyze(frame)
    assert {"frequency", "noise", "ela", "edge", "color", "temporal"} <= set(r["scores"])
    assert r["analysis_type"] == "frame_forensic" and r["frame_number"] == 1
    manual = float(np.clip(sum(r["scores"][k] * an.weights[k] for k in an.weights), 0.0, 1.0))
    assert abs(r["fake_probability"] - manual) < 1e-6
    ref = ForensicsRef((128, 128))
    assert abs(ref.analyze(frame)["fake_probability"] - r["fake_probability"]) < 1e-6
    rf = an.analyze_fast(frame)
    assert set(rf["scores"]) == {"frequency", "temporal", "edge"} and rf["analysis_type"] == "frame_forensic_fast"
    assert an.frame_count == 2 and an.prev_frame_gray is not None and an.analysis_size == (128, 128)
    an.reset()
    assert an.frame_count == 0 and an.prev_frame_gray is None and len(an.temporal_diffs) == 0
    smooth, noisy, edgy = F.smooth_image(), F.noisy_image(), F.gradient_image()
    rs_, rn = an.analyze(smooth), (an.reset(), an.analyze(noisy))[1]
    assert rs_["scores"]["frequency"] >= rn["scores"]["frequency"]
    an.reset()
    uni = an.analyze(np.full((256, 256, 3), 100, np.uint8))
    assert uni["scores"]["color"] >= rn["scores"]["color"]
    an.reset()
    assert rs_["scores"]["edge"] >= an.analyze(edgy)["scores"]["edge"]
    b0_handle.forensics_release(an.stream_id)
    with pytest.raises(ValueError):
        A(analysis_size=(128, 128))
    for bad in ((100, 100), (128, 256), (16, 16), (2048, 2048)):
        with pytest.raises(ValueError, match="multiple of 16"):
            A(analysis_size=bad, any_size=True)
    a, b = A((256, 256), handle=b0_handle), A((256, 256), any_size=True, handle=b0_handle)
    for f in (frame, noisy):
        ra, rb = a.analyze(f), b.analyze(f)
        assert ra == rb
        assert all(a.last_stats[k] == b.last_stats[k] or np.isnan(a.last_stats[k]) for k in a.last_stats)
    for x in (a, b):
        b0_handle.forensics_release(x.stream_id)


def test_any_size_from_the_environment(pkg, monkeypatch):
    A = pkg.frame_analysis.FrameForensicAnalyzer
    monkeypatch.setenv("DFD_FORENSIC_ANY_SIZE", "1")
    assert A((96, 96)).analysis_size == (96, 96)
    monkeypatch.setenv("DFD_FORENSIC_ANY_SIZE", "0")
    with pytest.raises(ValueError):
        A((96, 96))
    assert A((96, 96), any_size=True).any_size


# ------------------------------------------------------------------------------------------------ 8: detector
def test_detector_with_a_swapped_analyzer(pkg, b0_handle):
    D, A = pkg.deepfake_detection.DeepfakeDetector, pkg.frame_analysis.FrameForensicAnalyzer
    frames = [F.face_frame(seed=s) for s in (1, 2, 3)]
    sized = D(use_tta=False, handle=b0_handle)
    sized.frame_analyzer = A((128, 128), any_size=True, handle=b0_handle)
    plain = D(use_tta=False, handle=b0_handle)
    alone = A((128, 128), any_size=True, handle=b0_handle)
    for i, f in enumerate(frames):
        rs_, rp = sized.predict(f)[3], plain.predict(f)[3]
        full = (i + 1) % sized.full_forensic_interval == 0       # the detector counts the frame first (reference :597, :509)
        want = alone.analyze(f) if full else alone.analyze_fast(f)
        assert rs_["frame_forensic"] == want
        assert rs_["faces_detected"] == rp["faces_detected"] and rs_["face_results"] == rp["face_results"]
        assert rs_["frame_count"] == i + 1
    for x in (sized.frame_analyzer, plain.frame_analyzer, alone):
        b0_handle.forensics_release(x.stream_id)

"""No GPU: the table of tests/history_cases.py is complete against `_lib.SIGNATURES`, its histories' inputs differ from the
cases' in every position they share, the non-finite histories hold NaN and both infinities, the case inputs meet what
the cases need (checked on the existing oracles), and the comparison flags a single bit."""
import numpy as np
import pytest
import torch

import history_cases as H
from rtdfd_amd import _lib as L


# ------------------------------------------------------------------------------------------------ the coverage table
def test_every_export_has_a_case_or_an_exemption():
    missing, unknown, both = H.coverage()
    assert not missing, f"exports with neither a case nor an exemption in tests/history_cases.py: {missing}"
    assert not unknown, f"the table names what _lib.SIGNATURES does not export: {unknown}"
    assert not both, f"both reached by a case and exempt: {both}"
    assert all(isinstance(r, str) and r for r in H.EXEMPT.values())


def test_the_coverage_check_fails_for_a_new_export(monkeypatch):
    monkeypatch.setitem(L.SIGNATURES, "dfd_some_new_entry", (None, []))
    assert H.coverage()[0] == ["dfd_some_new_entry"]


def test_every_case_has_its_histories_and_a_unique_name():
    assert len({c.name for c in H.CASES}) == len(H.CASES)
    for c in H.CASES:
        assert c.histories and c.histories[0] == "repeat", c.name
        for name in c.histories:
            assert name in ("repeat", "cross") or name in H.HISTORIES[c.family], (c.name, name)
        if "cross" in c.histories:
            assert c.blob == "full" and c.family in H.CROSS, c.name
        # a family that takes floats from the caller has the non-finite history
        if c.family in H.nonfinite_inputs():
            assert "nonfinite" in c.histories, c.name
    assert set(H.HISTORIES) == set(H.CROSS)


def test_the_classifier_matrix_is_the_one_the_layer_tests_walk_plus_the_per_image_kernels():
    import b0_layer_oracle as B

    names = [n for n, _, _ in H.classifier_configs()]
    assert names[:9] == [c.name for c in B.FP32_CONFIGS + B.BF16_CONFIGS] and len(names) == 13
    per_image = [o for n, o, _ in H.classifier_configs() if n.startswith("per_image")]
    assert sorted((o["fuse_late_skip"], o["fuse_proj0"]) for o in per_image) == [(-1, 0), (-1, 1), (0, 0), (0, 1)]
    assert all(o["fuse_k5"] == 1 and o["fuse_k5_min"] == 1 for o in per_image)
    for c in B.FP32_CONFIGS + B.BF16_CONFIGS:
        taps = dict((n, t) for n, _, t in H.classifier_configs())[c.name]
        assert taps == tuple(c.taps())
    assert len([c for c in H.CASES if c.family == "classifier"]) == 13 * 3
    assert all(t in B.DEFAULT.taps() for t in H.THIN_TAPS)


# ------------------------------------------------------------------------------------------------ the inputs
FAMILY_HISTORIES = sorted({(c.family, name) for c in H.CASES for name in c.histories})


@pytest.mark.parametrize("family,hname", FAMILY_HISTORIES)
def test_history_inputs_differ_from_the_case_inputs_in_every_shared_position(family, hname):
    """every history a case of the family runs; one whose inputs this table does not hold fails here"""
    table = H.history_inputs()
    if hname == "repeat":
        return                                                # the case itself, by definition
    if hname == "cross":                                      # the `large` histories of the other families, each held below
        assert all(table[f]["large"] for f in H.CROSS if f != family)
        return
    if hname == "nonfinite":                                  # `large` with these arrays: nothing finite against finite case inputs
        assert H.nonfinite_inputs()[family] and all(np.isfinite(c).all() for _, c in table[family]["large"] if c.dtype.kind == "f")
        hname = "large"
    pairs = table[family][hname]
    assert pairs
    for hist, case in pairs:
        hv, cv = H.shared(np.asarray(hist), np.asarray(case))
        assert hv.size and not (hv == cv).any(), (family, hname, hist.shape, case.shape, int((hv == cv).sum()))


def test_nonfinite_histories_hold_nan_and_both_infinities_and_nothing_finite():
    for family, arrays in H.nonfinite_inputs().items():
        for a in arrays:
            assert a.dtype == np.float32 and not np.isfinite(a).any(), family
            if a.size >= 3:
                assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any(), family
    # bf16 operands of the GEMM history keep their kind when they are cut to 16 bits
    import gemm_oracle as G

    b = G.from_bits(G.to_bits(H.nonfinite_like(np.zeros(6, np.float32))))
    assert np.isnan(b[0]) and b[1] == np.inf and b[2] == -np.inf


def test_the_gemm_picks_are_ragged_and_cover_every_group():
    picks = H.gemm_picks()
    assert {c.group for c in picks} == {"pointwise", "pw8", "pw9", "gated", "conv", "bf16"}
    assert all(c.M % 16 for c in picks if c.conv is None and not (c.gated and c.group == "pw8"))     # (pw8's gated shapes are whole images)
    big = H.gemm_history_shapes()
    import gemm_oracle as G

    assert max(c.M for c in big) == max(c.M for c in G.CASES if c.conv is None)
    assert max(c.K for c in big) >= max(c.K for c in G.CASES if c.conv is None) and max(c.N for c in big) == max(c.N for c in G.CASES)


def test_the_ssd_case_frame_yields_rows_and_the_history_many():
    """on the oracle: the detector's rows of the case frame (at the looser of the case's thresholds) and the valid priors
    of the history's injected heads"""
    import ssd_stage_oracle as S
    from oracle import ssd_ref
    from rtdfd_amd import ssd_arch, weights

    sd = weights.to_torch(weights.seeded_ssd_state_dict(0))
    boxes = ssd_ref.detect_bounding_box(sd, ssd_arch, H.ssd_case_frame(), min(H.SSD_THRESHOLDS))
    print(f"the oracle's rows of the case frame at {min(H.SSD_THRESHOLDS)}: {len(boxes)}")
    assert len(boxes) >= 1
    hist = ssd_ref.detect_bounding_box(sd, ssd_arch, H.ssd_history_frames()[0], 0.01)       # what the `ssd` family's history asks for
    print(f"the oracle's rows of the 720p history frame at 0.01: {len(hist)}")
    assert len(hist) >= 100                                   # DetectionOutput keeps at most 200 rows: "many" = over half of that
    many =H.ssd_many_priors().reshape(-1)
    _, _, conf3 = S.head_case(ssd_arch, 3)
    p3 = 1.0 / (1.0 + np.exp((conf3[..., 0] - conf3[..., 1]).astype(np.float64)))
    assert many.size == 3 * S.P * 6 and ((p3 > 0.01).sum(axis=1) > 2000).all()
    b, p = H.ssd_one_prior()
    assert int((p > 0.01).sum()) == 1 and (b[..., 2:] > b[..., :2]).all()


def test_the_mtcnn_case_image_yields_candidates():
    import mtcnn_stage_oracle as M
    from oracle import mtcnn_ref
    from rtdfd_amd import weights

    sd = weights.to_torch(weights.seeded_mtcnn_state_dict(0))
    taps = {}
    mtcnn_ref.detect_face(sd, M.image(M.STALE_SMALL), taps)
    probs = [np.asarray(v) for k, v in taps.items() if k.startswith("pnet.prob")]
    assert probs and sum(int((p > H.MTCNN_CASE_THRESHOLDS[0]).sum()) for p in probs) >= 1
    taps = {}
    mtcnn_ref.detect_face(sd, M.image(H.MTCNN_EDGE), taps)             # the second image: at the default thresholds
    assert sum(int((np.asarray(v) > mtcnn_ref.THRESHOLDS[0]).sum()) for k, v in taps.items() if k.startswith("pnet.prob")) >= 1
    assert np.asarray(taps["rnet.prob"]).size >= 1


@pytest.mark.parametrize("level", H.TRAIN_LEVELS)
def test_the_trainer_cases_meet_the_gate_margin(level):
    margins = H.trainer_margins(level)
    print(f"{level}: gate margins {margins}")
    assert len(margins) == len(H.TRAIN_N) and min(margins) >= 1.0, margins


def test_jpeg_case_files_are_what_the_issue_names():
    from PIL import Image
    import io

    for kind, size, mode in (("420", (16, 16), "YCbCr"), ("gray", (17, 13), "L")):
        for f in H.jpeg_files(kind):
            im = Image.open(io.BytesIO(f))
            assert im.size == size and im.mode == {"YCbCr": "RGB", "L": "L"}[mode]
    im = Image.open(io.BytesIO(H.jpeg_files("420")[0]))
    assert im.layer[0][1:3] == (2, 2)                       # 4:2:0
    hist = H.jpeg_files("history")
    assert len(hist) == 8 and all(Image.open(io.BytesIO(f)).size == (512, 512) for f in hist)
    assert all(b"\xff\xdd" in f for f in H.jpeg_files("restart"))     # DRI
    assert [a.shape[:2] for a in H.jpeg_encode_images()] == [(1, 1), (13, 17)]


# ------------------------------------------------------------------------------------------------ the comparison
def _result():
    rs = np.random.RandomState(0)
    return {"tap": rs.randn(3, 5).astype(np.float32), "nested": {"bf16": rs.randint(0, 60000, 7).astype(np.uint16),
                                                                   "f64": rs.randn(4), "c64": (rs.randn(4) + 1j * rs.randn(4)).astype(np.complex64)},
            "file": b"\xff\xd8abc\xff\xd9", "boxes": [(1, 2, 3, 4), (5, 6, 7, 8)], "count": 2, "prob": 0.25, "rows": np.arange(10, dtype=np.int32)}


def _copy(r):
    import copy

    return copy.deepcopy(r)


def test_equal_results_compare_equal_bit_for_bit():
    assert H.compare(_result(), _copy(_result())) == []
    a = {"x": np.array([np.nan, 1.0], np.float32)}
    assert H.compare(a, _copy(a)) == []                      # the same NaN bits are the same result


def test_a_single_flipped_mantissa_bit_is_flagged():
    a, b = _result(), _copy(_result())
    b["tap"].view(np.uint32)[1, 2] ^= 1
    d = H.compare(a, b)
    assert len(d) == 1 and d[0].name == "tap" and d[0].count == 1 and d[0].first == (1, 2)
    assert np.allclose(a["tap"], b["tap"], rtol=1e-6, atol=0)          # a tolerance would not have seen it
    b = _copy(a)
    b["nested"]["f64"].view(np.uint64)[3] ^= 1
    d = H.compare(a, b)
    assert [x.name for x in d] == ["nested.f64"] and d[0].first == (3,)
    b = _copy(a)
    b["nested"]["bf16"][6] ^= 1
    b["nested"]["c64"].view(np.uint32)[7] ^= 1
    assert [x.name for x in H.compare(a, b)] == ["nested.bf16", "nested.c64"]
    b = _copy(a)
    b["prob"] = float(np.nextafter(0.25, 1.0))
    assert [x.name for x in H.compare(a, b)] == ["prob"]
    assert "tap" in H.report(H.compare(a, {**_copy(a), "tap": a["tap"] + np.float32(1e-7)}))


def test_a_nan_against_a_number_is_flagged_and_so_is_a_negative_zero():
    a, b = _result(), _copy(_result())
    b["tap"][0, 0] = np.nan
    d = H.compare(a, b)
    assert len(d) == 1 and d[0].count == 1 and "more NaN" in d[0].detail
    assert len(H.compare(b, a)) == 1
    z = {"x": np.zeros(3, np.float32)}
    assert len(H.compare(z, {"x": np.array([0.0, -0.0, 0.0], np.float32)})) == 1
    n1 = {"x": np.array([0x7FC00000], np.uint32).view(np.float32)}
    n2 = {"x": np.array([0x7FC00001], np.uint32).view(np.float32)}
    assert len(H.compare(n1, n2)) == 1                       # two NaNs of other bits differ too


def test_a_count_off_by_one_a_missing_row_and_a_changed_byte_are_flagged():
    a = _result()
    b = _copy(a)
    b["count"] = 3
    assert [x.name for x in H.compare(a, b)] == ["count"]
    b = _copy(a)
    b["boxes"].append((9, 9, 9, 9))
    names = [x.name for x in H.compare(a, b)]
    assert names[0] == "boxes.len" and "boxes[2].len" in names
    b = _copy(a)
    b["boxes"][1] = (5, 6, 7, 9)
    assert [x.name for x in H.compare(a, b)] == ["boxes[1][3]"]
    b = _copy(a)
    b["file"] = b"\xff\xd8abd\xff\xd9"
    d = H.compare(a, b)
    assert d[0].name == "file" and d[0].first == (4,) and d[0].count == 1
    b = _copy(a)
    b["rows"] = b["rows"][:9]
    assert H.compare(a, b)[0].count == -1                    # a shape is no element
    b = _copy(a)
    del b["tap"]
    assert H.compare(a, b)[0].name == "tap"
    b = _copy(a)
    b["rows"] = b["rows"].astype(np.int64)
    assert len(H.compare(a, b)) == 1


def test_the_first_difference_reported_is_the_first_output_in_launch_order():
    a = {"b0.dw": np.zeros(4, np.float32), "b1.dw": np.zeros(4, np.float32), "logits": np.zeros(2, np.float32)}
    b = _copy(a)
    b["logits"][0] = 1
    b["b1.dw"][3] = 1
    d = H.compare(a, b)
    assert [x.name for x in d] == ["b1.dw", "logits"] and H.report(d).startswith("2 outputs differ; first: b1.dw: 1 elements differ, first at (3,)")

"""GPU: every device path is held to a fresh handle's bits after other calls on the same handle (tests/history_cases.py
holds the cases, the histories, the inputs and the comparison; tests/test_history_cases.py checks those without a GPU).

One test per (case, history).  The case runs on a handle made for it with nothing run before and again on a second
handle after the history.  Where a case is a list of independent calls (taps, detections, decodes, ...) the history is
repeated in front of EVERY call whose output is recorded; where it is one sequence that belongs together (a trainer
session from begin to end, a stream's frames) the history ends in front of the sequence, or of each of its parts.  Under
"cross" - fourteen families' largest calls - the classifier's n = 3 cases record every fourth tap (and all their other
outputs) so that the history can still run in front of every recorded call; no history and no configuration is thinned.
Every output must be equal bit for bit: floats as their uint32 / uint16 / uint64 patterns, JPEG files as bytes, rows,
boxes and counts exactly, no NaN where the fresh handle has none.  No tolerance, no element left out.  One output is put
in order first: the records of "pnet.cand" are sorted (np.lexsort) on both sides, because the launch appends them with an
atomic counter and their order is not part of the result (the precedent: test_mtcnn_stages_gpu.py's stale-scratch test);
the set of records and the counter are compared exactly.  Neither handle calls warmup().

So that no baseline is vacuous, the fresh results are also held to references of their own: at n = 3 every tap of the
nine b0_layer_oracle configurations to its float64 layer reference at the bars of test_b0_layers_gpu.py, from the crops
to the logit; the four per-image configurations to the bits of the form they replace (default / late_all), tap by tap; the
logits of every configuration at n = 1, 3 and 5 to the "logit" bar from the handle's own pooled features (that check
alone holds the head MLP only), its rms part pooled over the three; every expand a plan fuses must be refused as a tap,
which shows that the per-image kernels ran; JPEG decodes equal Pillow's pixels and dfd_jpeg_decode_counts shows the batch
on the device decoder; JPEG encodes equal Pillow's bytes.

`test_the_harness_reports_a_stream_that_was_not_reset` runs the one case whose output legitimately depends on the
history - `forensics` on a stream the history fed and did not release - through the same harness and requires it to
report a difference: the comparison can fail on the device.

The issue names 200 as a `forensic_tap_sized` size; the entry takes multiples of 16 only (DFD_ERR_ARG otherwise), so the
case runs 64 and 208 and records the refusal of 200 as one of its outputs.  The issue's MTCNN image, STALE_SMALL, has no
P-Net candidate at the default thresholds (the stale-scratch test relies on that): it runs at 0.3, and a three-level
edge image with seven candidates at the defaults runs beside it.

Cases (tests/history_cases.py lists each one's calls and shapes):
  classifier        13 configurations (b0_layer_oracle's FP32_CONFIGS + BF16_CONFIGS; the per-image kernels forced on with
                    "fuse_k5_min" = 1, "fuse_late_skip" unset and 0, "fuse_proj0" on and off) x n = 1, 3, 5 crops on
                    stress_state_dict(0), max_batch 16: at n = 3 every tap the plan materialises, at n = 1 and 5 b0.dw,
                    b1.dw, b6.dw, b8.gate, b11.dw, b15.out; always feat, logits, extract_trunk at 14 and 15, gradcam
                    logits and heat; at n = 3 the device-pointer entries
  gemm_tap          ten ragged shapes of gemm_oracle.CASES (pw6 / pw7 at N % 4 != 0 and == 0, pw8 plain / gated / bf16,
                    pw9, gated, a dilated 3 x 3 conv, bf16 plain / gated) after M = 8200, K = 264, N = 672
  gradcam_tap       start "z" with fp32 and bf16 z, start "x", n = 3, every stage and guard row, after n = 16
  face_path         100 x 100 frame, boxes 1 x 1, 8 x 8 and one at the border, after 16 boxes at 1080p
  ssd, variants     both thresholds and every ssd_tap name at 240 x 320 after 720p; one valid prior after thousands
  mtcnn             detect / extract with landmarks, align, taps of STALE_SMALL and of the edge image after STALE_BIG and
                    600 O-Net / 300 R-Net windows, non-finite in that history (every P-Net tap of the small image:
                    test_mtcnn_stages_gpu.py's stale-scratch test, which stays as it is)
  haar              64 x 64, both entries and every tap of every scale, after 720p
  forensics         every tap at 256, 64 and 208 after 16 frames at 512 and 1080p streams; released-then-reused stream
                    ids through forensics, forensics_sized, reset, forensic_signals_device and analyze_streams_batch
  frequency, jpeg_decode (+ restart files, "jpeg_device_restart"), jpeg_encode, train_augment (every stage on),
  trainer_head / _conv / _block (begin with the same seed, accumulates at n = 2 and 5, taps, gradients, exports, apply,
  eval live and EMA, after a max_n = 64 session with forced gradients and an apply), fused_entries (240 x 320 after 720p)

MEASURED on one MI355X: the file's 321 tests (277 comparisons) run in 127 s, 106 s of it in the comparisons: classifier
80 s (195 comparisons, the slowest 2.0 s), forensics 6.3 s, haar 5.7 s, ssd 3.7 s, augment 2.1 s, every other family
under 1.5 s; the slowest tests are forensic_taps / cross 5.1 s, haar / cross 3.9 s and ssd / cross 2.8 s.  Outcome per
family and history - repeat / large / grow / nonfinite / cross ("-": the family takes 8-bit input only and has no such
history; the variant detectors run repeat and large):
  classifier  held / held / held / held / held      gemm_tap   held / held / held / held / held
  gradcam_tap held / held / held / held / held      face_path  held / held / held /  -   / held
  ssd         held / held / held /  -   / held      ssd_detection_tap held / held / - / held / held
  mtcnn       held / held / held / held / held      haar       held / held / held /  -   / held
  forensics   held / held / held /  -   / held      frequency  held / held / held /  -   / held
  jpeg_decode held / held / held /  -   / held      jpeg_encode held / held / held /  -   / held
  train_augment held / held / held / - / held       trainers   held / held / held / held / held
  fused_entries held / held / held / - / held
"held": all outputs bit for bit equal to the fresh handle's, in every case of the family.  `repeat` never differed: with
the candidate records in order, no path here is non-deterministic from run to run.  Fresh results: the worst tap of the
fp32 configurations is b8.out at 0.52 of its bar (split_gemm0: 0.62), of the bf16 ones the stem at exactly its 1 ulp; the
logits sit at 0.27 .. 0.79 of the pooled bar; the per-image configurations equal their forms in every tap.  The
sensitivity case reports forensics' mean_diff (-1.0 on a fresh stream, 51.16 after the history's frames) and frame count.
kernel bugs found: none.
"""
import time

import numpy as np
import pytest

import b0_layer_oracle as B
import history_cases as H

pytestmark = pytest.mark.gpu

_FRESH = {}                 # case name -> its result on a handle of its own, never modified (`fresh` makes it again when it is gone)
TIMES = {}
CONFIGS = {name: (opt, taps) for name, opt, taps in H.classifier_configs()}


def _config_of(case):
    return case.name[len("classifier-"):].rsplit("-n", 1)[0]


@pytest.fixture(scope="module", autouse=True)
def _report_and_release():
    yield
    if TIMES:
        slow = sorted(TIMES.items(), key=lambda kv: -kv[1])[:8]
        print(f"\n[call_history] {len(TIMES)} comparisons in {sum(TIMES.values()):.1f} s; slowest: " +
              ", ".join(f"{c}/{h} {t:.1f} s" for (c, h), t in slow))
        fam = {}
        for (c, h), t in TIMES.items():
            fam[H.BY_NAME[c].family] = fam.get(H.BY_NAME[c].family, 0.0) + t
        print("[call_history] per family: " + ", ".join(f"{k} {v:.1f} s" for k, v in sorted(fam.items())))
    _FRESH.clear()                          # the results and the cached inputs are of no use to the rest of the session
    for f in vars(H).values():
        if hasattr(f, "cache_clear"):
            f.cache_clear()


def _freeze(v):
    if isinstance(v, dict):
        for x in v.values():
            _freeze(x)
    elif isinstance(v, (list, tuple)):
        for x in v:
            _freeze(x)
    elif isinstance(v, np.ndarray):
        v.setflags(write=False)


def fresh(case):
    """the case on a handle of its own: computed once and shared - but a classifier configuration's taps are ~150 MB, so
    only the configuration last asked for stays; another is computed again when a test asks (in any order)"""
    if case.name not in _FRESH:
        if case.family == "classifier":
            for k in [k for k in _FRESH if k.startswith("classifier-") and _config_of(H.BY_NAME[k]) != _config_of(case)]:
                del _FRESH[k]
        h = H.new_handle(case.blob)
        try:
            out = case.run(h, H._noop)
        finally:
            h.close()
        _freeze(out)
        _FRESH[case.name] = out
    return _FRESH[case.name]


def after(case, hname):
    """-> the case's result after the history; under "cross" a thinnable case records every fourth tap, so that the
    fourteen families' largest calls can still run in front of every recorded call"""
    h = H.new_handle(case.blob)
    try:
        if hname == "repeat":
            case.run(h, H._noop)
            return case.run(h, H._noop)
        hist = H.history(case, hname)
        if hname == "cross" and case.thinnable:
            return case.run(h, lambda: hist(h), thin=True)
        return case.run(h, lambda: hist(h))
    finally:
        h.close()


def _id(p):
    return p.name if isinstance(p, H.Case) else str(p)


@pytest.mark.parametrize("case,hname", H.pairs(), ids=_id)
def test_bits_of_a_fresh_handle(case, hname):
    t0 = time.time()
    want = fresh(case)
    got = after(case, hname)
    if hname == "cross" and case.thinnable:
        assert set(got) < set(want) and len(got) >= 20, sorted(got)
        want = {k: want[k] for k in got}
    diffs = H.compare(want, got)
    TIMES[(case.name, hname)] = time.time() - t0
    print(f"[call_history] {case.name} after {hname}: {H.report(diffs)} ({TIMES[(case.name, hname)]:.2f} s)")
    assert not diffs, f"{case.name} after {hname}: {H.report(diffs)}"


@pytest.mark.parametrize("cfg", B.FP32_CONFIGS + B.BF16_CONFIGS, ids=lambda c: c.name)
def test_the_fresh_taps_hold_the_layer_bars_from_the_crops_to_the_logit(cfg):
    """the whole chain of test_b0_layers_gpu.py on the fresh n = 3 result, so the baseline of the bit comparison is right
    from the first launch on, not only self-consistent"""
    res = H.layer_checks(cfg, fresh(H.BY_NAME[f"classifier-{cfg.name}-n3"]))
    bad = {k: round(r["ratio"], 3) for k, r in res.items() if not r["ratio"] <= 1.0}
    worst = max(res, key=lambda k: res[k]["ratio"])
    print(f"[call_history] {cfg.name}: {len(res)} taps, worst {worst} at {res[worst]['ratio']:.3f} of its bar")
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(H.PER_IMAGE_FORM))
def test_the_per_image_kernels_give_their_forms_bits(name):
    """b0_plan.hip: the per-image launches replace a block's form with that form's bits - every tap both plans
    materialise, feat, logits, trunks and Grad-CAM equal those of the configuration the layer bars hold above"""
    mine = dict(fresh(H.BY_NAME[f"classifier-{name}-n3"]))
    form = fresh(H.BY_NAME[f"classifier-{H.PER_IMAGE_FORM[name]}-n3"])
    common = [k for k in mine if k in form and not k.startswith("refused.")]
    assert len(common) >= 50 and {"b8.dw", "b11.dw", "b15.out", "logits", "gradcam.heat"} <= set(common)
    diffs = H.compare({k: form[k] for k in common}, {k: mine[k] for k in common})
    assert not diffs, H.report(diffs)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_fresh_classifier_logits_hold_the_float64_bar(name):
    """the "logit" bar of b0_layer_oracle at n = 1, 3 and 5: the max bar per batch, the rms bar pooled over the three"""
    sqs = []
    for n in H.CLS_N:
        r = H.logit_check(fresh(H.BY_NAME[f"classifier-{name}-n{n}"]))
        sqs.append(r["sq"])
        print(f"[call_history] {name} n = {n}: logit max |d| / u at {r['ratio']:.3f} of its bar, {r['vs_yard']:.2f} x the yardstick")
        assert r["ratio"] <= 1.0, r
    p = B.pooled_rms_ratio(sqs)
    print(f"[call_history] {name}: logit rms pooled over {len(sqs)} batches at {p['ratio']:.3f} of its bar")
    assert p["ratio"] <= 1.0, (name, p)


@pytest.mark.parametrize("restart", [False, True], ids=["plain", "restart"])
def test_the_fresh_jpeg_decodes_are_pillows_and_ran_on_the_device(restart):
    """pixels equal Pillow's; dfd_jpeg_decode_counts rose by the batch's two frames on the device side and by none on the host's"""
    got = fresh(H.BY_NAME["jpeg_decode_restart" if restart else "jpeg_decode"])
    diffs = H.compare(H.jpeg_decode_expected(restart), got)
    assert not diffs, H.report(diffs)


def test_the_fresh_jpeg_encodes_are_pillows_bytes():
    diffs = H.compare(H.jpeg_encode_expected(), fresh(H.BY_NAME["jpeg_encode"]))
    assert not diffs, H.report(diffs)


def test_the_case_inputs_did_what_the_cases_need():
    """on the device's own results: the SSD case frame yields rows, the MTCNN edge image candidates, the one-prior
    detection one row, size 200 is refused, the Haar frame has more than one scale"""
    ssd = fresh(H.BY_NAME["ssd"])
    assert len(ssd[f"detect_{min(H.SSD_THRESHOLDS)}"]["boxes"]) >= 1
    assert int(fresh(H.BY_NAME["ssd_detection_tap"])["one_prior"]["count"][0]) == 1
    assert fresh(H.BY_NAME["mtcnn"])["tap_batch.pnet.cand"]["counter"] >= 1
    assert fresh(H.BY_NAME["forensic_taps"])["refused_200"] != 0
    assert fresh(H.BY_NAME["haar"])["n_scales"] >= 2


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_classifier_plan_is_the_one_the_configuration_names(name):
    """every expand the plan fuses is refused as a tap ("not materialised"): the per-image kernels really ran at n = 3"""
    out = fresh(H.BY_NAME[f"classifier-{name}-n3"])
    refused = {k: v for k, v in out.items() if k.startswith("refused.")}
    assert len(refused) == 15 - sum(t.endswith(".exp") for t in CONFIGS[name][1]) and all(v != 0 for v in refused.values()), refused
    if name.startswith("per_image_skip-1"):
        assert {"refused.b8.exp", "refused.b9.exp", "refused.b11.exp"} <= set(refused)


def test_the_harness_reports_a_stream_that_was_not_reset():
    case = H.SENSITIVITY
    diffs = H.compare(fresh(case), after(case, "unreleased"))
    print(f"[call_history] {case.name}: {H.report(diffs)}")
    assert diffs and diffs[0].name.startswith("forensics"), "a stream that kept its frames gave a fresh stream's answer"

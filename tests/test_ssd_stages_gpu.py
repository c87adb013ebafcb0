"""GPU: every launch of the SSD face detector (dfd_ssd_tap) against the per-launch references of
tests/ssd_stage_oracle.py, teacher-forced - each launch is compared from the HIP path's own input tap - and the
detector's tail (ssd_decode_kernel, ssd_nms_kernel) on injected inputs (dfd_ssd_detection_tap).

Bars (none invented here):
  * floating launches (conv1 from the bit-exact resized image, every trunk and head convolution, norm3, affine, add, the
    decode): the classifier suite's rule, imported from tests/b0_layer_oracle.py - rms(d) / rms(ref) <= 4 x the
    torch-fp32-on-CPU yardstick's + 2^-23 and max |d| / u <= 8 x the yardstick's + 2^-21 over every element, u = the op
    on magnitudes (ssd_stage_oracle.scale); the probability's u is 1.
  * bit-exact: every materialised max pool against the ceil-mode max of its input tap; the fused conv1 + pool1 launch
    against the pooled conv1 tap (see below); DetectionOutput rows and counts, order included, against
    oracle.ssd_ref.detection_output of the SAME call's boxes and probabilities; every image of a batched call against
    the same image sent alone.
  * zero threshold flips of the decode: the float64 probability of every prior lies on the side of the confidence
    threshold the HIP value lies on (tests/test_ssd_stage_oracle.py: no prior of the case within 1e-6 of it but the
    planted pair, 2e-6 either side, which is held to its side as well).
  * rows of the env-switched conv1 paths against the default path's: same count and <= 2e-4 (tests/test_ssd_gpu.py's bar).

Fused pool1 (ssd_conv1_pool_kernel) vs the pooled conv1 tap (ssd_conv1_mfma_kernel, which runs when conv1 is tapped or
has a second reader): both start each accumulator at the bias and issue, per pixel, the same MFMAs in the same order -
K-steps 0..4, inside a step the weight planes 2, 1, 0 (EXACT) or the six plane x term products smallest first - with the
same lane layout (lane = pixel, quarter-wave = 8 consecutive k), and the pool is a max.  So bit equality is ASSERTED,
for the EXACT and the non-EXACT instances.

Non-finite boxes are out of scope for DetectionOutput (the decode cannot produce them from finite heads); zero-area
boxes are in: their overlap is 0 (Caffe), they never suppress and are never suppressed.

What each defect the suite is there for would trip:
  * the third weight plane dropped (relative error ~2^-17 per product): the floating bar of test_every_launch_from_its_own_input -
    tests/test_ssd_stage_oracle.py applies the defect to the yardstick of res2a and lands at 3.1 x the bar;
  * the ceil-mode clamp off by one: the bit-exact pools (maxpool3s2_kernel in test_variant_arch_launches and the child
    processes; the fused pool against the pooled conv1 tap and against float64 in every frame) - last row / column;
  * `>=` in the confidence test: case conf_threshold (50 scores equal to the threshold: 120 rows instead of 70);
  * no division fallback in jaccard_above: case near_threshold (even a correctly rounded reciprocal decides 7 of its
    160 in-band pairs differently: tests/test_ssd_stage_oracle.py);
  * the index tiebreak lost from the key: cases all_equal, ties_straddle, crowded_bin (rows in index order among ties);
  * overlap word w + 1 read: cases words_visible_0 / _63 / _64 (victims and lone survivors on both sides of every word edge);
  * cut_bin == -1 ignored: cases valid_1 .. valid_400, conf_threshold, one_small, chains, zero_area and
    test_production_regime_rows (n_valid <= 400: every valid key sorted).

Measured on an MI355X, worst HIP error / torch-fp32 yardstick error per tensor over every case of this file (177 floating
comparisons; the bar allows 4 rms / 8 max):
  conv1 0.88 (VALU path 0.99)  pool1 (fused, from the image) 0.87  res2a 1.98  res2b 1.44  res3p 0.43  res3a 1.57  res3b 3.54
  res4p 1.18  res4a 3.45  res4b 4.85  res5a 3.88  res5b 3.11  conv6_1 0.95  conv6_2 3.14  conv7_1 1.09  conv7_2 1.45
  conv8_1 1.01  conv8_2 1.31  conv9_1 1.06  conv9_2 2.78  norm3 0.48  heads: norm3 2.63  res5b 3.27  conv6_2 3.20
  conv7_2 0.91  conv8_2 0.57  conv9_2 0.98  variant: bn1 0.33  aff1 0.33  sum1 0.34  sum2 0.33  decode: boxes 0.40  prob 0.33
The worst error / bar of any comparison is 0.978: res4b on the blank frame (rms 6.03e-7 against a yardstick of 1.24e-7;
the same launch is at 0.77 - 0.82 on the other frames, res5a at 0.75 - 0.84).  These are the K = 2304 convolutions
(3 x 3 x 256): the split-precision GEMM adds its 72 K-steps x 6 plane products to one fp32 accumulator in sequence, torch
sums in blocks, so the HIP rms grows with K where the yardstick's does not.  The products are exact and the launch is
correct; it is the closest to the bar this file measures, and the result is deterministic (every GEMM tile issues the
same MFMA sequence: tests/test_gemm_tiles_gpu.py).
Fused pool1 is bit-identical to the pooled conv1 tap on every frame (0 of 180,000 values differ), EXACT and non-EXACT.
Env-switched paths: DFD_SSD_CONV1_POOL=0 rows identical to the default path's; DFD_SSD_CONV1_MFMA=0 rows within 1.4e-6.
Every bit-exact comparison holds (pools, rows and counts of all 27 injected sets and of the 3-image batches, batch = alone).
n_valid: background_bias 8.0: face 248, natural 60, blank 0 (returns []); 7.0: face 1305, natural 597, blank 37;
default handle: face 6188, blank 6755, natural 6472, noise 6214.
Run time: 10 s for the file (45 tests), of which 5 s are the two child processes.
kernel bugs found: none.  Oracle bug fixed: ssd_ref.jaccard returned NaN (0 / 0) for touching zero-area boxes, and
detection_output then suppressed the box the kernel keeps; it now follows Caffe's rule (overlap 0 unless the
intersection has positive width and height).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ssd_ref
from tests import frames
from tests import ssd_stage_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
REPORT = {}                        # tensor -> worst HIP / yardstick ratio
WORST = {"ratio": 0.0, "n": 0}     # worst error / bar of any comparison, number of comparisons
NVALID = {}                        # (handle, frame) -> n_valid of the production-regime test
CASES = O.nms_cases()
_ROWS = {}                         # case -> oracle rows (computed once)

FRAMES = {
    "face_720p": lambda: frames.face_frame(1280, 720, 3),
    "blank": frames.blank_frame,
    "all_0": lambda: np.zeros((480, 640, 3), np.uint8),
    "all_255": lambda: np.full((480, 640, 3), 255, np.uint8),
    "noise_qvga": lambda: frames.noisy_image((240, 320), 9),
}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("MEASURED worst HIP / yardstick ratio per tensor:", {k: round(v, 2) for k, v in sorted(REPORT.items())})
    print(f"MEASURED worst error / bar {WORST['ratio']:.3f} over {WORST['n']} comparisons; n_valid {NVALID}")


@pytest.fixture(scope="module")
def S(pkg):
    return pkg.ssd_arch


@pytest.fixture(scope="module")
def default(pkg, b0_handle, ssd_sd, S):
    return (b0_handle, S) + O.sds(pkg, ssd_sd)


def _handle(pkg, seeded_sd, sd, arch=None):
    return pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, sd, ssd_arch=arch), device=0, max_batch=1)


@pytest.fixture(scope="module", params=["two_readers", "fused"])
def variant(request, pkg, seeded_sd, ssd_sd, S):
    arch = O.variant_arch(S, request.param == "two_readers")
    sd = O.variant_state_dict(ssd_sd, arch)
    h = _handle(pkg, seeded_sd, sd, arch)
    yield (h, arch) + O.sds(pkg, sd) + (request.param,)
    h.close()


@pytest.fixture(scope="module", params=[8.0, 7.0])
def trained_like(request, pkg, seeded_sd):
    h = _handle(pkg, seeded_sd, pkg.weights.seeded_ssd_state_dict(0, background_bias=request.param))
    yield h, request.param
    h.close()


# --------------------------------------------------------------------------- trunk and heads
class Taps:
    """the HIP path's taps of one frame, fetched on demand (each fetch runs the detector once) as (1, h, w, c) float32"""

    def __init__(self, h, arch, frame):
        self.h, self.arch, self.frame, self.shapes = h, arch, frame, O.shapes(arch)
        self.np = {"data": O.data_u8(frame, arch).astype(F32)}

    def raw(self, name):
        if name not in self.np:
            c, m = self.shapes[name]
            t = self.h.ssd_tap(self.frame, name, m * m * c)
            assert t.size == m * m * c, (name, t.size)
            self.np[name] = t.reshape(1, m, m, c).copy()
        return self.np[name]

    def get64(self, name):
        return O.to_nchw(self.raw(name), torch.float64)

    def get32(self, name):
        return O.to_nchw(self.raw(name), torch.float32)


def _record(r, where):
    print(f"{where} {r['tap']}: rms {r['rms']:.3e} max/u {r['max']:.3e} yard rms {r['yard']['rms']:.3e} max/u {r['yard']['max']:.3e} "
          f"ratio {r['ratio']:.3f} vs_yard {r['vs_yard']:.2f}")
    REPORT[r["tap"]] = max(REPORT.get(r["tap"], 0.0), r["vs_yard"])
    WORST["ratio"], WORST["n"] = max(WORST["ratio"], r["ratio"]), WORST["n"] + 1
    assert r["ratio"] <= 1.0, (where, r)


def _pool_ref(t: Taps, name):
    src, k, s = O._kinds(t.arch)[name][1]
    return F.max_pool2d(t.get32(src), k, s, 0, ceil_mode=True).permute(0, 2, 3, 1).numpy()


def _check_launches(t: Taps, sd32, sd64, where, names, fused=()):
    """names: the launches to check; fused: pools computed inside conv1's launch (no conv1 buffer to force from)"""
    kinds = O._kinds(t.arch)
    for name in names:
        if name in fused:
            ref, u = O.pooled_conv1(t.get64, sd64, t.arch, name)
            yard, _ = O.pooled_conv1(t.get32, sd32, t.arch, name)
            _record(O.compare(name, t.get64(name), ref, yard, u), where)
            # the unfused kernel's map (tapping conv1 turns the fusion off for that call), pooled: the same bits
            diff = int((t.raw(name) != _pool_ref(t, name)).sum())
            print(f"{where} fused {name} vs pooled conv1 tap: {diff} of {t.raw(name).size} values differ")
            assert diff == 0, (where, name, diff)
        elif not name.endswith(".head") and kinds[name][0] == "maxpool":
            assert np.array_equal(t.raw(name), _pool_ref(t, name)), (where, name)
        else:
            _record(O.check(name, t.get64(name), t.get64, t.get32, sd64, sd32, t.arch), where)


@pytest.mark.parametrize("fname", list(FRAMES))
def test_every_launch_from_its_own_input(default, fname):
    """D.1: all of ssd_arch.LAYERS and the six heads, every element (map borders, the ragged last MFMA tiles of the 150 map,
    the last fused 8 x 8 pooled tile of the 75 map); all-0 / all-255: the largest padding contrast, the EXACT input at its extremes"""
    h, S, sd32, sd64 = default
    t = Taps(h, S, FRAMES[fname]())
    _check_launches(t, sd32, sd64, fname, O.order(S), fused=("pool1",))


@pytest.mark.parametrize("fname", ["face_720p", "all_255"])
def test_variant_arch_launches(variant, fname):
    """D.2: non-integer input transform (the non-EXACT conv1 kernels), affine and add launches; with a second reader of
    conv1 the unfused ssd_conv1_mfma_kernel<false> and two maxpool3s2_kernel launches at 150 -> 75 (bit-exact from their
    input taps), without it the fused ssd_conv1_pool_kernel<false> (bar, and bit equality with the pooled conv1 tap)"""
    h, arch, sd32, sd64, kind = variant
    t = Taps(h, arch, FRAMES[fname]())
    if kind == "two_readers":
        names = ["conv1", "pool1", "bn1", "pool1b", "aff1", "sum1", "res2a", "res2b", "sum2", "res3a", "norm3", "conv9_2", "conv9_2.head"]
        _check_launches(t, sd32, sd64, f"variant2 {fname}", names)
    else:
        _check_launches(t, sd32, sd64, f"variant1 {fname}", ["conv1", "pool1", "aff1", "sum1", "res2b", "sum2", "res3p"], fused=("pool1",))


# --------------------------------------------------------------------------- env-switched conv1 paths
PATH_FRAMES = ("face_720p", "all_0")


def _conv1_path_dump(path: str):
    """child process (the switches are read once per process): conv1 and pool1 of this process's path on two frames
    against the bar, pool1 bit-exact from the conv1 tap (a separate launch on both switched paths), rows dumped"""
    import rtdfd_amd as pkg

    W = pkg.weights
    sd = W.seeded_ssd_state_dict(0)
    h = pkg._lib.Handle(W.pack_all(W.seeded_state_dict(0), sd), device=0, max_batch=1)
    sd32, sd64 = O.sds(pkg, sd)
    out = {}
    for fname in PATH_FRAMES:
        frame = FRAMES[fname]()
        t = Taps(h, pkg.ssd_arch, frame)
        _check_launches(t, sd32, sd64, f"child {fname}", ["conv1", "pool1"])
        ref, u = O.pooled_conv1(t.get64, sd64, t.arch)
        _record(O.compare("pool1", t.get64("pool1"), ref, O.pooled_conv1(t.get32, sd32, t.arch)[0], u), f"child {fname} (from the image)")
        out[fname] = h.ssd_tap(frame, "rows", 200 * 5)
    h.close()
    np.savez(path, **out)
    print("child worst HIP / yardstick:", {k: round(v, 2) for k, v in REPORT.items()}, "worst error / bar", round(WORST["ratio"], 3))


def test_conv1_paths_each_in_a_process_of_its_own(default, tmp_path):
    """D.3: DFD_SSD_CONV1_MFMA=0 (ssd_conv1_kernel + maxpool3s2_kernel) and DFD_SSD_CONV1_POOL=0 (ssd_conv1_mfma_kernel +
    maxpool3s2_kernel), one fresh child each, one after the other, stopping at the first that does not exit 0"""
    h = default[0]
    base = {f: h.ssd_tap(FRAMES[f](), "rows", 200 * 5).reshape(-1, 5) for f in PATH_FRAMES}
    for var in ("DFD_SSD_CONV1_MFMA", "DFD_SSD_CONV1_POOL"):
        path = str(tmp_path / f"{var}.npz")
        code = "import sys; sys.path.insert(0, %r); from tests import test_ssd_stages_gpu as T; T._conv1_path_dump(%r)" % (ROOT, path)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **{var: "0"}),
                           timeout=300, cwd=ROOT)
        print(var + "=0", r.stdout[-2500:])
        assert r.returncode == 0, (var, r.stdout[-3000:], r.stderr[-3000:])
        got = dict(np.load(path))
        for f in PATH_FRAMES:
            rows = got[f].reshape(-1, 5)
            assert len(rows) == len(base[f]), (var, f, len(rows), len(base[f]))
            d = float(np.abs(rows - base[f]).max()) if len(rows) else 0.0
            print(f"{var}=0 {f}: {len(rows)} rows, max |d| vs the default path {d:.3e}")
            assert d <= 2e-4, (var, f, d)


# --------------------------------------------------------------------------- decode on injected heads
def _rows_exact(rows, count, boxes, prob, S, where):
    want = ssd_ref.detection_output(boxes, prob, S.CONF_THRESHOLD, S.NMS_THRESHOLD, S.TOP_K, S.KEEP_TOP_K)
    assert int(count) == len(want), (where, int(count), len(want))
    w = O.rows_array(want, S.KEEP_TOP_K)
    bad = np.nonzero((rows != w).any(1))[0]
    assert bad.size == 0, (where, "first differing row", int(bad[0]), rows[bad[0]], w[bad[0]])
    return want


def test_decode_on_injected_heads(default):
    """D.4: three images of distinct head values in one call; boxes and probabilities against float64 at the bar (numpy
    float32 as yardstick), no threshold flips, the planted logits (p = 0.5, saturation to 1.0 and to 0, 0.01 -+ 2e-6),
    rows bit-exact from the call's own boxes / prob, every image bit-identical to itself sent alone"""
    h, S, _, _ = default
    heads, loc, conf = O.head_case(S)
    bo, po, rows, count = h.ssd_detection_tap(heads=O.flat_heads(heads))
    pri = ssd_ref.prior_boxes(S.SOURCES, S.INPUT)
    thr = F32(S.CONF_THRESHOLD)
    tt = torch.from_numpy
    for i in range(3):
        b64, p64, u = O.decode64(pri, loc[i], conf[i], S.VARIANCES)
        b32, p32 = O.decode32(pri, loc[i], conf[i], S.VARIANCES)
        _record(O.compare("boxes", tt(bo[i]).double(), tt(b64), tt(b32), tt(u)), f"heads image {i}")
        _record(O.compare("prob", tt(po[i]).double(), tt(p64), tt(p32), torch.ones(O.P, dtype=torch.float64)), f"heads image {i}")
        flips = (p64 > np.float64(thr)) != (po[i] > thr)
        assert not flips.any(), (i, np.nonzero(flips)[0], p64[flips], po[i][flips])
        _rows_exact(rows[i], count[i], bo[i], po[i], S, f"heads image {i}")
        b1, p1, r1, c1 = h.ssd_detection_tap(heads=O.flat_heads(heads, (i,)))
        assert np.array_equal(b1[0], bo[i]) and np.array_equal(p1[0], po[i]) and np.array_equal(r1[0], rows[i]) and c1[0] == count[i], i
    pl = {k: po[0][i] for k, (i, _) in O.PLANTED.items()}
    assert pl["half"] == 0.5 and pl["sat_hi30"] == 1.0 and pl["sat_hi100"] == 1.0, pl
    assert 0 <= pl["sat_lo100"] < 1e-40 and 0 < pl["sat_lo30"] < 1e-12, pl
    assert pl["thr_above"] > thr >= pl["thr_below"], pl


# --------------------------------------------------------------------------- DetectionOutput on injected boxes and prob
def _oracle_rows(name, S):
    if name not in _ROWS:
        c = CASES[name]
        rows = ssd_ref.detection_output(c["boxes"], c["prob"], S.CONF_THRESHOLD, S.NMS_THRESHOLD, S.TOP_K, S.KEEP_TOP_K)
        _ROWS[name] = (O.rows_array(rows, S.KEEP_TOP_K), len(rows))
    return _ROWS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_detection_output_on_injected_sets(default, name):
    """D.5: rows and count bit-exact, order included (what each case is for: ssd_stage_oracle.nms_cases)"""
    h, S, _, _ = default
    c = CASES[name]
    rows, count = h.ssd_detection_tap(boxes=c["boxes"][None], prob=c["prob"][None])
    want, n = _oracle_rows(name, S)
    print(f"{name}: n_valid {c['n_valid']} -> {int(count[0])} rows")
    assert int(count[0]) == n == c.get("count", n), (name, int(count[0]), n)
    bad = np.nonzero((rows[0] != want).any(1))[0]
    assert bad.size == 0, (name, "first differing row", int(bad[0]), rows[0][bad[0]], want[bad[0]])


def test_detection_output_batch_of_three(default):
    """three different cases in one call (a 0-valid image between two full ones): each equals itself alone and the
    oracle; a normal detector call on the handle gives the same rows before and after the injected calls"""
    h, S, _, _ = default
    frame = FRAMES["face_720p"]()
    before = h.ssd_tap(frame, "rows", 200 * 5)
    b = np.stack([CASES[n]["boxes"] for n in O.BATCH3])
    p = np.stack([CASES[n]["prob"] for n in O.BATCH3])
    rows, count = h.ssd_detection_tap(boxes=b, prob=p)
    for i, name in enumerate(O.BATCH3):
        r1, c1 = h.ssd_detection_tap(boxes=b[i:i + 1], prob=p[i:i + 1])
        want, n = _oracle_rows(name, S)
        assert count[i] == c1[0] == n and np.array_equal(rows[i], r1[0]) and np.array_equal(rows[i], want), name
    assert count[1] == 0
    assert np.array_equal(h.ssd_tap(frame, "rows", 200 * 5), before)


# --------------------------------------------------------------------------- the production regime through the real net
def _teacher_forced_rows(h, S, frame, where):
    prob = h.ssd_tap(frame, "prob", O.P).copy()
    boxes = h.ssd_tap(frame, "boxes", O.P * 4).reshape(O.P, 4).copy()
    rows = h.ssd_tap(frame, "rows", 200 * 5).reshape(-1, 5).copy()
    want = _rows_exact(O.rows_array(rows, S.KEEP_TOP_K), len(rows), boxes, prob, S, where)
    hh, ww = frame.shape[:2]
    assert h.detect_faces(frame, 0.5) == ssd_ref.postprocess(want, hh, ww, 0.5), where
    return int((prob > F32(S.CONF_THRESHOLD)).sum()), len(rows)


def test_production_regime_rows(trained_like, S):
    """D.6: detectors that leave few valid priors (the regime of a trained net: n_valid <= 400, cut_bin == -1)"""
    h, bias = trained_like
    seen = {}
    for fname, frame in (("face_720p", FRAMES["face_720p"]()), ("natural", frames.natural_like()), ("blank", frames.blank_frame())):
        nv, nr = _teacher_forced_rows(h, S, frame, f"bias {bias} {fname}")
        seen[fname] = NVALID[f"bias{bias:g}/{fname}"] = nv
        print(f"background_bias {bias} {fname}: n_valid {nv}, {nr} rows")
        if nv == 0:
            assert nr == 0 and h.detect_faces(frame, 0.5) == []
    if bias == 8.0:                                                            # three (handle, frame) pairs in the sorted-everything regime
        assert all(v <= O.TOPK for v in seen.values()) and seen["blank"] == 0 < seen["natural"], seen
    else:
        assert 0 < seen["blank"] <= O.TOPK, seen


ROW_FRAMES = {"face_720p": FRAMES["face_720p"], "blank": frames.blank_frame, "natural": frames.natural_like, "noise_qvga": FRAMES["noise_qvga"]}


@pytest.mark.parametrize("fname", list(ROW_FRAMES))
def test_default_handle_rows_teacher_forced(default, fname):
    """the histogram regime (thousands of valid priors) through the real net, rows bit-exact from the handle's own boxes / prob"""
    h, S, _, _ = default
    frame = ROW_FRAMES[fname]()
    nv, nr = _teacher_forced_rows(h, S, frame, f"default {fname}")
    NVALID[f"default/{fname}"] = nv
    print(f"default {fname}: n_valid {nv}, {nr} rows")
    assert nv > O.TOPK

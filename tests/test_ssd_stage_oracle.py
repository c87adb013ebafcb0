"""CPU: the SSD per-launch oracle (tests/ssd_stage_oracle.py) and its seeded cases, checked before any GPU sees them:
the float64 layer chain against oracle.ssd_ref.forward, DetectionOutput against an independent all-pairs restatement,
the properties every injected case claims, Caffe's rule for degenerate boxes, and that the bar of the GPU suite is
tight enough to see the defects it is there for (a dropped weight plane, a ceil-mode clamp off by one)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ssd_ref
from tests import frames
from tests import ssd_stage_oracle as O

F32 = np.float32


@pytest.fixture(scope="module")
def S(pkg):
    return pkg.ssd_arch


@pytest.fixture(scope="module")
def cases():
    return O.nms_cases()


def _det(S, b, p):
    return ssd_ref.detection_output(b, p, S.CONF_THRESHOLD, S.NMS_THRESHOLD, S.TOP_K, S.KEEP_TOP_K)


@pytest.fixture(scope="module")
def rows_of(S, cases):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _det(S, cases[name]["boxes"], cases[name]["prob"])
        return cache[name]
    return get


@pytest.mark.parametrize("variant", [False, True])
def test_float64_chain_reproduces_the_oracle_forward(pkg, S, ssd_sd, variant):
    """every tap of ssd_ref.forward (torch fp32, end to end) lies within float32 rounding of the float64 layer chain:
    rms(d) <= 2e-5 rms(ref) and max |d| <= 1e-4 max |ref| after up to 20 fp32 layers of ~1e-6 each"""
    arch = O.variant_arch(S, True) if variant else S
    sd = O.variant_state_dict(ssd_sd, arch) if variant else ssd_sd
    sd32, sd64 = O.sds(pkg, sd)
    frame = frames.noisy_image((240, 320), 9)
    taps = {}
    ssd_ref.forward(sd32, arch, frame, taps)
    c64 = O.chain(frame, sd64, arch)
    assert set(O.shapes(arch)) == set(c64)
    for name, (c, m) in O.shapes(arch).items():
        assert c64[name].shape == (1, c, m, m), (name, c64[name].shape)
    for name, _, _ in arch.LAYERS:
        ref, got = c64[name], taps[name].double()
        assert float((got - ref).pow(2).mean().sqrt()) <= 2e-5 * float(ref.pow(2).mean().sqrt()), name
        assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), name
    loc, conf = O.split_heads([c64[s[0] + ".head"].permute(0, 2, 3, 1).numpy() for s in arch.SOURCES], arch, 1)
    assert np.abs(loc[0] - taps["loc"]).max() <= 1e-4 * np.abs(loc).max()
    assert np.abs(conf[0] - taps["conf"]).max() <= 1e-4 * np.abs(conf).max()
    pri = ssd_ref.prior_boxes(arch.SOURCES, arch.INPUT)
    b64, p64, u = O.decode64(pri, loc[0].astype(F32), conf[0].astype(F32), arch.VARIANCES)
    b32, p32 = O.decode32(pri, taps["loc"], taps["conf"], arch.VARIANCES)
    assert np.abs(b32 - b64).max() <= 1e-4 and np.abs(p32 - p64).max() <= 1e-4 and (u > 0).all()


def test_degenerate_boxes_overlap_zero():
    """Caffe: the overlap is 0 unless the intersection has positive width and height - never 0 / 0"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        seg, pt = F32([.1, .1, .1, .3]), F32([.5, .5, .5, .5])
        assert ssd_ref.jaccard(seg, seg) == 0.0 and ssd_ref.jaccard(pt, pt) == 0.0
        assert ssd_ref.jaccard(F32([.2, .7, .25, .7]), F32([.25, .7, .3, .7])) == 0.0          # touching end to end
        assert ssd_ref.jaccard(F32([0, 0, .5, .5]), F32([.5, 0, 1, .5])) == 0.0                 # sharing an edge
        assert ssd_ref.jaccard(F32([.05, .05, .35, .35]), seg) == 0.0                           # a segment inside a box
        assert ssd_ref.jaccard(F32([0, 0, 1, 1]), F32([0, 0, 1, .5])) == 0.5


def test_detection_output_equals_the_all_pairs_restatement(S, cases, rows_of):
    for name, c in cases.items():
        want = O.detection_output_brute(c["boxes"], c["prob"], S.CONF_THRESHOLD, S.NMS_THRESHOLD, S.TOP_K, S.KEEP_TOP_K)
        got = rows_of(name)
        assert got == want, name
        assert all(np.isfinite(r).all() for r in got), name


def test_cases_have_the_properties_they_claim(S, cases, rows_of):
    thr = F32(S.CONF_THRESHOLD)
    for name, c in cases.items():
        assert c["boxes"].shape == (O.P, 4) and c["prob"].shape == (O.P,), name
        assert int((c["prob"] > thr).sum()) == c["n_valid"], (name, int((c["prob"] > thr).sum()))
        if "count" in c:
            assert len(rows_of(name)) == c["count"], (name, len(rows_of(name)))
        if "kept_before_cut" in c:
            uncut = ssd_ref.detection_output(c["boxes"], c["prob"], S.CONF_THRESHOLD, S.NMS_THRESHOLD, S.TOP_K, 10 ** 6)
            assert len(uncut) == c["kept_before_cut"] > S.KEEP_TOP_K, (name, len(uncut))
    assert sorted(c["n_valid"] for n, c in cases.items() if n.startswith("valid_")) == [0, 1, 2, 399, 400, 401, 512, 513, 4096, 8732]
    for k in (2, 399, 400, 401, 512, 513, 4096, 8732):                # distinct scores; chains really happen
        p = cases[f"valid_{k}"]["prob"]
        assert len(np.unique(p[p > thr])) == k
        assert len(rows_of(f"valid_{k}")) < min(k, S.KEEP_TOP_K) or k == 2
    # ties across the 400th rank
    c = cases["ties_straddle"]
    v, above, n = c["tie"]
    assert int((c["prob"] > F32(v)).sum()) == above < O.TOPK < above + n == above + int((c["prob"] == F32(v)).sum())
    # the crowded cut bin, by the kernel's own float32 binning
    c = cases["crowded_bin"]
    bin0, sub0, n_above, n_hi, n_crowd = c["crowded"]
    p = c["prob"][c["prob"] > thr]
    b = O.nms_bin(p)
    assert int((b > bin0).sum()) == n_above and int((b == bin0).sum()) == 3000
    s = O.nms_sub(p[b == bin0], bin0)
    assert int((s > sub0).sum()) == n_hi and int((s == sub0).sum()) == n_crowd
    assert n_above + n_hi < O.TOPK <= n_above + n_hi + n_crowd                    # the 400th rank lies inside the sub-bin
    assert len(np.unique(p[b == bin0][s == sub0])) == 4                           # 2^-22 / 2^-24: necessarily ties
    # strict threshold, exact 1.0
    c = cases["conf_threshold"]
    assert int((c["prob"] == thr).sum()) == 50 and int((c["prob"] == np.nextafter(thr, F32(1))).sum()) == 50
    assert cases["one_small"]["prob"].max() == 1.0 and int((cases["one_large"]["prob"] == 1.0).sum()) == 3
    assert O.nms_bin(F32(1.0)) == 2047 and O.nms_sub(F32(1.0), 2047) == 2047
    # word boundaries: exactly the named ranks are kept
    for sname in (0, 63, 64):
        c = cases[f"words_visible_{sname}"]
        ranked = np.sort(c["prob"][c["prob"] > thr])[::-1]
        assert [float(r[0]) for r in rows_of(f"words_visible_{sname}")] == [float(ranked[r]) for r in c["kept_ranks"]]
    # zero-area boxes all survive
    c = cases["zero_area"]
    rows = np.asarray(rows_of("zero_area"), F32)
    zero = (rows[:, 1] == rows[:, 3]) | (rows[:, 2] == rows[:, 4])
    assert int(zero.sum()) == c["zero_area"] == int(((c["boxes"][:, 0] == c["boxes"][:, 2]) | (c["boxes"][:, 1] == c["boxes"][:, 3]))[c["prob"] > thr].sum())
    assert set(O.BATCH3) <= set(cases)


def test_near_threshold_pairs_fall_inside_and_outside_the_band(S, cases):
    """the pairs' float32 IoU (the kernel's operation order) against the 1e-5 band in which jaccard_above divides:
    most of the 200 pairs lie inside it, with kept and suppressed pairs inside AND outside, and one at (float)0.45"""
    c = cases["near_threshold"]
    idx = np.nonzero(c["prob"] > F32(S.CONF_THRESHOLD))[0]
    idx = idx[np.argsort(-c["prob"][idx], kind="stable")]
    tall, short = idx[:c["pairs"]], idx[c["pairs"]:]
    b = c["boxes"]
    tally = {(i, s): 0 for i in (True, False) for s in (True, False)}
    exact = shortcut_flips = 0
    for a, o in zip(tall, short):
        assert b[a][0] == b[o][0] and b[a][2] == b[o][2]                       # the pair shares its column
        inter = F32(b[a][2] - b[a][0]) * F32(min(b[a][3], b[o][3]) - max(b[a][1], b[o][1]))
        uni = F32(F32(ssd_ref._area(b[a])) + F32(ssd_ref._area(b[o]))) - inter
        q = F32(inter / uni)
        assert float(q) == ssd_ref.jaccard(b[a], b[o])
        tally[(bool(abs(q - O.NMS32) <= F32(1e-5)), float(q) > S.NMS_THRESHOLD)] += 1
        exact += q == O.NMS32
        # the shortcut jaccard_above takes OUTSIDE the band, applied inside it with a correctly rounded reciprocal
        shortcut_flips += (F32(inter * F32(F32(1) / uni)) > O.NMS32) != (float(q) > S.NMS_THRESHOLD)
    print("near-threshold pairs (inside band, suppressed) -> count:", tally)
    assert tally[(True, True)] + tally[(True, False)] >= 150
    print("pairs a kernel without the division fallback would decide differently (correctly rounded reciprocal):", shortcut_flips)
    assert min(tally.values()) >= 15 and exact >= 1 and shortcut_flips >= 3
    rows = ssd_ref.detection_output(b, c["prob"], S.CONF_THRESHOLD, S.NMS_THRESHOLD, S.TOP_K, 10 ** 6)
    assert len(rows) == c["pairs"] + tally[(True, False)] + tally[(False, False)]


def test_head_case_is_distinct_and_clear_of_the_threshold(S):
    heads, loc, conf = O.head_case(S)
    flat = O.flat_heads(heads)
    assert flat.size == 3 * O.P * 6 and len(np.unique(loc)) == loc.size and abs(loc).max() <= 4 and abs(conf[1:]).max() <= 6
    assert len(np.unique(conf)) >= conf.size - 2 * len(O.PLANTED)
    assert np.array_equal(flat, O.flat_heads(heads, (0, 1, 2)))
    l2, c2 = O.split_heads(heads, S, 3)
    assert np.array_equal(l2, loc) and np.array_equal(c2, conf)
    pri = ssd_ref.prior_boxes(S.SOURCES, S.INPUT)
    planted = {k: i for k, (i, _) in O.PLANTED.items()}
    thr = float(F32(S.CONF_THRESHOLD))
    for img in range(3):
        _, p64, _ = O.decode64(pri, loc[img], conf[img], S.VARIANCES)
        _, p32 = O.decode32(pri, loc[img], conf[img], S.VARIANCES)
        near = np.nonzero(np.abs(p64 - thr) < 1e-6)[0]
        assert set(near) <= ({planted["thr_above"], planted["thr_below"]} if img == 0 else set()), (img, near, p64[near])
        if img == 0:
            assert p64[planted["thr_above"]] > thr + 1e-6 > thr - 1e-6 > p64[planted["thr_below"]]      # 2e-6 either side
            assert abs(p64[planted["thr_above"]] - thr) < 3e-6 and abs(p64[planted["thr_below"]] - thr) < 3e-6
            assert p32[planted["half"]] == 0.5 and p32[planted["sat_hi30"]] == 1.0 and p32[planted["sat_hi100"]] == 1.0
            assert 0 < p64[planted["sat_lo30"]] < 1e-12 and p32[planted["sat_lo100"]] < 1e-40     # a float32 denormal, or 0 where they flush


def test_the_bar_sees_a_dropped_weight_plane_and_a_clamp_off_by_one(pkg, S, ssd_sd):
    """What the GPU suite's bar is for, shown on the yardstick: res2a (3x3, 32 -> 32 on the 75 x 75 map) evaluated in
    fp32 with weights cut to two bf16 planes (16 significand bits - the third plane dropped) misses the bar by a wide
    margin, while the plain fp32 evaluation is the bar's unit; and a ceil-mode pool whose clamp stops one short differs
    in the last row and column, where the exact comparison looks."""
    sd32, sd64 = O.sds(pkg, ssd_sd)
    x = torch.from_numpy(np.random.RandomState(3).rand(1, 32, 75, 75).astype(F32))
    get32, get64 = (lambda k: x), (lambda k: x.double())
    w = sd32["res2a.weight"]
    hi = w.bfloat16().float()
    two = hi + (w - hi).bfloat16().float()                                       # planes 1 + 2 of the exact three-way split
    cut = dict(sd32, **{"res2a.weight": two})
    ref, u = O.layer("res2a", get64, sd64, S), O.scale("res2a", get64, sd64, S)
    ok = O.compare("res2a", O.layer("res2a", get32, sd32, S).double(), ref, O.layer("res2a", get32, sd32, S), u)
    bad = O.compare("res2a", O.layer("res2a", get32, cut, S).double(), ref, O.layer("res2a", get32, sd32, S), u)
    print(f"two-plane weights: error / bar = {bad['ratio']:.1f} (plain fp32: {ok['ratio']:.2f})")
    assert ok["ratio"] <= 1.0 < 2.0 < bad["ratio"]
    y = torch.relu(torch.from_numpy(np.random.RandomState(4).randn(1, 32, 150, 150).astype(F32)))
    good = F.max_pool2d(y, 3, 2, 0, ceil_mode=True)
    y2 = y.clone()
    y2[:, :, 149], y2[:, :, :, 149] = y2[:, :, 148], y2[:, :, :, 148]           # the clamp at H - 2 instead of H - 1
    short = F.max_pool2d(y2, 3, 2, 0, ceil_mode=True)
    assert good.shape == short.shape == (1, 32, 75, 75) and not torch.equal(good[:, :, -1], short[:, :, -1])

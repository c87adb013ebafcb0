"""CPU: the single-call split-GEMM oracle (tests/gemm_oracle.py) and the teeth of the checks tests/test_gemm_direct_gpu.py
asserts with it.

`emulate` restates the kernels' arithmetic in float64 (three bf16 terms per operand, the six products with i + j <= 2,
the sum rounded to fp32).  Unmutated, it must pass what the GPU test asserts - the fp32 bars on every input family at
every pointwise shape of the GPU test, bit-equality with float64 on the exact families.  Each mutant - a mistake a kernel
could make - must FAIL at least one of those checks at a named case, and that case must be among the calls the GPU test
makes (gemm_oracle.CASES).  Witnesses (family, K; what fails there):
  drop w0 x0 / w0 x1 / w0 x2     exact_x at K = 16 (pw6 / pw7 shape M = 129, N = 30): not bit-equal to float64
  drop w1 x0 / w2 x0             exact_w at K = 16 (same shape): not bit-equal
  drop w1 x1                     cancel at K = 16 (M = 129, N = 2) and K = 24 (N = 10): the output lives in the low-order
                                 terms, rms and max bars; exact_* cannot see it (x1 or w1 is zero there)
  gate row of image +-1          gated random, K = 96, HW = 49, M = 147
  K tail against non-zero weights   random, K = 40, N = 30 (one re-read octet) and K = 24
  residual on the wrong side     random with swish and a residual behind it: K = 72, N = 64 and K = 16, N = 2
  last row stored over row M - 2 random, K = 16, N = 2, M = 129
"""
import dataclasses

import numpy as np
import pytest
import torch

import gemm_oracle as G


def _find(**kw):
    hits = [c for c in G.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    assert hits, f"the GPU test has no case with {kw}"
    return hits[0]


def _fp32_pointwise_shapes():
    """the distinct (M, K, N, HW, gated) of every fp32 non-conv call of the GPU test"""
    seen = {}
    for c in G.CASES:
        if c.conv is None and not c.bf16:
            seen.setdefault((c.M, c.K, c.N, c.HW, c.gated), c)
    return list(seen.values())


def test_case_list_covers_what_it_claims():
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names)
    pw = [c for c in G.CASES if c.group == "pointwise" and c.family == "random"]
    assert {(c.M, c.K, c.N) for c in pw} == {(m, k, n) for m in G.PW_M for k, n in G.PW_KN}
    for a in G.ACTS:
        for r in G.RESIDUALS:
            assert {c.N % 4 == 0 for c in pw if c.act == a and c.res == r} == {True, False}, (a, r)
    p8 = [c for c in G.CASES if c.group == "pw8"]
    assert {c.K for c in p8 if not c.gated and not c.bf16} == set(G.PW8_K) and {c.N for c in p8} == set(G.PW8_N)
    assert {(c.K, c.M) for c in p8 if not c.gated and not c.bf16} == {(k, m) for k in G.PW8_K for m in G.PW8_M}
    assert {(c.K, c.HW) for c in p8 if c.gated and not c.bf16} >= {(k, hw) for k in G.PW8_K for hw in (16, 64)}
    assert {c.HW for c in p8 if c.gated} == {16, 64, 80, 144}
    assert all(c.M == 5 * c.HW for c in p8 if c.gated)
    assert {c.res for c in p8 if not c.gated and not c.bf16} == {None, "after"}
    assert {(c.bf16, c.planes) for c in p8} == {(False, 3), (True, 3), (True, 1)} and any(c.bf16 and c.gated for c in p8)
    p9 = [c for c in G.CASES if c.group == "pw9"]
    assert {(c.M, c.K, c.N) for c in p9} == {(m, k, n) for m in G.PW9_M for k, n in G.PW9_KN}
    assert all({c.act for c in p9 if c.K == k} == {None, "swish"} for k, _ in G.PW9_KN)
    gt = [c for c in G.CASES if c.group == "gated"]
    assert {(c.HW, c.M, c.K, c.N) for c in gt} == {(hw, m, k, n) for hw in G.GATED_HW for m in (3 * hw, 3 * hw - 5) if m > 0
                                                     for k, n in G.GATED_KN}
    cv = [c for c in G.CASES if c.group == "conv"]
    for i, vals in ((0, {3}), (3, {32, 64}), (4, {1, 2, 3}), (5, {1, 2}), (6, {0, 1}), (7, {1, 2})):
        assert {c.conv[i] for c in cv} == vals, i
    assert {(c.conv[1], c.conv[2]) for c in cv} == {(5, 7), (9, 6)} and {c.N for c in cv} == {10, 64}
    assert {c.act for c in cv} == {"prelu", "relu"} and {c.res for c in cv} == {"first", "after"}
    assert {(c.act, c.res) for c in cv} == {(a, r) for a in ("prelu", "relu") for r in ("first", "after")}
    assert all(c.HW % 16 != 0 for c in cv), "Ho * Wo must never be a multiple of 16"
    assert {(c.conv[4], c.conv[7]) for c in cv} >= {(3, 2), (2, 2), (3, 1)}              # dilation on a real k x k kernel
    bf = [c for c in G.CASES if c.group == "bf16"]
    assert {c.planes for c in bf} == {1, 3} and any(c.gated for c in bf) and any(not c.gated for c in bf)
    ex = [c for c in G.CASES if c.group == "exact"]
    assert {(c.family, c.K) for c in ex} >= {(f, k) for f in ("exact_x", "exact_w") for k in (16, 32)}
    assert {c.expect for c in ex} == {"", "pw8", "pw9"}


def test_exact_families_are_exact_in_every_term():
    """every partial sum of every term product is an integer below 2^24; at K = 16 (18-bit integers) all three terms of the
    wide operand carry bits, at K = 32 (17 bits) two do: round-to-nearest terms are signed, 8 + 9 bits fit two of them"""
    for c in (c for c in G.CASES if c.group == "exact"):
        inp = G.make_inputs(c)
        x, w = torch.from_numpy(inp["x"]).double(), torch.from_numpy(inp["w"]).double()
        xs, ws = G.split3(x), G.split3(w)
        assert torch.equal(xs[0] + xs[1] + xs[2], x) and torch.equal(ws[0] + ws[1] + ws[2], w)
        bound = sum(t.abs() for t in xs) @ sum(t.abs() for t in ws).t() + torch.from_numpy(inp["bias"]).double().abs()
        assert float(bound.max()) < 2.0 ** 24, c.name
        wide = xs if c.family == "exact_x" else ws
        assert all(float(t.abs().max()) > 0 for t in wide[:3 if c.K <= 16 else 2]), c.name
        assert float((x if c.family == "exact_x" else w).abs().max()) < 2.0 ** 24 / (4 * c.K)


def test_emulation_passes_every_family_at_every_pointwise_shape():
    worst = {}
    for base in _fp32_pointwise_shapes():
        for fam in G.FAMILIES:
            exact = fam.startswith("exact")
            c = dataclasses.replace(base, family=fam, group="oracle", act=None if exact else base.act)
            ref = G.Reference(c)
            m = ref.check(G.emulate(c, ref.inp).numpy())
            assert m["ratio"] <= 1.0, (c.name, m)
            if exact and not c.gated:
                assert m["exact"], c.name
            worst[fam] = max(worst.get(fam, 0.0), m["vs_yard"])
    print("emulation / yardstick, worst per family:", {k: round(v, 3) for k, v in worst.items()})


# mutant -> the witnesses: keyword filters into gemm_oracle.CASES
_EXACT_X = dict(group="exact", family="exact_x", K=16, N=30)
_EXACT_W = dict(group="exact", family="exact_w", K=16, N=30)
_CANCEL = (dict(family="cancel", K=16), dict(family="cancel", K=24))
WITNESSES = {
    "drop_w0x0": (_EXACT_X, _EXACT_W), "drop_w0x1": (_EXACT_X,), "drop_w0x2": (_EXACT_X,),
    "drop_w1x0": (_EXACT_W,), "drop_w2x0": (_EXACT_W,), "drop_w1x1": _CANCEL,
    "gate_prev": (dict(group="gated", K=96, HW=49, M=147),), "gate_next": (dict(group="gated", K=96, HW=49, M=147),),
    "tail": (dict(group="pointwise", family="random", K=40, N=30, M=129), dict(group="pointwise", family="random", K=24, M=129)),
    "res_side": (dict(group="pointwise", family="random", K=72, act="swish", res="after"),
                 dict(group="pointwise", family="random", K=16, act="swish", res="after")),
    "dup_row": (dict(group="pointwise", family="random", K=16, M=129),),
}


def test_every_mutant_has_a_witness():
    assert set(WITNESSES) == set(G.MUTANTS)


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_mutant_fails_an_asserted_check_at_a_case_the_gpu_test_runs(mutant):
    for kw in WITNESSES[mutant]:
        c = _find(**kw)
        ref = G.Reference(c)
        assert ref.passes(G.emulate(c, ref.inp).numpy()), f"{c.name}: the unmutated emulation must pass"
        m = ref.check(G.emulate(c, ref.inp, mutant).numpy())
        assert m["ratio"] > 1.0 or not m.get("exact", True), f"{mutant} survives {c.name}: {m}"


def test_low_order_drops_fail_the_bars_without_the_exact_check():
    """the low-order activation terms also fail the fp32 bars alone on the cancel family at K = 16 and 24 (the weights
    cancel exactly there, so their own low terms drop out of the result: exact_w is what sees those)"""
    for kw in _CANCEL:
        c = _find(**kw)
        ref = G.Reference(c)
        for mutant in ("drop_w1x1", "drop_w0x2"):
            assert ref.check(G.emulate(c, ref.inp, mutant).numpy())["ratio"] > 1.0, (mutant, c.name)


def test_bf16_mirror_rounds_where_the_kernel_rounds():
    c = _find(group="bf16", gated=True, planes=1)
    inp = G.make_inputs(c)
    for a in (inp["x"], inp["res"]):
        assert a is None or np.array_equal(G.from_bits(G.to_bits(a)), a)          # bf16 values survive the bit round trip
    mir = G.mirror(c, inp)
    assert np.array_equal(G.from_bits(G.to_bits(mir.float().numpy())), mir.float().numpy())      # a bf16 tensor
    ref = G.Reference(c, inp)
    assert ref.check(G.to_bits(mir.float().numpy()))["ratio"] == 0.0
    # a mirror that keeps the fp32 weights and the unrounded gated operand (planes = 1, gated) is past the bar
    wrong = G.B.rne_bf16(G.evaluate(c, inp, torch.float64))
    assert ref.check(G.to_bits(wrong.float().numpy()))["ratio"] > 1.0

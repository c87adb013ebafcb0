"""GPU: the head trainer (csrc/head_train.hip, dfd_head_train_*) against the float64 oracle across its settings and its row
range - one test per row of tests/head_train_cases.py, written like test_head_train_gpu.test_one_accumulate_matches_float64:
open the trainer, run both oracles, assert the preconditions on them (H.figures: gate margin >= 1 and what the case adds),
only then call the device, print every figure, require `O.bar_ratio` <= 1 for every tensor.  No tolerance of its own: the
bars are b0_layer_oracle's 4 x / 8 x over the float32 CPU oracle, floored at 2^-23 / 2^-21, as in every file of this
family.  Masks, the dropout-0 activations and the degenerate batch's BatchNorm outputs are compared exactly.  No element
is left out of any comparison.

What test_head_train_gpu.py ran before this file: dropout 0.5, gamma 2 / 0, alpha 0.25, smoothing 0.1 / 0, one weight
decay, default betas / eps / momentum, n <= 64 - so only the first 16-row tile of each wave in slab_gemm_xwt,
slab_gemm_dyw and the layer kernels.  Here: every float field of dfd_head_config away from its default, both ends of
every accepted range, n = 15, 17, 63, 65, 80, 129, 241, 255 and 256 in accumulate and in eval, twelve applies compared
step by step, and the saturated branches of focal_term.  tests/test_head_train_cases.py (CPU) shows which defect each
group catches; of its fourteen the old suite could not see two at all - a lost tile of the column statistics and of
the dY . W product (rows 64 and up).

The saturated cases are teacher-forced: at |logit| = 20 .. 90 torch's 1 - sigmoid(z) has no digits left in float64
either, so the reference is H.focal_restated (float64 numpy, cancellation-free; shown on the CPU to be O.focal and its
autograd to 1e-12) on the device's own logits and fc3 inputs, the yardstick the same in numpy float32.

Measured on one MI355X (worst `bar_ratio` per group, <= 1 passes; the device's own rows gave the recorded margins):
  group      cases                                                       worst ratio   where
  settings   34 accumulates at n = 16 / 37 and the degenerate batch      0.827         dropout-0.2-n16, grad b3
  rows       9 accumulates and 9 evals (live and EMA), n = 15 .. 256     0.165         rows-acc-n256, grad b3
  apply      12 cases x 12 steps, norm + 10 parameters + 10 shadows      0.698         apply-betas-0.5-0.9, param b3
  saturated  2 settings x 6 values of b3, loss + grad b3 + grad w3       0.155         saturated-defaults, loss
  stages     7 conv and 7 block cases, accumulate + three applies        0.757         block-dropout-0.2, param b3
Gate margins with the MI355X host's BLAS (recorded ones, from the authoring host, in H.RECORDED): 8.9 .. 130 for the
settings cases, 3585 for the degenerate batch; one accumulate 62, 43, 10, 12, 15, 5.3, 2.7, 3.0 and 1.36 at n = 15, 17,
63, 65, 80, 129, 241, 255 and 256; eval 5.2 or more at every n.  Stage cases on the device's own rows (bit-equal to
tests/golden/head_train_stage_rows.npz): conv margins 33 .. 73, rounding shares 0.24 .. 0.47; block margins 29 .. 116,
rounding shares 0.24 .. 0.40, storage shares 0.05 .. 0.12.
Run time: the file's 96 tests take 18 s on one MI355X, of which 1 s opens the two handles and 6 s are the twelve
12-step apply cases (24 exports of 790 k floats each); no other test reaches 0.5 s.
No case failed on the device: this file found no kernel bug.  What it did find is on the host side - dfd_head_train_begin
let a NaN focal_alpha, an infinite eps / clip_norm / focal_gamma and any weight_decay through, the accumulate entries
any lam and loss_scale - and those calls are refused now (test_new_refusals_*).
"""
import time

import numpy as np
import pytest

import b0_layer_oracle as B
import block15_train_oracle as BO
import head_train_cases as H
import head_train_oracle as O
import headconv_train_oracle as CO
from rtdfd_amd import head_training as T

pytestmark = pytest.mark.gpu

WORST = {}                                                      # group -> (ratio, case, tensor), printed by the last test


@pytest.fixture(scope="module")
def th(pkg, seeded_sd):
    """the handle the trainers of this module open on (classifier only)"""
    t0 = time.perf_counter()
    h = pkg._lib.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=2)
    print(f"handle opened in {time.perf_counter() - t0:.2f} s")
    yield h
    h.close()


def _open(pkg, h, case, params):
    cfg = pkg._lib.head_config(**case.library_kwargs())
    held = O.config_values(cfg)
    assert held == case.config(), (held, case.config())         # the table's defaults are the library's
    h.head_train_begin(params, cfg)
    return held


def _show(name, r):
    print(f"{name}: rms {r['rms']:.3e} (yard {r['yard_rms']:.3e}) max {r['max']:.3e} (yard {r['yard_max']:.3e}) ratio {r['ratio']:.3f}")


def _require(case, got, ref, yard):
    ratio, where = H.worst(got, ref, yard, _show)
    if not ratio <= WORST.get(case.group, (0.0,))[0]:
        WORST[case.group] = (ratio, case.name, where)
    print(f"{case.name}: worst ratio {ratio:.3f} at {where}")
    assert ratio <= 1.0, (case.name, where, ratio)


def _preconditions(case):
    fig = H.figures(case)
    print(f"{case.name}: " + ", ".join(f"{k} {v}" for k, v in fig.items() if k not in ("ref", "yard", "o64", "o32")) +
          f" (recorded margin {case.margin}, {case.qualified} of 250 seeds qualified)")
    assert fig["ok"]                                            # conditions on the inputs, checked on the oracles alone
    return fig


def _masks_follow(h, case, counter):
    rates = T.dropout_rates(case.config()["dropout"])
    for layer, (w, p) in enumerate(zip(T.LAYER_WIDTHS, rates)):
        got = h.head_train_tap(f"mask{layer}", case.n)
        assert set(np.unique(got)) <= {0.0, 1.0}
        assert np.array_equal(got > 0.5, T.dropout_keep_mask(case.seed, counter, layer, case.n, w, p)), (case.name, counter, layer)
    return rates


# --------------------------------------------------------------------------- 1. one accumulate: settings, rows
@pytest.mark.parametrize("case", H.SETTINGS_CASES + [H.DEGENERATE_CASE] + H.ROWS_ACC_CASES, ids=lambda c: c.name)
def test_one_accumulate_matches_float64(pkg, th, case):
    fig = _preconditions(case)
    params, x, ya, yb, lam, scale = H.acc_inputs(case)
    _open(pkg, th, case, params)
    try:
        loss, logits = th.head_train_accumulate(x, ya, yb, lam, scale)
        got = {"loss": np.array([loss]), "logits": logits, "z1": th.head_train_tap("z1", case.n), "z2": th.head_train_tap("z2", case.n)}
        got.update({"grad " + k: v for k, v in th.head_train_grads().items()})
        e = th.head_train_export()
        got.update({k: e[k] for k in O.STAT_FIELDS})
        rates = _masks_follow(th, case, 0)                      # all three layers, every n
        x0, a1, a2 = (th.head_train_tap(k, case.n) for k in ("x0", "a1", "a2"))
        if rates[0] == 0.0:                                     # every mask all ones, the scale exactly 1
            assert all(th.head_train_tap(f"mask{l}", case.n).all() for l in range(3))
            assert np.array_equal(x0, x)
            assert np.array_equal(a1, np.maximum(got["z1"], 0.0)) and np.array_equal(a2, np.maximum(got["z2"], 0.0))
        else:                                                   # relu(z) * keep * (float) 1 / (1 - p), one rounding
            for a, src, layer in ((x0, x, 0), (a1, np.maximum(got["z1"], 0.0), 1), (a2, np.maximum(got["z2"], 0.0), 2)):
                keep = th.head_train_tap(f"mask{layer}", case.n) > 0.5
                assert np.array_equal(a, np.where(keep, src * np.float32(1.0 / (1.0 - rates[layer])), np.float32(0.0)))
        if case.variant == "degenerate":                        # variance exactly 0: z = beta, nothing added to (1 - m) rv
            m = np.float32(case.config()["bn_momentum"])
            for z, be, rv in (("z1", "be1", "rv1"), ("z2", "be2", "rv2")):
                assert np.array_equal(got[z], np.broadcast_to(params[be], got[z].shape))
                assert np.array_equal(got[rv], np.full_like(got[rv], np.float32(1.0) - m))
        _require(case, got, fig["ref"], fig["yard"])
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 2. masks at the largest rate
@pytest.mark.parametrize("case", H.MASK_CASES, ids=lambda c: c.name)
def test_masks_at_the_largest_float_below_one(pkg, th, case):
    """thr = floor(p 2^32) = 2^32 - 256 and 1 / (1 - p) = 2^24 in layer 0; 0.7 p and 0.5 p behind it"""
    x, y = O.features(case.n, case.n), H.labels(case.n, case.n)
    _open(pkg, th, case, O.default_params(1))
    try:
        for counter in range(2):
            loss, logits = th.head_train_accumulate(x, y)
            assert np.isfinite(loss) and np.isfinite(logits).all()
            _masks_follow(th, case, counter)
            keep = th.head_train_tap("mask0", case.n) > 0.5
            assert np.array_equal(th.head_train_tap("x0", case.n), np.where(keep, x * np.float32(2.0 ** 24), np.float32(0.0)))
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 3. eval over the row range
@pytest.mark.parametrize("case", H.ROWS_EVAL_CASES, ids=lambda c: c.name)
def test_eval_matches_float64_and_any_chunking(pkg, th, case):
    fig = _preconditions(case)
    params, x, y, g, held = H.eval_inputs(case)
    _open(pkg, th, case, params)
    try:
        th.head_train_accumulate(x, y)
        th.head_train_grads(set_to=g)
        th.head_train_apply(H.EVAL_LR)                          # live and EMA parameters differ from here on
        got = {}
        for ema in (False, True):
            whole = th.head_train_eval(held, ema)
            got["eval logits, " + ("ema" if ema else "live")] = whole.copy()
            for chunk in (1, 64, 65):
                parts = np.concatenate([th.head_train_eval(held[i:i + chunk], ema) for i in range(0, case.n, chunk)])
                assert np.array_equal(parts, whole), (chunk, ema)
        assert not np.array_equal(got["eval logits, live"], got["eval logits, ema"])
        _require(case, got, fig["ref"], fig["yard"])
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 4. twelve applies, step by step
@pytest.mark.parametrize("case", H.APPLY_CASES, ids=lambda c: c.name)
def test_twelve_applies_match_adamw_and_ema(pkg, th, case):
    fig = _preconditions(case)
    print("forced norms", [round(v, 3) for v in fig["norms"]], "clip_norm", case.config()["clip_norm"])
    _open(pkg, th, case, O.default_params(H.APPLY_PARAM_SEED))
    try:
        for step, lr in enumerate(H.apply_lrs(case)):
            th.head_train_grads(set_to=H.forced_grads(H.APPLY_GRAD_SEED + step))
            got = {"grad norm": np.array([th.head_train_apply(lr)])}
            assert all(not v.any() for v in th.head_train_grads().values())     # zeroed exactly
            for ema in (False, True):
                e = th.head_train_export(ema)
                got.update({("ema " if ema else "param ") + k: e[k] for k in O.GRAD_FIELDS})
            print(f"-- step {step}, lr {lr:g}")
            _require(case, got, fig["ref"][step], fig["yard"][step])
            if case.name == "apply-lr-0":                       # nothing moves: decay 1 - 0 wd, step size 0
                start = O.default_params(H.APPLY_PARAM_SEED)
                assert all(np.array_equal(got["param " + k].ravel(), start[k].ravel()) for k in O.GRAD_FIELDS)
            if case.name == "apply-ema-1":                      # the shadow never moves
                start = O.default_params(H.APPLY_PARAM_SEED)
                assert all(np.array_equal(got["ema " + k].ravel(), start[k].ravel()) for k in O.GRAD_FIELDS)
            if case.name == "apply-ema-0":                      # the shadow is the parameter
                assert all(np.array_equal(got["ema " + k], got["param " + k]) for k in O.GRAD_FIELDS)
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 5. saturated loss, teacher-forced
@pytest.mark.parametrize("b3", H.SATURATED_B3)
@pytest.mark.parametrize("case", H.SATURATED_CASES, ids=lambda c: c.name)
def test_saturated_loss_keeps_both_tails(pkg, th, case, b3):
    params, x, ya = H.saturated_inputs(case, b3)
    assert 0.0 < ya.mean() < 1.0                                # labels of both classes
    cfg = _open(pkg, th, case, params)
    try:
        loss, logits = th.head_train_accumulate(x, ya)
        g = th.head_train_grads()
        z2, keep, a2 = th.head_train_tap("z2", case.n), th.head_train_tap("mask2", case.n) > 0.5, th.head_train_tap("a2", case.n)
        scale = np.float32(1.0 / (1.0 - T.dropout_rates(cfg["dropout"])[2]))
        assert np.array_equal(a2, np.where(keep, np.maximum(z2, 0.0) * scale, np.float32(0.0)))    # fc3's input is what the taps say
        off = float(np.abs(logits - b3).max())
        print(f"{case.name}, b3 {b3:g}: logits {logits.min():.3f} .. {logits.max():.3f}")
        assert off < 2.0                                        # the logits sit where the case wants them
        got = {"loss": np.array([loss]), "grad b3": g["b3"], "grad w3": g["w3"]}
        ref, yard = H.saturated_reference(logits, a2, ya, cfg, np.float64), H.saturated_reference(logits, a2, ya, cfg, np.float32)
        assert all(np.isfinite(v).all() for v in got.values()) and float(ref["loss"][0]) > 0.0
        _require(case, got, ref, yard)
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 6. the new refusals
def test_new_refusals_leave_the_trainer_as_it_was(pkg, th):
    """dfd_head_train_begin: NaN / infinity in any float field, negative weight_decay; _accumulate: NaN lam or loss_scale,
    lam outside [0, 1]; _apply: NaN or negative lr.  DFD_ERR_ARG with a message, and the calls around them give the bits
    of a run without them."""
    L = pkg._lib
    params, x, y, yb = O.default_params(0), O.features(0, 5), H.labels(0, 5), H.labels(1, 5)
    nan, inf = float("nan"), float("inf")

    def refused(fn, *a, **k):
        with pytest.raises(L.DfdError) as e:
            fn(*a, **k)
        assert e.value.code == -1 and len(str(e.value)) > 30, str(e.value)     # DFD_ERR_ARG with a message

    def run(with_refusals):
        if with_refusals:
            for field in H.DEFAULTS:
                for bad in (nan, inf, -inf):
                    refused(th.head_train_begin, params, L.head_config(max_n=8, **{field: bad}))
            refused(th.head_train_begin, params, L.head_config(max_n=8, weight_decay=-1e-3))
        for alpha in ((-0.5, 1.5, 0.25) if with_refusals else (0.25,)):        # any finite focal_alpha stays accepted
            th.head_train_begin(params, L.head_config(max_n=8, seed=3, focal_alpha=alpha))
            if alpha != 0.25:
                th.head_train_end()
        try:
            out = [th.head_train_accumulate(x, y, yb, 0.3, 0.5)]
            if with_refusals:
                for lam, scale in ((nan, 1.0), (1.0, nan), (-0.01, 1.0), (1.01, 1.0), (inf, 1.0), (-inf, 1.0)):
                    refused(th.head_train_accumulate, x, y, yb, lam, scale)
                    refused(th.head_train_accumulate, x, y, None, lam, scale)
            out.append(th.head_train_accumulate(x, yb, y, 1.0, 2.0))            # the counter did not move: same masks
            out.append(tuple(th.head_train_tap(f"mask{l}", 5) for l in range(3)))
            out.append(th.head_train_grads())
            if with_refusals:
                for lr in (nan, -1e-3, -inf):
                    refused(th.head_train_apply, lr)
            out.append(th.head_train_apply(1e-3))                               # the step number did not move either
            out.append(th.head_train_export(False))
            out.append(th.head_train_export(True))
            out.append(th.head_train_eval(x, True))
            return out
        finally:
            th.head_train_end()

    def flat(v):
        if isinstance(v, dict):
            return [a for k in sorted(v) for a in flat(v[k])]
        if isinstance(v, (tuple, list)):
            return [a for e in v for a in flat(e)]
        return [np.asarray(v)]

    clean, again = flat(run(False)), flat(run(True))
    assert len(clean) == len(again) and all(np.array_equal(a, b) for a, b in zip(clean, again))
    assert all(np.isfinite(a).all() for a in clean)


# --------------------------------------------------------------------------- 7. the settings that reach the conv and block stages
@pytest.fixture(scope="module")
def stress_sd():
    return B.stress_state_dict(0)


@pytest.fixture(scope="module")
def conv0(stress_sd):
    return CO.conv_params(stress_sd)


@pytest.fixture(scope="module")
def block0(stress_sd):
    return BO.block_params(stress_sd)


@pytest.fixture(scope="module")
def sh(pkg, stress_sd):
    """stress weights, classifier only: the handle of test_headconv_train_gpu.py and test_block15_train_gpu.py"""
    h = pkg._lib.Handle(pkg.weights.pack_b0(stress_sd), device=0, max_batch=16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def stage_rows(sh):
    """the first rows of those files' real-row fixtures (their first extraction call)"""
    x = B.random_crops(37, 42)[:16]
    return {"conv": sh.extract_trunk(x)[:H.STAGE_N].copy(), "block": sh.extract_trunk(x, block=14)[:H.STAGE_N].copy()}


def _stage_state(h, case, ema=None):
    """gradients (ema None) or parameters and statistics, under the oracles' names"""
    parts = [("", h.head_train_grads() if ema is None else h.head_train_export(ema)),
             ("conv.", h.head_train_conv_grads() if ema is None else h.head_train_export_conv(ema))]
    if case.stage == "block":
        parts.append(("b15.", h.head_train_block_grads() if ema is None else h.head_train_export_block(ema)))
    return {p + k: v for p, d in parts for k, v in d.items()}


def _is_stat(k):
    return k.split(".")[-1].startswith(("rm", "rv"))


@pytest.mark.parametrize("case", H.STAGE_CASES, ids=lambda c: c.name)
def test_stage_settings_match_float64(pkg, sh, conv0, block0, stage_rows, case):
    rows, head, ya = stage_rows[case.stage], O.default_params(case.seed), H.labels(case.seed + 200, case.n)
    fig = H.stage_figures(case, rows, conv0, block0)
    print(f"{case.name}: on the device's rows " + ", ".join(f"{k} {fig[k]:.3f}" for k in ("margin", "rounding", "storage") if k in fig) +
          f" (on the rows of tests/golden, bit-equal to these: {np.array_equal(rows, H.golden_rows(case.stage))}: {case.margin}, {case.rounding}, {case.storage}; {case.qualified} of 250 seeds qualified)")
    assert fig["ok"]                                            # conditions on the inputs, checked on the oracles alone
    cfg = pkg._lib.head_config(**case.library_kwargs())
    assert O.config_values(cfg) == case.config()
    kw = dict(case.stage_kw)
    sh.head_train_begin(head, cfg)
    try:
        sh.head_train_unfreeze_conv(conv0, **kw)
        if case.stage == "block":
            sh.head_train_unfreeze_block(block0, **{k: v for k, v in kw.items() if k != "lr_scale"})
            loss, logits = sh.head_train_accumulate_block(rows, ya)
        else:
            loss, logits = sh.head_train_accumulate_trunk(rows, ya)
        got = {"loss": np.array([loss]), "logits": logits}
        got.update({k: sh.head_train_tap(k, case.n) for k in H.stage_taps(case)})
        got.update({"grad " + k: v for k, v in _stage_state(sh, case).items()})
        got.update({k: v for k, v in _stage_state(sh, case, False).items() if _is_stat(k)})
        start = {k: v.copy() for k, v in _stage_state(sh, case, False).items() if not _is_stat(k)}
        _require(case, got, fig["ref"]["acc"], fig["yard"]["acc"])
        got = {}
        for step, lr in enumerate(H.STAGE_APPLY_LRS):
            g = H.stage_forced_grads(case, 50 + step)
            sh.head_train_grads(set_to={k: g[k] for k in O.GRAD_FIELDS})
            sh.head_train_conv_grads(set_to={k: g["conv." + k] for k in CO.CONV_GRAD_FIELDS})
            if case.stage == "block":
                sh.head_train_block_grads(set_to={k: g["b15." + k] for k in BO.BLOCK_GRAD_FIELDS})
            got[f"grad norm, step {step}"] = np.array([sh.head_train_apply(H.f32(lr))])
            assert all(not v.any() for v in _stage_state(sh, case).values())   # zeroed exactly, every group
        for ema in (False, True):
            got.update({("ema " if ema else "param ") + k: v for k, v in _stage_state(sh, case, ema).items() if not _is_stat(k)})
        print("-- three forced applies")
        _require(case, got, fig["ref"]["apply"], fig["yard"]["apply"])
        moved = {k: not np.array_equal(got["param " + k], start[k]) for k in start}
        if dict(case.stage_kw).get("lr_scale") == 0.0:          # rate 0: decay 1 - 0 wd, step 0 - the stages stand still, the head moves
            assert not any(v for k, v in moved.items() if "." in k) and all(v for k, v in moved.items() if "." not in k)
        else:
            assert all(moved.values())
    finally:
        sh.head_train_end()


def test_new_refusals_in_the_stages(pkg, sh, conv0, block0, stage_rows):
    """dfd_head_train_accumulate_trunk / _block: NaN lam or loss_scale, lam outside [0, 1]; the calls around the refusals
    give the bits of a run without them"""
    L = pkg._lib
    head, y, yb = O.default_params(0), H.labels(0, 5), H.labels(1, 5)
    nan, inf = float("nan"), float("inf")

    def refused(fn, *a, **k):
        with pytest.raises(L.DfdError) as e:
            fn(*a, **k)
        assert e.value.code == -1 and len(str(e.value)) > 30, str(e.value)     # DFD_ERR_ARG with a message

    for stage in ("conv", "block"):
        x = stage_rows[stage]
        seen = []
        for with_refusals in (False, True):
            sh.head_train_begin(head, L.head_config(max_n=8, seed=4))
            try:
                sh.head_train_unfreeze_conv(conv0)
                if stage == "block":
                    sh.head_train_unfreeze_block(block0)
                acc = sh.head_train_accumulate_block if stage == "block" else sh.head_train_accumulate_trunk
                out = [acc(x, y, yb, 0.3, 0.5)]
                if with_refusals:
                    for lam, scale in ((nan, 1.0), (1.0, nan), (-0.01, 1.0), (1.01, 1.0), (inf, 1.0)):
                        refused(acc, x, y, yb, lam, scale)
                        refused(acc, x, y, None, lam, scale)
                    for lr in (nan, -1e-3):
                        refused(sh.head_train_apply, lr)
                out.append(acc(x, yb, y, 0.0, 2.0))
                out.append(sh.head_train_grads())
                out.append(sh.head_train_conv_grads())
                out.append(sh.head_train_apply(1e-3))
                out.append(sh.head_train_export_conv(True))
                seen.append(out)
            finally:
                sh.head_train_end()

        def flat(v):
            if isinstance(v, dict):
                return [a for k in sorted(v) for a in flat(v[k])]
            if isinstance(v, (tuple, list)):
                return [a for e in v for a in flat(e)]
            return [np.asarray(v)]

        clean, again = flat(seen[0]), flat(seen[1])
        assert len(clean) == len(again) and all(np.array_equal(a, b) for a, b in zip(clean, again)), stage
        assert all(np.isfinite(a).all() for a in clean)


def test_worst_ratio_per_group():
    """prints what the docstring records (the groups that ran in this session)"""
    for group, (ratio, name, where) in sorted(WORST.items()):
        print(f"{group}: worst ratio {ratio:.3f} in {name} at {where}")
    assert all(v[0] <= 1.0 for v in WORST.values())

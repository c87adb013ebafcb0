"""GPU: the head trainer (csrc/head_train.hip, dfd_head_train_*) against the float64 oracle of tests/head_train_oracle.py.

Bars: every compared tensor's rms(d) / rms(ref) and max|d| / max|ref| against the float64 oracle may be at most
b0_layer_oracle's RMS_FACTOR (4) x / MAX_FACTOR (8) x the same metrics of the float32 CPU oracle on the same inputs,
floored at RMS_FLOOR / MAX_FLOOR (`O.bar_ratio`: <= 1 passes).  Every figure is printed before it is asserted.

Gate precondition: ReLU gates are discrete, so each comparison case fixes a seed for which the ORACLE shows
min|z| >= 8 max|z32 - z64| in both BatchNorm outputs and the same gates in both (`O.gate_margin` >= 1), asserted before
the device is looked at, at every forward of the case.  The seeds below were picked at authoring time by that
oracle-only condition.  In the multi-step case the float32 side of the condition is teacher-forced (`_five_steps`).

Batch sizes: 2 (BatchNorm's minimum), 5 and 37 (tile and reduction tails in all three GEMM forms), 16 (one tile),
64 (several tiles).  The other settings of dfd_head_config, n = 65 .. 256 and the new argument refusals:
tests/test_head_train_config_gpu.py, on the case table of tests/head_train_cases.py.
"""
import numpy as np
import pytest
import torch

import head_train_oracle as O
from rtdfd_amd import head_training as T

pytestmark = pytest.mark.gpu

NS = (2, 5, 16, 37, 64)
GATE_SEED = {2: 0, 5: 8, 16: 11, 37: 10, 64: 2}      # of seeds 0..11 the one with the largest oracle gate margin (30+ at n <= 5, 18, 5.3, 5.2)
ACC_SEED = 7                                        # accumulation case: margins 5.9 (n = 16) and 4.4 (n = 5)
FIVE_SEED = 152                                     # five-step case: of seeds 0..249 the largest smallest margin (5.9) over its
                                                    # five accumulates and two eval forwards, teacher-forced float32 oracle
VARIANTS = {"plain": {}, "mix": {}, "bce": {"label_smoothing": 0.0, "focal_gamma": 0.0}}


@pytest.fixture(scope="module")
def th(pkg, seeded_sd):
    """the handle the trainers of this module open on (classifier only)"""
    h = pkg._lib.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=2)
    yield h
    h.close()


def _labels(seed, n):
    return (np.random.RandomState(seed).rand(n) < 0.5).astype(np.float32)


def _open(pkg, h, params, **kw):
    cfg = pkg._lib.head_config(**kw)
    h.head_train_begin(params, cfg)
    return O.config_values(cfg)


def _check(name, got, ref64, yard32, record=None):
    r = O.bar_ratio(got, ref64, yard32)
    print(f"{name}: rms {r['rms']:.3e} (yard {r['yard_rms']:.3e}) max {r['max']:.3e} (yard {r['yard_max']:.3e}) ratio {r['ratio']:.3f}")
    if record is not None:
        record.append((name, r["ratio"]))
    return r["ratio"]


def _assert_all(record):
    bad = [(k, round(v, 3)) for k, v in record if not v <= 1.0]
    assert not bad, bad


# --------------------------------------------------------------------------- 1. masks
@pytest.mark.parametrize("n", NS)
def test_masks_follow_the_specification(pkg, th, n):
    seed = 40 + n
    params, x, y = O.default_params(1), O.features(n, n), _labels(n, n)
    rates = T.dropout_rates(0.5)
    seen = []
    for attempt in range(2):                                   # a re-opened trainer repeats the sequence
        _open(pkg, th, params, max_n=64, seed=seed)
        try:
            for counter in range(2):
                th.head_train_accumulate(x, y)
                for layer, (w, p) in enumerate(zip(T.LAYER_WIDTHS, rates)):
                    got = th.head_train_tap(f"mask{layer}", n)
                    assert set(np.unique(got)) <= {0.0, 1.0}
                    want = T.dropout_keep_mask(seed, counter, layer, n, w, p)
                    assert np.array_equal(got > 0.5, want), (counter, layer)
                    seen.append(((attempt, counter, layer), got > 0.5))
        finally:
            th.head_train_end()
    d = dict(seen)
    for layer in range(3):
        assert not np.array_equal(d[(0, 0, layer)], d[(0, 1, layer)])            # consecutive accumulates differ
        assert np.array_equal(d[(0, 0, layer)], d[(1, 0, layer)]) and np.array_equal(d[(0, 1, layer)], d[(1, 1, layer)])


# --------------------------------------------------------------------------- 2. forward and backward
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", NS)
def test_one_accumulate_matches_float64(pkg, th, n, variant):
    seed = GATE_SEED[n]
    params, x, ya = O.default_params(seed), O.features(seed + 100, n), _labels(seed + 200, n)
    yb, lam = (_labels(seed + 201, n), 0.7) if variant == "mix" else (None, 1.0)
    cfg = _open(pkg, th, params, max_n=64, seed=seed, **VARIANTS[variant])
    try:
        o64, o32 = O.pair(params, cfg)
        l64, z64 = o64.accumulate(x, ya, yb, lam, 1.0)
        l32, z32 = o32.accumulate(x, ya, yb, lam, 1.0)
        margin = O.gate_margin(o64, o32)
        print(f"gate margin {margin:.2f}")
        assert margin >= 1.0                                   # a condition on the inputs, checked on the oracle alone
        loss, logits = th.head_train_accumulate(x, ya, yb, lam, 1.0)
        rec = []
        _check("loss", [loss], [l64], [l32], rec)
        _check("logits", logits, z64, z32, rec)
        for k in ("z1", "z2"):
            _check(k, th.head_train_tap(k, n), o64.taps[k].numpy(), o32.taps[k].numpy(), rec)
        g, g64, g32 = th.head_train_grads(), o64.grads(), o32.grads()
        for k in O.GRAD_FIELDS:
            _check("grad " + k, g[k], g64[k], g32[k], rec)
        e, e64, e32 = th.head_train_export(), o64.export(), o32.export()
        for k in O.STAT_FIELDS:
            _check(k, e[k], e64[k], e32[k], rec)
        _assert_all(rec)
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 3. accumulation
def test_two_accumulates_add_up(pkg, th):
    seed = ACC_SEED
    params = O.default_params(seed)
    cfg = _open(pkg, th, params, max_n=64, seed=seed)
    try:
        o64, o32 = O.pair(params, cfg)
        for k, n in enumerate((16, 5)):
            x, y = O.features(seed + 300 + k, n), _labels(seed + 400 + k, n)
            o64.accumulate(x, y, None, 1.0, 0.5)
            o32.accumulate(x, y, None, 1.0, 0.5)
            margin = O.gate_margin(o64, o32)
            print(f"gate margin, accumulate {k}: {margin:.2f}")
            assert margin >= 1.0
            th.head_train_accumulate(x, y, None, 1.0, 0.5)
        rec = []
        g, g64, g32 = th.head_train_grads(), o64.grads(), o32.grads()
        for k in O.GRAD_FIELDS:
            _check("grad " + k, g[k], g64[k], g32[k], rec)
        e, e64, e32 = th.head_train_export(), o64.export(), o32.export()
        for k in O.STAT_FIELDS:
            _check(k, e[k], e64[k], e32[k], rec)
        _assert_all(rec)
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 4. apply, teacher-forced
def _forced_grads(seed):
    """magnitudes log-uniform in [1e-4, 1], random signs: Adam's g / (sqrt(v) + eps) is well conditioned everywhere"""
    rs = np.random.RandomState(seed)
    out = {}
    for k in O.GRAD_FIELDS:
        shape = pkg_shapes()[k]
        out[k] = (10.0 ** rs.uniform(-4.0, 0.0, shape) * np.where(rs.rand(*shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    return out


def pkg_shapes():
    import rtdfd_amd

    return rtdfd_amd._lib.HEAD_SHAPES


@pytest.mark.parametrize("clip_norm", [1.0e4, 1.0])            # the forced norm is ~2e2: coefficient 1, and far above the clip
def test_apply_matches_adamw_and_ema(pkg, th, clip_norm):
    params = O.default_params(3)
    cfg = _open(pkg, th, params, max_n=16, seed=0, clip_norm=clip_norm)
    try:
        o64, o32 = O.pair(params, cfg)
        rec = []
        for step, lr in enumerate((3e-4, 1.2e-5, 1e-3)):
            lr = float(np.float32(lr))
            g = _forced_grads(50 + step)
            th.head_train_grads(set_to=g)
            o64.set_grads(g)
            o32.set_grads(g)
            n64, n32 = o64.apply(lr), o32.apply(lr)
            norm = th.head_train_apply(lr)
            assert (n64 < clip_norm) == (clip_norm > 1.0)
            _check(f"grad norm, step {step}", [norm], [n64], [n32], rec)
            zero = th.head_train_grads()
            assert all(not v.any() for v in zero.values())     # zeroed exactly
        for ema in (False, True):
            e, e64, e32 = th.head_train_export(ema), o64.export(ema), o32.export(ema)
            for k in O.GRAD_FIELDS:
                _check(("ema " if ema else "param ") + k, e[k], e64[k], e32[k], rec)
        _assert_all(rec)
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 5. five full steps (7. commit builds on it)
def _five_steps(pkg, h):
    """Five accumulate + apply steps at n = 16 on fixed data; the trainer stays open -> (o64, o32, otf, held-out features).

    o32 is the free-running float32 yardstick of the bar.  Its parameters drift from the float64 oracle's after the
    first update (Adam normalises the rounding noise autograd leaves in the b1 / b2 gradients into steps of the size
    of lr), so max|z32 - z64| of a later forward measures that drift and not rounding.  The gate precondition is
    therefore taken against otf, a float32 oracle whose whole state is teacher-forced from the float64 one after every
    apply: its difference in the next forward is float32 rounding of that forward alone, and the condition
    min|z64| >= 8 max|ztf - z64| (and equal gates) is asserted at every one of the five accumulates, on the oracles,
    before the device runs that step."""
    seed = FIVE_SEED
    params = O.default_params(seed)
    cfg = _open(pkg, h, params, max_n=16, seed=seed)
    o64, o32 = O.pair(params, cfg)
    otf = O.Oracle(params, cfg, torch.float32)
    for k in range(5):
        x, y = O.features(seed + 500 + k, 16), _labels(seed + 600 + k, 16)
        o64.accumulate(x, y)
        o32.accumulate(x, y)
        otf.accumulate(x, y)
        margin = O.gate_margin(o64, otf)
        print(f"gate margin, step {k}: {margin:.2f} (free-running float32 oracle: {O.gate_margin(o64, o32):.2f})")
        assert margin >= 1.0
        h.head_train_accumulate(x, y)
        lr = float(np.float32(3e-4 * (k + 1)))
        for o in (o64, o32, otf):
            o.apply(lr)
        otf.force_from(o64)
        h.head_train_apply(lr)
    return o64, o32, otf, O.features(seed + 700, 16)


def test_five_steps_eval_logits(pkg, th):
    """The bar here comes from the free-running float32 oracle, which after five updates is 1.5e-4 (live) and 3.9e-5
    (EMA) off the float64 one: this case bounds the device no tighter than a few 1e-4 (a wrong update path, not
    rounding; measured device error 2.6e-7 / 1.7e-7); the per-tensor cases above carry the precision claim.  The figure against the teacher-forced float32 oracle is printed."""
    try:
        o64, o32, otf, held = _five_steps(pkg, th)
        rec = []
        for ema in (False, True):
            tag = "ema" if ema else "live"
            z64, z32, ztf = o64.evaluate(held, ema), o32.evaluate(held, ema), otf.evaluate(held, ema)
            margin = O.gate_margin(o64, otf)                   # the held-out forward has ReLU gates of its own
            print(f"gate margin, eval {tag}: {margin:.2f}")
            assert margin >= 1.0
            got = th.head_train_eval(held, ema)
            _check("eval logits, " + tag, got, z64, z32, rec)
            _check("eval logits, " + tag + ", against the teacher-forced float32 oracle (printed only)", got, z64, ztf)
        _assert_all(rec)
    finally:
        th.head_train_end()


# --------------------------------------------------------------------------- 6. outcome
def _clusters(seed, n, sep=3.0):
    rs = np.random.RandomState(seed)
    y = (np.arange(n) % 2).astype(np.float32)
    d = np.random.RandomState(99).randn(1280)
    d /= np.linalg.norm(d)
    return (1.0 + 0.3 * rs.randn(n, 1280) + np.outer(2 * y - 1, d) * sep).astype(np.float32), y


def test_fit_separates_two_clusters(pkg, th, seeded_sd):
    x, y = _clusters(1, 640)
    vx, vy = _clusters(2, 64)
    params = O.default_params(0)
    sd = dict(seeded_sd)
    sd.update({k: params[f] for k, f in T.KEYS.items()})
    kw = dict(epochs=10, batch_size=32, grad_accum=1, lr=1e-3, val=(vx, vy), patience=10)      # 200 optimizer steps
    with T.HeadTrainer(th, sd, max_n=32, seed=3, ema_decay=0.95) as tr:
        oracle = O.Oracle(params, O.config_values(tr.config), torch.float64)
        v0_ref = T.focal_loss(oracle.evaluate(vx, True), vy, *oracle.loss_settings)
        log_ref = T.fit_loop(oracle, x, y, rng=np.random.RandomState(5), **kw)
        z_ref = oracle.evaluate(vx, True)
        assert oracle.counter == 200
        assert ((z_ref > 0) == (vy > 0.5)).all() and np.abs(z_ref).min() > 1.0      # preconditions, on the oracle
        assert log_ref[-1]["val_loss"] < 0.5 * v0_ref
        v0 = T.focal_loss(tr.evaluate(vx, True), vy, *tr.loss_settings)
        log = tr.fit(x, y, rng=np.random.RandomState(5), **kw)
        z = tr.evaluate(vx, True)
        print(f"oracle: val loss {v0_ref:.5f} -> {log_ref[-1]['val_loss']:.5f}, min|z| {np.abs(z_ref).min():.3f}; "
              f"device: {v0:.5f} -> {log[-1]['val_loss']:.5f}, min|z| {np.abs(z).min():.3f}")
        assert tr.steps == 200 and len(log) == 10
        assert ((z > 0) == (z_ref > 0)).all()
        assert log[-1]["val_loss"] < 0.5 * v0
        assert set(log[-1]) == {"epoch", "train_loss", "train_acc", "val_loss", "val_acc", "val_f1", "val_auc", "lr", "time_seconds"}


# --------------------------------------------------------------------------- 7. commit
def test_commit_swaps_the_head_in_place(pkg, seeded_sd, b0_handle):
    imgs = (np.random.RandomState(9).randn(2, 3, 224, 224) * 0.8).astype(np.float32)
    untouched = b0_handle.classify(imgs).copy()
    h = pkg._lib.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=2)
    try:
        before = h.classify(imgs).copy()                       # also builds the cached weight splits of fc1 / fc2
        _five_steps(pkg, h)
        for ema in (False, True):
            h.head_train_commit(ema)
            out = h.head_train_export(ema)
            sd = dict(seeded_sd)
            sd.update({k: out[f] for k, f in T.KEYS.items()})
            fresh = pkg._lib.Handle(pkg.weights.pack_b0(sd), device=0, max_batch=2)
            try:
                got, want = h.classify(imgs), fresh.classify(imgs)
                print(f"use_ema={ema}: before {before.ravel()} committed {got.ravel()} fresh handle {want.ravel()}")
                assert np.array_equal(got, want)
                assert not np.array_equal(got, before)
                lg, heat = h.gradcam(imgs)
                lg2, heat2 = fresh.gradcam(imgs)
                assert np.array_equal(lg, got) and np.array_equal(lg2, want)
                assert np.array_equal(heat, heat2)
            finally:
                fresh.close()
        h.head_train_end()
        assert np.array_equal(h.classify(imgs), got)           # the committed head stays after the trainer is gone
    finally:
        h.close()
    assert np.array_equal(b0_handle.classify(imgs), untouched)  # a handle that never opened a trainer


def test_fit_head_updates_model_without_reopening(pkg):
    """DeepfakeEfficientNet.fit_head: features in, head committed on the SAME handle, state dict updated"""
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, seed=0)
    imgs = (np.random.RandomState(4).randn(2, 3, 224, 224) * 0.8).astype(np.float32)
    before, handle = m(imgs).copy(), m.handle
    x, y = _clusters(3, 64)
    log = m.fit_head(x, y, epochs=1, batch_size=16, grad_accum=2, lr=1e-3, trainer_config={"ema_decay": 0.5})
    assert len(log) == 1 and m.handle is handle and m.train(True).training and not m.eval().training
    after = m(imgs)
    assert not np.array_equal(after, before)
    fresh = pkg._lib.Handle(pkg.weights.pack_b0(m.state_dict()), device=0, max_batch=2)
    try:
        assert np.array_equal(fresh.classify(imgs), after)
    finally:
        fresh.close()
        handle.close()


# --------------------------------------------------------------------------- 8. errors
def test_argument_errors(pkg, th, seeded_sd):
    L = pkg._lib
    params, x, y = O.default_params(0), O.features(0, 4), _labels(0, 4)

    def refused(fn, *a, **k):
        with pytest.raises(L.DfdError) as e:
            fn(*a, **k)
        assert e.value.code == -1 and len(str(e.value)) > 30, str(e.value)     # DFD_ERR_ARG with a message

    for call in (lambda: th.head_train_accumulate(x, y), lambda: th.head_train_apply(1e-3), lambda: th.head_train_eval(x),
                 th.head_train_export, th.head_train_grads, lambda: th.head_train_tap("z1", 4), th.head_train_commit,
                 th.head_train_end):
        refused(call)                                          # no trainer is open
    refused(th.head_train_begin, params, L.head_config(max_n=257))
    refused(th.head_train_begin, params, L.head_config(max_n=1))
    refused(th.head_train_begin, params, L.head_config(dropout=1.0))
    refused(th.head_train_begin, params, L.head_config(dropout=-0.1))
    th.head_train_begin(params, L.head_config(max_n=4))
    refused(th.head_train_begin, params, L.head_config(max_n=4))                # a second begin
    refused(th.head_train_accumulate, x[:1], y[:1])                             # n < 2
    refused(th.head_train_accumulate, O.features(0, 5), _labels(0, 5))          # n > max_n
    refused(th.head_train_eval, O.features(0, 5))
    refused(th.head_train_tap, "z1", 4)                                         # nothing accumulated yet
    loss, logits = th.head_train_accumulate(x, y)
    assert np.isfinite(loss) and np.isfinite(logits).all()
    refused(th.head_train_tap, "z3", 4)
    th.head_train_end()
    refused(th.head_train_accumulate, x, y)                                     # after end
    # dfd_destroy with an open trainer frees it
    h = L.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=1)
    h.head_train_begin(params, L.head_config(max_n=4))
    h.head_train_accumulate(x, y)
    h.close()

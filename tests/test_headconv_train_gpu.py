"""GPU: the conv stage of the head trainer (csrc/head_train_conv.hip: dfd_head_train_unfreeze_conv, _accumulate_trunk,
_eval_trunk, _export_conv, _conv_grads) and the trunk extraction (dfd_extract_trunk, dfd_train_augment_trunk) against the
float64 oracle of tests/headconv_train_oracle.py.

Bars: as tests/test_head_train_gpu.py - every compared tensor's rms(d) / rms(ref) and max|d| / max|ref| against the float64
oracle at most 4 x / 8 x the same metrics of the float32 CPU oracle, floored at 2^-23 / 2^-21 (`O.bar_ratio` <= 1).  Every
figure is printed before it is asserted.

Inputs: "real" trunk rows are `extract_trunk` of b0_layer_oracle.stress_state_dict weights on random_crops (the conv
stage starts from the same state dict: running variances over four decades, gammas of both signs and exact zeros);
"synthetic" rows are standard normals.  Gate precondition: the head's ReLU gates are discrete, so every comparison
fixes a seed for which the two ORACLES agree on every gate with `gate_margin` >= 1, asserted before the device is looked
at.  The seeds were picked at authoring time on the CPU by conditions on the oracles alone (real rows from a float32 CPU
forward of the same weights and crops): of seeds 0..11 the largest margin per size - 72 (n = 5), 29 (16), 4.3 (37), 23
(synthetic 16); the n = 256 and two-accumulate seeds are noted at their constants.

Conditioning precondition: the pooled features reach the head as float32, and BatchNorm1d over very few rows can turn
half an ulp there into any error of the logit (a column of fc1's output whose two rows differ by less than sqrt(eps)).
`CO.rounding_share` measures that on the float64 oracle alone: the move of logits and loss when the oracle's own cfeat is
rounded to float32, in units of the bar's floor.  It is 0.33 .. 0.65 for every case from n = 5 up and anything from 0.08
to 107 at n = 2 (seeds 0..59; 95 at the seed with the largest gate margin of 0..11), so n = 2 takes, of the seeds 0..59
with a share <= 0.5 (30, 43, 55, 56), the one with the largest gate margin: 55 (margin 1517, share 0.29).  Share <= 1 is
asserted with the gate margin, before the device is looked at.

m = 49 n rows: 98, 245 and 1813 are no multiples of 16 (row masking in both GEMMs), 784 is; 256 crops are max_n.

Other values of lr_scale, bn_momentum, bn_eps and of the head's dropout: tests/test_head_train_config_gpu.py (stage cases).
"""
import numpy as np
import pytest
import torch

import b0_layer_oracle as B
import head_train_oracle as O
import headconv_train_oracle as CO
from rtdfd_amd import head_training as T
from rtdfd_amd import train_augment as TA

pytestmark = pytest.mark.gpu

REAL_SEED = {2: 55, 5: 9, 16: 7, 37: 3}
SYN16_SEED = 1
SYN256_SEED = 58                                    # of seeds 0..79 the largest margin at 256 crops (768 gates a crop): 2.3
ACC_SEED = 1                                        # two-accumulate case: of seeds 0..11 the largest smaller margin (17, 25)
VARIANTS = {"plain": (False, 1.0), "mix": (True, 1.0), "scaled": (False, 0.5)}     # (two label vectors with lam, loss_scale)
CASES = [("real", n, v) for n in (2, 5, 16, 37) for v in VARIANTS] + [("synthetic", 16, "plain"), ("synthetic", 256, "plain")]


@pytest.fixture(scope="module")
def stress_sd():
    return B.stress_state_dict(0)


@pytest.fixture(scope="module")
def conv0(stress_sd):
    return CO.conv_params(stress_sd)


@pytest.fixture(scope="module")
def sh(pkg, stress_sd):
    """the handle of this module's trainers and extractions: stress weights, classifier only"""
    h = pkg._lib.Handle(pkg.weights.pack_b0(stress_sd), device=0, max_batch=16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def real_trunk(sh):
    x = B.random_crops(37, 42)
    return np.concatenate([sh.extract_trunk(x[i:i + 16]) for i in range(0, 37, 16)])


def _labels(seed, n):
    return (np.random.RandomState(seed).rand(n) < 0.5).astype(np.float32)


def _open(pkg, h, head, conv, **kw):
    cfg = pkg._lib.head_config(**kw)
    h.head_train_begin(head, cfg)
    try:
        h.head_train_unfreeze_conv(conv)
    except Exception:
        h.head_train_end()
        raise
    return O.config_values(cfg)


def _check(name, got, ref64, yard32, record):
    r = O.bar_ratio(got, ref64, yard32)
    print(f"{name}: rms {r['rms']:.3e} (yard {r['yard_rms']:.3e}) max {r['max']:.3e} (yard {r['yard_max']:.3e}) ratio {r['ratio']:.3f}")
    record.append((name, r["ratio"]))


def _assert_all(record):
    bad = [(k, round(v, 3)) for k, v in record if not v <= 1.0]
    assert not bad, bad


def _all_grads(h):
    g = dict(h.head_train_grads())
    g.update({"conv." + k: v for k, v in h.head_train_conv_grads().items()})
    return g


def _all_export(h, ema=False):
    e = dict(h.head_train_export(ema))
    e.update({"conv." + k: v for k, v in h.head_train_export_conv(ema).items()})
    return e


GRAD_KEYS = tuple("conv." + k for k in CO.CONV_GRAD_FIELDS) + O.GRAD_FIELDS
STAT_KEYS = tuple("conv." + k for k in CO.CONV_STAT_FIELDS) + O.STAT_FIELDS


def _compare_state(h, o64, o32, rec):
    g, g64, g32 = _all_grads(h), o64.grads(), o32.grads()
    for k in GRAD_KEYS:
        _check("grad " + k, g[k], g64[k], g32[k], rec)
    e, e64, e32 = _all_export(h), o64.export(), o32.export()
    for k in STAT_KEYS:
        _check(k, e[k], e64[k], e32[k], rec)


# --------------------------------------------------------------------------- 1. one accumulate
@pytest.mark.parametrize("kind,n,variant", CASES)
def test_one_accumulate_matches_float64(pkg, sh, conv0, real_trunk, kind, n, variant):
    if kind == "real":
        seed, x = REAL_SEED[n], real_trunk[:n]
    else:
        seed = SYN16_SEED if n == 16 else SYN256_SEED
        x = CO.synthetic_trunk(seed + 100, n)
    two, scale = VARIANTS[variant]
    head, ya = O.default_params(seed), _labels(seed + 200, n)
    yb, lam = (_labels(seed + 201, n), 0.7) if two else (None, 1.0)
    cfg = _open(pkg, sh, head, conv0, max_n=max(n, 64), seed=seed)
    try:
        o64, o32 = CO.pair(conv0, head, cfg)
        l64, z64 = o64.accumulate(x, ya, yb, lam, scale)
        l32, z32 = o32.accumulate(x, ya, yb, lam, scale)
        margin = CO.gate_margin(o64, o32)
        share = CO.rounding_share(o64, ya, yb, lam)
        print(f"gate margin {margin:.2f}, rounding share {share:.3f}")
        assert margin >= 1.0 and share <= 1.0                  # conditions on the inputs, checked on the oracles alone
        loss, logits = sh.head_train_accumulate_trunk(x, ya, yb, lam, scale)
        rec = []
        _check("loss", [loss], [l64], [l32], rec)
        _check("logits", logits, z64, z32, rec)
        for k in ("cfeat", "cz", "dfeat"):
            _check(k, sh.head_train_tap(k, n), o64.taps[k].numpy(), o32.taps[k].numpy(), rec)
        _compare_state(sh, o64, o32, rec)
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 2. accumulation
def test_two_accumulates_add_up(pkg, sh, conv0, real_trunk):
    seed = ACC_SEED
    head = O.default_params(seed)
    cfg = _open(pkg, sh, head, conv0, max_n=16, seed=seed)
    try:
        o64, o32 = CO.pair(conv0, head, cfg)
        for k, x in enumerate((real_trunk[:16], real_trunk[16:21])):
            y = _labels(seed + 400 + k, x.shape[0])
            o64.accumulate(x, y, None, 1.0, 0.5)
            o32.accumulate(x, y, None, 1.0, 0.5)
            margin = CO.gate_margin(o64, o32)
            share = CO.rounding_share(o64, y)
            print(f"gate margin, accumulate {k}: {margin:.2f}, rounding share {share:.3f}")
            assert margin >= 1.0 and share <= 1.0
            sh.head_train_accumulate_trunk(x, y, None, 1.0, 0.5)
        rec = []
        _compare_state(sh, o64, o32, rec)
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 3. apply, teacher-forced
def _forced_grads(pkg, seed):
    """magnitudes log-uniform in [1e-4, 1], random signs: Adam's g / (sqrt(v) + eps) is well conditioned everywhere"""
    rs = np.random.RandomState(seed)
    shapes = {k: pkg._lib.HEAD_SHAPES[k] for k in O.GRAD_FIELDS}
    shapes.update({"conv." + k: pkg._lib.CONV_SHAPES[k] for k in CO.CONV_GRAD_FIELDS})
    return {k: (10.0 ** rs.uniform(-4.0, 0.0, s) * np.where(rs.rand(*s) < 0.5, -1.0, 1.0)).astype(np.float32) for k, s in shapes.items()}


@pytest.mark.parametrize("clip_norm", [1.0e4, 1.0])            # the forced norm is ~3e2: coefficient 1, and far above the clip
def test_apply_steps_both_groups_at_their_rates(pkg, sh, conv0, clip_norm):
    """Three forced applies.  The conv group steps at 0.1 x the head's rate: three Adam steps at the head's rate would
    move w / g / be by ~2.7 lr more, 1e-3 of their size - a thousand times the bar."""
    head = O.default_params(3)
    cfg = _open(pkg, sh, head, conv0, max_n=16, seed=0, clip_norm=clip_norm)
    try:
        o64, o32 = CO.pair(conv0, head, cfg)
        rec = []
        for step, lr in enumerate((3e-4, 1.2e-5, 1e-3)):
            lr = float(np.float32(lr))
            g = _forced_grads(pkg, 50 + step)
            sh.head_train_grads(set_to={k: g[k] for k in O.GRAD_FIELDS})
            sh.head_train_conv_grads(set_to={k: g["conv." + k] for k in CO.CONV_GRAD_FIELDS})
            o64.set_grads(g)
            o32.set_grads(g)
            n64, n32 = o64.apply(lr), o32.apply(lr)
            norm = sh.head_train_apply(lr)
            assert (n64 < clip_norm) == (clip_norm > 1.0)
            _check(f"grad norm, step {step}", [norm], [n64], [n32], rec)
            assert all(not v.any() for v in _all_grads(sh).values())          # zeroed exactly, both groups
        for ema in (False, True):
            e, e64, e32 = _all_export(sh, ema), o64.export(ema), o32.export(ema)
            for k in GRAD_KEYS:
                _check(("ema " if ema else "param ") + k, e[k], e64[k], e32[k], rec)
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 4. reproducibility and chunking
def test_a_step_is_reproducible_bit_for_bit(pkg, sh, conv0, real_trunk):
    head, y = O.default_params(1), _labels(5, 37)
    seen = []
    for _ in range(2):
        _open(pkg, sh, head, conv0, max_n=37, seed=11)
        try:
            loss, logits = sh.head_train_accumulate_trunk(real_trunk, y)
            seen.append((loss, logits.copy(), _all_grads(sh), _all_export(sh)))
        finally:
            sh.head_train_end()
    a, b = seen
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for k in GRAD_KEYS:
        assert np.array_equal(a[2][k], b[2][k]), k
        assert a[2][k].any() or k in ("b1", "b2"), k
    for k in STAT_KEYS:
        assert np.array_equal(a[3][k], b[3][k]), k


def test_eval_does_not_depend_on_the_chunking(pkg, sh, conv0):
    head = O.default_params(2)
    x = CO.synthetic_trunk(9, 256)
    _open(pkg, sh, head, conv0, max_n=256, seed=2)
    try:
        sh.head_train_accumulate_trunk(x[:16], _labels(1, 16))
        sh.head_train_apply(1e-3)                              # live and EMA parameters differ from here on
        for ema in (False, True):
            whole = sh.head_train_eval_trunk(x, ema)
            parts = np.concatenate([sh.head_train_eval_trunk(x[i:i + 64], ema) for i in range(0, 256, 64)])
            assert np.isfinite(whole).all() and np.array_equal(whole, parts)
        assert not np.array_equal(sh.head_train_eval_trunk(x[:8], False), sh.head_train_eval_trunk(x[:8], True))
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 5. commit
def test_commit_swaps_conv_and_head_in_place(pkg, stress_sd, real_trunk):
    imgs = B.random_crops(2, 7)
    L = pkg._lib
    blob = pkg.weights.pack_b0(stress_sd)
    h, never = L.Handle(blob, device=0, max_batch=2), L.Handle(blob, device=0, max_batch=2)

    def outputs(handle, mode):
        handle.set_option("bf16_activations", mode)
        try:
            lg = handle.classify(imgs).copy()
            lg2, heat = handle.gradcam(imgs)
            assert np.array_equal(lg, lg2)
            return lg, heat.copy()
        finally:
            handle.set_option("bf16_activations", 0)

    try:
        before = [outputs(h, mode) for mode in (0, 1)]         # also builds the cached weight splits of head.w / fc1 / fc2
        with T.HeadTrainer(h, stress_sd, train_conv_head=True, max_n=16, seed=4, ema_decay=0.5) as tr:
            for k in range(3):
                tr.accumulate(real_trunk[k:k + 16], _labels(20 + k, 16))
                tr.apply(1e-3)
            for mode in (0, 1):                                # an open, trained, uncommitted trainer changes nothing
                lg, heat = outputs(h, mode)
                lg0, heat0 = outputs(never, mode)
                assert np.array_equal(lg, lg0) and np.array_equal(heat, heat0)
                assert np.array_equal(lg, before[mode][0]) and np.array_equal(heat, before[mode][1])
            for ema in (False, True):
                tr.commit(use_ema=ema)
                sd = dict(stress_sd)
                exported = tr.export_state_dict(use_ema=ema)
                assert exported["net._conv_head.weight"].shape == (1280, 320, 1, 1) and int(exported["net._bn1.num_batches_tracked"]) == 3
                sd.update(exported)
                fresh = L.Handle(pkg.weights.pack_b0(sd), device=0, max_batch=2)
                try:
                    for mode in (0, 1):
                        got, want = outputs(h, mode), outputs(fresh, mode)
                        last = got if mode == 0 else last
                        print(f"use_ema={ema} bf16={mode}: before {before[mode][0].ravel()} committed {got[0].ravel()} fresh {want[0].ravel()}")
                        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                        assert not np.array_equal(got[0], before[mode][0])
                finally:
                    fresh.close()
            assert not np.array_equal(exported["net._conv_head.weight"], np.asarray(stress_sd["net._conv_head.weight"]))
        assert np.array_equal(outputs(h, 0)[0], last[0])        # the committed conv and head stay after the trainer is gone
        lg0, heat0 = outputs(never, 0)
        assert np.array_equal(lg0, before[0][0]) and np.array_equal(heat0, before[0][1])
    finally:
        h.close()
        never.close()


# --------------------------------------------------------------------------- 6. trunk extraction
def test_extract_trunk_is_the_b15_tap(pkg, sh):
    x = B.random_crops(5, 3)
    xd = sh.alloc(x.nbytes).upload(x)
    try:
        for mode in (0, 1):
            sh.set_option("bf16_activations", mode)
            got = sh.extract_trunk(x)
            want = sh.tap(xd.ptr, 5, "b15.out", 5 * 15680)
            assert got.shape == (5, 7, 7, 320) and want.size == 5 * 15680
            assert np.array_equal(got.ravel(), want) and np.abs(got).max() > 0
    finally:
        sh.set_option("bf16_activations", 0)
        xd.free()
    with pytest.raises(pkg._lib.DfdError):
        sh.extract_trunk(B.random_crops(17, 3))                # n > max_batch is the caller's chunking
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, seed=0)
    try:
        got = m.extract_trunk(x)                               # chunks of 2, 2, 1
        xd = m.handle.alloc(x.nbytes).upload(x)
        per = 3 * 224 * 224 * 4
        want = np.concatenate([m.handle.tap(xd.ptr + i * per, min(2, 5 - i), "b15.out", 2 * 15680) for i in range(0, 5, 2)])
        xd.free()
        assert got.shape == (5, 7, 7, 320) and np.array_equal(got.ravel(), want)
    finally:
        m.handle.close()


def test_train_augment_trunk_equals_augment_then_extract(pkg, seeded_sd):
    h = pkg._lib.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=2)
    try:
        rgb = np.random.RandomState(8).randint(0, 256, (5, 64, 96, 3)).astype(np.uint8)
        rows, batch = TA.draw_batch(TA.AugmentPolicy(), np.random.RandomState(6), 5, 64, 96, 224,
                                    mix=(TA.MIX_MIXUP, 0.8, np.array([4, 3, 0, 1, 2])))
        x = h.train_augment(rgb, rows, batch, 224)
        want = np.concatenate([h.extract_trunk(x[i:i + 2]) for i in range(0, 5, 2)])
        got = h.train_augment_trunk(rgb, rows, batch)
        assert got.shape == (5, 7, 7, 320) and np.array_equal(got, want)
        buf = h.alloc(rgb.nbytes).upload(rgb)
        try:
            assert np.array_equal(h.train_augment_trunk(buf, rows, batch, shape=rgb.shape[:3]), want)
        finally:
            buf.free()
    finally:
        h.close()


# --------------------------------------------------------------------------- 7. outcome
def _two_classes(seed, n, sep=0.35):
    rs = np.random.RandomState(seed)
    y = (np.arange(n) % 2).astype(np.float32)
    d = np.random.RandomState(99).randn(320)
    d /= np.linalg.norm(d)
    x = rs.randn(n, 49, 320) + (2 * y - 1)[:, None, None] * d * sep * np.sqrt(320.0) / 4.0
    return x.reshape(n, -1).astype(np.float32), y


def test_fit_separates_two_classes_of_trunk_rows(pkg, sh, stress_sd, conv0):
    """40 optimizer steps at n = 16, oracle and device side by side; smallest |logit| on the held-out rows as printed."""
    x, y = _two_classes(1, 160)
    vx, vy = _two_classes(2, 32)
    head = O.default_params(0)
    sd = dict(stress_sd)
    sd.update({k: head[f] for k, f in T.KEYS.items()})
    kw = dict(epochs=4, batch_size=16, grad_accum=1, lr=1e-3, val=(vx, vy), patience=10)           # 40 optimizer steps
    with T.HeadTrainer(sh, sd, train_conv_head=True, max_n=16, seed=3, ema_decay=0.9) as tr:
        oracle = CO.ConvOracle(conv0, head, O.config_values(tr.config), torch.float64)
        v0_ref = T.focal_loss(oracle.evaluate(vx, True), vy, *oracle.loss_settings)
        log_ref = T.fit_loop(oracle, x, y, rng=np.random.RandomState(5), **kw)
        z_ref = oracle.evaluate(vx, True)
        assert oracle.counter == 40
        assert ((z_ref > 0) == (vy > 0.5)).all()               # precondition, on the oracle
        assert log_ref[-1]["val_loss"] < v0_ref
        v0 = T.focal_loss(tr.evaluate(vx, True), vy, *tr.loss_settings)
        log = tr.fit(x, y, rng=np.random.RandomState(5), **kw)
        z = tr.evaluate(vx.reshape(-1, 7, 7, 320), True)       # both row layouts are taken
        print(f"oracle: val loss {v0_ref:.5f} -> {log_ref[-1]['val_loss']:.5f}, min|z| {np.abs(z_ref).min():.4f}; "
              f"device: {v0:.5f} -> {log[-1]['val_loss']:.5f}, min|z| {np.abs(z).min():.4f}")
        assert tr.steps == 40 and len(log) == 4
        assert ((z > 0) == (z_ref > 0)).all()
        assert log[-1]["val_loss"] < v0
        sdo = tr.export_state_dict(True)
        assert set(T.CONV_KEYS) <= set(sdo) and int(sdo[T.CONV_TRACKED]) == 40


def test_fit_head_trains_conv_and_head_on_the_models_handle(pkg):
    """DeepfakeEfficientNet.fit_head(train_conv_head=True): images in (trunk rows extracted here), then uint8 crops with
    `augment=` (every batch through `train_augment_trunk`); conv and head committed on the SAME handle, state dict updated"""
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, seed=0)
    try:
        imgs = (np.random.RandomState(4).randn(6, 3, 224, 224) * 0.8).astype(np.float32)
        y = (np.arange(6) % 2).astype(np.float32)
        before, handle, w0 = m(imgs[:2]).copy(), m.handle, np.array(m.state_dict()["net._conv_head.weight"])
        log = m.fit_head(imgs, y, epochs=1, batch_size=3, grad_accum=1, lr=1e-3, train_conv_head=True, trainer_config={"ema_decay": 0.5})
        assert len(log) == 1 and m.handle is handle
        after, w1 = m(imgs[:2]).copy(), np.array(m.state_dict()["net._conv_head.weight"])
        assert not np.array_equal(after, before) and w1.shape == w0.shape and not np.array_equal(w1, w0)
        crops = np.random.RandomState(14).randint(0, 256, (8, 32, 32, 3)).astype(np.uint8)
        y8 = (np.arange(8) % 2).astype(np.float32)
        log = m.fit_head(crops, y8, epochs=1, batch_size=4, grad_accum=2, lr=1e-3, mix_alpha=0.4, cutmix_alpha=0.3, train_conv_head=True,
                         augment=TA.AugmentPolicy(), val=(crops[:3], y8[:3]), rng=np.random.RandomState(2))
        assert len(log) == 1 and np.isfinite(log[0]["train_loss"]) and np.isfinite(log[0]["val_loss"]) and m.handle is handle
        last = m(imgs[:2])
        assert not np.array_equal(last, after) and int(m.state_dict()["net._bn1.num_batches_tracked"]) == 4
        fresh = pkg._lib.Handle(pkg.weights.pack_b0(m.state_dict()), device=0, max_batch=2)
        try:
            assert np.array_equal(fresh.classify(imgs[:2]), last)
        finally:
            fresh.close()
    finally:
        m.handle.close()


# --------------------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_handle_usable(pkg, sh, conv0):
    L = pkg._lib
    head, x, y = O.default_params(0), CO.synthetic_trunk(0, 4), _labels(0, 4)
    feat = O.features(0, 4)

    def refused(fn, *a, **k):
        with pytest.raises(L.DfdError) as e:
            fn(*a, **k)
        assert e.value.code == -1 and len(str(e.value)) > 30, str(e.value)     # DFD_ERR_ARG with a message

    refused(sh.head_train_unfreeze_conv, conv0)                                 # no trainer is open
    sh.head_train_begin(head, L.head_config(max_n=4))
    try:
        for call in (lambda: sh.head_train_accumulate_trunk(x, y), lambda: sh.head_train_eval_trunk(x), sh.head_train_export_conv,
                     sh.head_train_conv_grads):
            refused(call)                                                       # the stage is not unfrozen
        sh.head_train_accumulate(feat, y)                                       # the head-only trainer still works
        refused(sh.head_train_tap, "cfeat", 4)
        refused(sh.head_train_unfreeze_conv, conv0)                             # after the first accumulate
    finally:
        sh.head_train_end()
    sh.head_train_begin(head, L.head_config(max_n=4))
    try:
        refused(sh.head_train_unfreeze_conv, conv0, lr_scale=-1.0)
        refused(sh.head_train_unfreeze_conv, conv0, bn_eps=0.0)
        sh.head_train_unfreeze_conv(conv0)
        refused(sh.head_train_unfreeze_conv, conv0)                             # a second time
        refused(sh.head_train_accumulate, feat, y)                              # pooled rows, once unfrozen
        refused(sh.head_train_eval, feat)
        refused(sh.head_train_accumulate_trunk, x[:1], y[:1])                   # n < 2
        refused(sh.head_train_accumulate_trunk, CO.synthetic_trunk(0, 5), _labels(0, 5))   # n > max_n
        refused(sh.head_train_eval_trunk, CO.synthetic_trunk(0, 5))
        refused(sh.head_train_tap, "cz", 4)                                     # nothing accumulated yet
        loss, logits = sh.head_train_accumulate_trunk(x, y)
        assert np.isfinite(loss) and np.isfinite(logits).all()
        assert sh.head_train_tap("cz", 4).shape == (4, 49, 1280)
        assert np.isfinite(sh.head_train_apply(1e-3)) and np.isfinite(sh.head_train_eval_trunk(x)).all()
    finally:
        sh.head_train_end()
    refused(sh.head_train_accumulate_trunk, x, y)                               # after end
    assert np.isfinite(sh.classify(B.random_crops(1, 0))).all()
    # dfd_destroy with an open trainer and stage frees both
    h = L.Handle(pkg.weights.pack_b0(pkg.weights.seeded_state_dict(0)), device=0, max_batch=1)
    h.head_train_begin(head, L.head_config(max_n=4))
    h.head_train_unfreeze_conv(conv0)
    h.head_train_accumulate_trunk(x, y)
    h.close()

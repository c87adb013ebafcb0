"""CPU: the head trainer's host pieces and the test oracle itself (tests/head_train_oracle.py)."""
import numpy as np
import pytest
import torch

import head_train_oracle as O
from rtdfd_amd import head_training as T


@pytest.mark.parametrize("dtype,p", [(torch.float64, 0.5), (torch.float64, 0.35), (torch.float32, 0.5), (torch.float32, 0.25)])
def test_mask_path_equals_nn_dropout(dtype, p):
    """multiplying by keep / (1 - p) is nn.Dropout(p) in train mode on the same keep pattern"""
    torch.manual_seed(3)
    x = torch.rand(37, 512, dtype=dtype) + 0.5                 # no zeros: the keep pattern is y != 0
    y = torch.nn.Dropout(p).train()(x)
    keep = (y != 0).numpy()
    assert 0.0 < keep.mean() < 1.0
    mult = torch.from_numpy(keep.astype(np.float64) / (1.0 - p)).to(dtype)      # Oracle.masks' multiplier
    eps = torch.finfo(dtype).eps
    assert float(((x * mult - y).abs() / y.abs().clamp_min(1e-30)).max()) <= 2 * eps
    assert bool(((x * mult == 0) == (y == 0)).all())


def test_one_cycle_lr_equals_torch():
    total, max_lr = 50, 3e-4
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))], lr=1.0)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total, pct_start=0.1, anneal_strategy="cos",
                                              div_factor=25, final_div_factor=1000)
    for k in range(total):
        want = sch.get_last_lr()[0]
        got = T.one_cycle_lr(k, total, max_lr)
        assert abs(got - want) <= 1e-12 * abs(want), (k, got, want)
        if k + 1 < total:
            opt.step()
            sch.step()


def test_dropout_keep_mask_properties():
    n, w, p = 64, 1280, 0.5
    base = T.dropout_keep_mask(7, 3, 1, n, w, p)
    assert base.dtype == np.bool_ and base.shape == (n, w)
    assert np.array_equal(base, T.dropout_keep_mask(7, 3, 1, n, w, p))                 # deterministic
    for other in (T.dropout_keep_mask(8, 3, 1, n, w, p), T.dropout_keep_mask(7, 4, 1, n, w, p),
                  T.dropout_keep_mask(7, 3, 2, n, w, p), T.dropout_keep_mask(7 + (1 << 32), 3, 1, n, w, p),
                  T.dropout_keep_mask(7, 3 + (1 << 32), 1, n, w, p)):
        assert 0.4 < float((other != base).mean()) < 0.6                                  # seed, counter, layer each matter
    assert T.dropout_keep_mask(7, 3, 1, n, w, 0.0).all()                                  # p = 0 keeps all
    for q in (0.5, 0.35, 0.25, 0.9):
        keep = T.dropout_keep_mask(11, 0, 0, n, w, q).mean()
        sd = np.sqrt(q * (1 - q) / (n * w))
        assert abs(keep - (1 - q)) <= 5 * sd, (q, keep)
    # a prefix of the rows is the same mask: the hash sees row * width + col only
    assert np.array_equal(T.dropout_keep_mask(7, 3, 1, 5, w, p), base[:5])


def test_dropout_rates_follow_the_float_setting():
    p0, p1, p2 = T.dropout_rates(0.3)
    d = float(np.float32(0.3))
    assert (p0, p1, p2) == (d, 0.7 * d, 0.5 * d)


class _StubHandle:
    """records the begin call and hands back zero arrays of the library's shapes"""

    def __init__(self):
        self.begun = None
        self._p = 1

    def head_train_begin(self, params, config):
        self.begun = params

    def head_train_export(self, use_ema=False):
        import rtdfd_amd

        return rtdfd_amd._lib._head_arrays()[1]

    def head_train_end(self):
        self._p = None


class _StubModel:
    def __init__(self, sd):
        self.handle = _StubHandle()
        self._sd = sd

    def state_dict(self):
        return dict(self._sd)


def test_export_state_dict_names_and_shapes(pkg, seeded_sd):
    model = _StubModel(seeded_sd)
    tr = T.HeadTrainer(model)
    for key, field in T.KEYS.items():
        assert np.array_equal(model.handle.begun[field], np.asarray(seeded_sd[key], np.float32))
    sd = tr.export_state_dict()
    want = {k: v for k, v in seeded_sd.items() if k.startswith("net._fc.")}
    assert sorted(sd) == sorted(want)
    for k, v in want.items():
        assert sd[k].shape == np.asarray(v).shape, k
        assert sd[k].dtype == np.asarray(v).dtype, k
    tr.close()
    assert model.handle._p is None


def test_oracle_yardstick_tracks_reference():
    """the float32 oracle is a float32-accurate copy of the float64 one (sanity of the bar's yardstick)"""
    cfg = {"max_n": 16, "seed": 1, "dropout": 0.5, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 0.05,
           "focal_gamma": 2.0, "focal_alpha": 0.25, "label_smoothing": 0.1, "clip_norm": 1.0, "ema_decay": 0.999,
           "bn_momentum": 0.1}
    o64, o32 = O.pair(O.default_params(0), cfg)
    x, y = O.features(5, 16), (np.arange(16) % 2).astype(np.float32)
    l64, z64 = o64.accumulate(x, y)
    l32, z32 = o32.accumulate(x, y)
    assert abs(l64 - l32) <= 1e-5 * abs(l64)
    assert O.metrics(z32, z64)["rms"] < 1e-5
    g64, g32 = o64.grads(), o32.grads()
    assert O.metrics(g32["w1"], g64["w1"])["rms"] < 1e-4
    assert o64.apply(3e-4) == pytest.approx(o32.apply(3e-4), rel=1e-5)


def test_teacher_forced_oracle_does_not_drift():
    """force_from copies the whole state (parameters, statistics, shadow, Adam moments): after it the float32 oracle's
    next forward differs from the float64 one by rounding only, and evaluate keeps its BatchNorm outputs as taps"""
    cfg = {"max_n": 16, "seed": 2, "dropout": 0.5, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 0.05,
           "focal_gamma": 2.0, "focal_alpha": 0.25, "label_smoothing": 0.1, "clip_norm": 1.0, "ema_decay": 0.999,
           "bn_momentum": 0.1}
    o64, otf = O.pair(O.default_params(1), cfg)
    y = (np.arange(16) % 2).astype(np.float32)
    for k in range(3):
        x = O.features(20 + k, 16)
        o64.accumulate(x, y)
        otf.accumulate(x, y)
        assert float((otf.taps["z1"].double() - o64.taps["z1"]).abs().max()) < 2e-5
        o64.apply(1e-3)
        otf.apply(1e-3)
        otf.force_from(o64)
        e64, etf = o64.export(), otf.export()
        for f in O.FIELDS:
            assert np.array_equal(etf[f], e64[f].astype(np.float32)), f
        m64 = o64.opt.state[o64.tensors["w1"]]["exp_avg"]
        assert torch.equal(otf.opt.state[otf.tensors["w1"]]["exp_avg"], m64.float())
    held = O.features(30, 8)
    z64, ztf = o64.evaluate(held, True), otf.evaluate(held, True)
    assert O.metrics(ztf, z64)["rms"] < 1e-5
    assert o64.taps["z1"].shape == (8, 512) and otf.taps["z2"].shape == (8, 256)

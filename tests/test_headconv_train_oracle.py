"""CPU: the oracle of the head trainer's conv stage (tests/headconv_train_oracle.py) against independent statements of
the same arithmetic - b0_layer_oracle's head op (layout and eps), the closed-form backward the kernels implement, and
the two learning rates `dfd_head_train_apply` documents."""
import numpy as np
import torch

import b0_layer_oracle as B
import head_train_oracle as O
import headconv_train_oracle as CO
import rtdfd_amd
from rtdfd_amd import head_training as T


def _cfg(**kw):
    base = dict(max_n=16, seed=3, dropout=0.5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, focal_gamma=2.0, focal_alpha=0.25,
                label_smoothing=0.1, clip_norm=1.0, ema_decay=0.999, bn_momentum=0.1)
    base.update(kw)
    return base


def test_eval_forward_is_the_layer_oracles_head_op():
    sd = B.stress_state_dict(0)
    trunk = CO.synthetic_trunk(1, 3)
    o = CO.ConvOracle(CO.conv_params(sd), O.default_params(0), _cfg(), torch.float64)
    with torch.no_grad():
        feat, y = o.features(trunk, False)
    sd64 = B.to_torch(sd)
    a = torch.from_numpy(trunk).double().permute(0, 3, 1, 2)            # NHWC rows -> the oracle's NCHW
    want = B.op_head(sd64, a).mean(dim=(2, 3))
    assert feat.shape == (3, 1280)
    assert float((feat - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert T.BN_EPS_BACKBONE == B.EPS and o.bn.eps == B.EPS and o.bn.momentum == T.BN_MOMENTUM_BACKBONE


def test_closed_form_backward_equals_autograd():
    sd = B.stress_state_dict(0)
    conv = CO.conv_params(sd)
    for n, seed in ((2, 0), (5, 1)):
        trunk, y = CO.synthetic_trunk(10 + seed, n), (np.arange(n) % 2).astype(np.float32)
        o = CO.ConvOracle(conv, O.default_params(seed), _cfg(), torch.float64)
        o.accumulate(trunk, y)
        g = o.grads()
        dw, dg, db = CO.closed_form_backward(trunk, conv["w"], conv["g"].astype(np.float64), conv["be"].astype(np.float64),
                                             o.taps["dfeat"].numpy())
        for name, got, want in (("w", dw, g["conv.w"]), ("g", dg, g["conv.g"]), ("be", db, g["conv.be"])):
            assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), name
        assert np.abs(g["conv.w"]).max() > 0
        # running statistics: m / (m - 1) times the biased variance
        z = trunk.reshape(-1, 320).astype(np.float64) @ conv["w"].astype(np.float64).T
        rv = 0.99 * conv["rv"].astype(np.float64) + 0.01 * z.var(0, ddof=1)
        assert np.abs(o.export()["conv.rv"] - rv).max() <= 1e-12 * np.abs(rv).max()


def test_two_group_rates():
    sd = rtdfd_amd.weights.seeded_state_dict(0)
    conv, head = CO.conv_params(sd), O.default_params(0)
    o = CO.ConvOracle(conv, head, _cfg(clip_norm=1e9, weight_decay=0.0), torch.float64, lr_scale=0.1)
    lr = float(np.float32(1e-3))
    assert o.group_rates(lr) == (lr, lr * float(np.float32(0.1)))
    rs = np.random.RandomState(0)
    g = {k: rs.choice([-1.0, 1.0], size=rtdfd_amd._lib.HEAD_SHAPES[k]).astype(np.float32) for k in O.GRAD_FIELDS}
    g.update({"conv." + k: rs.choice([-1.0, 1.0], size=rtdfd_amd._lib.CONV_SHAPES[k]).astype(np.float32) for k in CO.CONV_GRAD_FIELDS})
    o.set_grads(g)
    o.apply(lr)
    assert [grp["lr"] for grp in o.opt.param_groups] == list(o.group_rates(lr))
    e = o.export()
    # Adam's first step is rate * sign(g) (eps 1e-8 aside): each group moved by its own rate
    assert np.allclose(e["w1"] - head["w1"], -lr * g["w1"], rtol=1e-6, atol=0)
    assert np.allclose(e["conv.w"] - conv["w"].astype(np.float64), -0.1 * lr * g["conv.w"], rtol=1e-6, atol=0)
    assert np.allclose(e["conv.g"] - conv["g"].astype(np.float64), -0.1 * lr * g["conv.g"], rtol=1e-6, atol=0)
    ema = o.export(True)
    assert np.allclose(ema["conv.w"] - conv["w"], 0.001 * (e["conv.w"] - conv["w"]), rtol=1e-6, atol=1e-15)

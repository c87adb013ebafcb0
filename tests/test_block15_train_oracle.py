"""CPU: the oracle of block 15's stage of the head trainer (tests/block15_train_oracle.py) against independent statements
of the same arithmetic - b0_layer_oracle's block 15 and head ops (layouts, padding, eps), the closed-form backward the
kernels implement, the state-dict names of `head_training.BLOCK_KEYS` and the three learning rates
`dfd_head_train_apply` documents."""
import numpy as np
import torch

import b0_layer_oracle as B
import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
import rtdfd_amd
from rtdfd_amd import head_training as T


def _cfg(**kw):
    base = dict(max_n=16, seed=3, dropout=0.5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, focal_gamma=2.0, focal_alpha=0.25,
                label_smoothing=0.1, clip_norm=1.0, ema_decay=0.999, bn_momentum=0.1)
    base.update(kw)
    return base


def test_block_keys_cover_block_15_of_the_state_dict():
    sd = rtdfd_amd.weights.seeded_state_dict(0)
    want = {k for k in sd if k.startswith("net._blocks.15.")}
    assert set(T.BLOCK_KEYS) == want and len(want) == 22
    shapes = rtdfd_amd._lib.BLOCK_SHAPES
    fields = [f for f in T.BLOCK_KEYS.values() if not f.startswith("nbt")]
    assert sorted(fields) == sorted(rtdfd_amd._lib.BLOCK_FIELDS) == sorted(shapes)
    for k, f in T.BLOCK_KEYS.items():
        if f.startswith("nbt"):
            assert k.endswith("num_batches_tracked") and np.asarray(sd[k]).shape == ()
            continue
        assert int(np.prod(sd[k].shape)) == int(np.prod(shapes[f])), k
        assert sd[k].shape == T.BLOCK_SD_SHAPES.get(f, shapes[f]), k
        assert tuple(d for d in sd[k].shape if d != 1) == tuple(d for d in shapes[f] if d != 1), k
    assert sorted(T.BLOCK_TRACKED) == sorted(k for k in want if k.endswith("num_batches_tracked")) and len(T.BLOCK_TRACKED) == 3
    trainable = sum(int(np.prod(shapes[f])) for f in BO.BLOCK_GRAD_FIELDS)
    assert trainable == 717232 and len(BO.BLOCK_GRAD_FIELDS) == 13
    assert rtdfd_amd._lib.BLOCK14_ROW == 9408 == BO.BlockOracle.row_width


def test_eval_forward_is_the_layer_oracles_block_15_and_head():
    sd = B.stress_state_dict(0)
    rows = BO.synthetic_rows(1, 3)
    o = BO.BlockOracle(BO.block_params(sd), CO.conv_params(sd), O.default_params(0), _cfg(), torch.float64)
    with torch.no_grad():
        x15, _, ad, gate = o.forward_block(rows, False)
        feat, _ = o.features(x15, False)
    sd64 = B.to_torch(sd)
    a = torch.from_numpy(rows).double().permute(0, 3, 1, 2)             # NHWC rows -> the oracle's NCHW
    assert B.BLOCKS[15] == (3, 1, 6, 192, 320) and not B.has_skip(15)
    d = B.op_dw(sd64, 15, B.op_expand(sd64, 15, a))
    g = B.op_gate(sd64, 15, d)
    out = B.op_out(sd64, 15, d, g, None)
    want = B.op_head(sd64, out).mean(dim=(2, 3))
    for name, got, ref in (("dw", ad, d), ("gate", gate, g), ("out", x15, out), ("feat", feat, want)):
        assert got.shape == ref.shape, name
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name
    for bn in (o.bn0, o.bn1, o.bn2):
        assert bn.eps == B.EPS == T.BN_EPS_BACKBONE and bn.momentum == T.BN_MOMENTUM_BACKBONE
    # evaluate() is this forward and the head, and leaves parameters and statistics alone
    before = o.export()
    z = o.evaluate(rows)
    assert z.shape == (3,) and all(np.array_equal(before[k], v) for k, v in o.export().items())


def test_closed_form_backward_equals_autograd():
    sd = B.stress_state_dict(0)
    block, conv = BO.block_params(sd), CO.conv_params(sd)
    n, seed = 3, 1
    rows, y = BO.synthetic_rows(10 + seed, n), (np.arange(n) % 2).astype(np.float32)
    o = BO.BlockOracle(block, conv, O.default_params(seed), _cfg(), torch.float64)
    o.accumulate(rows, y)
    g = o.grads()
    dx = BO.conv_input_gradient(o.taps["b15.out"].numpy(), conv["w"], conv["g"].astype(np.float64), conv["be"].astype(np.float64),
                                o.taps["dfeat"].numpy())
    want_dx = o.taps["b15.dout"].numpy().reshape(-1, 320)
    assert np.abs(want_dx).max() > 0 and np.abs(dx - want_dx).max() <= 1e-10 * np.abs(want_dx).max()
    cf = BO.closed_form_backward(rows, block, dx)
    for k in BO.BLOCK_GRAD_FIELDS:
        want = g["b15." + k]
        assert np.abs(want).max() > 0, k
        # be2's gradient is the column sum of dX15, zero in exact arithmetic (the conv stage's BatchNorm takes a constant
        # per input channel out again): both sides hold rounding noise, measured against the size of the summed terms
        size = np.abs(want).max() if k != "be2" else np.abs(want_dx).sum(0).max()
        assert np.abs(cf[k].reshape(want.shape) - want).max() <= 1e-10 * size, k
    assert np.abs(g["b15.be2"]).max() <= 1e-12 * np.abs(want_dx).sum(0).max()
    want = o.taps["b15.dae"].numpy().reshape(-1, 1152)
    assert np.abs(cf["dae"] - want).max() <= 1e-10 * np.abs(want).max()
    # running statistics: m / (m - 1) times the biased variance
    z = rows.reshape(-1, 192).astype(np.float64) @ block["exp_w"].astype(np.float64).T
    rv = 0.99 * block["rv0"].astype(np.float64) + 0.01 * z.var(0, ddof=1)
    assert np.abs(o.export()["b15.rv0"] - rv).max() <= 1e-12 * np.abs(rv).max()


def test_storage_rounding_moves_little_and_only_with_store():
    sd = B.stress_state_dict(0)
    block, conv, head = BO.block_params(sd), CO.conv_params(sd), O.default_params(2)
    rows, y = BO.synthetic_rows(3, 5), (np.arange(5) % 2).astype(np.float32)
    o64, o32, ost = BO.triple(block, conv, head, _cfg())
    l64, l32, lst = (o.accumulate(rows, y)[0] for o in (o64, o32, ost))
    share = BO.storage_share(o64, o32, ost, (l64, l32, lst))
    assert lst != l64 and abs(lst - l64) < 1e-5 * abs(l64)
    assert set(share) == {"loss", "logits", "max"} | {"grad " + k for k in o64.grads()}
    assert 0 < share["max"] < 100 and share["max"] == max(v for k, v in share.items() if k != "max")
    plain = BO.BlockOracle(block, conv, head, _cfg(), torch.float64)
    lp, zp = plain.accumulate(rows, y)
    assert lp == l64 and np.array_equal(zp, o64.taps["z"].numpy())


def test_three_group_rates():
    sd = rtdfd_amd.weights.seeded_state_dict(0)
    block, conv, head = BO.block_params(sd), CO.conv_params(sd), O.default_params(0)
    o = BO.BlockOracle(block, conv, head, _cfg(clip_norm=1e9, weight_decay=0.0), torch.float64, lr_scale=0.1)
    lr = float(np.float32(1e-3))
    scaled = lr * float(np.float32(0.1))
    assert o.group_rates(lr) == (lr, scaled, scaled)
    rs = np.random.RandomState(0)
    L = rtdfd_amd._lib
    g = {k: rs.choice([-1.0, 1.0], size=L.HEAD_SHAPES[k]).astype(np.float32) for k in O.GRAD_FIELDS}
    g.update({"conv." + k: rs.choice([-1.0, 1.0], size=L.CONV_SHAPES[k]).astype(np.float32) for k in CO.CONV_GRAD_FIELDS})
    g.update({"b15." + k: rs.choice([-1.0, 1.0], size=L.BLOCK_SHAPES[k]).astype(np.float32) for k in BO.BLOCK_GRAD_FIELDS})
    o.set_grads(g)
    o.apply(lr)
    assert [grp["lr"] for grp in o.opt.param_groups] == list(o.group_rates(lr))
    assert sum(p.numel() for p in o.opt.param_groups[2]["params"]) == 717232
    e = o.export()
    # Adam's first step is rate * sign(g) (eps 1e-8 aside): each group moved by its own rate
    assert np.allclose(e["w1"] - head["w1"], -lr * g["w1"], rtol=1e-6, atol=0)
    assert np.allclose(e["conv.w"] - conv["w"].astype(np.float64), -0.1 * lr * g["conv.w"], rtol=1e-6, atol=0)
    for k in BO.BLOCK_GRAD_FIELDS:                          # BatchNorm parameters and squeeze-excite biases included
        assert np.allclose(e["b15." + k] - block[k].astype(np.float64), -0.1 * lr * g["b15." + k], rtol=1e-6, atol=0), k
    ema = o.export(True)
    assert np.allclose(ema["b15.proj_w"] - block["proj_w"], 0.001 * (e["b15.proj_w"] - block["proj_w"]), rtol=1e-6, atol=1e-15)
    sdo = o.state_dict(sd)
    assert set(sdo) == set(sd) and sdo["net._blocks.15._depthwise_conv.weight"].shape == (1152, 1, 3, 3)

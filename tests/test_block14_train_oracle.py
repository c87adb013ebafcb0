"""CPU: the oracle of block 14's stage of the head trainer (tests/block14_train_oracle.py) against independent statements
of the same arithmetic - a plain torch.nn.functional restatement of efficientnet_pytorch's MBConvBlock with drop_connect
under autograd, the closed-form backward the kernels implement (the 5 x 5 depthwise conv at the 7 x 7 border, the masked
BN2 gradient), the specification of the drop-connect mask with the recorded masks of the seeds the GPU tests use, and
the state-dict names of `head_training.BLOCK14_KEYS`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import b0_layer_oracle as B
import block14_history  # noqa: F401  (registers the new exports and their case with the call-history table)
import block14_train_oracle as B4
import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
import rtdfd_amd
from rtdfd_amd import head_training as T

P_REF = 0.2 * 14 / 16


def _cfg(**kw):
    base = dict(max_n=16, seed=3, dropout=0.5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, focal_gamma=2.0, focal_alpha=0.25,
                label_smoothing=0.1, clip_norm=1.0, ema_decay=0.999, bn_momentum=0.1)
    base.update(kw)
    return base


def test_block14_keys_cover_block_14_of_the_state_dict():
    sd = rtdfd_amd.weights.seeded_state_dict(0)
    want = {k for k in sd if k.startswith("net._blocks.14.")}
    assert set(T.BLOCK14_KEYS) == want and len(want) == 22
    shapes = rtdfd_amd._lib.BLOCK14_SHAPES
    assert shapes["dw_w"] == (1152, 5, 5) and shapes["proj_w"] == (192, 1152) and shapes["g2"] == shapes["rv2"] == (192,)
    assert shapes["exp_w"] == (1152, 192) and shapes["se_w1"] == (48, 1152) and shapes["se_w2"] == (1152, 48) and shapes["g0"] == (1152,)
    fields = [f for f in T.BLOCK14_KEYS.values() if not f.startswith("nbt")]
    assert sorted(fields) == sorted(rtdfd_amd._lib.BLOCK_FIELDS) == sorted(shapes)
    for k, f in T.BLOCK14_KEYS.items():
        if f.startswith("nbt"):
            assert k.endswith("num_batches_tracked") and np.asarray(sd[k]).shape == ()
            continue
        assert sd[k].shape == T.BLOCK14_SD_SHAPES.get(f, shapes[f]), k
        assert tuple(d for d in sd[k].shape if d != 1) == tuple(d for d in shapes[f] if d != 1), k
    assert len(T.BLOCK14_TRACKED) == 3
    trainable = sum(int(np.prod(shapes[f])) for f in B4.BLOCK_GRAD_FIELDS)
    assert trainable == 587952
    assert B.BLOCKS[14] == (5, 1, 6, 192, 192) and B.has_skip(14)
    assert T.DROP_CONNECT_BLOCK14 == P_REF


# --------------------------------------------------------------------------- the mask
# recorded with the trainer's hash at authoring time: the trainer seeds tests/test_block14_train_gpu.py uses, at the
# float32-rounded reference rate, counter 0 (and counter 1 where noted); 1 = kept
RECORDED = {
    (5, 3, 0): "11100", (11, 3, 0): "11100111110", (37, 3, 0): "1110011111010100111011111011111111111",
    (2, 9, 0): "00", (16, 2, 0): "1011111111110111", (5, 2, 1): "11100",
}


def test_drop_connect_keep_is_the_trainers_hash_with_a_fourth_layer():
    p32 = float(np.float32(P_REF))
    for seed in (0, 9, 1234567890123):
        for counter in (0, 1, 7):
            got = T.drop_connect_keep(seed, counter, 37, P_REF)
            assert got.shape == (37,) and got.dtype == bool
            assert np.array_equal(got, T.dropout_keep_mask(seed, counter, 3, 37, 1, p32).reshape(37))
    assert T.drop_connect_keep(3, 0, 8, 0.0).all()
    for (n, seed, counter), bits in RECORDED.items():
        got = T.drop_connect_keep(seed, counter, n, P_REF)
        assert "".join("1" if k else "0" for k in got) == bits[:n], (n, seed, counter)
    # the enumeration the GPU cases were chosen from
    keep2 = [T.drop_connect_keep(s, 0, 2, P_REF) for s in range(60)]
    assert [s for s in range(80) if not T.drop_connect_keep(s, 0, 2, P_REF).any()] == [9, 14, 50, 55, 75]
    assert sum(k.all() for k in keep2) == 40 and sum(k.sum() == 1 for k in keep2) == 16
    mixed = lambda n: sum(0 < T.drop_connect_keep(s, 0, n, P_REF).sum() < n for s in range(60))
    assert (mixed(5), mixed(11), mixed(37)) == (34, 51, 60)
    assert [s for s in range(16) if not T.drop_connect_keep(s, 0, 2, 0.5).any()] == [0, 9, 13, 14, 15]


# --------------------------------------------------------------------------- the block
def _mbconv(x, w, keep, p, eps=1e-3, momentum=0.01):
    """efficientnet_pytorch's MBConvBlock.forward (train mode, static same padding 2 for k5 at 7 x 7) with its
    utils.drop_connect, in torch.nn.functional; w: leaf tensors by field, x NCHW"""
    bn = lambda t, l: F.batch_norm(t, w[f"rm{l}"].clone(), w[f"rv{l}"].clone(), w[f"g{l}"], w[f"be{l}"], True, momentum, eps)
    swish = lambda t: t * torch.sigmoid(t)
    a = swish(bn(F.conv2d(x, w["exp_w"].reshape(1152, 192, 1, 1)), 0))
    a = swish(bn(F.conv2d(F.pad(a, (2, 2, 2, 2)), w["dw_w"].reshape(1152, 1, 5, 5), groups=1152), 1))
    s = F.adaptive_avg_pool2d(a, 1)
    s = F.conv2d(swish(F.conv2d(s, w["se_w1"].reshape(48, 1152, 1, 1), w["se_b1"])), w["se_w2"].reshape(1152, 48, 1, 1), w["se_b2"])
    a = torch.sigmoid(s) * a
    y = bn(F.conv2d(a, w["proj_w"].reshape(192, 1152, 1, 1)), 2)
    if p > 0:
        keep_prob = 1 - p
        binary = torch.from_numpy(np.asarray(keep, np.float64)).reshape(-1, 1, 1, 1)
        y = y / keep_prob * binary
    return y + x


@pytest.mark.parametrize("p,keep", [(0.0, (True, True, True)), (float(np.float32(P_REF)), (True, False, True))])
def test_block_equals_a_plain_restatement_of_mbconv_with_drop_connect(p, keep):
    sd = B.stress_state_dict(0)
    b14 = B4.block14_params(sd)
    n = 3
    rows = B4.synthetic_rows(5, n)
    o = B4.Block14Oracle(b14, BO.block_params(sd), CO.conv_params(sd), O.default_params(0), _cfg(), torch.float64, drop_connect=p)
    out, _, _, _, factor = o.forward_block14(rows, True, np.asarray(keep) if p > 0 else None)
    rs = np.random.RandomState(1)
    up = torch.from_numpy(rs.randn(n, 192, 7, 7))
    (out * up).sum().backward()
    x = B4.nchw(rows, torch.float64).requires_grad_(True)
    w = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(k in B4.BLOCK_GRAD_FIELDS) for k, v in b14.items()}
    want = _mbconv(x, w, keep, p)
    (want * up).sum().backward()
    assert float((out - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert np.array_equal(factor.numpy(), np.asarray(keep, np.float64) / (1.0 - p))
    for i in range(n):
        if not keep[i]:
            assert torch.equal(out[i].detach(), x[i].detach())          # a dropped crop is its input, bit for bit
    # the input gradient, through the oracle's own graph on a leaf input
    o2 = B4.Block14Oracle(b14, BO.block_params(sd), CO.conv_params(sd), O.default_params(0), _cfg(), torch.float64, drop_connect=p)
    leaf = B4.nchw(rows, torch.float64).requires_grad_(True)
    saved, B4.nchw = B4.nchw, (lambda r, dt: leaf)
    try:
        out2 = o2.forward_block14(rows, True, np.asarray(keep) if p > 0 else None)[0]
    finally:
        B4.nchw = saved
    (out2 * up).sum().backward()
    assert float((leaf.grad - x.grad).abs().max()) <= 1e-11 * float(x.grad.abs().max())
    g = o.grads()
    for k in B4.BLOCK_GRAD_FIELDS:
        ref = w[k].grad.numpy().reshape(g["b14." + k].shape)
        assert np.abs(ref).max() > 0, k
        assert np.abs(g["b14." + k] - ref).max() <= 1e-10 * np.abs(ref).max(), k
    # running statistics move before the mask: a dropped crop contributes
    z = rows.reshape(-1, 192).astype(np.float64) @ b14["exp_w"].astype(np.float64).T
    rv = 0.99 * b14["rv0"].astype(np.float64) + 0.01 * z.var(0, ddof=1)
    assert np.abs(o.export()["b14.rv0"] - rv).max() <= 1e-12 * np.abs(rv).max()


@pytest.mark.parametrize("p,seed", [(0.0, 4), (float(np.float32(P_REF)), 3)])
def test_closed_form_backward_equals_autograd(p, seed):
    sd = B.stress_state_dict(0)
    b14, b15, conv = B4.block14_params(sd), BO.block_params(sd), CO.conv_params(sd)
    n = 5
    rows, y = B4.synthetic_rows(20, n), (np.arange(n) % 2).astype(np.float32)
    o = B4.Block14Oracle(b14, b15, conv, O.default_params(1), _cfg(seed=seed), torch.float64, drop_connect=p)
    keep = o.keep(n)
    assert keep.all() if p == 0 else (0 < keep.sum() < n)      # seed 3 at n = 5: crops 3 and 4 dropped
    o.accumulate(rows, y)
    g = o.grads()
    factor = o.taps["b14.keep"].numpy()
    assert np.array_equal(factor, keep / (1.0 - p))
    dout = o.taps["b14.dout"].numpy().reshape(-1, 192)
    # dOut14 = dZe15 . We15: block 15's closed form from dX15 gives dae15, BN0's backward, and the product
    x14 = o.taps["b14.out"].numpy()
    cf15 = BO.closed_form_backward(x14, b15, o.taps["b15.dout"].numpy().reshape(-1, 320))
    we15 = b15["exp_w"].astype(np.float64).reshape(1152, 192)
    xh0, istd0, ye = BO._bn_fwd(x14.reshape(-1, 192) @ we15.T, b15["g0"].astype(np.float64), b15["be0"].astype(np.float64), 1e-3)
    dze15, _, _ = BO._bn_bwd(cf15["dae"] * BO._dswish(ye), xh0, istd0, b15["g0"].astype(np.float64))
    assert np.abs(dze15 @ we15 - dout).max() <= 1e-10 * np.abs(dout).max()
    cf = B4.closed_form_backward(rows, b14, dout, factor)
    assert np.abs(cf["out"] - x14.reshape(-1, 192)).max() <= 1e-12 * np.abs(x14).max()
    masked = dout * np.repeat(factor, 49)[:, None]
    for k in B4.BLOCK_GRAD_FIELDS:
        want = g["b14." + k]
        assert np.abs(want).max() > 0, k
        # with every crop kept be2's gradient is the column sum of dOut14, zero in exact arithmetic (block 15's train-mode
        # BN0 removes a per-channel constant): rounding noise, measured against the size of the summed terms
        size = np.abs(want).max() if not (k == "be2" and p == 0) else np.abs(masked).sum(0).max()
        assert np.abs(cf[k].reshape(want.shape) - want).max() <= 1e-10 * size, k
    if p == 0:
        assert np.abs(g["b14.be2"]).max() <= 1e-12 * np.abs(dout).sum(0).max()
    want = o.taps["b14.dae"].numpy().reshape(-1, 1152)
    assert np.abs(cf["dae"] - want).max() <= 1e-10 * np.abs(want).max()
    # the 7 x 7 border: a corner output of the 5 x 5 conv sees 9 of its 25 taps
    ae = torch.zeros(1, 1152, 7, 7, dtype=torch.float64)
    ae[:, :, :3, :3] = 1.0
    with torch.no_grad():
        corner = o.dw14(o.pad14(ae))[0, :, 0, 0]
        inside = o.dw14(o.pad14(torch.ones(1, 1152, 7, 7, dtype=torch.float64)))[0, :, 0, 0]
    wd = o.dw14.weight.detach()[:, 0]
    assert torch.allclose(corner, wd[:, 2:, 2:].sum((1, 2)), rtol=1e-12, atol=0) and torch.allclose(inside, corner, rtol=1e-12, atol=0)


def test_storage_share_covers_block_14_and_four_group_rates():
    sd = B.stress_state_dict(0)
    b14, b15, conv, head = B4.block14_params(sd), BO.block_params(sd), CO.conv_params(sd), O.default_params(2)
    rows, y = B4.synthetic_rows(3, 5), (np.arange(5) % 2).astype(np.float32)
    o64, o32, ost = B4.triple(b14, b15, conv, head, _cfg())
    l64, l32, lst = (o.accumulate(rows, y)[0] for o in (o64, o32, ost))
    share = B4.storage_share(o64, o32, ost, (l64, l32, lst))
    assert {"grad b14." + k for k in B4.BLOCK_GRAD_FIELDS} | {"tap " + k for k in B4.TAPS} <= set(share)
    assert 0 < share["max"] < 100 and share["max"] == max(v for k, v in share.items() if k != "max")
    lr = float(np.float32(1e-3))
    scaled = lr * float(np.float32(0.1))
    assert o64.group_rates(lr) == (lr, scaled, scaled, scaled)
    assert sum(p.numel() for p in o64.opt.param_groups[3]["params"]) == 587952
    sdo = o64.state_dict(sd)
    assert set(sdo) == set(sd) and sdo["net._blocks.14._depthwise_conv.weight"].shape == (1152, 1, 5, 5)

"""CPU: the oracle of the head trainer with block 11 unfrozen (tests/block11_train_oracle.py) against independent statements
of the same arithmetic - the inference oracle's eval forward of block 11 (tests/b0_layer_oracle.py: the pad 1 / 2, the
stride and the squeeze width), a plain torch.nn.functional restatement of block 11 under float64 autograd (every parameter
gradient, the running statistics), the closed form of the stride-2 depthwise input gradient as the kernel gathers it - the
RECORDED masks of the trainer seeds the GPU tests use, the preconditions of every GPU case on the oracles alone, the
state-dict names of `head_training.BLOCK11_KEYS`, and a list of planted defects the comparison must catch at the project's bars.

Defects carried (each fails `test_a_corrupted_block_11_fails_the_comparison` at the bars, so a device kernel with the same
defect cannot pass tests/test_block11_train_gpu.py): the padding the wrong way round (2 before, 1 after), the
squeeze-excite pool divided by the 196 input positions instead of the 49 output positions, an identity skip added."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import b0_layer_oracle as B
import block11_history  # noqa: F401  (registers the new exports and their case with the call-history table)
import block11_train_cases as C
import block11_train_oracle as B1
import block12_train_oracle as B2
import head_train_oracle as O
import rtdfd_amd
from rtdfd_amd import head_training as T


def test_block11_keys_cover_the_block_of_the_state_dict():
    sd = rtdfd_amd.weights.seeded_state_dict(0)
    shapes = rtdfd_amd._lib.BLOCK11_SHAPES
    want = {k for k in sd if k.startswith("net._blocks.11.")}
    assert set(T.BLOCK11_KEYS) == want and len(want) == 22 and len(T.BLOCK11_TRACKED) == 3
    assert rtdfd_amd._lib.BLOCK_SHAPES_AT[11] == shapes
    for k, f in T.BLOCK11_KEYS.items():
        if f.startswith("nbt"):
            assert k.endswith("num_batches_tracked") and np.asarray(sd[k]).shape == ()
            continue
        assert sd[k].shape == T.BLOCK11_SD_SHAPES.get(f, shapes[f]), k
    assert B.BLOCKS[11] == (5, 2, 6, 112, 192) and not B.has_skip(11)        # k5, stride 2, expand 6, 112 -> 192, no skip
    assert B.BLOCKS[10][4] == 112 and B.BLOCKS[12][3] == 192
    assert B1.C_SE == int(112 * 0.25) == 28 and B1.C_EXP == 6 * 112
    floats = sum(int(np.prod(shapes[k])) for k in B1.BLOCK_GRAD_FIELDS)
    assert floats == 262492                                     # the arena's static_assert


# --------------------------------------------------------------------------- the masks
# recorded with the trainer's hash at authoring time: (n, trainer seed, counter) -> the masks of blocks 14, 13, 12 at the
# float32-rounded reference rates 0.175, 0.1625, 0.15; 1 = kept.  The trainer seeds tests/test_block11_train_gpu.py uses.
RECORDED = {
    (2, 44, 0): ("11", "01", "10"),                                                   # the three differ pairwise
    (11, 7, 0): ("11010100110", "11111010111", "11111100111"),                        # crop 7 dropped in all three, crop 2 in block 14 only
    (37, 2, 0): ("1011111111110111111100111111111101111", "1111011111111100111111111111110101111",
                 "1110101111111111111111110111111101111"),                            # crop 32 dropped in all three, crop 1 in block 14 only
    (2, 0, 0): ("11", "11", "00"),                                                    # block 12 drops both crops, 13 and 14 keep both
    (16, 0, 0): ("1111111111001111", "1111110111101111", "0011101010111010"),         # two accumulates: counter 0 ..
    (5, 0, 1): ("10100", "11100", "11110"),                                           # .. and counter 1
}


def test_the_recorded_masks_are_what_the_hash_draws():
    for (n, seed, counter), want in RECORDED.items():
        got = C.masks(seed, counter, n)
        assert tuple(C.bits(got[b]) for b in (14, 13, 12)) == want, (n, seed, counter)
    assert C.pick_drop12_seed() == C.DROP12_SEED == 0           # the enumeration the seed came from
    assert (C.MASK_SEED[2], C.MASK_SEED[11], C.MASK_SEED[37], C.ACC_MASK_SEED) == (44, 7, 2, 0)
    m = C.masks(C.DROP12_SEED, 0, 2)
    assert not m[12].any() and m[13].all() and m[14].all()
    for n in (2, 11, 37):                                       # the masks of the three blocks differ
        m = C.masks(C.MASK_SEED[n], 0, n)
        assert len({C.bits(m[b]) for b in m}) == 3 and all(m[b].any() for b in m)
    with pytest.raises(ValueError):
        T.drop_connect_keep(0, 0, 4, 0.1, block=11)             # block 11 has no drop-connect


# --------------------------------------------------------------------------- block 11 against the inference oracle
def test_eval_forward_of_block_11_is_the_inference_oracles():
    """the float64 oracle's eval forward of block 11 on "b10.out" equals b0_layer_oracle.forward_taps's "b11.out" at float64
    rounding: the pad 1 / 2, the stride, the squeeze width and the pool over 49 are the inference network's"""
    sd = C.stress_sd()
    x = torch.from_numpy(B.random_crops(3, 5)).double()
    taps = B.forward_taps(B.to_torch(sd, torch.float64), x)
    b11, below, b14, b15, conv = C.start()
    o = B1.Block11Oracle(b11, below, b14, b15, conv, O.default_params(0), C.default_cfg(), torch.float64)
    with torch.no_grad():
        out, ae, ad, gate = o.forward_block11(taps["b10.out"], False)
        out12 = o.forward_skip(12, out, False)[0]
    want = taps["b11.out"]
    assert out.shape == want.shape == (3, 192, 7, 7) and ae.shape == (3, 672, 14, 14) and ad.shape == (3, 672, 7, 7)
    err = float((out - want).abs().max() / want.abs().max())
    print(f"b11.out against the inference oracle: max rel {err:.3e}")
    assert err <= 1e-12                                         # BatchNorm folded or not: a few float64 roundings
    assert float((gate - taps["b11.gate"]).abs().max()) <= 1e-12
    assert float((out12 - taps["b12.out"]).abs().max() / taps["b12.out"].abs().max()) <= 1e-12


# --------------------------------------------------------------------------- block 11 under autograd
def _block11_functional(x, w, eps=1e-3, momentum=0.01):
    """efficientnet_pytorch's MBConvBlock.forward of block 11 (train mode; Conv2dStaticSamePadding pads 14 -> 17 with
    (3 // 2, 3 - 3 // 2) = (1, 2) on both axes) in torch.nn.functional; w: leaf tensors by field, x NCHW"""
    bn = lambda t, l: F.batch_norm(t, w[f"rm{l}"], w[f"rv{l}"], w[f"g{l}"], w[f"be{l}"], True, momentum, eps)
    swish = lambda t: t * torch.sigmoid(t)
    a = swish(bn(F.conv2d(x, w["exp_w"].reshape(672, 112, 1, 1)), 0))
    a = swish(bn(F.conv2d(F.pad(a, (1, 2, 1, 2)), w["dw_w"].reshape(672, 1, 5, 5), stride=2, groups=672), 1))
    s = F.adaptive_avg_pool2d(a, 1)
    s = F.conv2d(swish(F.conv2d(s, w["se_w1"].reshape(28, 672, 1, 1), w["se_b1"])), w["se_w2"].reshape(672, 28, 1, 1), w["se_b2"])
    return bn(F.conv2d(torch.sigmoid(s) * a, w["proj_w"].reshape(192, 672, 1, 1)), 2)


@pytest.mark.parametrize("n", [2, 5])
def test_oracle_equals_torch_float64_autograd_of_block_11(n):
    b11, below, b14, b15, conv = C.start()
    rows, y = B1.synthetic_rows(40 + n, n), (np.arange(n) % 2).astype(np.float32)
    p14, drops = C.rates_of("ref")
    o = B1.Block11Oracle(b11, below, b14, b15, conv, O.default_params(1), C.default_cfg(seed=3), torch.float64, drop_connect=p14, drops=drops)
    o.accumulate(rows, y)
    up = o.taps["b11.dout"].reshape(n, 7, 7, 192).permute(0, 3, 1, 2)       # the gradient block 12 hands down drives the restatement
    w = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(k in B1.BLOCK_GRAD_FIELDS) for k, v in b11.items()}
    out = _block11_functional(B1.nchw(rows, torch.float64), w)
    (out * up).sum().backward()
    rel = lambda got, want: float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(np.asarray(want)).max())
    assert rel(o.taps["b11.out"].numpy(), B1.nhwc(out).numpy()) <= 1e-12
    g, e = o.grads(), o.export()
    for k in B1.BLOCK_GRAD_FIELDS:
        ref = w[k].grad.numpy().reshape(g["b11." + k].shape)
        assert np.abs(ref).max() > 0, k
        assert rel(g["b11." + k], ref) <= 1e-9, k
    for k in B1.BLOCK_STAT_FIELDS:
        assert not np.array_equal(w[k].numpy().reshape(-1), b11[k].astype(np.float64).reshape(-1)), k
        assert rel(e["b11." + k].reshape(-1), w[k].numpy().reshape(-1)) <= 1e-9, k
    # block 12 hands down dOut12 + dZe12 . We12: the closed form of tests/block12_train_oracle.py on block 12's own taps
    got = B2.skip_input_gradient(o.taps["b11.out"].numpy(), below[12], o.taps["b12.dout"].numpy(), o.taps["b12.dae"].numpy())
    assert rel(got, o.taps["b11.dout"].numpy().reshape(-1, 192)) <= 1e-9
    assert o.taps["b11.dae"].shape == (n, 196, 672) and o.taps["b11.ad"].shape == (n, 49, 672) and o.taps["b11.gate"].shape == (n, 672)
    assert "b11.keep" not in o.taps
    lr = float(np.float32(1e-3))
    assert o.group_rates(lr) == (lr,) + (lr * float(np.float32(0.1)),) * 6 and len(o.opt.param_groups) == 7
    assert [sum(p.numel() for p in grp["params"]) for grp in o.opt.param_groups[3:]] == [587952] * 3 + [262492]
    sd = C.stress_sd()
    sdo = o.state_dict(sd)
    assert set(sdo) == set(sd) and sdo["net._blocks.11._depthwise_conv.weight"].shape == (672, 1, 5, 5)


def test_the_gathered_depthwise_input_gradient_is_autograds():
    """the parity rule of the stride-2 input gradient (even iy: ky in {1, 3}; odd iy: ky in {0, 2, 4}) against autograd of
    the padded strided conv; and the tap counts the issue states"""
    rs = np.random.RandomState(3)
    n = 2
    ae = torch.from_numpy(rs.randn(n, B1.C_EXP, 14, 14)).requires_grad_(True)
    wd = torch.from_numpy(rs.randn(B1.C_EXP, 1, 5, 5))
    dzd = torch.from_numpy(rs.randn(n, B1.C_EXP, 7, 7))
    zd = F.conv2d(nn.ZeroPad2d(B1.PAD)(ae), wd, stride=2, groups=B1.C_EXP)
    assert zd.shape == dzd.shape
    (zd * dzd).sum().backward()
    got = B1.depthwise_input_gradient(dzd.permute(0, 2, 3, 1).numpy(), wd.numpy())
    want = ae.grad.permute(0, 2, 3, 1).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # live taps: output (oy, ox) reads input (2 oy - 1 + ky, 2 ox - 1 + kx)
    live = lambda oy, ox: sum(0 <= 2 * oy - 1 + ky < 14 and 0 <= 2 * ox - 1 + kx < 14 for ky in range(5) for kx in range(5))
    assert live(6, 6) == 9 and live(0, 0) == 16 and live(3, 3) == 25
    # an input element sums 4, 6 or 9 taps before the border removes some
    ones = B1.depthwise_input_gradient(np.ones((1, 7, 7, B1.C_EXP)), np.ones((B1.C_EXP, 5, 5)))[0, :, :, 0]
    assert ones[2, 2] == 4 and ones[2, 3] == 6 and ones[3, 3] == 9 and ones[0, 0] == 1 and ones[13, 13] == 4 and ones[13, 12] == 4
    assert set(np.unique(ones[1:12, 1:12])) == {4.0, 6.0, 9.0}


# --------------------------------------------------------------------------- planted defects
def _corrupt_pad(o):
    o.b11.pad = nn.ZeroPad2d((2, 1, 2, 1))


def _corrupt_pool(o):
    o.b11.pool_positions = B1.HW_IN


def _corrupt_skip(o):
    o.b11.skip = True


@pytest.mark.parametrize("defect", [_corrupt_pad, _corrupt_pool, _corrupt_skip], ids=["pad_2_1", "pool_over_196", "skip_added"])
def test_a_corrupted_block_11_fails_the_comparison(defect):
    """a float64 oracle with the defect, held to the float64 reference at the project's bars (the float32 oracle is the
    yardstick) as the device is in tests/test_block11_train_gpu.py: block 11's output, the logits and block 11's gradients
    must miss their bars"""
    n = 5
    x = C.cpu_rows()[:n]
    head, ya, yb, lam, scale = C.case_inputs(3, n, "plain")
    o64, o32 = C.oracles(head, C.default_cfg(seed=3), n=2)
    bad = C.oracles(head, C.default_cfg(seed=3), n=2)[0]
    defect(bad)
    for o in (o64, o32, bad):
        o.accumulate(x, ya, yb, lam, scale)
    ratios = {k: O.bar_ratio(bad.taps[k].numpy(), o64.taps[k].numpy(), o32.taps[k].numpy())["ratio"] for k in ("b11.out", "b11.dae", "z")}
    g, g64, g32 = bad.grads(), o64.grads(), o32.grads()
    ratios.update({k: O.bar_ratio(g[k], g64[k], g32[k])["ratio"] for k in ("b11.exp_w", "b11.dw_w", "b11.proj_w")})
    print({k: f"{v:.3g}" for k, v in ratios.items()})
    assert all(v > 1.0 for v in ratios.values()), ratios
    same = C.oracles(head, C.default_cfg(seed=3), n=2)[0]       # and without a defect the comparison passes at zero
    same.accumulate(x, ya, yb, lam, scale)
    assert O.bar_ratio(same.taps["b11.out"].numpy(), o64.taps["b11.out"].numpy(), o32.taps["b11.out"].numpy())["ratio"] == 0.0


# --------------------------------------------------------------------------- the preconditions of the GPU cases
@pytest.mark.parametrize("kind,n,variant,rates", C.single_cases())
def test_preconditions_of_the_single_accumulates(kind, n, variant, rates):
    seed, tseed = C.case_seeds(kind, n, rates)
    x = C.cpu_rows()[:n] if kind == "real" else B1.synthetic_rows(seed + 100, n)
    o64, o32, ost, losses, (ya, yb, lam, _) = C.run_oracles(x, seed, tseed, variant, rates)
    margin, rshare, sshare, worst = C.preconditions(o64, o32, ost, losses, ya, yb, lam)
    print(f"n {n} {variant} {rates}: gate margin {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f} ({worst})")
    assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5
    if rates == "ref":
        want = C.masks(tseed, 0, n)
        for b in want:
            assert np.array_equal(o64.taps[f"b{b}.keep"].numpy() != 0, want[b]), b
    else:
        assert all(bool((o64.taps[f"b{b}.keep"] == 1).all()) for b in (14, 13, 12))
    if kind == "real" and variant == "plain":                   # what was measured when the seed was picked
        m0, r0, s0, count = C.PICKED[(n, rates)]
        assert 0 < count <= 60 and m0 >= 1.0 and r0 <= 1.0 and s0 <= 0.5


def test_preconditions_of_the_all_dropped_the_two_accumulate_and_the_eval_cases():
    x = C.cpu_rows()[:2]
    o64, o32, ost, losses, (ya, yb, lam, _) = C.run_oracles(x, C.DROP_SEED, C.DROP12_SEED, "plain", "ref")
    margin, rshare, sshare, worst = C.preconditions(o64, o32, ost, losses, ya, yb, lam)
    print(f"block 12 all dropped: gate margin {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f} ({worst})")
    assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5
    assert torch.equal(o64.taps["b11.dout"], o64.taps["b12.dout"])            # dX12 == dOut12, element for element
    assert torch.equal(o64.taps["b12.out"], o64.taps["b11.out"])
    g = o64.grads()
    for k in B1.BLOCK_GRAD_FIELDS:
        assert not g["b12." + k].any() and g["b11." + k].any() and g["b13." + k].any(), k
    margin, rshare, sshare = C.acc_figures(C.cpu_rows(), C.ACC_SEED)
    print(f"two accumulates, the worse: gate margin {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f}")
    assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5
    live, ema = C.eval_margins(C.cpu_rows()[:5], C.EVAL_SEED)
    print(f"eval: gate margins {live:.2f} (live) {ema:.2f} (EMA)")
    assert live >= 1.0 and ema >= 1.0


def test_storage_share_covers_block_11():
    rows, y = B1.synthetic_rows(3, 5), (np.arange(5) % 2).astype(np.float32)
    o64, o32, ost = C.oracles(O.default_params(2), C.default_cfg())
    losses = tuple(o.accumulate(rows, y)[0] for o in (o64, o32, ost))
    share = B1.storage_share(o64, o32, ost, losses)
    for b in (14, 13, 12, 11):
        assert {f"grad b{b}." + k for k in B1.BLOCK_GRAD_FIELDS} <= set(share), b
    assert {"tap " + k for k in B1.TAPS} <= set(share)
    assert 0 < share["max"] < 100 and share["max"] == max(v for k, v in share.items() if k != "max")
    assert set(C.forced_grads(1)) == set(o64.grads())

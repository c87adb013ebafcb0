"""CPU: the oracle of the head trainer with blocks 13 and 12 unfrozen (tests/block12_train_oracle.py) against independent
statements of the same arithmetic - a plain torch.nn.functional restatement of the chain 12 -> 13 -> 14 -> 15 under float64
autograd with given per-block masks (every parameter gradient, dX of every block, the running statistics), the closed form
of the gradient a skip block hands down, dX_b = dOut_b + dZe_b . We_b - the specification of the per-block drop-connect
masks with the RECORDED masks of the trainer seeds the GPU tests use, the preconditions of every GPU case on the oracles
alone, and the state-dict names of `head_training.BLOCK13_KEYS` / `BLOCK12_KEYS`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import b0_layer_oracle as B
import block12_history  # noqa: F401  (registers the new exports and their case with the call-history table)
import block12_train_cases as C
import block12_train_oracle as B2
import block14_train_oracle as B4
import block15_train_oracle as BO
import head_train_oracle as O
import rtdfd_amd
from rtdfd_amd import head_training as T


def test_block13_and_block12_keys_cover_their_blocks_of_the_state_dict():
    sd = rtdfd_amd.weights.seeded_state_dict(0)
    shapes = rtdfd_amd._lib.BLOCK14_SHAPES
    for b, keys, tracked, sd_shapes in ((13, T.BLOCK13_KEYS, T.BLOCK13_TRACKED, T.BLOCK13_SD_SHAPES),
                                        (12, T.BLOCK12_KEYS, T.BLOCK12_TRACKED, T.BLOCK12_SD_SHAPES)):
        want = {k for k in sd if k.startswith(f"net._blocks.{b}.")}
        assert set(keys) == want and len(want) == 22
        assert rtdfd_amd._lib.BLOCK_SHAPES_AT[b] == shapes
        for k, f in keys.items():
            if f.startswith("nbt"):
                assert k.endswith("num_batches_tracked") and np.asarray(sd[k]).shape == ()
                continue
            assert sd[k].shape == sd_shapes.get(f, shapes[f]), k
        assert len(tracked) == 3
        assert B.BLOCKS[b] == (5, 1, 6, 192, 192) and B.has_skip(b)          # block 14's geometry exactly
    assert B.BLOCKS[11][4] == 192 and B.BLOCKS[11][1] == 2                   # block 11 ends at 7 x 7 x 192: block 12's input rows
    assert np.allclose((T.DROP_CONNECT_BLOCK14, T.DROP_CONNECT_BLOCK13, T.DROP_CONNECT_BLOCK12), (0.175, 0.1625, 0.15), rtol=1e-15, atol=0)
    assert C.RATES == {b: 0.2 * b / 16 for b in (14, 13, 12)}


# --------------------------------------------------------------------------- the masks
# recorded with the trainer's hash at authoring time: (n, trainer seed, counter) -> the masks of blocks 14, 13, 12 at the
# float32-rounded reference rates 0.175, 0.1625, 0.15; 1 = kept.  The trainer seeds tests/test_block12_train_gpu.py uses.
RECORDED = {
    (2, 44, 0): ("11", "01", "10"),                                                   # the three differ pairwise
    (11, 7, 0): ("11010100110", "11111010111", "11111100111"),                        # crop 7 dropped in all three, crop 2 in block 14 only
    (37, 2, 0): ("1011111111110111111100111111111101111", "1111011111111100111111111111110101111",
                 "1110101111111111111111110111111101111"),                            # crop 32 dropped in all three, crop 1 in block 14 only
    (2, 17, 0): ("11", "00", "11"),                                                   # block 13 drops both crops, the others keep both
    (16, 0, 0): ("1111111111001111", "1111110111101111", "0011101010111010"),         # two accumulates: counter 0 ..
    (5, 0, 1): ("10100", "11100", "11110"),                                           # .. and counter 1
}


def test_drop_connect_keep_draws_block_b_with_layer_17_minus_b():
    for b in (14, 13, 12):
        p32 = float(np.float32(C.RATES[b]))
        for seed in (0, 9, 1234567890123):
            for counter in (0, 1, 7):
                got = T.drop_connect_keep(seed, counter, 37, C.RATES[b], block=b)
                assert got.shape == (37,) and got.dtype == bool
                assert np.array_equal(got, T.dropout_keep_mask(seed, counter, 17 - b, 37, 1, p32).reshape(37))
    for seed in (0, 3, 9):                                      # the default is block 14: today's function, layer 3
        assert np.array_equal(T.drop_connect_keep(seed, 1, 16, 0.175), T.drop_connect_keep(seed, 1, 16, 0.175, block=14))
        assert np.array_equal(T.drop_connect_keep(seed, 1, 16, 0.175), T.dropout_keep_mask(seed, 1, 3, 16, 1, float(np.float32(0.175))).reshape(16))
    # the same rate under another layer index is another draw: the blocks drop independently
    assert any(not np.array_equal(T.drop_connect_keep(s, 0, 37, 0.175, block=14), T.drop_connect_keep(s, 0, 37, 0.175, block=13)) for s in range(4))
    with pytest.raises(ValueError):
        T.drop_connect_keep(0, 0, 4, 0.1, block=11)
    for (n, seed, counter), want in RECORDED.items():
        got = C.masks(seed, counter, n)
        assert tuple(C.bits(got[b]) for b in (14, 13, 12)) == want, (n, seed, counter)
    assert C.pick_mask_seeds() == (C.MASK_SEED, C.DROP13_SEED, C.ACC_MASK_SEED)       # the enumeration the seeds came from
    for n in (11, 37):                                          # one crop dropped in all three blocks, one in exactly one
        m = C.masks(C.MASK_SEED[n], 0, n)
        dropped = sum((~m[b]).astype(int) for b in m)
        assert (dropped == 3).any() and (dropped == 1).any()
        d2 = (~m[14]).astype(int) + (~m[13]).astype(int)        # and the same at depth 13, over its two blocks
        assert (d2 == 2).any() and (d2 == 1).any()


# --------------------------------------------------------------------------- the chain under autograd
def _mbconv(x, w, keep, p, ks, out_c, skip, eps=1e-3, momentum=0.01):
    """efficientnet_pytorch's MBConvBlock.forward (train mode, static same padding at 7 x 7) with its utils.drop_connect, in
    torch.nn.functional; w: leaf tensors by field (running statistics are updated in place), x NCHW"""
    bn = lambda t, l: F.batch_norm(t, w[f"rm{l}"], w[f"rv{l}"], w[f"g{l}"], w[f"be{l}"], True, momentum, eps)
    swish = lambda t: t * torch.sigmoid(t)
    pad = ks // 2
    a = swish(bn(F.conv2d(x, w["exp_w"].reshape(1152, 192, 1, 1)), 0))
    a = swish(bn(F.conv2d(F.pad(a, (pad, pad, pad, pad)), w["dw_w"].reshape(1152, 1, ks, ks), groups=1152), 1))
    s = F.adaptive_avg_pool2d(a, 1)
    s = F.conv2d(swish(F.conv2d(s, w["se_w1"].reshape(48, 1152, 1, 1), w["se_b1"])), w["se_w2"].reshape(1152, 48, 1, 1), w["se_b2"])
    a = torch.sigmoid(s) * a
    y = bn(F.conv2d(a, w["proj_w"].reshape(out_c, 1152, 1, 1)), 2)
    if not skip:
        return y
    if p > 0:
        keep_prob = 1 - p
        binary = torch.from_numpy(np.asarray(keep, np.float64)).reshape(-1, 1, 1, 1)
        y = y / keep_prob * binary
    return y + x


GIVEN_MASKS = {   # mixed masks that differ per block; crop 1 of n = 5 is dropped in all three, crop 0 of n = 3 in block 13 only
    3: {14: (True, True, False), 13: (False, True, True), 12: (True, False, True)},
    5: {14: (True, False, True, True, False), 13: (True, False, False, True, True), 12: (False, False, True, True, True)},
}


@pytest.mark.parametrize("n", [3, 5])
def test_oracle_equals_torch_float64_autograd_of_the_chain(n):
    sd = C.stress_sd()
    below, b14, b15, conv = C.start(12)
    params = {15: b15, 14: b14, 13: below[13], 12: below[12]}
    rates = {b: float(np.float32(C.RATES[b])) for b in (14, 13, 12)}
    rows, y = B2.synthetic_rows(40 + n, n), (np.arange(n) % 2).astype(np.float32)
    o = B2.Block12Oracle(below, b14, b15, conv, O.default_params(1), C.default_cfg(seed=3), torch.float64,
                         drop_connect=C.RATES[14], drops={13: C.RATES[13], 12: C.RATES[12]})
    o.masks = {b: np.asarray(m) for b, m in GIVEN_MASKS[n].items()}
    o.accumulate(rows, y)
    for b in (14, 13, 12):
        assert np.array_equal(o.taps[f"b{b}.keep"].numpy(), np.asarray(GIVEN_MASKS[n][b], np.float64) / (1.0 - rates[b]))
    # the restatement, driven by the gradient the conv stage hands block 15
    up = o.taps["b15.dout"].reshape(n, 7, 7, 320).permute(0, 3, 1, 2)
    w = {b: {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(k in B2.BLOCK_GRAD_FIELDS) for k, v in params[b].items()} for b in params}
    x = {11: B2.nchw(rows, torch.float64).requires_grad_(True)}
    for b in (12, 13, 14):
        x[b] = _mbconv(x[b - 1], w[b], GIVEN_MASKS[n][b], rates[b], 5, 192, True)
        x[b].retain_grad()
    x[15] = _mbconv(x[14], w[15], None, 0.0, 3, 320, False)
    (x[15] * up).sum().backward()
    rel = lambda got, want: float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(np.asarray(want)).max())
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).reshape(n, 49, -1).numpy()
    for b in (12, 13, 14):
        assert rel(o.taps[f"b{b}.out"].numpy(), nhwc(x[b])) <= 1e-12, b
        for i in np.flatnonzero(~np.asarray(GIVEN_MASKS[n][b])):
            assert torch.equal(x[b][i].detach(), x[b - 1][i].detach())      # a dropped crop is its input, bit for bit
    # dX of every block: what block b hands down arrives at block b - 1's output
    assert rel(o.taps["b14.dout"].numpy(), nhwc(x[14].grad)) <= 1e-9
    assert rel(o.taps["b13.dout"].numpy(), nhwc(x[13].grad)) <= 1e-9
    assert rel(o.taps["b12.dout"].numpy(), nhwc(x[12].grad)) <= 1e-9
    assert rel(o.taps["b12.dx"].numpy(), nhwc(x[11].grad)) <= 1e-9
    g, e = o.grads(), o.export()
    for b in (15, 14, 13, 12):
        for k in B2.BLOCK_GRAD_FIELDS:
            ref = w[b][k].grad.numpy().reshape(g[f"b{b}.{k}"].shape)
            assert np.abs(ref).max() > 0, (b, k)
            assert rel(g[f"b{b}.{k}"], ref) <= 1e-9, (b, k)
        for k in B2.BLOCK_STAT_FIELDS:
            assert not np.array_equal(w[b][k].numpy().reshape(-1), params[b][k].astype(np.float64).reshape(-1)), (b, k)
            assert rel(e[f"b{b}.{k}"].reshape(-1), w[b][k].numpy().reshape(-1)) <= 1e-9, (b, k)
    # the skip-gradient sum in closed form: dX_b = dOut_b + dZe_b . We_b
    inputs = {12: rows, 13: o.taps["b12.out"].numpy(), 14: o.taps["b13.out"].numpy()}
    handed = {12: o.taps["b12.dx"], 13: o.taps["b12.dout"], 14: o.taps["b13.dout"]}
    for b in (14, 13, 12):
        dout, dae = o.taps[f"b{b}.dout"].numpy(), o.taps[f"b{b}.dae"].numpy()
        got = B2.skip_input_gradient(inputs[b], params[b], dout, dae)
        want = handed[b].numpy().reshape(-1, 192)
        assert rel(got, want) <= 1e-9, b
        branch = got - dout.reshape(-1, 192)
        assert np.abs(branch).max() > 1e-3 * np.abs(want).max(), b          # neither term of the sum is negligible
        assert np.abs(dout).max() > 1e-3 * np.abs(want).max(), b
    # a dropped crop still receives a branch gradient through the batch statistics of the other crops
    i = int(np.flatnonzero(~np.asarray(GIVEN_MASKS[n][13]))[0])
    assert np.abs(o.taps["b13.dae"].numpy()[i]).max() > 0


def test_every_crop_of_block_13_dropped_gives_zero_gradients_and_hands_dout_down():
    below, b14, b15, conv = C.start(12)
    n = 2
    rows, y = C.cpu_rows(12)[:n], C.labels(7, n)
    for dtype in (torch.float64, torch.float32):
        o = B2.Block12Oracle(below, b14, b15, conv, O.default_params(1), C.default_cfg(seed=C.DROP13_SEED), dtype,
                             drop_connect=C.RATES[14], drops={13: C.RATES[13], 12: C.RATES[12]})
        assert not o.keep_of(13, n).any() and o.keep_of(14, n).all() and o.keep_of(12, n).all()
        o.accumulate(rows, y)
        g = o.grads()
        for k in B2.BLOCK_GRAD_FIELDS:
            assert not g["b13." + k].any(), k                                 # exactly zero
            assert g["b14." + k].any() and g["b12." + k].any() and g["b15." + k].any(), k
        assert torch.equal(o.taps["b12.dout"], o.taps["b13.dout"])            # dX_13 == dOut_13, element for element
        assert torch.equal(o.taps["b13.out"], o.taps["b12.out"])
        assert not torch.equal(o.taps["b12.dx"], o.taps["b12.dout"])          # block 12 still adds its branch
        e = o.export()
        assert not np.array_equal(e["b13.rm0"], below[13]["rm0"])             # the statistics come before the mask


# --------------------------------------------------------------------------- the preconditions of the GPU cases
@pytest.mark.parametrize("depth,kind,n,variant,rates", C.single_cases())
def test_preconditions_of_the_single_accumulates(depth, kind, n, variant, rates):
    seed, tseed = C.case_seeds(depth, kind, n, rates)
    x = C.cpu_rows(depth)[:n] if kind == "real" else B2.synthetic_rows(seed + 100, n)
    o64, o32, ost, losses, (ya, yb, lam, _) = C.run_oracles(depth, x, seed, tseed, variant, rates)
    margin, rshare, sshare, worst = C.preconditions(o64, o32, ost, losses, ya, yb, lam)
    print(f"depth {depth} n {n} {variant} {rates}: gate margin {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f} ({worst})")
    assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5
    if rates == "ref":
        want = C.masks(tseed, 0, n, depth)
        for b in want:
            assert np.array_equal(o64.taps[f"b{b}.keep"].numpy() != 0, want[b]), b
    else:
        assert all(bool((o64.taps[f"b{b}.keep"] == 1).all()) for b in C.blocks_of(depth))
    if kind == "real" and variant == "plain":                   # what was measured when the seed was picked
        m0, r0, s0, count = C.PICKED[(depth, n, rates)]
        assert 0 < count <= 60 and m0 >= 1.0 and r0 <= 1.0 and s0 <= 0.5


@pytest.mark.parametrize("depth", C.DEPTHS)
def test_preconditions_of_the_all_dropped_and_the_two_accumulate_cases(depth):
    x = C.cpu_rows(depth)[:2]
    o64, o32, ost, losses, (ya, yb, lam, _) = C.run_oracles(depth, x, C.DROP_SEED[depth], C.DROP13_SEED, "plain", "ref")
    margin, rshare, sshare, worst = C.preconditions(o64, o32, ost, losses, ya, yb, lam)
    print(f"depth {depth}, block 13 all dropped: gate margin {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f} ({worst})")
    assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5
    rows = C.cpu_rows(depth)
    below, b14, b15, conv = C.start(depth)
    p14, drops = C.rates_of(depth, "ref")
    seed = C.ACC_SEED[depth]
    os_ = B2.triple(below, b14, b15, conv, O.default_params(seed), C.default_cfg(max_n=16, seed=C.ACC_MASK_SEED), drop_connect=p14, drops=drops)
    for k, xk in enumerate((rows[:16], rows[16:21])):
        y = C.labels(seed + 400 + k, xk.shape[0])
        losses = tuple(o.accumulate(xk, y, None, 1.0, 0.5)[0] for o in os_)
        margin, rshare, sshare, worst = C.preconditions(*os_, losses, y)
        print(f"depth {depth}, accumulate {k}: gate margin {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f} ({worst})")
        assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5


def test_storage_share_covers_the_new_blocks_and_six_group_rates():
    sd = C.stress_sd()
    below, b14, b15, conv = C.start(12)
    rows, y = B2.synthetic_rows(3, 5), (np.arange(5) % 2).astype(np.float32)
    o64, o32, ost = B2.triple(below, b14, b15, conv, O.default_params(2), C.default_cfg())
    losses = tuple(o.accumulate(rows, y)[0] for o in (o64, o32, ost))
    share = B2.storage_share(o64, o32, ost, losses)
    for b in (14, 13, 12):
        assert {f"grad b{b}." + k for k in B2.BLOCK_GRAD_FIELDS} | {"tap " + k for k in B2.taps_of(b) if not k.endswith("keep")} <= set(share)
    assert 0 < share["max"] < 100 and share["max"] == max(v for k, v in share.items() if k != "max")
    lr = float(np.float32(1e-3))
    scaled = lr * float(np.float32(0.1))
    assert o64.group_rates(lr) == (lr,) + (scaled,) * 5 and len(o64.opt.param_groups) == 6
    assert [sum(p.numel() for p in grp["params"]) for grp in o64.opt.param_groups[3:]] == [587952] * 3
    sdo = o64.state_dict(sd)
    assert set(sdo) == set(sd) and sdo["net._blocks.12._depthwise_conv.weight"].shape == (1152, 1, 5, 5)
    # depth 13 is the same chain without block 12, and with nothing below block 14 it is block14_train_oracle's
    o13 = B2.Block12Oracle({13: below[13]}, b14, b15, conv, O.default_params(2), C.default_cfg())
    assert o13.depth == 13 and len(o13.opt.param_groups) == 5 and "b12.exp_w" not in o13.export()
    o14 = B4.Block14Oracle(b14, b15, conv, O.default_params(2), C.default_cfg())
    x13 = o64.taps["b13.out"].numpy()
    l14, z14 = o14.accumulate(x13, y)
    assert abs(l14 - losses[0]) <= 1e-5 * abs(l14)              # x13 went through float32 on the way in
    assert np.abs(o14.grads()["b14.exp_w"] - o64.grads()["b14.exp_w"]).max() <= 1e-3 * np.abs(o64.grads()["b14.exp_w"]).max()

"""CPU: the float64 teacher-forced layer oracle (tests/b0_layer_oracle.py) and the per-layer bars it defines for the
HIP classifier's taps.  The chain reproduces the fp32 oracle; the bars reject kernels that are subtly wrong, with a
margin of at least 3x; the stress weights and edge crops have the ranges they claim."""
import numpy as np
import pytest
import torch

import b0_layer_oracle as O

MARGIN = 3.0
OLD_BAR = 1e-3                          # test_b0_gpu's absolute bar on every tap


@pytest.fixture(scope="module")
def seeded(pkg):
    return pkg.weights.seeded_state_dict(0)


@pytest.fixture(scope="module")
def sds(seeded):
    return O.to_torch(seeded), O.to_torch(seeded, torch.float32)


@pytest.fixture(scope="module")
def taps32(sds):
    """fp32 oracle taps of 5 random crops (ragged against the 4-image groups of the 7 x 7 launches)"""
    return O.forward_taps(sds[1], torch.from_numpy(O.random_crops(5)))


def _getters(taps):
    return (lambda k: taps[k].double()), (lambda k: taps[k].float())


def _margin(cfg, name, taps, sds, num):
    """(how far the mutant `num` is over the fp32 bar, the mutant's output)"""
    g64, g32 = _getters(taps)
    ref, u = O.layer(cfg, name, g64, sds[0]), O.scale(cfg, name, g64, sds[0])
    yard = O.fp32_metrics(O.layer(cfg, name, g32, sds[1]), ref, u)
    mut = O.layer(cfg, name, g64, sds[0], num)
    return O.fp32_ratio(O.fp32_metrics(mut, ref, u), yard), mut


def test_round_bits_is_round_to_nearest_even():
    rs = np.random.RandomState(0)
    x = (rs.randn(200000) * 10.0 ** rs.uniform(-30, 30, 200000)).astype(np.float32)
    bits = x.view(np.uint32)
    bits[:50000] = (bits[:50000] & 0xFFFF0000) | 0x8000         # exact ties
    x = torch.from_numpy(bits.view(np.float32))
    want = x.to(torch.bfloat16).float()
    assert torch.equal(O.rne_bf16(x), want)
    assert torch.equal(O.rne_bf16(x.double()), want.double())   # from float64: the same single rounding
    rtz = O.rtz_bf16(x)
    assert bool((rtz.abs() <= x.abs()).all())
    assert 0.4 < float((rtz != want).double().mean()) < 0.7
    assert torch.equal(O.round_bits(x, 24), x)


def test_launch_plan_matches_the_fused_tap_rule():
    """Config.taps against the rule test_b0_gpu.test_taps_match_oracle states for fuse 0 / 1 / 2 (the shipped default
    also keeps the expand GEMM of blocks 8 and 9, "fuse_late_skip")"""
    for fuse, cfg in ((0, O.FP32_CONFIGS[0]), (1, O.FP32_CONFIGS[1]), (2, O.DEFAULT)):
        has_exp = {i for i in range(16) if i >= 1 and not (fuse and 1 <= i <= 5) and not (fuse == 2 and i != 11)}
        assert {O.parse(t)[0] for t in cfg.taps() if t.endswith(".exp")} == has_exp | ({8, 9} if fuse == 2 else set())
    assert {O.parse(t)[0] for t in O.FP32_CONFIGS[3].taps() if t.endswith(".exp")} == {11}
    assert [O.tap_shape(t, 2) for t in ("stem", "b3.exp", "b3.dw", "b3.gate", "b11.out", "head", "logit")] == [
        (2, 32, 112, 112), (2, 144, 56, 56), (2, 144, 28, 28), (2, 144), (2, 192, 7, 7), (2, 1280, 7, 7), (2, 1)]


@pytest.mark.parametrize("cfg", [O.FP32_CONFIGS[0], O.DEFAULT], ids=lambda c: c.name)
def test_float64_chain_reproduces_the_fp32_oracle(taps32, sds, cfg):
    """Fed the fp32 oracle's own taps, every float64 layer agrees with the oracle's tap to fp32 noise, and the oracle
    (itself a plain fp32 evaluation) passes the fp32 bar it is measured by."""
    g64, g32 = _getters(taps32)
    worst_rms, worst_max = 0.0, 0.0
    for name in cfg.taps():
        ref, u = O.layer(cfg, name, g64, sds[0]), O.scale(cfg, name, g64, sds[0])
        m = O.fp32_metrics(taps32[name], ref, u)
        yard = O.fp32_metrics(O.layer(cfg, name, g32, sds[1]), ref, u)
        worst_rms, worst_max = max(worst_rms, m["rms"]), max(worst_max, m["max"])
        assert m["rms"] <= 5e-6 and m["max"] <= 1e-4, (name, m["rms"], m["max"])
        assert O.fp32_ratio(m, yard) <= 1.0, name
    print(f"{cfg.name}: fp32 oracle vs float64 chain: worst rms {worst_rms:.2e}, worst max |d| / u {worst_max:.2e}")


def test_kernel_state_dict_is_the_packed_blob(seeded, sds, taps32):
    """The bf16 mirror's weights are pack_b0_tensors' (fp32 folded); with three planes the mirror's arithmetic, without
    its roundings, equals the unfolded float64 reference to fp32 folding noise."""
    import rtdfd_amd

    packed = rtdfd_amd.weights.pack_b0_tensors(seeded)
    ksd3 = O.kernel_state_dict(seeded, O.BF16_CONFIGS[0])
    w3 = ksd3["net._blocks.3._project_conv.weight"]
    assert torch.equal(w3.reshape(40, 144).float(), torch.from_numpy(packed["b3.proj.w"]))
    assert torch.equal(ksd3["net._blocks.3._bn2.bias"].float(), torch.from_numpy(packed["b3.proj.b"]))
    ksd1 = O.kernel_state_dict(seeded, O.BF16_CONFIGS[2])           # planes = 1, expand fused
    w1 = ksd1["net._blocks.3._project_conv.weight"]
    assert torch.equal(w1, O.rne_bf16(w3)) and not torch.equal(w1, w3)
    assert torch.equal(ksd1["net._blocks.3._expand_conv.weight"], ksd3["net._blocks.3._expand_conv.weight"])   # fused
    assert torch.equal(ksd1["net._blocks.11._expand_conv.weight"], O.rne_bf16(ksd3["net._blocks.11._expand_conv.weight"]))
    g64, _ = _getters(taps32)
    for name in ("stem", "b3.exp", "b3.dw", "b3.out", "b12.out", "head"):
        cfg = O.FP32_CONFIGS[0]
        m = O.fp32_metrics(O.layer(cfg, name, g64, ksd3), O.layer(cfg, name, g64, sds[0]), O.scale(cfg, name, g64, sds[0]))
        assert m["rms"] <= 2e-7 and m["max"] <= 2e-5, (name, m["rms"], m["max"])


def test_bars_reject_16_bit_operands_which_the_old_bar_accepts(taps32, sds):
    """Mutant (a): a 1x1 conv whose operands keep 16 significand bits (a three-term split that lost its third term)."""
    mutant = O.Numerics(operand=lambda t: O.round_bits(t, 16))
    for name in ("b12.out", "b3.exp"):
        ratio, mut = _margin(O.FP32_CONFIGS[0], name, taps32, sds, mutant)
        print(f"16-bit operands in {name}: {ratio:.1f}x the bar")
        assert ratio >= MARGIN, (name, ratio)
        assert float((mut - taps32[name].double()).abs().max()) <= OLD_BAR      # the gap the new bars close


def test_bars_reject_a_sigmoid_off_by_1e_4(taps32, sds):
    """Mutant (b): sigmoid scaled by 1 + 1e-4, in a gate and in depthwise swishes."""
    mutant = O.Numerics(sigmoid=lambda t: torch.sigmoid(t) * (1.0 + 1e-4))
    for name in ("b7.gate", "b4.dw", "b14.dw"):
        ratio, _ = _margin(O.DEFAULT, name, taps32, sds, mutant)
        print(f"sigmoid * (1 + 1e-4) in {name}: {ratio:.1f}x the bar")
        assert ratio >= MARGIN, (name, ratio)


def test_bars_reject_bf16_rounding_toward_zero(seeded, taps32):
    """Mutant (c): every bf16 store rounds toward zero instead of to nearest even (the input taps made bf16 first, as
    the bf16 path's are)."""
    taps = {k: (v.double() if k in ("x", "feat", "logit") or k.endswith(".gate") else O.rne_bf16(v.double()))
            for k, v in taps32.items()}
    mutant = O.Numerics(store=O.rtz_bf16, gated=lambda t: O.rtz_bf16(t.float().double()))
    for cfg in (O.BF16_CONFIGS[1], O.BF16_CONFIGS[2]):
        ksd = O.kernel_state_dict(seeded, cfg)
        for name in ("stem", "b1.dw", "b11.exp", "b12.out", "head"):
            m = O.bf16_metrics(O.layer(cfg, name, taps.__getitem__, ksd, mutant),
                               O.layer(cfg, name, taps.__getitem__, ksd, O.MIRROR), O.scale(cfg, name, taps.__getitem__, ksd))
            print(f"{cfg.name} {name}: round toward zero: {m['diff']:.1%} not bit-identical, max {m['ulp']:.2f} ulp")
            assert O.bf16_ratio(m) >= MARGIN, (cfg.name, name, m)


def test_bars_reject_one_slice_off_by_1e_4(taps32, sds):
    """Mutant (d): one (image, channel) slice of a 7 x 7 block scaled by 1 + 1e-4, in the last image (4 of 5), the
    only one of its 4-image group."""
    cfg, name = O.DEFAULT, "b12.dw"
    g64, g32 = _getters(taps32)
    ref, u = O.layer(cfg, name, g64, sds[0]), O.scale(cfg, name, g64, sds[0])
    yard = O.fp32_metrics(O.layer(cfg, name, g32, sds[1]), ref, u)
    mut = ref.clone()
    mut[4, 37] *= 1.0 + 1e-4
    ratio = O.fp32_ratio(O.fp32_metrics(mut, ref, u), yard)
    print(f"slice (4, 37) of {name} * (1 + 1e-4): {ratio:.1f}x the bar")
    assert ratio >= MARGIN


def test_metrics_on_known_differences():
    ref = torch.ones(2, 3, 4, 4, dtype=torch.float64)
    ref[1, 2] = 1e-3                                             # a small-scale slice is not hidden by the tensor's max
    got = ref.clone()
    got[1, 2, 0, 0] *= 1.0 + 1e-3
    m = O.fp32_metrics(got, ref, ref.abs())
    assert m["max"] == pytest.approx(1e-3) and m["rms"] < 1e-6
    u = ref.abs().clone()
    u[1, 2] = 1.0                                                # terms of scale 1 cancelled down to 1e-3
    assert O.fp32_metrics(got, ref, u)["max"] == pytest.approx(1e-6)
    zero = torch.zeros(2, 3, 4, 4, dtype=torch.float64)
    m = O.fp32_metrics(zero, zero, zero)
    assert m["rms"] == 0.0 and m["max"] == 0.0 and O.fp32_ratio(m, m) == 0.0
    b = torch.tensor([1.0, 1.0, 1.0, 1.0 + 2.0 ** -7], dtype=torch.float64)
    m = O.bf16_metrics(b, torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64))
    assert m == {"diff": 0.25, "ulp": 1.0} and O.bf16_ratio(m) == 25.0
    small = torch.tensor([2.0 ** -12 * (1 + 2.0 ** -7)], dtype=torch.float64)      # 1 ulp of itself, 1/16 ulp of 2^-8 u
    m = O.bf16_metrics(small, torch.tensor([2.0 ** -12], dtype=torch.float64), torch.ones(1, dtype=torch.float64))
    assert m["ulp"] == pytest.approx(1.0 / 16)


@pytest.fixture(scope="module")
def stress():
    return O.stress_state_dict(0)


def test_stress_state_dict_has_realistic_ranges(seeded, stress):
    assert set(stress) == set(seeded)
    for k, v in stress.items():
        assert v.dtype == seeded[k].dtype and v.shape == seeded[k].shape, k
    var = np.concatenate([stress[bn + ".running_var"] for _, bn in O.conv_bn_pairs()])
    g = np.concatenate([stress[bn + ".weight"] for _, bn in O.conv_bn_pairs()])
    beta = np.concatenate([stress[bn + ".bias"] for _, bn in O.conv_bn_pairs()])
    assert var.min() <= 1.01e-3 and var.max() / var.min() >= 1e4
    assert (g < 0).mean() > 0.3 and (g > 0).mean() > 0.3 and 5 <= (g == 0).sum() <= 0.05 * g.size
    assert 0.8 < beta.std() < 1.2
    assert (np.abs(g) / np.sqrt(var + O.EPS)).max() >= 20.0              # large folded scales


def test_stress_forward_is_finite_and_bounded_on_edge_crops(stress):
    """float64 forward of the stress weights on the edge crops: finite, every |tap| <= 1e3, gates saturated on both
    sides, and the crops give different logits."""
    x = O.edge_crops()
    assert x.shape == (7, 3, 224, 224) and x.dtype == np.float32
    taps = O.forward_taps(O.to_torch(stress), torch.from_numpy(x).double())
    for k, t in taps.items():
        assert bool(torch.isfinite(t).all()), k
    worst = max(taps, key=lambda k: float(taps[k].abs().max()))
    print(f"stress weights on the edge crops: largest |tap| {float(taps[worst].abs().max()):.1f} ({worst})")
    assert float(taps[worst].abs().max()) <= 1e3, worst
    gates = torch.cat([taps[f"b{i}.gate"].flatten() for i in range(16)])
    assert bool((gates < 1e-3).any()) and bool((gates > 0.999).any())
    assert float(taps["logit"].std()) > 1e-3

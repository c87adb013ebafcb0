"""GPU parity: HIP classifier (through the C ABI) vs the CPU oracle, stage by stage.

Tolerances: fp32 logits |d| <= 1e-3 (BASELINE.json north_star); intermediate activations
are O(1) so the same absolute bound is applied to every tap.
"""
import numpy as np
import pytest
import torch

from oracle import b0_ref

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3


def _inputs(n, seed=42):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, 3, 224, 224).astype(np.float32)
    scale = np.linspace(0.3, 2.0, n, dtype=np.float32).reshape(n, 1, 1, 1)
    shift = np.linspace(-1.0, 1.0, n, dtype=np.float32).reshape(n, 1, 1, 1)
    return x * scale + shift


@pytest.fixture(scope="module")
def ref(pkg, seeded_sd):
    x = _inputs(3)
    taps = {}
    y = b0_ref.forward(pkg.weights.to_torch(seeded_sd), torch.from_numpy(x), taps)
    return x, y.numpy(), taps


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy() if t.dim() == 4 else t.numpy()


@pytest.mark.parametrize("fuse", [0, 1, 2])
def test_taps_match_oracle(b0_handle, ref, fuse):
    """fuse=0: every layer as its own kernel (the expand outputs exist and are checked);
    fuse=1: blocks 1-5 compute expand inside the depthwise kernel, blocks 6-15 as separate launches (round 3's default);
    fuse=2: the shipped default - blocks 6-10 / 12-15 too (whole-image launches; only block 11 keeps an expand GEMM)."""
    x, _, taps = ref
    n = x.shape[0]
    xd = b0_handle.alloc(x.nbytes).upload(x)
    b0_handle.set_option("fuse_expand", int(fuse > 0))
    b0_handle.set_option("fuse_stem", int(fuse > 0))   # fused: the stem tap is a side copy out of the fused kernel
    b0_handle.set_option("fuse_late", int(fuse == 2))
    names = ["stem"]
    for i in range(16):
        has_exp = i >= 1 and not (fuse and 1 <= i <= 5) and not (fuse == 2 and i != 11)
        names += ([f"b{i}.exp"] if has_exp else []) + [f"b{i}.dw", f"b{i}.gate", f"b{i}.out"]
    names += ["head"]
    worst = {}
    for name in names:
        want = _nhwc(taps[name])
        if name.endswith(".gate"):
            want = want.reshape(n, -1)
        got = b0_handle.tap(xd.ptr, n, name, want.size).reshape(want.shape)
        err = float(np.abs(got - want).max())
        worst[name] = err
        assert err <= LOGIT_TOL, f"{name}: max|d|={err:.3e} (ref absmax {np.abs(want).max():.2f})"
    if fuse:
        with pytest.raises(Exception):
            b0_handle.tap(xd.ptr, n, "b1.exp", 10)             # not materialised when fused: loud, not silent
    b0_handle.set_option("fuse_expand", 1)
    b0_handle.set_option("fuse_stem", 1)
    b0_handle.set_option("fuse_late", 1)
    xd.free()
    print("worst tap errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:5])


def test_late_blocks_in_one_launch_match_oracle(b0_handle, ref):
    """Option "fuse_late": blocks 6-10 and 12-15 run expand + depthwise of whole images in one launch
    (mbconv_late_kernel); every tap downstream of them and the logits stay within the fp32 bar, and the expanded
    tensor of such a block is reported as not materialised."""
    x, want, taps = ref
    n = x.shape[0]
    xd = b0_handle.alloc(x.nbytes).upload(x)
    b0_handle.set_option("fuse_late", 1)
    b0_handle.set_option("fuse_late_skip", 0)               # every block the kernel covers (the default leaves 8 and 9 out)
    try:
        for i in range(6, 16):
            for kind in ("dw", "gate", "out"):
                name = f"b{i}.{kind}"
                w = _nhwc(taps[name])
                if kind == "gate":
                    w = w.reshape(n, -1)
                got = b0_handle.tap(xd.ptr, n, name, w.size).reshape(w.shape)
                err = float(np.abs(got - w).max())
                assert err <= LOGIT_TOL, f"{name}: max|d|={err:.3e}"
        with pytest.raises(Exception):
            b0_handle.tap(xd.ptr, n, "b9.exp", 10)
        got = b0_handle.classify(x)
        assert np.abs(got - want).max() <= LOGIT_TOL
        for m in (1, 2):                                    # 7 x 7 blocks hold four images: ragged last group
            assert np.abs(b0_handle.classify(x[:m]) - want[:m]).max() <= LOGIT_TOL
        # the default: blocks 8 and 9 keep expand GEMM + depthwise kernel (measured faster) - their expanded tensor exists
        b0_handle.set_option("fuse_late_skip", (1 << 8) | (1 << 9))
        w = _nhwc(taps["b9.exp"])
        assert np.abs(b0_handle.tap(xd.ptr, n, "b9.exp", w.size).reshape(w.shape) - w).max() <= LOGIT_TOL
        with pytest.raises(Exception):
            b0_handle.tap(xd.ptr, n, "b10.exp", 10)
        assert np.abs(b0_handle.classify(x) - want).max() <= LOGIT_TOL
    finally:
        b0_handle.set_option("fuse_late", 1)               # the defaults
        b0_handle.set_option("fuse_late_skip", (1 << 8) | (1 << 9))
        xd.free()


def test_fused_and_unfused_logits_agree(b0_handle, ref):
    x, want, _ = ref
    b0_handle.set_option("fuse_expand", 0)
    b0_handle.set_option("fuse_stem", 0)
    a = b0_handle.classify(x)
    b0_handle.set_option("fuse_expand", 1)
    b0_handle.set_option("fuse_stem", 1)
    b = b0_handle.classify(x)
    assert np.abs(a - want).max() <= LOGIT_TOL and np.abs(b - want).max() <= LOGIT_TOL
    assert np.abs(a - b).max() <= 1e-4


def test_logits_match_oracle(b0_handle, ref):
    x, want, _ = ref
    got = b0_handle.classify(x)
    assert got.shape == (x.shape[0], 1)
    assert np.abs(got - want).max() <= LOGIT_TOL, (got.ravel(), want.ravel())
    # the logits must actually differ between inputs, or this test says nothing
    assert np.ptp(want) > 0.1


def test_features_match_oracle(pkg, b0_handle, seeded_sd, ref):
    x, _, _ = ref
    want = b0_ref.extract_features(pkg.weights.to_torch(seeded_sd), torch.from_numpy(x)).numpy()
    got = b0_handle.extract_features(x)
    assert got.shape == (x.shape[0], 1280)
    assert np.abs(got - want).max() <= LOGIT_TOL


def test_batch_invariance_and_determinism(b0_handle):
    """Same crop alone, in a ragged batch (M not a multiple of any tile) and twice in a row gives
    bit-identical logits (reference tests/test_reliability.py:123-132 asserts out1 == out2)."""
    x = _inputs(11, seed=7)
    full = b0_handle.classify(x)
    again = b0_handle.classify(x)
    assert np.array_equal(full, again)
    for i in (0, 5, 10):
        one = b0_handle.classify(x[i:i + 1])
        assert np.array_equal(one, full[i:i + 1]), (i, one, full[i])
    part = b0_handle.classify(x[3:10])
    assert np.array_equal(part, full[3:10])


def test_reference_determinism_input(pkg, b0_handle, seeded_sd):
    """The reference's own determinism input: torch.manual_seed(42); randn(1,3,224,224)."""
    torch.manual_seed(42)
    x = torch.randn(1, 3, 224, 224)
    want = b0_ref.forward(pkg.weights.to_torch(seeded_sd), x).numpy()
    got = b0_handle.classify(x.numpy())
    assert abs(float(got[0, 0]) - float(want[0, 0])) <= LOGIT_TOL


def test_model_surface(pkg, seeded_sd, ref):
    """DeepfakeEfficientNet host mirror: shapes/ranges the reference tests pin
    (tests/test_functional.py:70-110)."""
    x, want, _ = ref
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, state_dict=seeded_sd).eval()
    fc = m.net._fc
    assert len(fc) == 10 and fc[1].in_features == 1280 and fc[1].out_features == 512 and fc[9].out_features == 1
    out = m(torch.from_numpy(x))
    assert tuple(out.shape) == (3, 1)
    assert np.abs(out.numpy() - want).max() <= LOGIT_TOL
    probs = torch.sigmoid(out)
    assert probs.min() >= 0.0 and probs.max() <= 1.0
    logits, proj = m.forward_with_projection(x)
    assert proj is None and logits.shape == (3, 1)
    assert m.extract_features(x[:1]).shape == (1, 1280)


def test_errors_are_loud(pkg, b0_handle):
    with pytest.raises(pkg._lib.DfdError):
        b0_handle.classify(np.zeros((17, 3, 224, 224), np.float32))   # capacity 16
    with pytest.raises(ValueError):
        b0_handle.classify(np.zeros((1, 3, 32, 32), np.float32))
    with pytest.raises(pkg._lib.DfdError):
        pkg._lib.Handle(b"not a blob", device=0, max_batch=1)
    for name in ("fuse_se", "se_in_proj", "se_thin"):                  # removed options are unknown names
        with pytest.raises(pkg._lib.DfdError):
            b0_handle.set_option(name, 0)


def test_split_gemm_matches_fp32_mfma_and_oracle(b0_handle, ref):
    """The split-precision GEMM (three exact bf16 terms per fp32 operand, six products on bf16 MFMA) and the
    plain fp32 MFMA kernel are two evaluations of the same fp32 dot products: both meet the oracle bound and
    they agree with each other to fp32 rounding noise at every 1x1-conv output."""
    x, y, taps = ref
    n = x.shape[0]
    xd = b0_handle.alloc(x.nbytes).upload(x)
    got = {}
    try:
        for mode in (0, 1):
            b0_handle.set_option("split_gemm", mode)
            got[mode] = {name: b0_handle.tap(xd.ptr, n, name, _nhwc(taps[name]).size)
                         for name in ("b7.out", "b12.out", "b15.out", "head")}
            got[mode]["logits"] = b0_handle.classify(x).reshape(-1)
    finally:
        b0_handle.set_option("split_gemm", 1)
    for name, want in taps.items():
        if name not in got[0]:
            continue
        w = _nhwc(want).reshape(-1)
        for mode in (0, 1):
            assert np.abs(got[mode][name] - w).max() <= LOGIT_TOL, (name, mode)
        scale = max(1.0, float(np.abs(w).max()))
        assert np.abs(got[0][name] - got[1][name]).max() <= 2e-5 * scale, name
    for mode in (0, 1):
        assert np.abs(got[mode]["logits"] - y.reshape(-1)).max() <= LOGIT_TOL, mode
    assert np.abs(got[0]["logits"] - got[1]["logits"]).max() <= 5e-5

"""GPU: option "fuse_proj0" - block 0's projection computed inside block 1's expand + depthwise launch
(mbconv_kernel, PROJ0) from block 0's depthwise output; the 16-channel block output never reaches HBM.

The fused prologue restates the separate GEMM's arithmetic operation for operation (gate multiply, three-way bf16 split,
the six products in s6_products' order, bias), so everything downstream must have THE SAME BITS as with the option off:
every bit-for-bit comparison here takes its reference from the unfused path of the same build.  Against the CPU oracle
the bar is the fp32 path's 1e-3 on every tap (tests/test_b0_gpu.py).

Batches 1, 2, 3 and 5: the network input size is fixed, so these are the smallest calls; odd n ends the image-major block
order raggedly; every image holds all four border cases of the halo (14 x 14 tiles of 8 x 8 outputs)."""
import numpy as np
import pytest
import torch

from oracle import b0_ref

pytestmark = pytest.mark.gpu

TAP_TOL = 1e-3
NMAX = 5
BATCHES = (1, 2, 3, 5)


def _crops(n, seed=314):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, 3, 224, 224).astype(np.float32)
    scale = np.linspace(0.4, 1.9, n, dtype=np.float32).reshape(n, 1, 1, 1)
    shift = np.linspace(-0.8, 0.8, n, dtype=np.float32).reshape(n, 1, 1, 1)
    return x * scale + shift


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy() if t.dim() == 4 else t.numpy()


@pytest.fixture(scope="module")
def ref(pkg, seeded_sd):
    """seeded crops, and the oracle's taps and logits for them (computed once, read only)"""
    x = _crops(NMAX)
    taps = {}
    y = b0_ref.forward(pkg.weights.to_torch(seeded_sd), torch.from_numpy(x), taps).numpy()
    want = {name: _nhwc(taps[name]) for name in ("b0.out", "b1.dw", "b1.out")}
    want["logits"] = y
    for v in want.values():
        v.setflags(write=False)
    x.setflags(write=False)
    return x, want


@pytest.fixture()
def handle(b0_handle):
    yield b0_handle
    b0_handle.set_option("fuse_proj0", 1)                 # the defaults
    b0_handle.set_option("bf16_activations", 0)


def _run(h, x, fuse, names=("b1.dw", "b1.out")):
    """taps (NHWC) and logits of the first len(x) crops with the option set to `fuse`"""
    n = x.shape[0]
    shapes = {"b0.out": (n, 112, 112, 16), "b1.dw": (n, 56, 56, 96), "b1.out": (n, 56, 56, 24)}
    h.set_option("fuse_proj0", fuse)
    xd = h.alloc(x.nbytes).upload(x)
    try:
        got = {name: h.tap(xd.ptr, n, name, int(np.prod(shapes[name]))).reshape(shapes[name]).copy() for name in names}
    finally:
        xd.free()
    got["logits"] = h.classify(x)
    return got


def test_profile_has_no_projection_launch_for_block_0(handle):
    """the option does what it says: with it on a forward has no b0.proj launch (b1.dw carries the work), off it has one"""
    x = _crops(2)
    xd = handle.alloc(x.nbytes).upload(x)
    yd = handle.alloc(64)
    seen = {}
    try:
        for fuse in (1, 0):
            handle.set_option("fuse_proj0", fuse)
            handle.profile_begin()
            handle.classify_device(xd.ptr, 2, yd.ptr)
            handle.sync()
            _, layers = handle.profile_end()
            seen[fuse] = [name for name, _ in layers]
    finally:
        xd.free()
        yd.free()
    assert "b0.proj" in seen[0] and "b1.dw" in seen[0]
    assert "b0.proj" not in seen[1] and "b1.dw" in seen[1]
    assert [s for s in seen[0] if s != "b0.proj"] == seen[1]


@pytest.mark.parametrize("n", BATCHES)
def test_fused_bits_equal_unfused_and_meet_the_oracle(handle, ref, n):
    """(a) b1.dw, b1.out and the logits: option on == option off, bit for bit; (b) each within 1e-3 of the oracle"""
    x, want = ref
    on = _run(handle, x[:n], 1)
    off = _run(handle, x[:n], 0)
    for name in ("b1.dw", "b1.out", "logits"):
        err = float(np.abs(on[name] - want[name][:n]).max())
        print(f"n={n} {name}: fused vs oracle max|d| = {err:.3e}; differing elements vs unfused: "
              f"{int(np.count_nonzero(on[name].view(np.uint32) != off[name].view(np.uint32)))}")
    for name in ("b1.dw", "b1.out", "logits"):
        assert np.array_equal(on[name].view(np.uint32), off[name].view(np.uint32)), name
        assert float(np.abs(on[name] - want[name][:n]).max()) <= TAP_TOL, name
    assert np.ptp(want["b1.dw"][:n]) > 0.1                # the tensors compared are not degenerate


def test_chunk_invariance(handle, ref):
    """(c) five crops in one call == the same crops in calls of two and three"""
    x, _ = ref
    handle.set_option("fuse_proj0", 1)
    whole = handle.classify(x)
    parts = np.concatenate([handle.classify(x[:2]), handle.classify(x[2:])])
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))


def test_block0_output_tap_is_unchanged(handle, ref):
    """(d) a b0.out tap with the option on (that call runs the two launches) returns the bits it returns with it off"""
    x, want = ref
    n = 3
    on = _run(handle, x[:n], 1, names=("b0.out",))["b0.out"]
    off = _run(handle, x[:n], 0, names=("b0.out",))["b0.out"]
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert float(np.abs(on - want["b0.out"][:n]).max()) <= TAP_TOL


def test_bf16_activations_ignore_the_option(handle, ref):
    """(e) bf16 activation storage keeps its launches: the logits do not depend on the option"""
    x, _ = ref
    handle.set_option("bf16_activations", 1)
    got = {}
    for fuse in (1, 0):
        handle.set_option("fuse_proj0", fuse)
        got[fuse] = handle.classify(x)
    assert np.array_equal(got[1].view(np.uint32), got[0].view(np.uint32))
    assert np.all(np.isfinite(got[1]))

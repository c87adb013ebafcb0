"""GPU: option "fuse_k5" for blocks 6, 7 (k3, stride 1, 14 x 14) and 11 (k5, stride 2, 14 -> 7) - the instances of
mbconv_k5_kernel that round 7 added beside those of blocks 8-10 (tests/test_b0_fuse_k5_gpu.py): one thread block per image
walks every 32-channel chunk.

The rule is the one of blocks 8-10: the kernel gives a block the bits of the form it would run otherwise, so for every
value of "fuse_late_skip" the option on and the option off give THE SAME BITS in every tap and in the logits.  Blocks 6
and 7 replace mbconv_late_kernel (expand bias in front of the products).  Block 11 has no mbconv_late_kernel form: it always
replaces expand GEMM + dw_kernel (bias after the products), and bit 11 of an explicit mask keeps those two launches.

What a wrong tile geometry would do: the zero border of the stride-2 tile (17 wide: one row / column on the low side, two
on the high side) and of the k3 tile (16 wide, one each side) enters every border output of b11.dw / b6.dw / b7.dw, so a
border in the wrong place, or one that a producer overwrote, shows as differing bits in those taps.

The plan takes the kernel only from "fuse_k5_min" images in the last round of blocks on; these tests set it to 1, or to
a value between the batch sizes they compare.  Batches 1, 2, 3 and 5: the shapes are fixed by the network, what varies is
the grid (one block per image)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NMAX = 5
BATCHES = (1, 2, 3, 5)
SKIP_NEW = (1 << 6) | (1 << 7) | (1 << 11)
TAPS = {"b6.dw": (14, 14, 480), "b6.gate": (480,), "b7.dw": (14, 14, 480), "b7.out": (14, 14, 80), "b11.dw": (7, 7, 672),
        "b11.gate": (672,), "b11.out": (7, 7, 192), "b15.out": (7, 7, 320)}
B11_EXP = 14 * 14 * 672


def _crops(n, seed=613):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, 3, 224, 224).astype(np.float32)
    scale = np.linspace(0.4, 1.9, n, dtype=np.float32).reshape(n, 1, 1, 1)
    shift = np.linspace(-0.8, 0.8, n, dtype=np.float32).reshape(n, 1, 1, 1)
    return x * scale + shift


@pytest.fixture(scope="module")
def crops():
    x = _crops(NMAX)
    x.setflags(write=False)
    return x


@pytest.fixture()
def handle(b0_handle):
    yield b0_handle
    b0_handle.set_option("fuse_k5", 1)                    # the defaults
    b0_handle.set_option("fuse_k5_min", 0)
    b0_handle.set_option("fuse_late_skip", -1)


def _run(h, x, k5, skip):
    """taps (NHWC) and logits of crops x with "fuse_k5" = k5 and "fuse_late_skip" = skip"""
    n = x.shape[0]
    h.set_option("fuse_k5", k5)
    h.set_option("fuse_k5_min", 1)                        # the kernel at every batch size
    h.set_option("fuse_late_skip", skip)
    xd = h.alloc(x.nbytes).upload(x)
    try:
        got = {name: h.tap(xd.ptr, n, name, n * int(np.prod(s))).reshape((n,) + s).copy() for name, s in TAPS.items()}
    finally:
        xd.free()
    got["logits"] = h.classify(x)
    return got


def _bits_differ(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


@pytest.mark.parametrize("skip", [-1, 0, SKIP_NEW])
@pytest.mark.parametrize("n", BATCHES)
def test_the_option_changes_no_bit(handle, crops, n, skip):
    """option on == option off, every tap and the logits bit for bit, with "fuse_late_skip" unset (blocks 6, 7 and 11 in
    the new kernel against mbconv_late_kernel / GEMM + depthwise), 0 (the same for these three) and with blocks 6, 7 and 11
    masked explicitly (they keep their separate launches either way; blocks 8-10 move)"""
    on = _run(handle, crops[:n], 1, skip)
    off = _run(handle, crops[:n], 0, skip)
    for name in on:
        print(f"n={n} skip={skip} {name}: differing elements {_bits_differ(on[name], off[name])}, max|d| = "
              f"{float(np.abs(on[name] - off[name]).max()):.3e}")
    for name in on:
        assert np.all(np.isfinite(on[name])), name
        assert np.array_equal(on[name].view(np.uint32), off[name].view(np.uint32)), (skip, name)
    for name in ("b6.dw", "b7.dw", "b11.dw", "b11.out", "b15.out"):   # the tensors compared are not degenerate
        assert np.ptp(on[name]) > 0.1, name


@pytest.mark.parametrize("skip", [-1, 0])
def test_batch_invariance_across_the_threshold(handle, crops, skip):
    """five crops in one call (at "fuse_k5_min" = 3: the new kernel) == the same crops in calls of two (below it: the older
    forms) and three (the new kernel), bit for bit; also with every block unmasked"""
    handle.set_option("fuse_k5", 1)
    handle.set_option("fuse_late_skip", skip)
    handle.set_option("fuse_k5_min", 3)
    whole = handle.classify(crops)
    parts = np.concatenate([handle.classify(crops[:2]), handle.classify(crops[2:])])
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    handle.set_option("fuse_k5_min", 1)
    assert np.array_equal(handle.classify(crops).view(np.uint32), whole.view(np.uint32))


def test_block_11_expanded_tensor_exists_only_below_the_threshold(pkg, handle, crops):
    """below "fuse_k5_min" block 11 keeps its expand GEMM (the b11.exp tap exists), from it on the expanded tensor is not
    materialised; bit 11 of an explicit mask brings the GEMM back"""
    x = crops[:3]
    handle.set_option("fuse_k5", 1)
    handle.set_option("fuse_late_skip", -1)
    xd = handle.alloc(x.nbytes).upload(x)
    try:
        handle.set_option("fuse_k5_min", 4)
        below = handle.tap(xd.ptr, 3, "b11.exp", 3 * B11_EXP).copy()
        assert below.size == 3 * B11_EXP and np.ptp(below) > 0.1
        handle.set_option("fuse_k5_min", 0)               # the default threshold is far above 3 crops
        assert handle.tap(xd.ptr, 3, "b11.exp", 3 * B11_EXP).size == 3 * B11_EXP
        handle.set_option("fuse_k5_min", 3)
        with pytest.raises(pkg._lib.DfdError, match="not materialised"):
            handle.tap(xd.ptr, 3, "b11.exp", 3 * B11_EXP)
        handle.set_option("fuse_late_skip", (1 << 8) | (1 << 9) | (1 << 11))   # the unset mask's blocks, and block 11
        masked = handle.tap(xd.ptr, 3, "b11.exp", 3 * B11_EXP)
        assert np.array_equal(masked.view(np.uint32), below.view(np.uint32))
    finally:
        xd.free()


def test_bf16_activations_ignore_the_option(handle, crops):
    """bf16 activation storage keeps its launches: the logits do not depend on the option"""
    got = {}
    try:
        handle.set_option("bf16_activations", 1)
        handle.set_option("fuse_k5_min", 1)
        handle.set_option("fuse_late_skip", -1)
        for k5 in (1, 0):
            handle.set_option("fuse_k5", k5)
            got[k5] = handle.classify(crops)
    finally:
        handle.set_option("bf16_activations", 0)
    assert np.array_equal(got[1].view(np.uint32), got[0].view(np.uint32))
    assert np.all(np.isfinite(got[1]))

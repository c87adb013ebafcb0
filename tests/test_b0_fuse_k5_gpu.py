"""GPU: option "fuse_k5" - blocks 8-10 (k5, stride 1, 14 x 14) through mbconv_k5_kernel, one thread block per image that
walks every 32-channel chunk, instead of mbconv_late_kernel (one block per image and chunk) or expand GEMM + depthwise.

Which existing form can be matched bit for bit, established on an MI355X at n = 1, 2, 3 and 5: today's fused path
("fuse_late_skip" = 0, mbconv_late_kernel) and today's separate path (pw9_kernel + dw_kernel) do NOT agree for blocks 8
and 9 - b8.dw differs in 66,927 of 94,080 elements per crop by at most 2.9e-6, b9.dw by at most 3.1e-6, the logits by at
most 2.0e-6.  The products and their order are the same; the fused launch starts its accumulators at the expand bias, the
GEMM adds the bias after the products.  The new kernel has both forms, and the plan gives a block the form of what it
would run otherwise: a block the unset mask covers (8, 9) gets the bits of the SEPARATE launches, an unmasked block those
of mbconv_late_kernel, an explicitly masked block keeps its separate launches.  So for every value of "fuse_late_skip"
the option on and the option off must give THE SAME BITS in every tap and in the logits.  (Different masks still differ
from each other in blocks 8 and 9, as they always did.)

The plan takes the kernel only from "fuse_k5_min" images in the last round of blocks on (one block per image: a small
batch leaves the CUs idle); these tests set it to 1, or to a value between the batch sizes they compare.

Batches 1, 2, 3 and 5: the kernel's shapes are fixed by the network, what varies is the grid (one block per image)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NMAX = 5
BATCHES = (1, 2, 3, 5)
SKIP89 = (1 << 8) | (1 << 9)
TAPS = {"b8.dw": (14, 14, 480), "b8.gate": (480,), "b9.dw": (14, 14, 672), "b10.dw": (14, 14, 672), "b10.out": (14, 14, 112),
        "b15.out": (7, 7, 320)}


def _crops(n, seed=271):
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


@pytest.mark.parametrize("n", BATCHES)
def test_k5_bits_equal_the_forms_it_replaces(handle, crops, n):
    """option on (all three blocks in the new kernel) == option off with blocks 8 and 9 as separate launches and block 10
    in mbconv_late_kernel: every tap and the logits bit for bit"""
    on = _run(handle, crops[:n], 1, -1)
    off = _run(handle, crops[:n], 0, SKIP89)
    for name in on:
        print(f"n={n} {name}: differing elements {_bits_differ(on[name], off[name])}, max|d| = "
              f"{float(np.abs(on[name] - off[name]).max()):.3e}")
    for name in on:
        assert np.all(np.isfinite(on[name])), name
        assert np.array_equal(on[name].view(np.uint32), off[name].view(np.uint32)), name
    assert np.ptp(on["b8.dw"]) > 0.1 and np.ptp(on["b10.dw"]) > 0.1       # the tensors compared are not degenerate


@pytest.mark.parametrize("n", BATCHES)
def test_the_option_changes_no_bit_under_any_mask(handle, crops, n):
    """ "fuse_late_skip" = 0 (blocks 8-10 unmasked: the new kernel against mbconv_late_kernel for all three), blocks 8 + 9
    (masked explicitly: separate launches either way, block 10 moves) and unset + the option off against the first test's
    plan: on == off, bit for bit"""
    for skip in (0, SKIP89):
        on = _run(handle, crops[:n], 1, skip)
        off = _run(handle, crops[:n], 0, skip)
        for name in on:
            assert np.array_equal(on[name].view(np.uint32), off[name].view(np.uint32)), (skip, name)
    a = _run(handle, crops[:n], 1, -1)
    b = _run(handle, crops[:n], 0, -1)
    for name in a:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


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


def test_the_threshold_decides_which_launches_run(pkg, handle, crops):
    """below "fuse_k5_min" block 8 keeps its expand GEMM (the tap exists), from it on the expanded tensor is not materialised"""
    x = crops[:3]
    handle.set_option("fuse_k5", 1)
    handle.set_option("fuse_late_skip", -1)
    xd = handle.alloc(x.nbytes).upload(x)
    try:
        handle.set_option("fuse_k5_min", 4)
        assert handle.tap(xd.ptr, 3, "b8.exp", 3 * 14 * 14 * 480).size == 3 * 14 * 14 * 480
        handle.set_option("fuse_k5_min", 0)               # the default threshold is far above 3 crops
        assert handle.tap(xd.ptr, 3, "b8.exp", 3 * 14 * 14 * 480).size == 3 * 14 * 14 * 480
        handle.set_option("fuse_k5_min", 3)
        with pytest.raises(pkg._lib.DfdError, match="not materialised"):
            handle.tap(xd.ptr, 3, "b8.exp", 3 * 14 * 14 * 480)
    finally:
        xd.free()


def test_expanded_tensor_is_not_materialised(pkg, handle, crops):
    """with the option on (and no mask) block 8's expanded tensor never exists: the tap says so"""
    x = crops[:2]
    handle.set_option("fuse_k5", 1)
    handle.set_option("fuse_k5_min", 1)
    handle.set_option("fuse_late_skip", -1)
    xd = handle.alloc(x.nbytes).upload(x)
    try:
        with pytest.raises(pkg._lib.DfdError, match="not materialised"):
            handle.tap(xd.ptr, 2, "b8.exp", 2 * 14 * 14 * 480)
    finally:
        xd.free()


def test_bf16_activations_ignore_the_option(handle, crops):
    """bf16 activation storage keeps its launches (blocks 8 and 9 separate by default): the logits do not depend on the option"""
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

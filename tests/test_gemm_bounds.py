"""CPU: the split GEMM's 32-bit addressing guard (gemm_split.hip s6_chunk_rows, exported as dfd_gemm_chunk_rows).

The kernels address activations with 32-bit byte offsets; a launch therefore never spans 2^31 bytes of X and larger
batches are issued as several launches over whole images.  These cases walk the arithmetic at the capacities
dfd_create accepts (max_batch <= 4096) for the B0 layers with the largest rows-per-image x K products.

pw8_kernel addresses the output Y and the residual R with 32 bits too, so the launchers bound a chunk by the LARGEST of
the X, Y and R rows (max(K, N) elements; a convolution: the larger of an image's input and output): for N > K a launch
keeps rows * N * sizeof at or below 2^31 - 1 as well (test_chunks_bound_the_output_rows_too)."""
import pytest

LIM = (1 << 31) - 1
# (name, rows per image, K): block 0 project, block 2 project, block 1 expand (unfused), head
LAYERS = [("b0.proj", 112 * 112, 32), ("b2.proj", 56 * 56, 144), ("b1.exp", 112 * 112, 16), ("head", 49, 320),
          ("b12.proj", 49, 1152)]


@pytest.fixture(scope="module")
def lib(pkg):
    import os

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return pkg._lib.load()


@pytest.mark.parametrize("name,hw,k", LAYERS)
@pytest.mark.parametrize("batch", [1, 16, 256, 1189, 1190, 1337, 1338, 2675, 4096])
def test_chunks_stay_below_2g_and_cover_the_batch(lib, name, hw, k, batch):
    rows, row_bytes = batch * hw, k * 4
    chunk = lib.dfd_gemm_chunk_rows(rows, row_bytes, hw)
    assert chunk > 0
    assert chunk * row_bytes <= LIM, "one launch would wrap the 32-bit offset"
    if rows * row_bytes <= LIM:
        assert chunk == rows                      # small batches: one launch, as before
    else:
        assert chunk % hw == 0 and chunk < rows   # whole images, so the gate index m / HW stays chunk-relative
        # the largest whole-image chunk that fits
        assert (chunk + hw) * row_bytes > LIM
    launches = -(-rows // chunk)
    assert (launches - 1) * chunk < rows <= launches * chunk


# Layers with N > K: the output row is the larger one.  pw8_kernel addresses Y and the residual R with 32-bit byte
# offsets as it does X, so the launchers (launch_pointwise_split, launch_conv_gemm_split, dfd_gemm_tap) pass the
# LARGEST of the three rows, max(K, N) elements, as row_bytes.  (name, rows per image, K, N, bytes per element):
# block 1's expand (unfused), the head conv, the thin 16 -> 48 shape dfd_gemm_tap can hand pw8, the head in bf16
WIDE = [("b1.exp", 112 * 112, 16, 96, 4), ("head", 49, 320, 1280, 4), ("thin 16 -> 48", 1, 16, 48, 4), ("head bf16", 49, 320, 1280, 2),
        ("b1.exp bf16", 112 * 112, 16, 96, 2)]


# the layers at batches up to max_batch = 4096; the thin shape also at the 22.4 M rows of tests/test_gemm_direct_gpu.py
WIDE_CASES = [w + (b,) for w in WIDE for b in (1, 256, 445, 446, 447, 892, 893, 1784, 1785, 4096, 22_400_000) if b <= 4096 or w[1] == 1]


@pytest.mark.parametrize("name,hw,k,n,esz,batch", WIDE_CASES)
def test_chunks_bound_the_output_rows_too(lib, name, hw, k, n, esz, batch):
    assert n > k
    rows, row_bytes = batch * hw, max(k, n) * esz
    chunk = lib.dfd_gemm_chunk_rows(rows, row_bytes, hw)
    assert chunk > 0
    assert chunk * n * esz <= LIM, "one launch would wrap the 32-bit offset into Y / R"
    assert chunk * k * esz <= LIM
    if rows * n * esz <= LIM:
        assert chunk == rows
    else:
        assert chunk % hw == 0 and chunk < rows and (chunk + hw) * n * esz > LIM
        # bounded by X alone (the rule before) the same call would have spanned more than 2^31 bytes of Y
        old = lib.dfd_gemm_chunk_rows(rows, k * esz, hw)
        assert old * n * esz > LIM
    launches = -(-rows // chunk)
    assert (launches - 1) * chunk < rows <= launches * chunk


def test_an_image_that_cannot_fit_is_reported(lib):
    assert lib.dfd_gemm_chunk_rows(4 * (1 << 20), 4096, 1 << 20) == -1      # 4 GiB per image
    assert lib.dfd_gemm_chunk_rows(10, 16, 0) == 10                         # rows_per_image <= 0 is treated as 1


def test_tile_count_is_exported(lib):
    assert 16 <= lib.dfd_gemm_tile_count() <= 128

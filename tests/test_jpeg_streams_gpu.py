"""GPU: the device half of the JPEG path - the IDCT / upsampling / colour kernels (csrc/jpeg_decode.hip) and the device
entropy decoder (csrc/jpeg_gpu_entropy.h) - against libjpeg itself (Pillow's decode), bit for bit, on the valid files that
Pillow never writes: the corpus of tests/jpeg_stream_cases.py (reversed Annex K tables: the 13 to 16-bit branch of
jg_decode and de-stuffing with several stuffed zeros per 16-byte piece; six tables: handed to the host decoder; table ids 2
and 3; blocks of 2 bits; 16-bit DQT; fill bytes; bytes behind EOI; hand-made coefficients that reach the clamp; chroma
planes one or two samples wide, which libjpeg replicates).  jpeg_decode_counts() says which decoder did the work: a file
that is quietly rerouted to the host decoder fails its row."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_stream_cases as C

pillow = C.pillow

pytestmark = pytest.mark.gpu


class _device_entropy:
    """the device entropy decoder always (and for restart-interval files too, if asked); the defaults afterwards"""

    def __init__(self, h, restart=False, chunk=None):
        self.h, self.restart, self.chunk = h, restart, chunk

    def __enter__(self):
        self.h.set_option("jpeg_device_entropy", 1)
        if self.restart:
            self.h.set_option("jpeg_device_restart", 1)
        if self.chunk:
            self.h.set_option("jpeg_chunk_bytes", self.chunk)
        return self.h

    def __exit__(self, *exc):
        self.h.set_option("jpeg_device_restart", 0)
        self.h.set_option("jpeg_device_entropy", 2)
        self.h.set_option("jpeg_chunk_bytes", 512)
        return False


def _decode_counted(h, datas):
    d0, h0 = h.jpeg_decode_counts()
    got = h.decode_jpeg_batch(datas)
    d1, h1 = h.jpeg_decode_counts()
    return got, (d1 - d0, h1 - h0)


def _check_batch(h, name, chunk=None):
    row = C.BY_NAME[name]
    datas, want = [f.data for f in C.files(name)], pillow(name)
    with _device_entropy(h, restart=row.restart, chunk=chunk):
        got, moved = _decode_counted(h, datas)
    for i in range(3):
        d = int(np.abs(got[i].astype(int) - want[i].astype(int)).max()) if got[i].shape == want[i].shape else -1
        print(f"{name}[{i}] chunk {chunk}: max |device - Pillow| = {d}; (device, host) = {moved}")
        assert np.array_equal(got[i], want[i]), (name, i, d)
    if row.route == "dri":
        assert sum(moved) == 3, (name, moved)
    elif row.route is not None:
        assert moved == row.route, (name, moved)


@pytest.mark.parametrize("name", C.DECODABLE)
def test_single_file_decode_equals_libjpeg(b0_handle, name):
    """dfd_decode_jpeg: host entropy decoder, then jpeg_idct_kernel and jpeg_color_kernel"""
    for i, (f, want) in enumerate(zip(C.files(name), pillow(name))):
        got = b0_handle.decode_jpeg(f.data)
        d = int(np.abs(got.astype(int) - want.astype(int)).max()) if got.shape == want.shape else -1
        print(f"{name}[{i}]: max |device - Pillow| = {d}")
        assert np.array_equal(got, want), (name, i, d)


@pytest.mark.parametrize("name", C.DECODABLE)
def test_device_entropy_batch_equals_libjpeg(b0_handle, name):
    """dfd_decode_jpeg_batch of the row's three files with the device entropy decoder on: Pillow's pixels, decoded where
    the row says (jpeg_color4_kernel / jpeg_color420_kernel / jpeg_color_kernel by width and alignment)"""
    _check_batch(b0_handle, name)


@pytest.mark.parametrize("chunk", [256, 4096])
@pytest.mark.parametrize("name", ["reversed-444", "reversed-422", "reversed-420", "two_bit_blocks-flat", "two_bit_blocks-stripes"])
def test_long_codes_and_short_blocks_at_other_chunk_sizes(b0_handle, name, chunk):
    _check_batch(b0_handle, name, chunk)


@pytest.mark.parametrize("name", [r.name for r in C.ROWS if r.kind != "decode"])
def test_files_that_are_not_decoded_are_refused(pkg, b0_handle, name):
    for f in C.files(name):
        with pytest.raises(pkg._lib.DfdError) as e:
            b0_handle.decode_jpeg(f.data)
        assert e.value.code == b0_handle.UNSUPPORTED


@pytest.mark.parametrize("name", ["adobe0", "rgb_ids"])
def test_rgb_samples_are_refused_loudly_and_the_handle_goes_on(pkg, b0_handle, name):
    """RGB samples (jdapimin.c: Adobe transform 0, or ids R, G, B, without JFIF) are not YCbCr -> RGB converted into wrong
    pixels: DFD_ERR_UNSUPPORTED from every entry point, and the handle still decodes a good batch on the device"""
    h = b0_handle
    bad, good = C.files(name)[0].data, C.files("adobe1")[0].data     # both 48 x 64, 4:4:4
    with pytest.raises(pkg._lib.DfdError) as e:
        h.decode_jpeg(bad)
    assert e.value.code == h.UNSUPPORTED and "RGB" in str(e.value)
    with _device_entropy(h):
        for batch in ([good, bad], [bad, good]):
            with pytest.raises(pkg._lib.DfdError) as e:
                h.decode_jpeg_batch(batch)
            assert e.value.code == h.UNSUPPORTED
    with pytest.raises(pkg._lib.DfdError) as e:
        h.analyze_jpeg(bad, True, stream_id=830, max_faces=4)
    assert e.value.code == h.UNSUPPORTED
    datas, want = [f.data for f in C.files("adobe1")], pillow("adobe1")
    with _device_entropy(h):
        got, moved = _decode_counted(h, datas)
    assert all(np.array_equal(got[i], want[i]) for i in range(3)) and moved == (3, 0)


def test_server_answers_an_rgb_jpeg_as_for_the_pillow_decoded_frame(pkg, b0_handle):
    """/analyze on an Adobe transform-0 file: the library refuses it (-7), the server's Pillow path decodes it, and the
    response is the one the Pillow-decoded frame gets"""
    srv = pkg.backend_server
    pkg.runtime.set_default_handle(b0_handle)
    data = C.adobe0_frame(240, 320, 7)
    with pytest.raises(pkg._lib.DfdError) as e:
        b0_handle.decode_jpeg(data)
    assert e.value.code == b0_handle.UNSUPPORTED
    frame = srv.decode_image(data)
    assert np.array_equal(frame, np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]))
    srv.app.config["TESTING"] = True
    with srv.app.test_client() as client:
        client.post("/reset")
        srv._last_request_time = 0.0
        r = client.post("/analyze", data={"frame": (io.BytesIO(data), "frame.jpg")}, content_type="multipart/form-data")
        assert r.status_code == 200, r.get_data()
        got = r.get_json()
        client.post("/reset")
        want = srv.detector.analyze_request(frame)
        client.post("/reset")
    for k, v in want.items():
        assert got[k] == v, k

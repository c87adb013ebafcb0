"""Restart-interval JPEGs on the device entropy decoder (csrc/jpeg_gpu_entropy.h, option "jpeg_device_restart").
Pillow's decode is the reference, bit for bit.  Every test switches the option on (and "jpeg_device_entropy" to 1:
always) and checks through jpeg_decode_counts() that the frames were decoded ON THE DEVICE, not quietly rerouted to the
host decoder.  The inputs are checked on their bytes first (DRI present, marker count, a stuffed zero directly in front
of a marker): a Pillow that encodes differently fails loudly."""
import io
import re

import numpy as np
import pytest
from PIL import Image

import frames as F


def _img(h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(xx / (7.0 + c) + c) * np.cos(yy / (11.0 - c)) for c in range(3)], -1)
    return np.clip(base + rs.randn(h, w, 3) * 12, 0, 255).astype(np.uint8)


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(50, 200, (h, w, 3), dtype=np.uint8)


def _gray(h, w, seed):
    return _img(h, w, seed)[..., 1]


def _jpeg(bgr, **kw):
    buf = io.BytesIO()
    im = Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])) if bgr.ndim == 3 else Image.fromarray(bgr)
    im.save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _pil_bgr(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def _scan(data):
    return data[data.index(b"\xff\xda"):]


def _markers(data):
    """offsets (in the file) of the FF of every RSTn marker of the scan"""
    at = data.index(b"\xff\xda")
    return [at + m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", data[at:])]


def _dri(data):
    i = data.index(b"\xff\xdd")
    return data[i + 4] * 256 + data[i + 5]


# name, source, (h, w), save arguments, DRI, RSTn markers, a stuffed zero directly in front of a marker somewhere in the batch
INPUTS = [
    ("mcu1", _img, (64, 96), dict(quality=80, restart_marker_blocks=1), 1, 23, False),         # several boundaries per chunk, numbers wrap past 7
    ("blocks5", _img, (50, 70), dict(quality=85, restart_marker_blocks=5), 5, 3, False),       # 20 MCUs; sizes no multiple of 16
    ("444", _img, (33, 17), dict(quality=75, subsampling=0, restart_marker_blocks=2), 2, 7, False),   # very short segments
    ("422rows", _img, (41, 95), dict(quality=60, subsampling=1, restart_marker_rows=1), 6, 5, False),
    ("gray", _gray, (45, 77), dict(quality=88, restart_marker_blocks=3), 3, 19, False),
    ("longseg", _noise, (240, 320), dict(quality=95, restart_marker_rows=1), 20, 14, True),    # segments of ~10 chunks
    ("optimised", _noise, (240, 320), dict(quality=95, optimize=True, restart_marker_blocks=7), 7, 42, True),   # own Huffman tables
    ("nomarker", _img, (8, 9), dict(quality=90, restart_marker_blocks=1), 1, 0, False),        # DRI and a single MCU
    ("1080p_mcu1", _noise, (1080, 1920), dict(quality=85, restart_marker_blocks=1), 1, 8159, True),   # large table, markers across piece / block edges
    ("1080p_rows", _img, (1080, 1920), dict(quality=85, restart_marker_rows=1), 120, 67, False),
]
_BY_NAME = {row[0]: row for row in INPUTS}
_cache = {}


def _batch(name):
    """the row's three files (seeds + i) and Pillow's decode of each - made once, shared, never modified"""
    if name not in _cache:
        _, src, (h, w), kw, dri, nmark, stuffed = _BY_NAME[name]
        datas = [_jpeg(src(h, w, h * 1000 + w + i), **kw) for i in range(3)]
        for d in datas:
            assert b"\xff\xdd" in d and _dri(d) == dri, (name, _dri(d))
            assert len(_markers(d)) == nmark, (name, len(_markers(d)))
        if stuffed:
            assert sum(len(re.findall(rb"\xff\x00\xff[\xd0-\xd7]", _scan(d))) for d in datas) >= 1, name
        _cache[name] = (datas, [_pil_bgr(d) for d in datas])
    return _cache[name]


class _restart_on:
    """both options on for the block, defaults afterwards"""

    def __init__(self, h):
        self.h = h

    def __enter__(self):
        self.h.set_option("jpeg_device_restart", 1)
        self.h.set_option("jpeg_device_entropy", 1)
        return self.h

    def __exit__(self, *exc):
        self.h.set_option("jpeg_device_restart", 0)
        self.h.set_option("jpeg_device_entropy", 2)
        self.h.set_option("jpeg_chunk_bytes", 512)
        self.h.set_option("jpeg_rounds", 16)
        return False


def _decode_counted(h, datas):
    d0, h0 = h.jpeg_decode_counts()
    got = h.decode_jpeg_batch(datas)
    d1, h1 = h.jpeg_decode_counts()
    return got, (d1 - d0, h1 - h0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [row[0] for row in INPUTS])
def test_restart_batch_equals_libjpeg_on_the_device(b0_handle, name):
    datas, want = _batch(name)
    with _restart_on(b0_handle) as h:
        got, moved = _decode_counted(h, datas)
    for i in range(3):
        assert np.array_equal(got[i], want[i]), (name, i)
    assert moved == (3, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [2, 16])
@pytest.mark.parametrize("chunk", [256, 512, 4096, 65536])
@pytest.mark.parametrize("name", ["mcu1", "longseg", "optimised"])
def test_restart_result_does_not_depend_on_chunk_size_or_rounds(b0_handle, name, chunk, rounds):
    """The pixels equal Pillow's for every chunk size and round count, and the frames are decoded on the device: two
    rounds must do even for the q95 noise files at 256-byte chunks (a call with "jpeg_chunk_bytes" 512 takes 256 for a
    batch this small), where a lane that guessed its start needs many chunks to fall into step with the true decode -
    the restart round kernel iterates inside a launch over the consecutive chunks of its block."""
    datas, want = _batch(name)
    with _restart_on(b0_handle) as h:
        h.set_option("jpeg_chunk_bytes", chunk)
        h.set_option("jpeg_rounds", rounds)
        got, moved = _decode_counted(h, datas)
    print(f"{name}: chunk {chunk} rounds {rounds}: device / host {moved}")
    for i in range(3):
        assert np.array_equal(got[i], want[i]), (name, chunk, rounds, i)
    assert moved == (3, 0), (name, chunk, rounds)


@pytest.mark.gpu
def test_restart_and_restartless_files_share_a_batch(b0_handle):
    kws = [dict(), dict(restart_marker_blocks=1), dict(restart_marker_blocks=5), dict(restart_marker_rows=1)]
    datas = [_jpeg(_img(64, 96, 300 + i), quality=80, **kw) for i, kw in enumerate(kws)]
    assert b"\xff\xdd" not in datas[0] and [_dri(d) for d in datas[1:]] == [1, 5, 6]
    with _restart_on(b0_handle) as h:
        got, moved = _decode_counted(h, datas)
    for i, d in enumerate(datas):
        assert np.array_equal(got[i], _pil_bgr(d)), i
    assert moved == (4, 0)


@pytest.mark.gpu
def test_analyze_jpegs_host_takes_restart_files_only_with_the_option(pkg, seeded_sd):
    W = pkg.weights
    h = pkg._lib.Handle(W.pack_all(seeded_sd, W.seeded_ssd_state_dict(0)), device=0, max_batch=16)
    try:
        datas = [_jpeg(F.natural_like(270, 480, seed=160 + i), quality=85, restart_marker_rows=1) for i in range(5)]
        assert all(_dri(d) == 30 and len(_markers(d)) == 16 for d in datas)
        decoded = np.stack([_pil_bgr(d) for d in datas])
        boxes = [[(40, 30, 120, 140), (250, 60, 160, 180)]] * len(datas)
        fd = h.alloc(decoded.nbytes).upload(decoded)
        want = h.analyze_batch_device(fd.ptr, len(datas), 270, 480, forced_boxes=boxes, max_faces=2, with_forensics=True)
        fd.free()
        # off (the default): refused, as before
        with pytest.raises(pkg._lib.DfdError) as e:
            h.analyze_jpegs_host(datas, 3, forced_boxes=boxes, max_faces=2, with_forensics=True)
        assert e.value.code == h.UNSUPPORTED
        with _restart_on(h):
            d0, h0 = h.jpeg_decode_counts()
            got = h.analyze_jpegs_host(datas, 3, forced_boxes=boxes, max_faces=2, with_forensics=True)
            assert h.jpeg_decode_counts() == (d0 + 5, h0)
        assert got[3] == (270, 480) and got[0] == want[0]
        assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
        assert np.array_equal(got[2], want[2])
        with pytest.raises(pkg._lib.DfdError) as e:
            h.analyze_jpegs_host(datas, 3, forced_boxes=boxes, max_faces=2, with_forensics=True)
        assert e.value.code == h.UNSUPPORTED
    finally:
        h.close()


def _outcome(pkg, h, datas):
    try:
        return ("pixels", [a.copy() for a in h.decode_jpeg_batch(datas)])
    except pkg._lib.DfdError as e:
        return ("error", type(e), e.code)


@pytest.mark.gpu
def test_malformed_restart_structure_goes_to_the_host_decoder(pkg, b0_handle):
    """a marker missing, a marker with the wrong number, a marker too many: the device decoder does not vouch for the
    frame, so the batch ends as it does with the option off (the host decoder's pixels or its error), and the handle
    goes on decoding good batches on the device"""
    datas, want = _batch("mcu1")
    good = datas[0]
    at = _markers(good)
    assert len(at) == 23 and good[at[10] + 1] == 0xD0 + 10 % 8
    variants = {
        "deleted": good[:at[10]] + good[at[10] + 2:],
        "wrong number": good[:at[10] + 1] + bytes([0xD0 + 5]) + good[at[10] + 2:],
        "extra": good[:at[10]] + b"\xff\xd0" + good[at[10]:],
    }
    h = b0_handle
    for what, bad in variants.items():
        assert len(_markers(bad)) == {"deleted": 22, "wrong number": 23, "extra": 24}[what]
        h.set_option("jpeg_device_entropy", 1)
        try:
            off = _outcome(pkg, h, [good, bad])
            with _restart_on(h):
                d0, h0 = h.jpeg_decode_counts()
                on = _outcome(pkg, h, [good, bad])
                d1, h1 = h.jpeg_decode_counts()
                again, moved = _decode_counted(h, datas)
        finally:
            h.set_option("jpeg_device_entropy", 2)
        assert on[0] == off[0], what
        if on[0] == "error":
            assert on[1:] == off[1:], what
        else:
            assert all(np.array_equal(a, b) for a, b in zip(on[1], off[1])), what
            assert np.array_equal(on[1][0], want[0]), what
            assert (d1 - d0, h1 - h0) == (1, 1), what               # the good file on the device, the variant handed over
        assert moved == (3, 0) and all(np.array_equal(again[i], want[i]) for i in range(3)), what


@pytest.mark.gpu
def test_server_route_takes_the_option_from_the_environment(pkg, seeded_sd, monkeypatch):
    """DFD_JPEG_DEVICE_RESTART=1 when the handle is created: analyze_request_batch (dfd_analyze_stream_batch) decodes
    restart-interval JPEGs on the device and answers as for the same frames encoded without restart markers"""
    frames = [F.natural_like(270, 480, seed=180 + i) for i in range(4)]
    plain = [_jpeg(f, quality=85) for f in frames]
    rst = [_jpeg(f, quality=85, restart_marker_rows=1) for f in frames]
    assert all(b"\xff\xdd" in d and len(_markers(d)) == 16 for d in rst) and all(b"\xff\xdd" not in d for d in plain)
    if not all(np.array_equal(_pil_bgr(a), _pil_bgr(b)) for a, b in zip(plain, rst)):
        pytest.skip("this Pillow decodes other pixels from the files with restart markers")
    monkeypatch.setenv("DFD_JPEG_DEVICE_RESTART", "1")
    W = pkg.weights
    h = pkg._lib.Handle(W.pack_all(seeded_sd, W.seeded_ssd_state_dict(0)), device=0, max_batch=16)
    try:
        h.set_option("jpeg_device_entropy", 1)
        D = pkg.deepfake_detection.DeepfakeDetector
        det = D(use_tta=False, num_tta_augmentations=1, detection_threshold=0.55, handle=h)
        want = det.analyze_request_batch(plain)
        d0, h0 = h.jpeg_decode_counts()
        det = D(use_tta=False, num_tta_augmentations=1, detection_threshold=0.55, handle=h)
        got = det.analyze_request_batch(rst)
        d1, h1 = h.jpeg_decode_counts()
        assert got == want
        assert (d1 - d0, h1 - h0) == (4, 0)
    finally:
        h.close()

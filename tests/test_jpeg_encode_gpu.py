"""GPU: the device JPEG encoder (csrc/jpeg_encode.hip; dfd_encode_jpeg*, Handle.encode_jpeg*, MTCNN save_path,
DeepfakeDetector.explain_face(as_jpeg=True)) writes Pillow's file, byte for byte, over the corpus of jpeg_encode_cases.py
(tests/test_jpeg_encode_oracle.py holds the numpy restatement to the same files and checks what the corpus covers)."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

import jpeg_encode_cases as CS
import jpeg_encode_oracle as O
import mt_images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pillow():
    return {c[0]: O.pillow_bytes(*c[1:]) for c in CS.CASES}


def _first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def _same(got, want, what):
    assert got == want, f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {_first_diff(got, want)}"


@pytest.mark.parametrize("case", CS.PLAIN, ids=[c[0] for c in CS.PLAIN])
def test_bytes_equal_pillow(b0_handle, pillow, case):
    name, img, q, sub, rb = case
    _same(b0_handle.encode_jpeg(img, q, sub, rb), pillow[name], name)


@pytest.mark.parametrize("case", CS.RESTART, ids=[c[0] for c in CS.RESTART])
def test_restart_intervals_equal_pillow(b0_handle, pillow, case):
    name, img, q, sub, rb = case
    got = b0_handle.encode_jpeg(img, q, sub, rb)
    _same(got, pillow[name], name)
    if CS._mcus(case) > 8 * rb:
        assert got.count(b"\xff\xd0") >= 2                        # FF D0 is RST0 wherever it stands: the counter wrapped


def test_big_case_spans_several_scan_workgroups(pkg):
    src = open(os.path.join(ROOT, "real-time-video-deepfake-detection_amd", "csrc", "jpeg_encode.hip")).read()
    tile = int(re.search(r"constexpr int kEncScanTile = (\d+);", src).group(1))
    assert tile == pkg._lib.JPEG_ENC_SCAN_TILE
    assert CS.BIG_BLOCKS > tile
    assert any(c[1].shape[:2] == CS.BIG and c[3] == 0 for c in CS.PLAIN)


def test_rgb_order_flag(b0_handle, pillow):
    name, img, q, sub, rb = next(c for c in CS.PLAIN if c[0].startswith("natural-640x360-420"))
    _same(b0_handle.encode_jpeg(np.ascontiguousarray(img[..., ::-1]), q, sub, rb, rgb=True), pillow[name], name)


def test_shuffled_mixed_batch_equals_the_singles(b0_handle, pillow):
    """every case of the corpus in ONE call, in a shuffled order, and again in another: each file is Pillow's"""
    for seed in (0, 1):
        order = np.random.RandomState(seed).permutation(len(CS.CASES))
        cases = [CS.CASES[i] for i in order]
        got = b0_handle.encode_jpegs([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases])
        for c, g in zip(cases, got):
            _same(g, pillow[c[0]], f"batch order {seed}: {c[0]}")


def test_device_source_equals_host_source(b0_handle, pillow):
    cases = [c for c in CS.CASES if "360" in c[0] or "53" in c[0] or "1x1" in c[0]]
    bufs, srcs = [], []
    for c in cases:
        img = c[1]
        stride = img.shape[1] * (1 if img.ndim == 2 else 3) + 5                    # rows 5 bytes apart from packed
        padded = np.full((img.shape[0], stride), 0xEE, np.uint8)
        padded[:, :stride - 5] = img.reshape(img.shape[0], -1)
        buf = b0_handle.alloc(padded.nbytes).upload(padded)
        bufs.append(buf)
        srcs.append((buf.ptr, img.shape[0], img.shape[1], stride, 1 if img.ndim == 2 else 3))
    got = b0_handle.encode_jpegs_device(srcs, [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases])
    for buf in bufs:
        buf.free()
    for c, g in zip(cases, got):
        _same(g, pillow[c[0]], "device source " + c[0])


def _pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def test_device_decoders_read_the_files(b0_handle, pillow):
    """dfd_decode_jpeg and the batched device entropy decoder (restart files included) on the encoder's output = Pillow's
    decode of Pillow's file"""
    singles = [c for c in CS.CASES if "160x160" in c[0] or "17x13" in c[0] or "640x360-420" in c[0]]
    for c in singles:
        got = b0_handle.encode_jpeg(*c[1:])
        assert np.array_equal(b0_handle.decode_jpeg(got), _pil_decode(pillow[c[0]])), c[0]
    batch = [c for c in CS.CASES if "160x160-420" in c[0]]
    assert any(c[4] for c in batch) and len(batch) >= 3
    b0_handle.set_option("jpeg_device_restart", 1)
    b0_handle.set_option("jpeg_device_entropy", 1)
    try:
        before = b0_handle.jpeg_decode_counts()
        files = b0_handle.encode_jpegs([c[1] for c in batch], [c[2] for c in batch], [c[3] for c in batch], [c[4] for c in batch])
        frames = b0_handle.decode_jpeg_batch(files)
        after = b0_handle.jpeg_decode_counts()
    finally:
        b0_handle.set_option("jpeg_device_restart", 0)
        b0_handle.set_option("jpeg_device_entropy", 2)
    print("frames decoded on the device / on the host:", after[0] - before[0], after[1] - before[1])
    for c, f in zip(batch, frames):
        assert np.array_equal(f, _pil_decode(pillow[c[0]])), c[0]


def test_short_capacity_reports_the_size_and_writes_nothing(pkg, b0_handle, pillow):
    name, img, q, sub, rb = next(c for c in CS.PLAIN if c[0].startswith("noise-256x256-420"))
    want = pillow[name]
    lib, ln = b0_handle._lib, C.c_size_t()
    for cap in (0, 100, len(want) - 1):
        out = np.full(len(want) + 4096, 0xA5, np.uint8)
        rc = lib.dfd_encode_jpeg(b0_handle._p, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], 0, q, sub, rb,
                                 out.ctypes.data, cap, C.byref(ln))
        assert rc == -1 and ln.value == len(want), (cap, rc, ln.value)
        assert (out == 0xA5).all(), cap                                            # nothing written, guard included
    out = np.full(len(want) + 4096, 0xA5, np.uint8)
    rc = lib.dfd_encode_jpeg(b0_handle._p, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], 0, q, sub, rb,
                             out.ctypes.data, len(want), C.byref(ln))
    assert rc == 0 and ln.value == len(want) and out[:len(want)].tobytes() == want
    assert (out[len(want):] == 0xA5).all()
    assert lib.dfd_encode_jpeg_bound(img.shape[0], img.shape[1], sub) >= len(want)


def test_bound_covers_the_corpus(b0_handle, pillow):
    for c in CS.CASES:
        sub = 3 if c[1].ndim == 2 else c[3]
        assert b0_handle._lib.dfd_encode_jpeg_bound(c[1].shape[0], c[1].shape[1], sub) >= len(pillow[c[0]]), c[0]


def test_bad_arguments_and_oversize(pkg, b0_handle):
    lib, ln = b0_handle._lib, C.c_size_t()
    img = np.zeros((16, 16, 3), np.uint8)
    out = np.zeros(4096, np.uint8)

    def call(hh=16, ww=16, stride=48, q=75, sub=2, rb=0, pixels=img.ctypes.data):
        return lib.dfd_encode_jpeg(b0_handle._p, pixels, hh, ww, stride, 0, q, sub, rb, out.ctypes.data, out.size, C.byref(ln))

    assert call() == 0
    for kw in (dict(hh=0), dict(ww=0), dict(hh=-3), dict(q=0), dict(q=101), dict(sub=4), dict(sub=-1), dict(stride=47),
               dict(rb=-1), dict(rb=65536), dict(pixels=None)):
        assert call(**kw) == -1, kw
    # above 2^24 pixels: refused from the arguments alone, before a pixel is read
    assert call(hh=4097, ww=4096, stride=4096 * 3) == -7
    assert call(hh=4096, ww=4097, stride=4097 * 3, sub=0) == -7
    assert lib.dfd_encode_jpeg_bound(4097, 4096, 2) == 0 and lib.dfd_encode_jpeg_bound(0, 5, 2) == 0
    with pytest.raises(pkg._lib.DfdError):
        b0_handle.encode_jpeg(img, quality=0)


def _pil_save(crop_rgb_u8):
    buf = io.BytesIO()
    Image.fromarray(crop_rgb_u8).save(buf, format="JPEG")
    return buf.getvalue()


def _crop_u8(t):
    return np.ascontiguousarray(np.asarray(t).transpose(1, 2, 0)).astype(np.uint8)


@pytest.mark.parametrize("post_process", [False, True])
def test_mtcnn_save_path(pkg, mt_handle, tmp_path, post_process):
    rgb = mt_images.textured(300, 280, 100)                                        # 5 faces with the default cascade
    raw = pkg.mtcnn.MTCNN(post_process=False, select_largest=False, keep_all=True, handle=mt_handle)(rgb)
    assert raw is not None and len(raw) > 2
    # keep_all: name.jpg, name_2.jpg, ...
    m = pkg.mtcnn.MTCNN(post_process=post_process, select_largest=False, keep_all=True, handle=mt_handle)
    path = str(tmp_path / "all" / "face.jpg")
    faces = m(rgb, save_path=path)
    assert np.array_equal(np.asarray(faces), np.asarray(m(rgb)))                   # the return value does not change
    for k in range(len(raw)):
        name = path if k == 0 else str(tmp_path / "all" / f"face_{k + 1}.jpg")
        _same(open(name, "rb").read(), _pil_save(_crop_u8(raw[k])), name)
    assert not os.path.exists(str(tmp_path / "all" / f"face_{len(raw) + 1}.jpg"))
    # one face; forward and extract; a list of images with a list of paths
    one = pkg.mtcnn.MTCNN(post_process=post_process, select_largest=False, handle=mt_handle)
    raw1 = pkg.mtcnn.MTCNN(post_process=False, select_largest=False, handle=mt_handle)(rgb)
    p1, p2 = str(tmp_path / "one.jpeg"), str(tmp_path / "two.jpg")
    one(rgb, save_path=p1)
    _same(open(p1, "rb").read(), _pil_save(_crop_u8(raw1)), p1)
    boxes, _ = one.detect(rgb)
    one.extract(rgb, boxes, save_path=p2)
    _same(open(p2, "rb").read(), _pil_save(_crop_u8(raw1)), p2)
    rgb2 = mt_images.textured(260, 340, 121)
    raw2 = pkg.mtcnn.MTCNN(post_process=False, select_largest=False, handle=mt_handle)(rgb2)
    pl = [str(tmp_path / "l0.jpg"), str(tmp_path / "l1.jpg")]
    one([rgb, rgb2], save_path=pl)
    _same(open(pl[0], "rb").read(), _pil_save(_crop_u8(raw1)), pl[0])
    _same(open(pl[1], "rb").read(), _pil_save(_crop_u8(raw2)), pl[1])
    with pytest.raises(ValueError):
        one(rgb, save_path=str(tmp_path / "face.png"))


def test_explain_face_as_jpeg(pkg, mt_handle):
    rs = np.random.RandomState(11)
    frame = rs.randint(40, 215, (480, 640, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:480, 0:640]
    frame = np.clip(frame * 0.4 + (110 + 60 * np.sin(xx / 19.0) * np.cos(yy / 27.0))[..., None] * 0.6, 0, 255).astype(np.uint8)
    det = pkg.deepfake_detection.DeepfakeDetector(enable_gradcam=True, use_tta=False, num_tta_augmentations=1, handle=mt_handle)
    seen = 0
    for x, y, w, h in ([20, 30, 300, 280], [330, 40, 200, 180]):
        face = np.ascontiguousarray(frame[y:y + h, x:x + w])
        plain, res = det.explain_face(face), det.explain_face(face, as_jpeg=True)
        if plain is None:
            assert res is None
            continue
        seen += 1
        assert sorted(plain) == ["fake_probability", "heatmap", "overlay"]         # the default call: no new key
        assert sorted(res) == ["fake_probability", "heatmap", "overlay", "overlay_jpeg"]
        assert np.array_equal(res["overlay"], plain["overlay"])
        _same(res["overlay_jpeg"], O.pillow_bytes(res["overlay"], 95, 2), "overlay")
    assert seen > 0

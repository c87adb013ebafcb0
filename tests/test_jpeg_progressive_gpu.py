"""GPU: progressive JPEGs through every entry that takes JPEG bytes, with option "jpeg_progressive" = 1: decoded frames equal
Pillow's BGR bit for bit on the corpus of tests/test_jpeg_progressive.py (the chain behind the coefficient planes -
dequantisation, IDCT, upsampling, colour - is the baseline decoder's), the analysing entries equal the same call on
Pillow's frame, a damaged file gives the host decoder's status and leaves the handle usable, the server takes the variable
DFD_JPEG_PROGRESSIVE, and a progressive batch after larger batches equals a fresh handle's bits.  With the option off (the
default) the same calls refuse the files as before."""
import io

import numpy as np
import pytest

import frames as F
import history_cases as H
import jpeg_progressive_cases as PC
import jpeg_progressive_history as PH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = H.new_handle()
    h.set_option("jpeg_progressive", 1)
    yield h
    h.close()


@pytest.fixture(params=[0, 1], ids=["host_pool", "device"])
def device(request, handle):
    """option "jpeg_device_progressive" for the test: 0 = the host pool decodes the scans in batch calls, 1 = the device"""
    handle.set_option("jpeg_device_progressive", request.param)
    yield request.param
    handle.set_option("jpeg_device_progressive", 0)


def _code(call):
    try:
        call()
        return 0
    except H.L.DfdError as e:
        return e.code


def test_the_option_is_off_by_default_and_switches_every_entry(handle):
    h = H.new_handle()
    try:
        p = PC.by_name("96x128.420.q85").progressive
        calls = (lambda: h.decode_jpeg(p), lambda: h.decode_jpeg_batch([p, p]), lambda: h.analyze_jpeg(p, True, stream_id=900),
                 lambda: h.analyze_jpegs_host([p, p], 2), lambda: h.analyze_stream_batch([p, p], [True, False], stream_id=901),
                 lambda: h.analyze_streams_batch([p, p], [902, 903], [True, True]))
        assert [_code(c) for c in calls] == [-7] * 6
        h.set_option("jpeg_progressive", 1)
        assert [_code(c) for c in calls] == [0] * 6
        h.set_option("jpeg_progressive", 0)
        assert [_code(c) for c in calls] == [-7] * 6
    finally:
        h.close()


def test_decode_jpeg_and_the_batch_equal_pillow_on_the_corpus(handle, device):
    for p in PC.corpus() + PC.scripted():
        want = PC.pillow_bgr(p.progressive)
        assert np.array_equal(handle.decode_jpeg(p.progressive), want), p.name
        n = 2 if p.name.startswith("1464") else 3                    # (the large file batched with itself: the one-size rule)
        d0, h0 = handle.jpeg_decode_counts()
        got = handle.decode_jpeg_batch([p.progressive] * n)
        d1, h1 = handle.jpeg_decode_counts()
        assert all(np.array_equal(g, want) for g in got), p.name    # (the device's coefficients are the host path's: the frames say so)
        assert (d1 - d0, h1 - h0) == ((n, 0) if device else (0, n)), p.name


def test_a_batch_mixes_baseline_progressive_restart_and_optimised_files(handle, device):
    names = ("96x128.420.q85", "96x128.420.restart3", "96x128.420.optimize", "96x128.420.q100")
    files = [PC.by_name(names[0]).baseline] + [PC.by_name(n).progressive for n in names]
    for entropy in (2, 1):                                          # the default, and the device decoder asked for: the host pool takes a mixed batch
        handle.set_option("jpeg_device_entropy", entropy)
        try:
            d0, h0 = handle.jpeg_decode_counts()
            got = handle.decode_jpeg_batch(files)
            d1, h1 = handle.jpeg_decode_counts()
        finally:
            handle.set_option("jpeg_device_entropy", 2)
        # counted like the others: with the device option its four progressive files, the baseline one by the host decoder
        assert (d1 - d0, h1 - h0) == ((4, 1) if device else (0, 5))
        for g, f in zip(got, files):
            assert np.array_equal(g, PC.pillow_bgr(f))


def test_analyze_jpeg_equals_analyze_frame_on_pillows_frame(handle):
    h = handle
    for i, frame in enumerate((F.natural_like(480, 640, seed=9), F.face_frame(640, 480, 2))):
        data = PC.pillow(np.ascontiguousarray(frame[..., ::-1]), quality=85, progressive=True)
        decoded = PC.pillow_bgr(data)
        h.forensics_reset(910 + i)
        h.forensics_reset(920 + i)
        a = h.analyze_frame(decoded, True, stream_id=910 + i, max_faces=4)
        b = h.analyze_jpeg(data, True, stream_id=920 + i, max_faces=4)
        diffs = H.compare({"result": list(a)}, {"result": list(b[:4])})     # field for field, bit for bit (the same NaN is the same result)
        assert not diffs, H.report(diffs)
        assert b[4] == (480, 640)


def _same_results(got, want):
    assert len(got) == len(want)
    diffs = H.compare({"results": [list(g) for g in got]}, {"results": [list(w) for w in want]})
    assert not diffs, H.report(diffs)


def test_the_batched_entries_take_a_progressive_part_and_equal_the_call_on_the_decoded_frame(handle, device):
    h = handle
    counted = ((2, 1) if device else (0, 3))                        # (device, host): two progressive parts and a baseline one

    def counting(call):
        d0, h0 = h.jpeg_decode_counts()
        out = call()
        d1, h1 = h.jpeg_decode_counts()
        assert (d1 - d0, h1 - h0) == counted
        return out

    frames = [F.natural_like(240, 320, seed=20 + i) for i in range(3)]
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames]
    parts = [PC.pillow(rgb[0], quality=85), PC.pillow(rgb[1], quality=85, progressive=True),
             PC.pillow(rgb[2], quality=85, progressive=True, optimize=True)]
    decoded = [PC.pillow_bgr(p) for p in parts]
    full = [True, True, False]
    for s in range(930, 936):
        h.forensics_reset(s)
    _same_results(counting(lambda: h.analyze_streams_batch(parts, [930, 931, 930], full, max_faces=4)),
                  h.analyze_streams_batch(decoded, [932, 933, 932], full, max_faces=4))
    got, shape = counting(lambda: h.analyze_stream_batch(parts, full, stream_id=934, max_faces=4))
    want, _ = h.analyze_stream_batch(decoded, full, stream_id=935, max_faces=4)
    _same_results(got, want)
    assert shape == (240, 320)
    # dfd_analyze_jpegs_host: as dfd_analyze_batch_device on the decoded frames, chunk by chunk
    a = counting(lambda: h.analyze_jpegs_host(parts, 2, max_faces=4, with_forensics=True))      # chunks (baseline, progressive), (progressive)
    # a restart-interval baseline chunk IN FRONT of the progressive file: decided once every chunk is parsed
    first = PC.pillow(rgb[0], quality=85, restart_marker_blocks=3)
    c = h.analyze_jpegs_host([first, parts[0], parts[1], parts[2]], 2, max_faces=4, with_forensics=True)
    diffs = H.compare({"r": [c[0][1:], c[1][1:], c[2][1:]]}, {"r": [a[0], a[1], a[2]]})     # (frames 1..3 of it are the call above)
    assert not diffs, H.report(diffs)
    b = h.analyze_jpegs_host([PC.pillow(r, quality=85) for r in rgb], 2, max_faces=4, with_forensics=True)
    diffs = H.compare({"results": list(a)}, {"results": list(b)})  # (the baseline files of the same pixels: the device decoder's route)
    assert not diffs, H.report(diffs)


def test_a_damaged_file_in_a_batch_gives_the_host_decoders_status_and_nothing_moves(handle, device, monkeypatch, capfd):
    monkeypatch.setenv("DFD_JPEG_VERBOSE", "1")                     # the device route says which frame it hands to the host decoder
    handed_back = 0
    good = [PC.by_name(n).progressive for n in ("37x53.420.restart3", "37x53.420.q85", "37x53.420.optimize")]
    want = handle.decode_jpeg_batch(good)
    rejected = [(n, f) for n, f in PC.damaged() if n.startswith("37x53") and PC.walker_verdict(f)[0] is None]
    assert len(rejected) >= 12
    for name, bad in rejected[::3]:
        try:
            H.L.jpeg_coefficients(bad, progressive=True)
            status, in_scan = 0, False
        except H.L.DfdError as e:
            status, in_scan = e.code, "in scan" in str(e)           # the host decoder names the scan whose data is defective
        assert status in (-1, -7)
        capfd.readouterr()
        assert _code(lambda: handle.decode_jpeg_batch([good[0], bad, good[2]])) == status, name
        said = "jpeg device progressive: frame 1 defect" in capfd.readouterr().err
        # a file whose headers parse (-1 comes from a scan) reaches the device, which finds the defect and hands it back
        assert said == bool(device and in_scan), (name, status)
        handed_back += said
        assert _code(lambda: handle.decode_jpeg(bad)) == status, name
        assert np.array_equal(handle.decode_jpeg_batch(good), want), name       # the batch without it: the same bits afterwards
    assert sum(1 for n, f in rejected[::3] if ".cut" not in n) >= 2 and (handed_back >= 2 if device else handed_back == 0)


@pytest.mark.parametrize("dev", [0, 1], ids=["host_pool", "device"])
def test_the_server_takes_the_variable_and_decodes_progressive_requests_in_the_library(pkg, monkeypatch, dev):
    monkeypatch.setenv("DFD_JPEG_PROGRESSIVE", "1")
    h = H.new_handle()                                              # the variable is read when a handle is made
    h.set_option("jpeg_device_progressive", dev)
    srv = pkg.backend_server
    before = pkg.runtime.peek_default_handle()
    det = srv.detector                                              # it keeps the handle it first resolved: hand it this one, and the old one back
    kept = (det._handle, det.frame_analyzer._handle)
    try:
        pkg.runtime.set_default_handle(h)
        det._handle = det.frame_analyzer._handle = None
        srv.app.config["TESTING"] = True
        frame = F.natural_like(480, 640, 33)
        data = PC.pillow(np.ascontiguousarray(frame[..., ::-1]), quality=85, progressive=True)
        assert _code(lambda: h.decode_jpeg(data)) == 0               # no set_option: the variable did it
        with srv.app.test_client() as client:
            client.post("/reset")
            srv._last_request_time = 0.0
            r = client.post("/analyze", data={"frame": (io.BytesIO(data), "frame.jpg")}, content_type="multipart/form-data")
            assert r.status_code == 200
            a = r.get_json()
            client.post("/reset")
            want = srv.detector.analyze_request(srv.decode_image(data))       # Pillow's decode + raw upload
            for k, v in want.items():
                assert a[k] == v, k
            client.post("/reset")
            srv._last_request_time = 0.0
            d0, h0 = h.jpeg_decode_counts()
            r = client.post("/analyze_batch", data={"frame": [(io.BytesIO(data), f"f{i}.jpg") for i in range(3)]},
                            content_type="multipart/form-data")
            assert r.status_code == 200 and r.get_json()["frames"] == 3
            d1, h1 = h.jpeg_decode_counts()
            assert (d1 - d0, h1 - h0) == ((3, 0) if dev else (0, 3))      # decoded by the library, not by Pillow
            client.post("/reset")
    finally:
        det._handle, det.frame_analyzer._handle = kept
        pkg.runtime.set_default_handle(before)
        h.close()


@pytest.mark.parametrize("dev", [0, 1], ids=["host_pool", "device"])
def test_a_progressive_batch_after_larger_batches_equals_a_fresh_handles_bits(dev):
    """the case jpeg_progressive_history registers with the call-history table, after its own history"""
    fresh = H.new_handle()
    try:
        want = PH.run(fresh, device=dev)
    finally:
        fresh.close()
    colour, gray = PH.case_files()
    assert np.array_equal(want["batch"], np.stack([PC.pillow_bgr(f) for f in colour]))
    assert np.array_equal(want["batch_gray"][0], PC.pillow_bgr(gray[0]))
    used = H.new_handle()
    try:
        for name, history in PH.HISTORIES.items():
            history(used, dev)
            diffs = H.compare(want, PH.run(used, device=dev))
            assert not diffs, f"{name}: {H.report(diffs)}"
        diffs = H.compare(want, PH.run(used, device=dev))            # and once more: "repeat"
        assert not diffs, H.report(diffs)
    finally:
        used.close()

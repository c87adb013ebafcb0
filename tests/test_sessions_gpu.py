"""GPU: one device pass over frames of many streams (dfd_analyze_streams_batch), the session pool and the session routes.

Every result is compared bit for bit with the existing per-stream entry points (dfd_analyze_jpeg / dfd_analyze_frame,
DeepfakeDetector.analyze_request) run on each stream's frames alone, in order."""
import io
import threading
import time

import numpy as np
import pytest
from PIL import Image

import frames as F

pytestmark = pytest.mark.gpu


def _jpeg(frame_bgr, **kw):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format="JPEG", quality=85, **kw)
    return buf.getvalue()


def _frame(h, w, seed):
    return F.natural_like(h, w, seed) if seed % 4 else F.face_frame(w, h, seed)


def _single(h, item, sid, full, max_faces):
    """the existing one-frame entry points -> (scores, prob, boxes, logits, n_detected)"""
    if isinstance(item, bytes):
        scores, prob, boxes, logits, shape = h.analyze_jpeg(item, full, stream_id=sid, max_faces=max_faces)
    else:
        scores, prob, boxes, logits = h.analyze_frame(item, full, stream_id=sid, max_faces=max_faces)
        shape = item.shape[:2]
    small = shape[0] < 30 or shape[1] < 30
    return scores, prob, boxes, logits, 0 if small or not boxes else h.last_detection_count()


def _same(a, b):
    sa, pa, ba, la, na = a[:5]
    sb, pb, bb, lb, nb = b[:5]
    assert sa == sb and pa == pb and ba == bb and na == nb
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))


def _workload(seed):
    """12 frames of 5 streams in 3 sizes, JPEG and raw parts interleaved, stream 1 twice in a row, one 24 x 24 frame"""
    sizes = [(405, 720), (540, 720), (720, 405)]
    order = [0, 1, 1, 2, 3, 4, 0, 2, 3, 1, 4, 0]
    items = []
    for k, s in enumerate(order):
        if k == 7:
            fr = F.natural_like(24, 24, seed + k)
        else:
            hh, ww = sizes[(s + k) % 3]
            fr = _frame(hh, ww, seed + k)
        items.append(_jpeg(fr) if (k + s) % 2 else fr)
    return order, items, [(seed + k) % 3 == 0 for k in range(len(order))]


def test_streams_batch_equals_separate_streams(b0_handle):
    h = b0_handle
    base_ref, base_new = 7100, 7200
    for rnd in range(2):                                           # the second call continues every stream
        order, items, full = _workload(10 * rnd + 1)
        got = h.analyze_streams_batch(items, [base_new + s for s in order], full, max_faces=4)
        for k, s in enumerate(order):
            _same(got[k], _single(h, items[k], base_ref + s, full[k], 4))
        for s in set(order):
            assert h.forensics_state(base_new + s) == h.forensics_state(base_ref + s)
        assert got[7][5] == (24, 24) and got[7][2] == [] and got[7][4] == 0
        assert {g[5] for g in got} == {(405, 720), (540, 720), (720, 405), (24, 24)}
    for s in range(5):
        h.forensics_release(base_new + s)
        h.forensics_release(base_ref + s)


def test_refused_part_moves_nothing(b0_handle):
    h = b0_handle
    frames = [_frame(405, 720, 50 + i) for i in range(3)]
    items = [_jpeg(frames[0]), frames[1], _jpeg(frames[2], progressive=True)]
    h.analyze_streams_batch(items[:2], [7301, 7302], [True, True])
    before = [h.forensics_state(s) for s in (7301, 7302, 7303)]
    with pytest.raises(Exception) as e:
        h.analyze_streams_batch(items, [7301, 7302, 7303], [False, False, False])
    assert e.value.code == h.UNSUPPORTED and e.value.bad_index == 2
    assert [h.forensics_state(s) for s in (7301, 7302, 7303)] == before
    for s in (7301, 7302, 7303):
        h.forensics_release(s)


def _device_free_bytes():
    """hipMemGetInfo of the HIP runtime the library runs on (after the library's calls, which all synchronise)"""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_released_stream_starts_fresh_and_planes_are_reused(b0_handle):
    h = b0_handle
    fr = [_frame(405, 720, 60 + i) for i in range(3)]
    h.analyze_streams_batch(fr, [7401] * 3, [True, False, False])
    assert h.forensics_state(7401) == (3, 2, True)
    h.forensics_release(7401)
    assert h.forensics_state(7401) == (0, 0, False)
    res = h.analyze_streams_batch([fr[2]], [7401], [False])
    assert res[0][0]["temporal"] == 0.0 and h.forensics_state(7401) == (1, 0, True)
    want = h.analyze_frame(fr[2], False, stream_id=7402)           # a new stream's first frame
    assert res[0][0] == want[0] and res[0][1] == want[1]
    h.forensics_release(7401)
    h.forensics_release(7402)
    # 512 short-lived streams: without the free list that is 32 MiB of device planes
    tiny = F.natural_like(24, 24, 1)
    h.analyze_streams_batch([tiny], [7500], [True])
    h.forensics_release(7500)
    free0 = _device_free_bytes()
    for k in range(512):
        h.analyze_streams_batch([tiny], [7501 + k], [True])
        h.forensics_release(7501 + k)
    assert free0 - _device_free_bytes() < (8 << 20)


def _session_frames(n_sessions, n_frames):
    return {f"s{i}": [_jpeg(_frame(405, 720, 100 * i + t)) if (i + t) % 3 else _frame((405, 540, 720)[i % 3], 720, 100 * i + t)
                      for t in range(n_frames)] for i in range(n_sessions)}


def test_pool_matches_dedicated_detectors_in_one_pass_per_round(pkg, b0_handle):
    D = pkg.deepfake_detection.DeepfakeDetector
    work = _session_frames(16, 3)
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=b0_handle, lock=lock)
    got = {sid: [] for sid in work}
    for t in range(3):
        passes = pool.passes
        with lock:                                  # all 16 queue while the handle is "busy": one library call
            futs = {sid: pool.submit(sid, [frames[t]]) for sid, frames in work.items()}
        for sid, fu in futs.items():
            got[sid] += fu.result(timeout=120)
        assert pool.passes == passes + 1
    for sid, frames in work.items():
        det = D(detection_threshold=0.55, handle=b0_handle)
        want = [det.analyze_request(jpeg=f) if isinstance(f, bytes) else det.analyze_request(f) for f in frames]
        assert got[sid] == want, sid
        det.release()
    for sid in work:
        pool.close(sid)


def test_server_sessions_equal_dedicated_detectors(pkg, b0_handle, monkeypatch):
    srv = pkg.backend_server
    pkg.runtime.set_default_handle(b0_handle)
    srv.app.config["TESTING"] = True
    monkeypatch.setattr(srv, "_session_pool", pkg.sessions.SessionPool(handle=b0_handle, lock=srv._detector_lock))
    monkeypatch.setattr(srv, "_session_last", {})
    with srv.app.test_client() as c:
        c.post("/reset")
    g0 = (srv.detector.frame_count, len(srv.detector.temporal_tracker.score_history))
    work = {sid: [f if isinstance(f, bytes) else _jpeg(f) for f in frames] for sid, frames in _session_frames(6, 3).items()}
    got = {sid: [] for sid in work}

    def client(sid):
        with srv.app.test_client() as c:
            for p in work[sid]:
                r = c.post(f"/analyze?session={sid}", data={"frame": (io.BytesIO(p), "f.jpg")}, content_type="multipart/form-data")
                assert r.status_code == 200, r.get_data()
                b = r.get_json()
                b.pop("processing_time_ms")
                got[sid].append(b)
                time.sleep(0.11)                     # the session's own 100 ms limiter

    th = [threading.Thread(target=client, args=(sid,)) for sid in work]
    for t in th:
        t.start()
    for t in th:
        t.join()
    D = pkg.deepfake_detection.DeepfakeDetector
    for sid, payloads in work.items():
        det = D(detection_threshold=0.55, handle=b0_handle)
        assert got[sid] == [det.analyze_request(jpeg=p) for p in payloads], sid
        det.release()
    assert (srv.detector.frame_count, len(srv.detector.temporal_tracker.score_history)) == g0
    with srv.app.test_client() as c:
        assert c.get(f"/stats?session=s0").get_json()["frame_count"] == 3
    for sid in work:
        srv._session_pool.close(sid)


def test_one_pass_over_16_sessions_costs_less_than_four_single_requests(pkg, b0_handle):
    """estimated bound (from the 8-frame batch test), printed with the measured ratio"""
    D = pkg.deepfake_detection.DeepfakeDetector
    payloads = [_jpeg(_frame(405, 720, 300 + i)) for i in range(16)]
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=b0_handle, lock=lock)

    def one_pass():
        with lock:
            futs = [pool.submit(f"c{i}", [p]) for i, p in enumerate(payloads)]
            t = time.perf_counter()
        for fu in futs:
            fu.result(timeout=120)
        return time.perf_counter() - t

    det = D(detection_threshold=0.55, handle=b0_handle)

    def singles():
        ts = []
        for p in payloads:
            t = time.perf_counter()
            det.analyze_request(jpeg=p)
            ts.append(time.perf_counter() - t)
        return ts

    one_pass(), singles()                            # warm-up: buffers, GEMM tiles of both batch sizes
    ts = singles()
    tp = min(one_pass() for _ in range(3))
    single = sorted(ts)[len(ts) // 2]
    print(f"one pass over 16 sessions: {tp * 1e3:.2f} ms; one single request: {single * 1e3:.2f} ms; ratio {tp / single:.2f}")
    assert tp < 4 * single, (tp, single)
    det.release()
    for i in range(16):
        pool.close(f"c{i}")


def _truncated(frame_bgr):
    """a JPEG whose headers parse but whose scan is cut off: refused while decoding, not while parsing"""
    data = _jpeg(frame_bgr)
    return data[: int(len(data) * 0.6)]


def test_scan_that_fails_while_decoding_is_reported_with_its_index(b0_handle):
    h = b0_handle
    frames = [_frame(405, 720, 80 + i) for i in range(4)]
    cut = _truncated(frames[2])
    items = [_jpeg(frames[0]), _jpeg(frames[1]), cut, _jpeg(frames[3])]            # one run of four 720x405 JPEGs
    h.analyze_streams_batch(items[:2], [7601, 7602], [True, True])
    before = [h.forensics_state(s) for s in (7601, 7602, 7603)]
    with pytest.raises(Exception) as e:
        h.analyze_streams_batch(items, [7601, 7602, 7603, 7601], [False] * 4)
    assert e.value.code == -1 and e.value.bad_index == 2
    assert [h.forensics_state(s) for s in (7601, 7602, 7603)] == before
    for s in (7601, 7602, 7603):
        h.forensics_release(s)


def test_truncated_jpeg_of_one_session_leaves_the_others_alone(pkg, b0_handle, monkeypatch):
    D = pkg.deepfake_detection.DeepfakeDetector
    work = {sid: [f if isinstance(f, bytes) else _jpeg(f) for f in frames] for sid, frames in _session_frames(4, 2).items()}
    cut = _truncated(_frame(405, 720, 91))
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=b0_handle, lock=lock)
    got = {sid: [] for sid in work}
    for t in range(2):
        with lock:                                   # one pass: the cut-off JPEG of s1 among everyone's frames
            futs = {sid: pool.submit(sid, [frames[t]]) for sid, frames in work.items()}
            bad = pool.submit("s1", [cut])
        for sid, fu in futs.items():
            got[sid] += fu.result(timeout=120)
        with pytest.raises(pkg.sessions.InvalidFrame):
            bad.result(timeout=120)
    for sid, frames in work.items():
        det = D(detection_threshold=0.55, handle=b0_handle)
        assert got[sid] == [det.analyze_request(jpeg=f) for f in frames], sid
        det.release()
    for sid in work:
        pool.close(sid)
    # the sender gets what it gets without a session
    srv = pkg.backend_server
    pkg.runtime.set_default_handle(b0_handle)
    srv.app.config["TESTING"] = True
    monkeypatch.setattr(srv, "_session_pool", pkg.sessions.SessionPool(handle=b0_handle, lock=srv._detector_lock))
    monkeypatch.setattr(srv, "_session_last", {})
    with srv.app.test_client() as c:
        srv._last_request_time = 0.0
        plain = c.post("/analyze", data={"frame": (io.BytesIO(cut), "f.jpg")}, content_type="multipart/form-data")
        sess = c.post("/analyze?session=sender", data={"frame": (io.BytesIO(cut), "f.jpg")}, content_type="multipart/form-data")
        assert (sess.status_code, sess.get_json()) == (plain.status_code, plain.get_json())
        assert plain.status_code == 400
        c.post("/reset")


def test_jpeg_damaged_inside_a_block_of_one_session_leaves_the_others_alone(pkg, b0_handle):
    """as above with the device entropy decoder on and a frame whose LAST chunk holds a block with a coefficient index
    past 63 (tests/jpeg_damage_cases.py): every block behind it stays aligned and the block total matches, so only the
    decoders' own checks can tell.  The library refuses the part (-1) like the cut-off file; unlike that one libjpeg
    decodes it (a warning), so - the rule of InvalidFrame: neither the device path nor Pillow - its session is answered
    from Pillow's pixels, as the sender is without a session, never from coefficients the device decoder made up; the
    other sessions get their answers"""
    import jpeg_damage_cases as DC

    D = pkg.deepfake_detection.DeepfakeDetector
    work = {sid: [f if isinstance(f, bytes) else _jpeg(f) for f in frames] for sid, frames in _session_frames(4, 2).items()}
    damaged, _ = DC.damaged_frame(_frame(405, 720, 91), 85, "index", "lastchunk", 256)
    with pytest.raises(pkg._lib.DfdError) as e:
        pkg._lib.jpeg_coefficients(damaged)
    assert e.value.code == -1
    decoded = DC.pillow(damaged)
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=b0_handle, lock=lock)
    got = {sid: [] for sid in list(work) + ["damaged"]}
    b0_handle.set_option("jpeg_device_entropy", 1)
    b0_handle.set_option("jpeg_chunk_bytes", 256)
    try:
        with pytest.raises(pkg._lib.DfdError) as e:                  # the library itself: refused, with the part's index
            b0_handle.analyze_streams_batch([work["s0"][0], damaged], [7701, 7702], [False, False])
        assert e.value.code == -1 and e.value.bad_index == 1
        for s in (7701, 7702):
            b0_handle.forensics_release(s)
        for t in range(2):
            with lock:                                               # one pass: the damaged JPEG among everyone's frames
                futs = {sid: pool.submit(sid, [frames[t]]) for sid, frames in work.items()}
                futs["damaged"] = pool.submit("damaged", [damaged])
            for sid, fu in futs.items():
                got[sid] += fu.result(timeout=120)
        for sid, frames in work.items():
            det = D(detection_threshold=0.55, handle=b0_handle)
            assert got[sid] == [det.analyze_request(jpeg=f) for f in frames], sid
            det.release()
        det = D(detection_threshold=0.55, handle=b0_handle)
        assert got["damaged"] == [det.analyze_request(decoded.copy()) for _ in range(2)]
        det.release()
    finally:
        b0_handle.set_option("jpeg_device_entropy", 2)
        b0_handle.set_option("jpeg_chunk_bytes", 512)
        for sid in got:
            pool.close(sid)

"""GPU: sized forensic streams (dfd_forensics_open) through the fused and batched device passes - dfd_analyze_frame,
dfd_analyze_jpeg, dfd_analyze_stream_batch, dfd_analyze_streams_batch with streams of different analysis sizes in one call,
DeepfakeDetector(forensic_size=S) and the session pool under DFD_FORENSIC_SIZE.

Every fused result is compared bit for bit with the separate entries (dfd_forensics_sized, dfd_detect_faces,
dfd_classify_crops) or with each stream run alone in order; scores also against oracle.forensics_ref.ForensicsRef((S, S))
within the 1e-6 of tests/test_forensic_sized_gpu.py (the fixtures sit away from every threshold:
tests/test_forensic_sized_fused_fixtures.py)."""
import threading

import numpy as np
import pytest

import forensic_fused_frames as X
import frames as F
from oracle.forensics_ref import ForensicsRef

pytestmark = pytest.mark.gpu

STATE_ERR, ARG_ERR = -5, -1              # DFD_ERR_STATE, DFD_ERR_ARG
MAX_FACES = 4                            # the shared handle classifies 16 crops a pass


def _fresh(h, sid):
    h.forensics_release(sid)
    return sid


_jpeg = X.jpeg


def _bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _single(h, item, sid, full):
    """the one-frame fused entries -> (scores, prob, boxes, logits, n_detected, (H, W))"""
    if isinstance(item, bytes):
        scores, prob, boxes, logits, shape = h.analyze_jpeg(item, full, stream_id=sid, max_faces=MAX_FACES)
    else:
        scores, prob, boxes, logits = h.analyze_frame(item, full, stream_id=sid, max_faces=MAX_FACES)
        shape = tuple(item.shape[:2])
    small = shape[0] < 30 or shape[1] < 30
    return scores, prob, boxes, logits, 0 if small or not boxes else h.last_detection_count(), shape


def _same(a, b, what=None):
    """scores (NaN positions are absent keys), probability, boxes, detection count equal; logits bit-equal"""
    assert a[0] == b[0] and a[1] == b[1], (what, a[:2], b[:2])
    assert a[2] == b[2] and a[4] == b[4], (what, a[2], b[2], a[4], b[4])
    assert _bits(a[3], b[3]), (what, a[3], b[3])


def _parts(h, frame):
    """detection and classification as separate calls -> (boxes, logits)"""
    if frame.shape[0] < 30 or frame.shape[1] < 30:
        return [], np.zeros(0, np.float32)
    boxes = h.detect_faces(frame, confidence_threshold=0.5)[:MAX_FACES]
    logits = h.classify_crops(frame, boxes, apply_clahe=True)[:, 0] if boxes else np.zeros(0, np.float32)
    return boxes, logits


def _against_oracle(scores, prob, res):
    assert set(scores) == set(res["scores"])
    for k, want in res["scores"].items():
        assert abs(scores[k] - want) <= 1e-6, (k, scores[k], want)
    assert abs(prob - res["fake_probability"]) <= 1e-6


# ------------------------------------------------------------------------------------------------ 1: open semantics
def test_open_semantics(pkg, b0_handle):
    h, E = b0_handle, pkg._lib.DfdError
    seq = X.moving()
    sid, twin = _fresh(h, 8001), _fresh(h, 8002)
    h.forensics_open(sid, 80)
    assert h.forensics_state(sid) == (0, 0, False)
    got = h.analyze_frame(seq[0], True, stream_id=sid, max_faces=MAX_FACES)
    want = h.forensics_sized(seq[0], 80, True, twin)
    assert got[0] == want[0] and got[1] == want[1]                 # the first fused frame ran at 80
    state = h.forensics_state(sid)
    assert state == (1, 0, True)
    h.forensics_open(sid, 80)                                      # the same size: a no-op
    assert h.forensics_state(sid) == state
    for other in (96, 256):
        with pytest.raises(E) as e:
            h.forensics_open(sid, other)
        assert e.value.code == STATE_ERR and h.forensics_state(sid) == state
    got = h.analyze_frame(seq[1], False, stream_id=sid, max_faces=MAX_FACES)      # ... and the stream still runs at 80
    want = h.forensics_sized(seq[1], 80, False, twin)
    assert got[0] == want[0] and got[1] == want[1] and h.forensics_state(sid) == h.forensics_state(twin)
    for bad in (100, 16, 1040, 0, -32):
        with pytest.raises(E) as e:
            h.forensics_open(_fresh(h, 8003), bad)
        assert e.value.code == ARG_ERR and h.forensics_state(8003) == (0, 0, False)
    h.forensics_release(sid)                                       # after release: any size
    h.forensics_open(sid, 96)
    with pytest.raises(E) as e:
        h.forensics_open(sid, 80)
    assert e.value.code == STATE_ERR
    h.forensics_release(sid)
    h.forensics_open(sid, 272)
    # a stream nobody opened is a 256 x 256 stream on the specialised kernels, as before
    a, b = _fresh(h, 8004), _fresh(h, 8005)
    for f, full in zip(seq, X.PATTERN):
        got = h.analyze_frame(f, full, stream_id=a, max_faces=MAX_FACES)
        want = h.forensics(f, full, b)
        assert got[0] == want[0] and got[1] == want[1]
        assert h.forensics_state(a) == h.forensics_state(b)
    with pytest.raises(E) as e:                                    # it holds 256 now
        h.forensics_open(a, 80)
    assert e.value.code == STATE_ERR
    h.forensics_open(a, 256)                                       # the same size: a no-op, the stream stays where it is
    got = h.analyze_frame(seq[0], True, stream_id=a, max_faces=MAX_FACES)
    want = h.forensics(seq[0], True, b)
    assert got[0] == want[0] and got[1] == want[1]
    for s in (sid, twin, 8003, a, b):
        h.forensics_release(s)


# ------------------------------------------------------------------------------------------------ 2: fused single frame
@pytest.mark.parametrize("S", X.SIZES)
def test_fused_single_frame(b0_handle, S):
    h = b0_handle
    a, b = _fresh(h, 8010), _fresh(h, 8011)
    h.forensics_open(a, S)
    ref = ForensicsRef((S, S))
    for f, full in zip(X.moving(), X.PATTERN):
        scores, prob, boxes, logits = h.analyze_frame(f, full, stream_id=a, max_faces=MAX_FACES)
        ws, wp, _ = h.forensics_sized(f, S, full, b)
        assert scores == ws and prob == wp, (S, scores, ws)
        assert h.forensics_state(a) == h.forensics_state(b)
        wb, wl = _parts(h, f)
        assert boxes == wb and _bits(logits, wl)
        _against_oracle(scores, prob, ref.analyze(f) if full else ref.analyze_fast(f))
        if S < 64:
            assert (scores["noise"], scores["ela"]) == (0.0, 0.0) if full else "noise" not in scores
    face = F.face_frame(seed=1)                                    # a frame the detector fires on
    scores, prob, boxes, logits = h.analyze_frame(face, True, stream_id=a, max_faces=MAX_FACES)
    ws, wp, _ = h.forensics_sized(face, S, True, b)
    wb, wl = _parts(h, face)
    assert scores == ws and prob == wp and boxes == wb and _bits(logits, wl)
    print(f"S={S}: {len(boxes)} boxes on the face frame")
    h.forensics_release(a)
    h.forensics_release(b)


# ------------------------------------------------------------------------------------------------ 3: fused JPEG
def test_fused_jpeg(b0_handle):
    h, S = b0_handle, 80
    a, b = _fresh(h, 8020), _fresh(h, 8021)
    h.forensics_open(a, S)
    ref = ForensicsRef((S, S))
    for f, full in zip(X.moving(), X.PATTERN):
        data = _jpeg(f)
        scores, prob, boxes, logits, shape = h.analyze_jpeg(data, full, stream_id=a, max_faces=MAX_FACES)
        dec = h.decode_jpeg(data)
        assert shape == dec.shape[:2] == f.shape[:2]
        ws, wp, _ = h.forensics_sized(dec, S, full, b)
        assert scores == ws and prob == wp
        assert h.forensics_state(a) == h.forensics_state(b)
        wb, wl = _parts(h, dec)
        assert boxes == wb and _bits(logits, wl)
        _against_oracle(scores, prob, ref.analyze(dec) if full else ref.analyze_fast(dec))
    h.forensics_release(a)
    h.forensics_release(b)


# ------------------------------------------------------------------------------------------------ 4: one stream, one batch
def test_stream_batch_equals_single_fused_calls(b0_handle):
    h, S = b0_handle, 80
    a, b = _fresh(h, 8030), _fresh(h, 8031)
    h.forensics_open(a, S)
    h.forensics_open(b, S)
    seq = X.moving(6)
    full = [True, False, False, True, False]
    items = [_jpeg(f) if i % 2 else f for i, f in enumerate(seq[:5])]
    got, shape = h.analyze_stream_batch(items, full, stream_id=a, max_faces=MAX_FACES)
    assert shape == seq[0].shape[:2]
    for i in range(5):
        _same(got[i], _single(h, items[i], b, full[i]), i)
    assert h.forensics_state(a) == h.forensics_state(b) == (5, 4, True)
    _same(_single(h, seq[5], a, True), _single(h, seq[5], b, True), "next")      # the plane was written back
    h.forensics_release(a)
    h.forensics_release(b)


# ------------------------------------------------------------------------------------------------ 5: mixed sizes, one pass
STREAM_SIZE = {0: None, 1: None, 2: 32, 3: 80, 4: 272}           # None: never opened (256 x 256, specialised kernels)
ORDER = [0, 3, 1, 2, 4, 3, 0, 1, 2, 3, 4, 0]                     # stream 3 three times: an in-call predecessor


def _mixed_pass(seed):
    """12 frames interleaved from the 5 streams, all three source sizes, JPEG and raw parts"""
    seen, items = {}, []
    for k, s in enumerate(ORDER):
        t = seen.get(s, 0)
        seen[s] = t + 1
        fr = X.stream_frames(s, 1, start=3 * seed + t)[0]
        items.append(_jpeg(fr) if (k + s) % 2 else fr)
    return items, [(seed + k) % 3 == 0 for k in range(len(ORDER))]


def _open_all(h, base):
    for s, size in STREAM_SIZE.items():
        _fresh(h, base + s)
        if size:
            h.forensics_open(base + s, size)


def _chain_kinds_in_one_pass(pkg, seeded_sd, h):
    """the three kinds of chain in ONE batched call - a 256 stream nobody opened (256x256 kernels), an opened 256 stream
    (general chain at 256) and a 48 stream (one block: fewer than 4) - with one frame a chunk, so the opened stream's
    three frames take three chunks of its group; every frame against the single entries on a fresh handle"""
    sizes, order, base = {0: None, 1: 256, 2: 48}, [0, 1, 2, 1, 0, 2, 1], 8700
    fresh = pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, pkg.weights.seeded_ssd_state_dict(0)), device=0, max_batch=16)
    try:
        for s, size in sizes.items():
            _fresh(h, base + s)
            if size:
                h.forensics_open(base + s, size)
        seen, items = {}, []
        for s in order:
            seen[s] = seen.get(s, 0) + 1
            items.append(X.stream_frames(s, 1, start=seen[s] - 1)[0])
        full = [k % 2 == 0 for k in range(len(order))]
        h.set_option("forensic_chunk_bytes", 1)
        try:
            got = h.analyze_streams_batch(items, [base + s for s in order], full, max_faces=MAX_FACES)
        finally:
            h.set_option("forensic_chunk_bytes", 0)                # the default
        for k, s in enumerate(order):
            if sizes[s]:
                scores, prob, _ = fresh.forensics_sized(items[k], sizes[s], full[k], base + s)
            else:
                scores, prob, _ = fresh.forensics(items[k], full[k], base + s)
            assert got[k][0] == scores and got[k][1] == prob, (k, s, got[k][:2], scores, prob)
            if sizes[s] == 48 and full[k]:
                assert (scores["noise"], scores["ela"]) == (0.0, 0.0)
        for s in sizes:
            assert h.forensics_state(base + s) == fresh.forensics_state(base + s) == (seen[s], seen[s] - 1, True), s
    finally:
        fresh.close()
        for s in sizes:
            h.forensics_release(base + s)


def test_streams_of_mixed_sizes_in_one_pass(pkg, seeded_sd, b0_handle):
    h = b0_handle
    new, ref = 8100, 8200
    _open_all(h, new)
    _open_all(h, ref)
    warm = X.moving(1, 90, 144)[0]                                 # the 272 stream holds a stored plane from an earlier call
    _same(_single(h, warm, new + 4, True), _single(h, warm, ref + 4, True), "warm")
    shapes = set()
    for rnd in range(2):                                           # the second pass continues every stream
        items, full = _mixed_pass(rnd)
        got = h.analyze_streams_batch(items, [new + s for s in ORDER], full, max_faces=MAX_FACES)
        for k, s in enumerate(ORDER):
            want = _single(h, items[k], ref + s, full[k])
            _same(got[k], want, (rnd, k, s))
            assert got[k][5] == want[5]
            shapes.add(got[k][5])
            if got[k][5] == (24, 40):
                assert got[k][2] == [] and got[k][4] == 0          # forensics, no detection
        for s in STREAM_SIZE:
            assert h.forensics_state(new + s) == h.forensics_state(ref + s), (rnd, s)
    assert shapes == set(X.SOURCES)
    assert h.forensics_state(new + 3) == (6, 5, True) and h.forensics_state(new + 4) == (5, 4, True)
    for s in STREAM_SIZE:
        h.forensics_release(new + s)
        h.forensics_release(ref + s)
    _chain_kinds_in_one_pass(pkg, seeded_sd, h)


# ------------------------------------------------------------------------------------------------ 6: chunking
@pytest.mark.parametrize("budget", (1, 3_000_000))               # one / two 272 x 272 frames (1.4 MB of work memory each) a chunk
def test_chunking_changes_nothing(b0_handle, budget):
    h, S = b0_handle, 272
    ids = {"a": (8300, 8310), "b": (8301, 8311)}
    for pair in ids.values():
        for sid in pair:
            h.forensics_open(_fresh(h, sid), S)
    frames = X.stream_frames(0, 4) + X.stream_frames(1, 2)
    order = ["a", "b", "a", "a", "b", "a"]                         # every frame of `a` after the first has its predecessor
    it = {"a": iter(frames[:4]), "b": iter(frames[4:])}            # one or two chunks back
    items = [next(it[s]) for s in order]
    full = [True, False, False, True, True, False]
    want = h.analyze_streams_batch(items, [ids[s][1] for s in order], full, max_faces=MAX_FACES)
    h.set_option("forensic_chunk_bytes", budget)
    try:
        got = h.analyze_streams_batch(items, [ids[s][0] for s in order], full, max_faces=MAX_FACES)
    finally:
        h.set_option("forensic_chunk_bytes", 0)                    # the default
    for k in range(len(order)):
        _same(got[k], want[k], k)
    nxt = X.stream_frames(2, 1)[0]
    for pair in ids.values():
        assert h.forensics_state(pair[0]) == h.forensics_state(pair[1])
        _same(_single(h, nxt, pair[0], True), _single(h, nxt, pair[1], True), "next")
        for sid in pair:
            h.forensics_release(sid)


# ------------------------------------------------------------------------------------------------ 7: atomicity
def test_refused_part_moves_no_sized_stream(pkg, b0_handle):
    h = b0_handle
    new, ref = 8400, 8500
    _open_all(h, new)
    _open_all(h, ref)
    items, full = _mixed_pass(0)
    ids = [new + s for s in ORDER]
    h.analyze_streams_batch(items[:6], ids[:6], full[:6], max_faces=MAX_FACES)
    for k in range(6):
        _single(h, items[k], ref + ORDER[k], full[k])
    before = [h.forensics_state(new + s) for s in STREAM_SIZE]
    bad = items[6:]
    bad[-1] = _jpeg(X.stream_frames(0, 1, start=5)[0], progressive=True)
    with pytest.raises(pkg._lib.DfdError) as e:
        h.analyze_streams_batch(bad, ids[6:], full[6:], max_faces=MAX_FACES)
    assert e.value.code == h.UNSUPPORTED and e.value.bad_index == len(bad) - 1
    assert [h.forensics_state(new + s) for s in STREAM_SIZE] == before
    nxt = X.moving(2, 90, 144)[1]
    for s in STREAM_SIZE:                                          # the next frame of every listed stream: as if nothing had been tried
        _same(_single(h, nxt, new + s, True), _single(h, nxt, ref + s, True), s)
        h.forensics_release(new + s)
        h.forensics_release(ref + s)


# ------------------------------------------------------------------------------------------------ 8: class and pool surface
def test_detector_at_a_forensic_size(pkg, b0_handle):
    h = b0_handle
    D, A = pkg.deepfake_detection.DeepfakeDetector, pkg.frame_analysis.FrameForensicAnalyzer
    frames = [F.face_frame(seed=s) for s in (1, 2, 3)]
    det = D(forensic_size=80, use_tta=False, handle=h)
    assert det.frame_analyzer.analysis_size == (80, 80) and det.frame_analyzer.any_size
    swapped = D(use_tta=False, handle=h)
    swapped.frame_analyzer = A((80, 80), any_size=True, handle=h)
    plain = D(use_tta=False, handle=h)
    twin = _fresh(h, 8600)
    for i, f in enumerate(frames):                                 # predict
        r, rs_, rp = det.predict(f)[3], swapped.predict(f)[3], plain.predict(f)[3]
        full = (i + 1) % det.full_forensic_interval == 0
        scores, prob, stats = h.forensics_sized(f, 80, full, twin)
        assert r["frame_forensic"] == {"scores": scores, "fake_probability": prob, "frame_number": int(stats["frame_count"]),
                                       "analysis_type": "frame_forensic" if full else "frame_forensic_fast"}
        boxes = h.detect_faces(f, confidence_threshold=0.5)
        assert r["faces_detected"] == len(boxes) == rp["faces_detected"] and r["face_results"] == rp["face_results"]
        logits = [v for i in range(0, len(boxes), h.max_batch)      # the handle classifies max_batch crops a call
                  for v in h.classify_crops(f, boxes[i:i + h.max_batch], apply_clahe=True)[:, 0]]
        want = [{"face_prob": float(p), "combined_prob": float(p), "bbox": {"x": x, "y": y, "w": w, "h": hh}}
                for (x, y, w, hh), p in ((b, det._finish_face(lg, b[3], b[2])) for b, lg in zip(boxes, logits)) if p is not None]
        assert r["face_results"] == want
        assert r == rs_
    for d in (det, swapped, plain):
        d.release()
    h.forensics_release(twin)
    # the /analyze flow, frame by frame and as one batch
    det, swapped, batch = D(forensic_size=80, use_tta=False, handle=h), D(use_tta=False, handle=h), D(forensic_size=80, use_tta=False, handle=h)
    swapped.frame_analyzer = A((80, 80), any_size=True, handle=h)
    singles = []
    for i, f in enumerate(frames):
        r = det.analyze_request(jpeg=_jpeg(f)) if i == 1 else det.analyze_request(f)
        rs_ = swapped.analyze_request(jpeg=_jpeg(f)) if i == 1 else swapped.analyze_request(f)
        src = h.decode_jpeg(_jpeg(f)) if i == 1 else f
        full = i % det.full_forensic_interval == 0                 # forensics before the frame counter moves
        scores, prob, _ = h.forensics_sized(src, 80, full, twin)
        assert r["frame_forensic_probability"] == prob and det.last_frame_forensic_result["scores"] == scores
        boxes = h.detect_faces(src, confidence_threshold=0.5)
        assert r["faces_detected"] == len(boxes)
        if boxes and r["analysis_mode"] == "face+frame":
            x, y, w, hh = boxes[0]
            assert r["face_bbox"] == {"x": x, "y": y, "width": w, "height": hh}
            assert r["face_probability"] == float(det._finish_face(h.classify_crops(src, boxes[:1], apply_clahe=True)[0, 0], hh, w))
        assert r == rs_
        singles.append(r)
    assert batch.analyze_request_batch([_jpeg(f) if i == 1 else f for i, f in enumerate(frames)]) == singles
    assert batch.frame_analyzer.frame_count == det.frame_analyzer.frame_count == 3
    for d in (det, swapped, batch):
        d.release()
    h.forensics_release(twin)


def test_pool_under_the_forensic_size_variable(pkg, b0_handle, monkeypatch):
    D = pkg.deepfake_detection.DeepfakeDetector
    monkeypatch.setenv("DFD_FORENSIC_SIZE", "80")
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=b0_handle, lock=lock)
    monkeypatch.delenv("DFD_FORENSIC_SIZE")
    assert pool.forensic_size == 80
    work = {"p0": [_jpeg(F.face_frame(seed=4)), X.moving()[1]], "p1": [X.stream_frames(1, 1)[0], _jpeg(F.face_frame(seed=5))]}
    got = {sid: [] for sid in work}
    for t in range(2):
        passes = pool.passes
        with lock:                                                 # both queue while the handle is "busy": one library call
            futs = {sid: pool.submit(sid, [fr[t]]) for sid, fr in work.items()}
        for sid, fu in futs.items():
            got[sid] += fu.result(timeout=120)
        assert pool.passes == passes + 1
    for sid, fr in work.items():
        det = D(detection_threshold=0.55, handle=b0_handle, forensic_size=80)
        want = [det.analyze_request(jpeg=f) if isinstance(f, bytes) else det.analyze_request(f) for f in fr]
        assert got[sid] == want, sid
        det.release()
        pool.close(sid)


def test_sized_sessions_join_while_passes_run(pkg, b0_handle):
    """the worker is never parked: 8 clients start one after the other, each creating its sized session from its own
    thread while earlier sessions' passes are on the handle - building a session makes no library call, its stream is
    opened inside the pass, under the pool's lock"""
    D = pkg.deepfake_detection.DeepfakeDetector
    pool = pkg.sessions.SessionPool(handle=b0_handle, forensic_size=80)
    work = {f"j{i}": X.stream_frames(i, 4) for i in range(8)}
    got, errors = {sid: [] for sid in work}, []

    def client(sid):
        try:
            for f in work[sid]:
                got[sid] += pool.submit(sid, [f]).result(timeout=120)
        except BaseException as e:      # noqa: BLE001  (reported below)
            errors.append((sid, e))

    th = [threading.Thread(target=client, args=(sid,)) for sid in work]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for sid, fr in work.items():
        det = D(detection_threshold=0.55, handle=b0_handle, forensic_size=80)
        assert got[sid] == [det.analyze_request(f) for f in fr], sid
        det.release()
        pool.close(sid)

"""GPU: test-time augmentation inside the batched device pass.

The references are the ones the per-face path is pinned to: oracle/tta_ref.py for the augmented pixels, and the existing
per-face library calls (preprocess_face_quality -> tta_augment -> classify_crops, DeepfakeDetector.analyze_face) for the
logits and probabilities.  Everything is compared bit for bit: the batched path runs the same arithmetic on the same
pixels, only in one pass."""
import io
import random
import threading

import numpy as np
import pytest
from PIL import Image

import frames as F
from oracle import tta_ref
from test_pipeline_gpu import _mt_stream, _stream

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5

# flip on and off; alpha 0.9, 1.1 and 1.0; angle -3.0 and 2.4; angle exactly 0.0 with flip
DRAWS = [(True, 1.1, 2.4), (False, 0.9, -3.0), (True, 1.0, 0.0), (False, 1.07, 1.3), (True, 0.9, -3.0), (False, 1.0, 2.4),
         (False, 1.1, -0.7), (True, 0.93, 2.4), (True, 1.1, 0.0), (False, 0.9, 2.4), (True, 1.0, -3.0), (False, 1.1, 3.0)]


def _draws(n):
    return [DRAWS[i % len(DRAWS)] for i in range(n)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_logits(a, b):
    """bit-equal float32 arrays, NaN positions included"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def _jpeg(frame_bgr):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format="JPEG", quality=85)
    return buf.getvalue()


def _per_face(h, frame, boxes, copies, draws):
    """the per-face path: CLAHE, then per copy an augment and a batch-1 classification -> (n, 1 + copies)"""
    out = np.empty((len(boxes), 1 + copies), np.float32)
    out[:, 0] = h.classify_crops(frame, boxes)[:, 0]
    for i, (x, y, w, hh) in enumerate(boxes):
        pre = h.preprocess_face_quality(np.ascontiguousarray(frame[y:y + hh, x:x + w]))
        for j in range(copies):
            aug = h.tta_augment(pre, *draws[i * copies + j])
            out[i, 1 + j] = h.classify_crops(aug, [(0, 0, w, hh)], apply_clahe=False)[0, 0]
    return out


# ------------------------------------------------------------------------------------------------ 1. the kernel
def test_batched_augment_is_bit_identical_to_the_oracle(b0_handle):
    frame = F.natural_like(480, 640, seed=11)
    frame[100:120, 100:130] = 255                                   # saturating pixels for convertScaleAbs
    frame[450:460, 610:620] = 255
    frame[10, 10] = 255
    boxes = [(10, 10, 1, 1),                                        # smallest case
             (50, 60, 37, 2),                                       # odd width, centre at a half pixel
             (600, 440, 40, 40),                                    # the frame's bottom-right corner: stride != 3w
             (100, 100, 133, 81),                                   # ordinary ragged case
             (300, 100, 260, 300),                                  # wider than one 256 strip
             (20, 200, 3, 257)]                                     # taller than one block
    copies = 2
    draws = _draws(len(boxes) * copies)
    assert {d[0] for d in draws} == {True, False} and {0.9, 1.0, 1.1} <= {d[1] for d in draws}
    assert {-3.0, 2.4} <= {d[2] for d in draws} and any(d[0] and d[2] == 0.0 for d in draws)
    got = b0_handle.tta_augment_crops(frame, boxes, copies, draws)
    changed = 0
    for i, (x, y, w, hh) in enumerate(boxes):
        crop = np.ascontiguousarray(frame[y:y + hh, x:x + w])
        for j in range(copies):
            want = tta_ref.augment(crop, *draws[i * copies + j])
            assert got[i][j].shape == want.shape
            assert np.array_equal(got[i][j], want), (boxes[i], draws[i * copies + j])
            changed += not np.array_equal(got[i][j], crop)
    assert changed > 0


# ------------------------------------------------------------------------------------------------ 2. the library path
def test_classify_crops_tta_equals_the_per_face_path(b0_handle):
    h = b0_handle
    frame = F.natural_like(480, 640, seed=12)
    frame[200:230, 200:260] = 255
    boxes = [(5, 7, 31, 45), (180, 150, 133, 81), (300, 100, 260, 300), (599, 379, 41, 101), (60, 300, 224, 97)]
    copies = 2
    draws = _draws(len(boxes) * copies)
    got = h.classify_crops_tta(frame, boxes, copies, draws)
    want = _per_face(h, frame, boxes, copies, draws)
    _same_logits(got, want)
    assert not np.isnan(got).any()
    assert (got[:, 1:] != got[:, :1]).any(), "the copies did not change a logit"
    # without CLAHE: column 0 and the copies come straight from the frame
    raw = h.classify_crops_tta(frame, boxes[:2], copies, draws[:4], apply_clahe=False)
    assert np.array_equal(_bits(raw[:, 0]), _bits(h.classify_crops(frame, boxes[:2], apply_clahe=False)[:, 0]))
    for i, (x, y, w, hh) in enumerate(boxes[:2]):
        for j in range(copies):
            aug = h.tta_augment(np.ascontiguousarray(frame[y:y + hh, x:x + w]), *draws[i * copies + j])
            assert _bits(raw[i, 1 + j]) == _bits(h.classify_crops(aug, [(0, 0, w, hh)], apply_clahe=False)[0, 0])


def test_classify_crops_tta_with_the_mtcnn_stage(mt_handle):
    """every image of the call goes through the cascade together; a rejected copy is NaN exactly where the per-face path
    returns NaN, and is never classified"""
    h = mt_handle
    copies = 2
    kept = rejected = 0
    for frame in _mt_stream(2, seed=3):                             # a textured frame and a face frame
        boxes = h.detect_faces(frame)[:10]
        assert boxes
        draws = _draws(len(boxes) * copies)
        before = h.classifier_crop_count()
        got = h.classify_crops_tta(frame, boxes, copies, draws)
        assert h.classifier_crop_count() - before == int((~np.isnan(got)).sum())
        _same_logits(got, _per_face(h, frame, boxes, copies, draws))
        kept += int((~np.isnan(got[:, 1:])).sum())
        rejected += int(np.isnan(got[:, 1:]).sum())
    assert kept > 0 and rejected > 0, (kept, rejected)              # both outcomes occur among the copies


# ------------------------------------------------------------------------------------------------ 3. chunking
def test_copies_straddle_classifier_chunks(pkg, b0_handle, seeded_sd):
    frame = F.natural_like(480, 640, seed=13)
    boxes = [(40, 30, 200, 240), (300, 100, 224, 224), (10, 300, 97, 133)]
    draws = _draws(6)
    want = b0_handle.classify_crops_tta(frame, boxes, 2, draws)
    small = pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, pkg.weights.seeded_ssd_state_dict(0)), device=0, max_batch=4)
    try:
        before = small.classifier_crop_count()
        got = small.classify_crops_tta(frame, boxes, 2, draws)      # 9 images: chunks of 4, 4 and 1
        assert small.classifier_crop_count() - before == 9
    finally:
        small.close()
    _same_logits(got, want)


# ------------------------------------------------------------------------------------------------ 4. fused calls
def _expected_block(h, frame, boxes, copies, draws, first_face):
    if not boxes:
        return np.empty((0, 1 + copies), np.float32)
    return h.classify_crops_tta(frame, boxes, copies, draws[first_face * copies:(first_face + len(boxes)) * copies])


def test_armed_frame_and_jpeg_calls(b0_handle):
    h = b0_handle
    copies, max_faces = 2, 4
    frame = F.natural_like(480, 640, seed=101)
    draws = _draws(max_faces * copies)
    faces = 0
    for k, item in enumerate((frame, _jpeg(frame))):
        sid_a, sid_b = 7700 + 2 * k, 7701 + 2 * k
        if isinstance(item, bytes):
            plain = h.analyze_jpeg(item, True, stream_id=sid_a, max_faces=max_faces)
            armed = h.analyze_jpeg(item, True, stream_id=sid_b, max_faces=max_faces, tta=(copies, draws))
            assert armed[4] == plain[4]
            pixels = h.decode_jpeg(item)
        else:
            plain = h.analyze_frame(item, True, stream_id=sid_a, max_faces=max_faces)
            armed = h.analyze_frame(item, True, stream_id=sid_b, max_faces=max_faces, tta=(copies, draws))
            pixels = item
        assert armed[0] == plain[0] and armed[1] == plain[1] and armed[2] == plain[2]
        assert armed[3].shape == (len(plain[2]), 1 + copies)
        _same_logits(armed[3][:, 0], plain[3])
        _same_logits(armed[3], _expected_block(h, pixels, armed[2], copies, draws, 0))
        assert h.forensics_state(sid_a) == h.forensics_state(sid_b)
        faces += len(armed[2])
        h.forensics_release(sid_a)
        h.forensics_release(sid_b)
    assert faces >= 2, faces


def test_armed_streams_batch(b0_handle):
    h = b0_handle
    copies, max_faces = 2, 3
    items = [F.natural_like(480, 640, seed=102), F.blank_frame(640, 480), F.natural_like(405, 720, seed=101)]
    full = [True, False, True]
    draws = _draws(len(items) * max_faces * copies)
    plain = h.analyze_streams_batch(items, [7710, 7711, 7710], full, max_faces=max_faces)
    armed = h.analyze_streams_batch(items, [7712, 7713, 7712], full, max_faces=max_faces, tta=(copies, draws))
    first = 0
    for p, a, frame in zip(plain, armed, items):
        assert a[0] == p[0] and a[1] == p[1] and a[2] == p[2] and a[4] == p[4] and a[5] == p[5]
        _same_logits(a[3][:, 0], p[3])
        _same_logits(a[3], _expected_block(h, frame, a[2], copies, draws, first))     # rows: frame-major, then face order
        first += len(a[2])
    assert armed[1][2] == [] and armed[1][3].shape == (0, 1 + copies)                # the blank frame
    assert first >= 2, first
    assert h.forensics_state(7710) == h.forensics_state(7712) and h.forensics_state(7711) == h.forensics_state(7713)
    # the single-stream batch entry point takes the arming the same way
    one = h.analyze_stream_batch([items[0], items[1]], [True, False], stream_id=7714, max_faces=max_faces,
                                 tta=(copies, draws[:2 * max_faces * copies]))[0]
    ref = h.analyze_stream_batch([items[0], items[1]], [True, False], stream_id=7715, max_faces=max_faces)[0]
    assert one[0][2] == ref[0][2] and one[0][3].shape == (len(ref[0][2]), 1 + copies)
    _same_logits(one[0][3], _expected_block(h, items[0], one[0][2], copies, draws, 0))
    for s in range(7710, 7716):
        h.forensics_release(s)


def test_arming_rules(pkg, b0_handle):
    h = b0_handle
    frame = F.natural_like(480, 640, seed=101)
    plain = h.analyze_frame(frame, True, stream_id=7720, max_faces=4)
    assert len(plain[2]) >= 1
    state = h.forensics_state(7720)
    # too small a capacity: refused at entry, nothing moved - and the arming is gone
    h.tta_arm(2, _draws(2), 1)
    with pytest.raises(pkg._lib.DfdError) as e:
        h.analyze_frame(frame, False, stream_id=7720, max_faces=4)
    assert e.value.code == ERR_ARG
    assert h.forensics_state(7720) == state
    again = h.analyze_frame(frame, True, stream_id=7721, max_faces=4)                 # unarmed: max_faces 4 passes
    assert again[2] == plain[2] and h.tta_logits().shape[0] == 0
    _same_logits(again[3], plain[3])
    # a call that fails its own validation consumes the arming too
    h.tta_arm(2, _draws(2), 1)
    assert h._lib.dfd_analyze_frame(h._p, 7720, None, 480, 640, 1920, 1, 0.5, 1, 1, None, None, None, None, None) == ERR_ARG
    assert h.forensics_state(7720) == state
    h.analyze_frame(frame, False, stream_id=7722, max_faces=4)                        # would be refused if still armed
    assert h.tta_logits().shape[0] == 0
    # the benchmark's loops do not take copies: armed, they say so instead of ignoring it
    fd = h.alloc(frame.nbytes).upload(frame)
    try:
        h.tta_arm(2, _draws(8), 4)
        with pytest.raises(pkg._lib.DfdError) as e:
            h.analyze_batch_device(fd.ptr, 1, 480, 640, max_faces=4)
        assert e.value.code == ERR_STATE and "TTA not built for this entry" in str(e.value)
        boxes, logits, _ = h.analyze_batch_device(fd.ptr, 1, 480, 640, max_faces=4)   # unarmed again
        assert boxes[0] == plain[2]
    finally:
        fd.free()
    for bad in (0, -1):
        with pytest.raises(pkg._lib.DfdError) as e:
            h._check(h._lib.dfd_tta_arm(h._p, bad, pkg._lib.tta_draws(_draws(1), 1, 1), 1))
        assert e.value.code == ERR_ARG
    with pytest.raises(pkg._lib.DfdError) as e:
        h.classify_crops_tta(frame, [(0, 0, 40, 40)], 64, _draws(64))
    assert e.value.code == -6
    for s in (7720, 7721, 7722):
        h.forensics_release(s)


# ------------------------------------------------------------------------------------------------ 5. the detector
def test_predict_with_the_default_constructor_equals_the_per_face_loop(pkg, b0_handle):
    D = pkg.deepfake_detection.DeepfakeDetector
    h = b0_handle
    det, ref = D(handle=h), D(handle=h)                            # the reference's defaults: TTA on, K = 3
    assert det.use_tta and det.num_tta_augmentations == 3
    stream = _stream(4, seed=50)
    random.seed(2024)
    results, levels, votes = [], [], []
    for frame in stream:
        before = h.classifier_crop_count()
        got = det.predict(frame)[3]
        assert h.classifier_crop_count() - before == got['faces_detected'] * 3    # no second classification
        results.append(got)
        levels.append(det.temporal_tracker.get_confidence_level())
        votes.append(det.temporal_tracker.get_voting_stats())
    state = random.getstate()
    assert sum(r['faces_detected'] for r in results) >= 2
    random.seed(2024)
    for frame, got, level, vote in zip(stream, results, levels, votes):
        boxes = h.detect_faces(frame, 0.5)
        assert got['faces_detected'] == len(boxes)
        want = []
        for (x, y, w, hh) in boxes:
            p = ref.analyze_face(frame[y:y + hh, x:x + w])[0]       # today's per-face path
            if p is None:
                continue
            ref.temporal_tracker.update(p)
            want.append((float(p), {'x': x, 'y': y, 'w': w, 'h': hh}))
        if not boxes:
            ref.temporal_tracker.update(got['frame_forensic']['fake_probability'])
        assert [(r['face_prob'], r['bbox']) for r in got['face_results']] == want
        assert ref.temporal_tracker.get_voting_stats() == vote
        assert ref.temporal_tracker.get_confidence_level() == level
        if boxes or got['frame_count'] > 1:
            assert got['confidence_level'] == level
    assert random.getstate() == state
    det.release()


def test_analyze_request_honours_use_tta(pkg, b0_handle):
    D = pkg.deepfake_detection.DeepfakeDetector
    h = b0_handle
    det, ref = D(handle=h, request_tta=True), D(handle=h)          # TTA on, K = 3, and the /analyze flow opted in
    stream = _stream(4, seed=60)
    random.seed(77)
    got, counts = [], []
    for frame in stream:
        before = h.classifier_crop_count()
        got.append(det.analyze_request(frame))
        counts.append(h.classifier_crop_count() - before)
    state = random.getstate()
    random.seed(77)
    faces = 0
    for frame, g, c in zip(stream, got, counts):
        box = g.get('face_bbox')
        assert c == (3 if box else 0)
        if box:
            p = ref.analyze_face(frame[box['y']:box['y'] + box['height'], box['x']:box['x'] + box['width']])[0]
            assert g['fake_probability'] == float(p) and g['face_probability'] == float(p)
            faces += 1
    assert faces >= 2 and random.getstate() == state
    # without the opt-in a default-constructed detector answers /analyze as it always has: one classification
    for plain in (D(use_tta=False, handle=h), D(handle=h)):
        before = h.classifier_crop_count()
        assert plain.analyze_request(stream[0])['fake_probability'] != got[0]['fake_probability'], "the copies changed nothing"
        assert h.classifier_crop_count() - before == 1
        plain.release()
    det.release()


# ------------------------------------------------------------------------------------------------ 6. the session pool
def test_session_pool_pass_equals_lone_detectors(pkg, b0_handle):
    D = pkg.deepfake_detection.DeepfakeDetector
    work = {"a": [F.natural_like(480, 640, seed=101), _jpeg(F.natural_like(405, 720, seed=102))],
            "b": [_jpeg(F.natural_like(480, 640, seed=102)), F.blank_frame(640, 480)]}
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=b0_handle, lock=lock, use_tta=True, num_tta_augmentations=2)
    random.seed(31)
    with lock:                                                      # one pass: both submissions queue while the handle is held
        futs = {sid: pool.submit(sid, items) for sid, items in work.items()}
    got = {sid: fu.result(timeout=120) for sid, fu in futs.items()}
    assert pool.passes == 1 and pool.frames == 4
    state = random.getstate()
    # the pool's draw order: submissions in queue order, a submission's frames in stream order
    random.seed(31)
    for sid, items in work.items():
        lone = D(enable_gradcam=False, use_tta=True, num_tta_augmentations=2, detection_threshold=0.55, handle=b0_handle,
                 request_tta=True)
        want = [lone.analyze_request(jpeg=it) if isinstance(it, bytes) else lone.analyze_request(it) for it in items]
        assert got[sid] == want, sid
        lone.release()
    assert random.getstate() == state
    assert sum(r['analysis_mode'] == 'face+frame' for rs in got.values() for r in rs) >= 2
    for sid in work:
        pool.close(sid)

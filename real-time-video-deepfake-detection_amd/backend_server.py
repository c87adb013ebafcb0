"""Flask surface of the reference's ``backend_server.py``, unchanged for clients.

Routes, methods, status codes and JSON keys follow reference backend_server.py:82-255 (the wire
contract the Chrome extension reads): ``POST /analyze`` (multipart field
``frame``), ``GET /health``, ``POST /reset``, ``GET /stats``; 400 for a missing/undecodable
frame, 429 from the 100 ms rate limiter, 500 with ``{'error': ...}`` for anything else.  The
per-request work is `DeepfakeDetector.analyze_request` (one GPU call).  Differences: sequential-Huffman
JPEGs (what the extension sends) are decoded on the GPU from the request bytes (dfd_analyze_jpeg: entropy decoding
on the host, IDCT / upsampling / colour on the device, bit-identical to libjpeg) and everything else with
Pillow (cv2 is not a dependency here; with ``DFD_JPEG_PROGRESSIVE=1`` in the environment when the handle is made,
complete progressive JPEGs - what mozjpeg and most web pipelines write - are decoded by the library too instead of by
Pillow); ``POST /analyze_batch`` takes several ``frame`` parts of one stream in one
request; CORS headers are added by hand (no
flask_cors), and the rate limiter and detector are guarded by locks (the reference shares them
unsynchronised across Flask's worker threads, :57,62-80,275).

Sessions (not in the reference): an optional ``?session=<id>`` on ``/analyze``, ``/analyze_batch``, ``/stats`` and
``/reset`` gives each client its own detector and its own 100 ms limiter, and the frames of all sessions are served in
shared batched device passes (`sessions.SessionPool`).  Session ids are chosen by the client and are NOT a security
boundary: whoever knows an id can post to, read or reset that session.  Without the parameter nothing changes.
"""
from __future__ import annotations

import io
import logging
import os
import re
import threading
import time
import traceback
from functools import wraps

import numpy as np
from flask import Flask, jsonify, request

from . import runtime
from .deepfake_detection import DEVICE, DeepfakeDetector, forensic_size_from_env, model, mtcnn  # noqa: F401  (reference :39)
from .face_detection import detect_bounding_box  # noqa: F401                      (reference :40)
from .sessions import InvalidFrame, SessionClosed, SessionPool, SessionPoolFull

logging.basicConfig(level=logging.INFO, format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%H:%M:%S')
logger = logging.getLogger(__name__)

app = Flask(__name__)
# cv2.imdecode has no request-size notion; Flask would buffer any body.  32 MiB holds a 4K PNG or a 32-frame JPEG batch.
app.config['MAX_CONTENT_LENGTH'] = 32 << 20
MAX_BATCH_FRAMES = 32                     # /analyze_batch: frames per request (one lock hold, one device batch)
# /analyze_batch: pixels per request, summed over the parts' HEADERS before anything is decoded or allocated (a flat
# 8192 x 8192 JPEG is ~1 MB: 32 of them fit the body limit and would ask for ~13 GB of pinned coefficients).  32 frames
# of 1080p; the library enforces its own budget too (dfd_common.h kMaxBatchPixels).
MAX_BATCH_PIXELS = 32 * 1920 * 1088
MAX_FRAME_PIXELS = 1 << 26                # one part (the GPU JPEG path's own cap; Pillow's bomb guard is of this order)


@app.after_request
def _cors(resp):                                  # reference :46-53 (CORS(app, origins="*", GET/POST/OPTIONS))
    resp.headers["Access-Control-Allow-Origin"] = "*"
    resp.headers["Access-Control-Allow-Methods"] = "GET, POST, OPTIONS"
    resp.headers["Access-Control-Allow-Headers"] = "Content-Type"
    return resp


# DFD_TTA_AUGMENTATIONS=<K> (K > 1): test-time augmentation with K images per face, inside the one batched device pass of
# every route.  Unset: off, as the reference ships its server (:57 "Disabled for real-time speed").
try:
    TTA_AUGMENTATIONS = max(1, int(os.environ.get("DFD_TTA_AUGMENTATIONS", "1")))
except ValueError:
    TTA_AUGMENTATIONS = 1
# DFD_FORENSIC_SIZE=<S>: the forensic analysis runs at S x S instead of 256 x 256 (S a multiple of 16 in 32..1024, on the
# general kernel chain; implies DFD_FORENSIC_ANY_SIZE) for the global detector and every session's detector, through the same
# fused and batched device passes.  An invalid value fails here, at start-up.  Unset: nothing changes.
FORENSIC_SIZE = forensic_size_from_env()
detector = DeepfakeDetector(enable_gradcam=False, use_tta=TTA_AUGMENTATIONS > 1, num_tta_augmentations=TTA_AUGMENTATIONS,
                            detection_threshold=0.55, request_tta=TTA_AUGMENTATIONS > 1,                       # reference :57
                            forensic_size=FORENSIC_SIZE)

_last_request_time = 0.0
_min_request_interval = 0.1                                                 # reference :63
_rate_lock = threading.Lock()
_detector_lock = threading.Lock()

# Sessions (optional `?session=<id>` on /analyze, /analyze_batch, /stats, /reset; no reference counterpart): each id gets
# its own DeepfakeDetector in the pool (own vote window, frame counter, forensic stream) and its own 100 ms limiter, and
# the frames of all sessions share batched device passes (sessions.SessionPool).  Ids are chosen by the client and are
# not a security boundary: anyone who knows an id can read or reset that session.  Without the parameter every route
# takes the session-less path above (global detector, global limiter) exactly as before.
_SESSION_ID = re.compile(r'[A-Za-z0-9_-]{1,64}')
_session_pool = None                      # built on first use; tests may install their own
_session_last: dict = {}                  # session id -> time of its last admitted request (under _rate_lock)


def _pool():
    global _session_pool
    with _rate_lock:
        if _session_pool is None:
            _session_pool = SessionPool(lock=_detector_lock, detection_threshold=0.55, use_tta=TTA_AUGMENTATIONS > 1,
                                        num_tta_augmentations=TTA_AUGMENTATIONS, forensic_size=FORENSIC_SIZE)
        return _session_pool


def _session_arg():
    """(session id or None, error response or None)"""
    sid = request.args.get('session')
    if sid is None:
        return None, None
    if not _SESSION_ID.fullmatch(sid):
        return None, (jsonify({'error': 'Invalid session id (1-64 characters of A-Z a-z 0-9 _ -)'}), 400)
    return sid, None


def _session_rate_limited(sid):
    """the per-session form of the reference's limiter (:66-80): a 429 response, or None"""
    with _rate_lock:
        now = time.time()
        elapsed = now - _session_last.get(sid, 0.0)
        if elapsed < _min_request_interval:
            return jsonify({'error': 'Rate limited', 'retry_after_ms': int((_min_request_interval - elapsed) * 1000)}), 429
        if len(_session_last) > 4096:                               # forget sessions that are past their interval
            for k in [k for k, t in _session_last.items() if now - t >= _min_request_interval]:
                del _session_last[k]
        _session_last[sid] = now
    return None


def rate_limit(f):
    """reference :66-80; with ?session= the session's own limiter instead (the session id is checked first)"""
    @wraps(f)
    def decorated(*args, **kwargs):
        global _last_request_time
        sid, bad = _session_arg()
        if bad is not None:
            return bad
        if sid is not None:
            limited = _session_rate_limited(sid)
            return limited if limited is not None else f(*args, **kwargs)
        with _rate_lock:
            now = time.time()
            elapsed = now - _last_request_time
            if elapsed < _min_request_interval:
                return jsonify({'error': 'Rate limited',
                                'retry_after_ms': int((_min_request_interval - elapsed) * 1000)}), 429
            _last_request_time = now
        return f(*args, **kwargs)
    return decorated


def _session_results(sid, items, single=False):
    """the pool's responses for one request of session `sid` (list of dicts), or an error response: a part that does not
    decode gets the 400 of the session-less route (`single`: /analyze's body), and no other session notices it"""
    try:
        return _pool().submit(sid, items).result(), None
    except SessionPoolFull as e:
        return None, (jsonify({'error': 'Too many active sessions', 'retry_after_ms': e.retry_after_ms}), 503)
    except InvalidFrame as e:
        return None, (jsonify({'error': 'Invalid image format' if single else str(e)}), 400)
    except SessionClosed:
        return None, (jsonify({'error': f'Session {sid} was closed'}), 410)


def image_size(image_bytes: bytes):
    """(width, height) from the file's header alone (nothing is decoded), or None."""
    from PIL import Image

    try:
        with Image.open(io.BytesIO(image_bytes)) as im:
            return im.size
    except Exception:
        return None


def decode_image(image_bytes: bytes):
    """cv2.imdecode(..., IMREAD_COLOR) stand-in: BGR uint8 (H,W,3) or None (reference :139-145)."""
    from PIL import Image

    try:
        with Image.open(io.BytesIO(image_bytes)) as im:
            if im.size[0] * im.size[1] > MAX_FRAME_PIXELS:
                return None
            rgb = np.asarray(im.convert("RGB"))
    except Exception:
        return None
    if rgb.ndim != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        return None
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _gpu_name():
    try:
        import torch

        return torch.cuda.get_device_name(runtime.device_index()) if torch.cuda.is_available() else None
    except Exception:
        return None


@app.route('/health', methods=['GET'])
def health_check():
    """reference :82-99"""
    name = _gpu_name()
    h = runtime.peek_default_handle()
    # reference :93: face detection is the DNN or its Haar fallback (face_detection.py:58-61)
    has_det = bool(h.has_detector or h.has_haar) if h is not None else bool(
        runtime.detector_loaded or runtime.detector_synthetic or runtime.haar_loaded)
    # the reference's keys (:84-99) plus what was actually loaded: without trained weights the verdicts mean nothing
    return jsonify({'status': 'healthy', 'model_loaded': bool(runtime.model_loaded), 'detector_loaded': bool(runtime.detector_loaded),
                    'mtcnn_loaded': bool(runtime.mtcnn_loaded), 'synthetic_weights': bool(runtime.detector_synthetic),
                    'device': DEVICE, 'gpu_name': name, 'frame_count': detector.frame_count,
                    'capabilities': {'face_detection': has_det, 'frame_forensics': True, 'temporal_tracking': True}}), 200


@app.route('/reset', methods=['POST'])
def reset_detector():
    """reference :101-115; ?session= resets only that session"""
    sid, bad = _session_arg()
    if bad is not None:
        return bad
    try:
        if sid is not None:
            _pool().reset(sid)                                      # an unknown session has nothing to reset
            return jsonify({'success': True, 'message': 'Detector reset successfully'}), 200
        with _detector_lock:
            detector.reset()
        return jsonify({'success': True, 'message': 'Detector reset successfully'}), 200
    except Exception as e:
        logger.error("Reset failed: %s", e)
        return jsonify({'success': False, 'error': str(e)}), 500


@app.route('/analyze', methods=['POST'])
@rate_limit
def analyze_frame():
    """reference :117-238"""
    start_time = time.time()
    try:
        if 'frame' not in request.files:
            return jsonify({'error': 'No frame provided'}), 400
        image_bytes = request.files['frame'].read()
        response = None
        sid = request.args.get('session')
        if sid is not None:                                         # the session's detector, in the pool's next pass
            if image_bytes[:2] == b'\xff\xd8' and image_size(image_bytes) is not None:
                item = image_bytes                                  # decoded on the device (Pillow if the library refuses it)
            else:
                item = decode_image(image_bytes)
                if item is None:
                    return jsonify({'error': 'Invalid image format'}), 400
            results, err = _session_results(sid, [item], single=True)
            if err is not None:
                return err
            response = results[0]
        elif image_bytes[:2] == b'\xff\xd8':                      # JPEG: decode on the device, no raw upload
            try:
                with _detector_lock:
                    response = detector.analyze_request(jpeg=image_bytes)
            except runtime.DfdError as e:
                if e.code not in (-7, -1):                          # unsupported flavour / not decodable here: Pillow decides
                    raise
        if response is None:
            frame = decode_image(image_bytes)
            if frame is None:
                return jsonify({'error': 'Invalid image format'}), 400
            with _detector_lock:
                response = detector.analyze_request(frame)
        ms = (time.time() - start_time) * 1000
        # key order as the reference builds it (:178-195 / :213-225)
        bbox = response.pop('face_bbox', None)
        response['processing_time_ms'] = round(ms, 1)
        if bbox is not None:
            response['face_bbox'] = bbox
        logger.info("Frame %d%s | %.0f%% | Verdict: %s | %.0fms", response['frame_count'],
                    "" if bbox else " [NO FACE]", response['fake_probability'] * 100, response['confidence_level'], ms)
        return jsonify(response), 200
    except Exception as e:
        logger.error("Error analyzing frame: %s", e)
        logger.error(traceback.format_exc())
        return jsonify({'error': str(e)}), 500


@app.route('/analyze_batch', methods=['POST'])
@rate_limit
def analyze_batch():
    """Several consecutive frames of ONE stream in a single request (multipart parts all named ``frame``, in stream
    order): the same per-frame flow and vote order as /analyze, one JSON object per frame under ``results``.  Not in the
    reference (its extension posts one frame per request, throttled to 10 per second, backend_server.py:62-80); this
    is the batched entry SURVEY 8(f) N2 asks for.  Every part is read and validated BEFORE the detector is touched (a
    rejected request leaves the stream's state alone); then ONE library call does the GPU work of all frames
    (`DeepfakeDetector.analyze_request_batch`: JPEG scans entropy-decoded in parallel on host threads, one forensic /
    detector / classifier pass) and the votes are replayed in order.  At most MAX_BATCH_FRAMES parts."""
    start_time = time.time()
    try:
        files = request.files.getlist('frame')
        if not files:
            return jsonify({'error': 'No frame provided'}), 400
        if len(files) > MAX_BATCH_FRAMES:
            return jsonify({'error': f'Too many frames in one request ({len(files)} > {MAX_BATCH_FRAMES})'}), 400
        blobs = [f.read() for f in files]
        pixels = 0
        for k, data in enumerate(blobs):                            # headers only: the budget is checked before any decode
            size = image_size(data)
            if size is None:
                return jsonify({'error': f'Invalid image format (frame {k})'}), 400
            pixels += size[0] * size[1]
        if pixels > MAX_BATCH_PIXELS:
            return jsonify({'error': f'Batch too large ({pixels} pixels > {MAX_BATCH_PIXELS})'}), 400
        items = []
        for k, data in enumerate(blobs):
            if data[:2] == b'\xff\xd8':
                items.append(data)                                  # decoded on the device
            else:
                frame = decode_image(data)
                if frame is None:
                    return jsonify({'error': f'Invalid image format (frame {k})'}), 400
                items.append(frame)
        sid = request.args.get('session')
        if sid is not None:                                         # the session's detector; sizes may differ
            results, err = _session_results(sid, items)
            if err is not None:
                return err
            ms = (time.time() - start_time) * 1000
            return jsonify({'success': True, 'frames': len(results), 'processing_time_ms': round(ms, 1), 'results': results}), 200
        results = None
        with _detector_lock:
            try:
                results = detector.analyze_request_batch(items)
            except (runtime.DfdError, ValueError) as e:
                # a JPEG flavour the device path does not take, or parts of different sizes: nothing has moved yet
                if isinstance(e, runtime.DfdError) and e.code not in (-7, -1):
                    raise
        if results is None:
            frames = []
            for k, it in enumerate(items):
                frame = decode_image(it) if isinstance(it, bytes) else it
                if frame is None:
                    return jsonify({'error': f'Invalid image format (frame {k})'}), 400
                frames.append(frame)
            with _detector_lock:
                if len({fr.shape for fr in frames}) == 1:
                    results = detector.analyze_request_batch(frames)
                else:
                    results = [detector.analyze_request(fr) for fr in frames]
        ms = (time.time() - start_time) * 1000
        return jsonify({'success': True, 'frames': len(results), 'processing_time_ms': round(ms, 1), 'results': results}), 200
    except Exception as e:
        logger.error("Error analyzing batch: %s", e)
        logger.error(traceback.format_exc())
        return jsonify({'error': str(e)}), 500


@app.route('/stats', methods=['GET'])
def get_stats():
    """reference :240-255; ?session= reports that session (404 when there is none)"""
    sid, bad = _session_arg()
    if bad is not None:
        return bad
    try:
        if sid is not None:
            s = _pool().stats(sid)
            if s is None:
                return jsonify({'error': f'Unknown session {sid}'}), 404
            s['device'] = DEVICE
            return jsonify(s), 200
        t = detector.temporal_tracker
        return jsonify({'frame_count': detector.frame_count, 'temporal_average': float(t.get_temporal_average()),
                        'stability_score': float(t.get_stability_score()), 'confidence_level': t.get_confidence_level(),
                        'history_length': len(t.score_history), 'voting': t.get_voting_stats(), 'device': DEVICE}), 200
    except Exception as e:
        return jsonify({'error': str(e)}), 500


if __name__ == '__main__':
    app.run(host='0.0.0.0', port=5000, debug=False, threaded=True)         # reference :275

"""Host mirror of the reference's ``deepfake_detection.py`` over the HIP path.

`DeepfakeDetector` keeps the constructor, attributes, methods and result dictionaries of
reference deepfake_detection.py:292-726 and the module keeps its globals (`DEVICE`, `model`,
`mtcnn`, `detector`, `predict`, `predict_with_forensics`; :21-32,729-747).  Per frame the GPU
does forensics, face detection, crop -> CLAHE -> 224x224 -> EfficientNet-B0 in ONE call
(`dfd_analyze_frame`); calibration, the small-face heuristic and the vote stay on the host as in
the reference.  The MTCNN align/crop of reference :376-380 runs inside the same library call when the handle's
weights carry the cascade (`mtcnn` below is its module-level mirror); a crop in which it finds no face yields no
prediction, exactly as the reference's `None` (:378-380, :616-617, backend_server.py:166).  GradCAM (:5-7 imports
`GradCAM`, `ClassifierOutputTarget`, `show_cam_on_image`, re-exported here from `gradcam`) runs on the GPU for the
head conv the reference hooks (`dfd_gradcam_crops`); `DeepfakeDetector.explain_face` returns a face's probability with
its heat map and BGR overlay, while `analyze_face` keeps returning None in its third slot whatever `enable_gradcam` is,
as the reference does (:543-546; GradCAM is disabled in its shipped configurations, :730-736 and
backend_server.py:57).  Deliberate differences: frames are returned un-annotated, nothing is
printed per frame.  TTA (:408-443): `analyze_face`
keeps the per-face path (`analyze_face_with_tta` over `dfd_tta_augment`); `predict`, `analyze_request` and
`analyze_request_batch` (these two with `request_tta=True`) carry every face's augmented copies inside their one library call (`dfd_tta_arm`; draws and the
`random` stream: `tta_draw_table` / `tta_commit_draws`) - the same probabilities, bit for bit.  Face detection inside the fused call follows the reference's
`detect_bounding_box` (face_detection.py:58-66): the SSD when the handle carries one, else - and after an SSD failure -
the Haar cascade, else no faces ('frame_only').
"""
from __future__ import annotations

import logging
import os
import pickle
import random
import threading
from typing import List, Optional

import numpy as np

from . import runtime
from ._lib import DfdError, Handle
from .face_detection import detect_bounding_box
from .frame_analysis import FrameForensicAnalyzer
from .gradcam import ClassifierOutputTarget, GradCAM, show_cam_on_image  # noqa: F401  (reference :5-7)
from .tracker import TemporalTracker

log = logging.getLogger(__name__)

DEVICE = f"cuda:{runtime.device_index()}"
from .mtcnn import MTCNN  # noqa: E402

mtcnn = MTCNN(select_largest=False, post_process=False, device=DEVICE)     # reference :24-28


def _sigmoid32(logit) -> float:
    """torch.sigmoid on a float32 scalar, then .item() (reference :397-398)."""
    x = np.float32(logit)
    return float(np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32)))


def tta_draw_table(capacity_faces: int, copies: int):
    """The draws of a call that may return up to `capacity_faces` faces, taken from Python's global `random` in the
    reference's order (:419-426: per face, per copy `random() > 0.5`, `uniform(0.9, 1.1)`, `uniform(-3, 3)` - all three
    always) -> (the generator state before the first draw, [(flip, brightness, angle_deg)] face-major).  The number of
    faces is known only after the call: `tta_commit_draws` then leaves the stream where the used rows end."""
    state = random.getstate()
    draws = [(random.random() > 0.5, random.uniform(0.9, 1.1), random.uniform(-3, 3))
             for _ in range(int(capacity_faces) * int(copies))]
    return state, draws


def tta_commit_draws(state, n_faces: int, copies: int):
    """Rewind `random` to `state` and draw again exactly the rows `n_faces` faces used: the global stream is then where
    the reference's per-face loop would have left it (untouched for a call without faces)."""
    random.setstate(state)
    for _ in range(int(n_faces) * int(copies)):
        random.random()
        random.uniform(0.9, 1.1)
        random.uniform(-3, 3)


def forensic_size_from_env() -> Optional[int]:
    """DFD_FORENSIC_SIZE=<S>: the analysis size the server gives its global detector and every session's detector (it
    implies any_size).  Unset or empty: None, the reference's 256x256.  Not an integer: ValueError; a size the
    analyzer does not take fails with the analyzer's ValueError where the detector is built."""
    v = os.environ.get("DFD_FORENSIC_SIZE", "").strip()
    if not v:
        return None
    try:
        return int(v)
    except ValueError:
        raise ValueError(f"DFD_FORENSIC_SIZE={v!r}: analysis_size must be an integer S, a multiple of 16 in 32..1024") from None


class _LazyModel:
    """`model` global of the reference (:32): the classifier bound to the default handle."""

    def __call__(self, rgb_input, freq_input=None):
        x = rgb_input.detach().cpu().numpy() if hasattr(rgb_input, "detach") else np.asarray(rgb_input)
        out = runtime.default_handle().classify(np.ascontiguousarray(x, dtype=np.float32))
        if hasattr(rgb_input, "detach"):
            import torch

            return torch.from_numpy(out)
        return out

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self


model = _LazyModel()


class DeepfakeDetector:
    def __init__(self, enable_gradcam=False, use_tta=True, num_tta_augmentations=3, detection_threshold=0.5,
                 face_weight=0.70, forensic_weight=0.30, *, handle: Optional[Handle] = None, request_tta: bool = False,
                 forensic_size: Optional[int] = None):
        """forensic_size: None = the reference's 256x256 analysis, or S = a (S, S) analysis on the general forensic chain
        (a multiple of 16 in 32..1024, else the analyzer's ValueError); every fused and batched call runs at that size.
        Construction makes no library call: the forensic stream is opened by the first call that uses it."""
        self.enable_gradcam = enable_gradcam
        self.use_tta = use_tta
        # the /analyze flow (analyze_request, analyze_request_batch, the session pool) carries the copies only when this is
        # set as well: callers of that flow construct detectors with the reference's constructor defaults (TTA on) and
        # rely on the single classification it has always made there; `predict` follows use_tta alone, as before
        self.request_tta = bool(request_tta)
        self.num_tta_augmentations = num_tta_augmentations
        self.detection_threshold = detection_threshold
        self.face_weight = face_weight                  # stored, never used - as in the reference
        self.forensic_weight = forensic_weight
        self.temporal_tracker = TemporalTracker(window_size=60, high_confidence_threshold=0.6, voting_window=10,
                                                detection_threshold=detection_threshold)
        self.frame_count = 0
        self._handle = handle
        if forensic_size is None:
            self.frame_analyzer = FrameForensicAnalyzer(analysis_size=(256, 256), handle=handle)
        else:
            self.frame_analyzer = FrameForensicAnalyzer(analysis_size=(int(forensic_size), int(forensic_size)), handle=handle,
                                                        any_size=True, defer_open=True)
        self.full_forensic_interval = 3
        self.last_frame_forensic_result = None
        self.calibrator = None
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights", "calibrator.pkl")
        if os.path.exists(path):
            try:
                with open(path, "rb") as f:
                    self.calibrator = pickle.load(f)
            except Exception:                             # reference :341-342
                log.warning("could not load calibrator")
        self._lock = threading.Lock()                     # a handle is single-caller; Flask is threaded

    # ------------------------------------------------------------------ plumbing
    @property
    def handle(self) -> Handle:
        if self._handle is None:
            self._handle = runtime.default_handle()
            self.frame_analyzer._handle = self._handle
        return self._handle

    def reset(self):
        """reference :344-355"""
        self.temporal_tracker.reset()
        self.frame_count = 0
        self.frame_analyzer.reset()
        self.last_frame_forensic_result = None

    # ------------------------------------------------------------------ scalars after the network
    def apply_calibration(self, raw_prob):
        """reference :445-455"""
        if self.calibrator is None:
            return raw_prob
        try:
            return self.calibrator.predict_proba([[raw_prob]])[0][1]
        except Exception:
            return raw_prob

    FREQ_MAX_SIDE = 4096                    # DFD_FREQ_MAX_SIDE of the library

    @staticmethod
    def _frequency_verdict(high, total) -> float:
        """reference :480-485, in double on the host"""
        return 0.15 if float(high) / (float(total) + 1e-10) < 0.15 else 0.0

    def analyze_frequency_domain(self, face_region):
        """reference :457-487, the GAN-artefact check: 0.15 when less than 15 % of the magnitude of the crop's 2-D
        spectrum (at the crop's own h x w) lies outside the central min(h, w) // 4 square, else 0.0.  The spectrum and
        both sums are computed on the GPU (`dfd_frequency_domain`).  0.0 wherever the reference's bare `except` gives
        it: an empty region, or an input that is not (h, w, 3).  Unlike the reference: a side
        above 4096 or a non-uint8 array raises ValueError."""
        face = np.asarray(face_region)
        if face.dtype != np.uint8:
            raise ValueError(f"analyze_frequency_domain takes a uint8 BGR crop, got {face.dtype}")
        if face.ndim != 3 or face.shape[2] != 3 or face.shape[0] < 1 or face.shape[1] < 1:
            return 0.0
        if max(face.shape[:2]) > self.FREQ_MAX_SIDE:
            raise ValueError(f"analyze_frequency_domain: crop {face.shape[1]} x {face.shape[0]}, sides above "
                             f"{self.FREQ_MAX_SIDE} are not supported")
        with self._lock:
            high, total = self.handle.frequency_domain(np.ascontiguousarray(face))[0]
        return self._frequency_verdict(high, total)

    def analyze_frequency_domain_boxes(self, frame, boxes):
        """`analyze_frequency_domain` of every box (x, y, w, h) of a BGR frame, from ONE library call -> list of 0.15 /
        0.0.  Boxes must lie inside the frame (DfdError otherwise); no boxes: []."""
        frame = np.asarray(frame)
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("analyze_frequency_domain_boxes takes an (H, W, 3) uint8 BGR frame")
        b = np.asarray(boxes, np.int64).reshape(-1, 4)
        if b.shape[0] == 0:
            return []
        if b[:, 2:].max() > self.FREQ_MAX_SIDE:
            raise ValueError(f"analyze_frequency_domain_boxes: sides above {self.FREQ_MAX_SIDE} are not supported")
        with self._lock:
            sums = self.handle.frequency_domain(np.ascontiguousarray(frame), b)
        return [self._frequency_verdict(hi, tot) for hi, tot in sums]

    def apply_heuristics(self, fake_prob, face_region):
        """reference :489-502: +0.10 for crops under 80 px, clipped to [0,1]."""
        h, w = face_region.shape[:2]
        return self._heuristics_hw(fake_prob, h, w)

    @staticmethod
    def _heuristics_hw(fake_prob, h, w):
        adjustment = 0.10 if (h < 80 or w < 80) else 0.0
        return np.clip(fake_prob + adjustment, 0, 1)

    def _tta_copies(self, request: bool = False) -> int:
        """augmented copies per face the fused calls carry (0: TTA off; reference :524); request: for the /analyze flow"""
        if request and not self.request_tta:
            return 0
        return self.num_tta_augmentations - 1 if self.use_tta and self.num_tta_augmentations > 1 else 0

    def _armed(self, call, capacity_faces, request, **kw):
        """`call(**kw)`; with TTA on, armed with the draws of `capacity_faces` faces, and `random` is left after the
        draws of the faces the call returned (none when it raises)"""
        copies = self._tta_copies(request)
        if copies == 0:
            return call(**kw)
        state, draws = tta_draw_table(capacity_faces, copies)
        used = 0
        try:
            out = call(tta=(copies, draws), **kw)
            used = self.handle.tta_logits().shape[0]
            return out
        finally:
            tta_commit_draws(state, used, copies)

    def _finish_face(self, logit, h, w):
        """None when the MTCNN stage found no face in the crop (NaN logit from the library).  `logit` is a scalar, or -
        from a call that carried augmented copies - the face's row (original, copies): the mean of the sigmoids of
        the images the cascade kept, in `analyze_face_with_tta`'s arithmetic (reference :436-441)."""
        if logit is not None and np.ndim(logit) == 1:
            predictions = [_sigmoid32(v) for v in logit if not np.isnan(v)]
            if not predictions:
                return None
            return self._heuristics_hw(self.apply_calibration(float(np.mean(predictions))), h, w)
        if logit is None or np.isnan(logit):
            return None
        p = self.apply_calibration(_sigmoid32(logit))
        return self._heuristics_hw(p, h, w)

    # ------------------------------------------------------------------ reference methods
    def preprocess_face_quality(self, face_region):
        """BGR -> Lab, CLAHE(2.0, 8x8) on L, Lab -> BGR on the GPU (reference :357-370)."""
        with self._lock:
            return self.handle.preprocess_face_quality(np.ascontiguousarray(face_region))

    def _forensic_is_full(self) -> bool:
        return self.frame_count % self.full_forensic_interval == 0          # reference :509

    def analyze_frame_forensics(self, frame):
        """reference :504-515"""
        with self._lock:
            if self._forensic_is_full():
                result = self.frame_analyzer.analyze(frame)
            else:
                result = self.frame_analyzer.analyze_fast(frame)
        self.last_frame_forensic_result = result
        return result

    def _single_prediction(self, face_region):
        """sigmoid(model(...)) of an already quality-preprocessed crop, or None (reference :372-406)"""
        h, w = face_region.shape[:2]
        with self._lock:
            logit = self.handle.classify_crops(face_region, [(0, 0, w, h)], apply_clahe=False)[0, 0]
        return None if np.isnan(logit) else _sigmoid32(logit)

    def analyze_face_with_tta(self, face_region):
        """reference :408-443: the original plus num_tta_augmentations - 1 randomly augmented copies (horizontal flip
        with probability 1/2, brightness x U(0.9, 1.1), rotation by U(-3, 3) degrees about the centre), each through
        `_single_prediction`, averaged.  The draws come from Python's `random` in the reference's order."""
        predictions = []
        pred = self._single_prediction(face_region)
        if pred is not None:
            predictions.append(pred)
        for _ in range(self.num_tta_augmentations - 1):
            flip = random.random() > 0.5
            brightness = random.uniform(0.9, 1.1)
            angle = random.uniform(-3, 3)
            with self._lock:
                aug = self.handle.tta_augment(face_region, flip, brightness, angle)
            pred = self._single_prediction(aug)
            if pred is not None:
                predictions.append(pred)
        return float(np.mean(predictions)) if predictions else None

    def analyze_face(self, face_region):
        """(fake_prob, fake_prob, None) or (None, None, None) (reference :517-550)."""
        try:
            face = np.ascontiguousarray(face_region)
            if face.ndim != 3 or face.shape[2] != 3 or face.shape[0] < 1 or face.shape[1] < 1:
                return None, None, None
            h, w = face.shape[:2]
            if self.use_tta and self.num_tta_augmentations > 1:               # reference :524-527
                with self._lock:
                    pre = self.handle.preprocess_face_quality(face)
                raw = self.analyze_face_with_tta(pre)
                if raw is None:
                    return None, None, None
                p = self._heuristics_hw(self.apply_calibration(raw), h, w)
                return p, p, None
            with self._lock:
                logit = self.handle.classify_crops(face, [(0, 0, w, h)], apply_clahe=True)[0, 0]
            p = self._finish_face(logit, h, w)
            if p is None:
                return None, None, None
            return p, p, None
        except (DfdError, ValueError) as e:
            log.warning("face analysis error: %s", e)
            return None, None, None

    def explain_face(self, face_region, as_jpeg=False):
        """Where in the face the classifier saw a fake: {'fake_probability' (as `analyze_face` without TTA: same
        calibration and small-face heuristic), 'heatmap' (224,224) float32 Grad-CAM map of the head conv in [0,1],
        'overlay' (224,224,3) BGR uint8 (show_cam_on_image on the classifier input)}, or None when the MTCNN stage
        finds no face.  The maps are in the 224x224 classifier frame of the (MTCNN-aligned) face.  `as_jpeg`: also
        'overlay_jpeg', the overlay as a JPEG file encoded on the device at cv2.imwrite's defaults (quality 95, 4:2:0)."""
        face = np.ascontiguousarray(face_region)
        if face.ndim != 3 or face.shape[2] != 3 or face.shape[0] < 1 or face.shape[1] < 1:
            return None
        h, w = face.shape[:2]
        with self._lock:
            logits, heat, overlay = self.handle.gradcam_crops(face, [(0, 0, w, h)], apply_clahe=True, overlay=True)
        p = self._finish_face(logits[0, 0], h, w)
        if p is None:
            return None
        res = {'fake_probability': p, 'heatmap': heat[0], 'overlay': overlay[0]}
        if as_jpeg:
            with self._lock:
                res['overlay_jpeg'] = self.handle.encode_jpeg(overlay[0], quality=95, subsampling=2)
        return res

    def _open_stream(self):
        """before a fused call: a sized analyzer's stream holds its analysis size on this detector's handle (a no-op
        in the library when it does already; a released stream is opened again)"""
        self.frame_analyzer.open(self.handle)

    def _forensics_only(self, frame, full):
        """'frame_only' mode (no detector of either kind): the analyzer's call alone -> (scores, probability)"""
        a = self.frame_analyzer
        if a.sized:
            return self.handle.forensics_sized(frame, a.analysis_size[0], full=full, stream_id=a.stream_id)[:2]
        return self.handle.forensics(frame, full=full, stream_id=a.stream_id)[:2]

    def _frame_on_gpu(self, frame, max_faces, jpeg: Optional[bytes] = None, request: bool = False):
        """forensics + detection + per-face logits in one library call (with TTA on: every face's row of logits, original
        and augmented copies, from the same call).  With `jpeg` the frame is decoded on the
        device from the request's bytes (dfd_analyze_jpeg) instead of uploaded raw; returns its (H, W) as 4th item."""
        full = self._forensic_is_full()
        with self._lock:
            self._open_stream()                     # a sized analyzer: the fused call runs its stream at its own size
            if jpeg is not None:
                scores, prob, boxes, logits, shape = self._armed(
                    self.handle.analyze_jpeg, max_faces, request, data=jpeg, full_forensics=full,
                    stream_id=self.frame_analyzer.stream_id, confidence_threshold=0.5, max_faces=max_faces)
                number = self.frame_analyzer.frame_count
                forensic = {'scores': scores, 'fake_probability': prob,
                            'analysis_type': 'frame_forensic' if full else 'frame_forensic_fast', 'frame_number': number}
                self.last_frame_forensic_result = forensic
                return forensic, boxes, logits, shape
            if self.handle.has_detector or self.handle.has_haar:
                # SSD, or the reference's Haar fallback (face_detection.py:58-61), inside the same library call
                scores, prob, boxes, logits = self._armed(
                    self.handle.analyze_frame, max_faces, request, frame=frame, full_forensics=full,
                    stream_id=self.frame_analyzer.stream_id, confidence_threshold=0.5, max_faces=max_faces)
            else:                                   # no detector of either kind: 'frame_only' mode (runtime.py)
                scores, prob = self._forensics_only(frame, full)
                boxes, logits = [], []
            number = self.frame_analyzer.frame_count
        forensic = {'scores': scores, 'fake_probability': prob,
                    'analysis_type': 'frame_forensic' if full else 'frame_forensic_fast', 'frame_number': number}
        self.last_frame_forensic_result = forensic
        return forensic, boxes, logits

    def predict(self, frame):
        """(frame, trigger_forensic, forensic_frame, result_data) (reference :588-686)."""
        self.frame_count += 1
        frame = np.ascontiguousarray(frame)
        small = frame.shape[0] < 30 or frame.shape[1] < 30
        frame_forensic, faces, logits = self._frame_on_gpu(frame, max_faces=200)       # DetectionOutput keeps <= 200
        if small:
            faces, logits = [], []
        trigger_forensic, forensic_frame = False, None
        face_results: List[dict] = []
        confidence_level = self.temporal_tracker.get_confidence_level()
        if len(faces) > 0:
            for (x, y, w, h), logit in zip(faces, logits):
                # with TTA `logit` is the face's row from the same call (original + augmented copies): what the
                # reference's analyze_face computes per face (:614), without a second classification
                fake_prob = self._finish_face(logit, h, w)
                if fake_prob is None:                                        # reference :616-617
                    continue
                self.temporal_tracker.update(fake_prob)
                confidence_level = self.temporal_tracker.get_confidence_level()
                if self.temporal_tracker.should_trigger_forensic_analysis():
                    trigger_forensic, forensic_frame = True, frame.copy()
                face_results.append({'face_prob': float(fake_prob), 'combined_prob': float(fake_prob),
                                     'bbox': {'x': int(x), 'y': int(y), 'w': int(w), 'h': int(h)}})
        else:
            self.temporal_tracker.update(frame_forensic['fake_probability'])
            confidence_level = self.temporal_tracker.get_confidence_level()
            if self.temporal_tracker.should_trigger_forensic_analysis():
                trigger_forensic, forensic_frame = True, frame.copy()
        result_data = {
            'frame_count': self.frame_count,
            'faces_detected': len(faces),
            'face_results': face_results,
            'frame_forensic': frame_forensic,
            'confidence_level': confidence_level if faces or self.frame_count > 1 else 'UNCERTAIN',
            'temporal_average': float(self.temporal_tracker.get_temporal_average()),
            'stability_score': float(self.temporal_tracker.get_stability_score()),
            'analysis_mode': 'face+frame' if len(faces) > 0 else 'frame_only',
        }
        return frame, trigger_forensic, forensic_frame, result_data

    def analyze(self, frame):
        """`result_data` of `predict` - the name BASELINE.json's north_star uses."""
        return self.predict(frame)[3]

    def analyze_request(self, frame=None, *, jpeg: Optional[bytes] = None):
        """The /analyze flow of the reference server (backend_server.py:147-233): forensics BEFORE the
        frame counter moves, only faces[0] is classified, one vote per request.  Returns the response
        dict without timing.  `jpeg`: the request's bytes, decoded on the device; raises
        DfdError (code -7 / -1) when the library does not decode that file - the caller then passes a frame."""
        if jpeg is not None:
            if not (self.handle.has_detector or self.handle.has_haar):
                frame = self.handle.decode_jpeg(jpeg)              # frame_only mode has no fused JPEG entry point
                jpeg = None
            else:
                frame_forensic, faces, logits, shape = self._frame_on_gpu(None, max_faces=1, jpeg=jpeg, request=True)
                small = shape[0] < 30 or shape[1] < 30
        if jpeg is None:
            frame = np.ascontiguousarray(frame)
            small = frame.shape[0] < 30 or frame.shape[1] < 30
            frame_forensic, faces, logits = self._frame_on_gpu(frame, max_faces=1, request=True)
        n_detected = 0 if small else self._last_face_count(frame, faces)
        return self._request_response(frame_forensic['fake_probability'], [] if small else faces, logits, n_detected)

    def _request_response(self, fprob, faces, logits, n_detected):
        """One frame of the /analyze flow once its GPU work is done (reference backend_server.py:166-233): the frame
        counter moves, faces[0] (if any) or the forensic probability votes, and the response dict without timing is
        returned.  `faces` is empty for frames under 30 px.  Shared by analyze_request, analyze_request_batch and the
        session pool (sessions.SessionPool)."""
        self.frame_count += 1
        tr = self.temporal_tracker
        fake_prob = None
        if len(faces) > 0:
            x, y, w, h = faces[0]
            fake_prob = self._finish_face(logits[0], h, w)
        if fake_prob is not None:                                            # backend_server.py:166
            tr.update(fake_prob)
            return {'success': True, 'analysis_mode': 'face+frame', 'faces_detected': n_detected,
                    'fake_probability': float(fake_prob), 'face_probability': float(fake_prob),
                    'frame_forensic_probability': float(fprob), 'real_probability': float(1 - fake_prob),
                    'confidence_level': tr.get_confidence_level(), 'temporal_average': float(tr.get_temporal_average()),
                    'stability_score': float(tr.get_stability_score()), 'frame_count': self.frame_count,
                    'face_bbox': {'x': int(x), 'y': int(y), 'width': int(w), 'height': int(h)}}
        tr.update(fprob)
        return {'success': True, 'analysis_mode': 'frame_only', 'faces_detected': n_detected,
                'fake_probability': float(fprob), 'frame_forensic_probability': float(fprob),
                'real_probability': float(1 - fprob), 'confidence_level': tr.get_confidence_level(),
                'temporal_average': float(tr.get_temporal_average()), 'stability_score': float(tr.get_stability_score()),
                'frame_count': self.frame_count}

    def release(self):
        """Frees this detector's forensic stream on the device (dfd_forensics_release): its gray plane goes back to the
        handle for the next new stream of its analysis size.  Used again afterwards, the detector's forensic stream
        starts fresh (at the analyzer's analysis size)."""
        h = self.frame_analyzer._existing_handle()
        if h is not None:
            h.forensics_release(self.frame_analyzer.stream_id)

    def analyze_request_batch(self, items):
        """`analyze_request` for several consecutive frames of this stream in ONE library call (POST /analyze_batch):
        `items` are JPEG bytes and / or BGR frames of one size.  The GPU work of all frames is batched
        (dfd_analyze_stream_batch); the frame counter, the full / fast forensic schedule (reference
        deepfake_detection.py:509-512) and the votes (backend_server.py:166-176,205-211) advance frame by frame in
        request order, so the responses equal those of len(items) single requests.  Raises DfdError (-7 / -1) BEFORE
        any state has moved when a JPEG part is not decodable on the device path or the sizes differ."""
        n = len(items)
        full = [(self.frame_count + i) % self.full_forensic_interval == 0 for i in range(n)]
        with self._lock:
            self._open_stream()
            if self.handle.has_detector or self.handle.has_haar:
                res, shape = self._armed(self.handle.analyze_stream_batch, n, True, items=items, full_flags=full,
                                         stream_id=self.frame_analyzer.stream_id, confidence_threshold=0.5, max_faces=1)
            else:                                                   # no detector of either kind: forensics only, frame by frame
                res, shape = [], None
                for it, fl in zip(items, full):
                    fr = self.handle.decode_jpeg(it) if isinstance(it, (bytes, bytearray)) else np.ascontiguousarray(it)
                    scores, prob = self._forensics_only(fr, fl)
                    res.append((scores, prob, [], [], 0))
                    shape = fr.shape[:2]
            first_number = self.frame_analyzer.frame_count - n + 1
        out = []
        small = shape[0] < 30 or shape[1] < 30
        for i, (scores, fprob, faces, logits, n_detected) in enumerate(res):
            self.last_frame_forensic_result = {'scores': scores, 'fake_probability': fprob,
                                               'analysis_type': 'frame_forensic' if full[i] else 'frame_forensic_fast',
                                               'frame_number': first_number + i}
            out.append(self._request_response(fprob, [] if small else faces, logits, 0 if small else n_detected))
        return out

    def _last_face_count(self, frame, faces):
        """`faces_detected` of the server response counts ALL detections (backend_server.py:181); the fused call
        classified only the first and the library remembers how many there were."""
        if not faces:
            return 0
        return self.handle.last_detection_count()


_detector: Optional[DeepfakeDetector] = None
_detector_lock = threading.Lock()


def _global_detector() -> DeepfakeDetector:
    """reference :730-736: module-level instance, built on first use instead of at import."""
    global _detector
    with _detector_lock:
        if _detector is None:
            _detector = DeepfakeDetector(use_tta=False, num_tta_augmentations=1, detection_threshold=0.5,
                                         face_weight=0.70, forensic_weight=0.30)
        return _detector


def __getattr__(name):
    if name == "detector":
        return _global_detector()
    raise AttributeError(name)


def predict(frame):
    """reference :739-742"""
    return _global_detector().predict(frame)[0]


def predict_with_forensics(frame):
    """reference :745-747"""
    return _global_detector().predict(frame)

"""Many video streams on one handle: one `DeepfakeDetector` per session, one batched device pass across sessions.

`SessionPool` maps a client-chosen session id to its own detector (vote window, frame counter, full / fast forensic
schedule, forensic stream on the device), all on one shared handle.  `submit` queues a session's frames and returns a
future; ONE worker thread takes everything queued when it becomes free (whole submissions, capped by frame count and
pixel budget), makes ONE `Handle.analyze_streams_batch` call over the frames of every session in it and then replays
each session's votes in submission order - so every session's responses equal those of a dedicated detector's
`analyze_request` on the same frames.  There is no timer and no tuning option: under load the queue itself forms the
batches.  Not in the reference (one global detector, SURVEY 8(b) "Threading").

Every handle call on this path, resets included, holds `lock` (the server passes its detector lock): no handle is
ever called from two threads.  Session ids are chosen by the client and are not a security boundary.
"""
from __future__ import annotations

import io
import threading
import time
from collections import OrderedDict, deque
from concurrent.futures import Future
from typing import Optional

import numpy as np

from ._lib import DfdError, Handle
from .deepfake_detection import DeepfakeDetector, forensic_size_from_env, tta_commit_draws, tta_draw_table
from .frame_analysis import check_analysis_size

MAX_PASS_FRAMES = 256                     # frames of one device pass (the classifier runs them in max_batch chunks)
MAX_PASS_PIXELS = 1 << 27                 # the library's per-call budget (dfd_common.h kMaxBatchPixels)


class SessionPoolFull(RuntimeError):
    """Every slot holds a session that is not idle; `retry_after_ms`: when the least recently used one will be."""

    def __init__(self, retry_after_ms: int):
        super().__init__("session pool is full")
        self.retry_after_ms = int(retry_after_ms)


class InvalidFrame(ValueError):
    """A part of the submission that neither the device path nor Pillow decodes (the server answers 400, as without
    sessions); `index`: its position in the submission."""

    def __init__(self, index: int):
        super().__init__(f"Invalid image format (frame {index})")
        self.index = int(index)


class SessionClosed(KeyError):
    """The session was closed while this submission was still queued."""


class _Session:
    def __init__(self, sid: str, detector: DeepfakeDetector):
        self.sid = sid
        self.detector = detector
        self.last_used = time.monotonic()
        self.pending = 0                  # submissions queued or in a pass
        self.closed = False


def _pixels(item) -> int:
    if isinstance(item, (bytes, bytearray, memoryview)):
        from PIL import Image

        try:
            with Image.open(io.BytesIO(bytes(item))) as im:
                return im.size[0] * im.size[1]
        except Exception:
            return 0                      # unreadable: the library refuses it and the Pillow fallback reports it
    return int(item.shape[0]) * int(item.shape[1])


MAX_FRAME_PIXELS = 1 << 26               # one part decoded by Pillow (backend_server.MAX_FRAME_PIXELS)


def _pillow_bgr(data: bytes):
    """backend_server.decode_image: BGR uint8 (H, W, 3) or None"""
    from PIL import Image

    try:
        with Image.open(io.BytesIO(bytes(data))) as im:
            if im.size[0] * im.size[1] > MAX_FRAME_PIXELS:
                return None
            rgb = np.asarray(im.convert("RGB"))
    except Exception:
        return None
    if rgb.ndim != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        return None
    return np.ascontiguousarray(rgb[:, :, ::-1])


class SessionPool:
    def __init__(self, handle: Optional[Handle] = None, lock=None, detection_threshold: float = 0.55,
                 max_sessions: int = 1024, idle_seconds: float = 300, use_tta: bool = False, num_tta_augmentations: int = 1,
                 forensic_size: Optional[int] = None):
        self._handle = handle
        # analysis size of every session's forensic stream: None = the environment variable DFD_FORENSIC_SIZE (unset:
        # 256x256).  Streams of any sizes share the pass's one library call; an invalid size fails here.
        self.forensic_size = forensic_size_from_env() if forensic_size is None else int(forensic_size)
        if self.forensic_size is not None:
            check_analysis_size((self.forensic_size, self.forensic_size))                       # ValueError for a bad size
        # test-time augmentation for every session: the pass's one library call is armed with the draws of all its frames.
        # Draw order = the order results are applied to sessions: submissions in queue order, a submission's frames in
        # stream order (Python's global `random`, left where that many per-face calls would have left it)
        self.use_tta = bool(use_tta)
        self.num_tta_augmentations = int(num_tta_augmentations)
        self.lock = lock if lock is not None else threading.Lock()
        self.detection_threshold = detection_threshold
        self.max_sessions = int(max_sessions)
        self.idle_seconds = float(idle_seconds)
        self._sessions: "OrderedDict[str, _Session]" = OrderedDict()   # least recently used first
        self._meta = threading.Lock()                                   # the map and the queue (no handle calls)
        self._queue: deque = deque()                                    # (session, items, pixels, future)
        self._wake = threading.Condition(self._meta)
        self._worker: Optional[threading.Thread] = None
        self.passes = 0                   # library calls made by the worker
        self.frames = 0                   # frames they carried

    @property
    def handle(self) -> Handle:
        if self._handle is None:
            from . import runtime

            self._handle = runtime.default_handle()
        return self._handle

    # ------------------------------------------------------------------ sessions
    def _get(self, sid: str, create: bool, evicted: Optional[list] = None) -> Optional[_Session]:
        """under self._meta; a session evicted to make room is appended to `evicted` (released by the caller, outside
        self._meta: the worker takes self.lock before self._meta)"""
        s = self._sessions.get(sid)
        if s is not None:
            self._sessions.move_to_end(sid)
            s.last_used = time.monotonic()
            return s
        if not create:
            return None
        if len(self._sessions) >= self.max_sessions:
            evicted.append(self._evict_one())
        s = _Session(sid, DeepfakeDetector(enable_gradcam=False, use_tta=self.use_tta,
                                           num_tta_augmentations=self.num_tta_augmentations,
                                           request_tta=self.use_tta,
                                           detection_threshold=self.detection_threshold, handle=self.handle,
                                           forensic_size=self.forensic_size))
        self._sessions[sid] = s
        return s

    def _evict_one(self) -> _Session:
        """under self._meta: the least recently used idle session leaves the map, else SessionPoolFull"""
        now = time.monotonic()
        for sid, s in self._sessions.items():
            if s.pending == 0 and now - s.last_used >= self.idle_seconds:
                del self._sessions[sid]
                s.closed = True
                return s
        oldest = next(iter(self._sessions.values()))
        raise SessionPoolFull(max(1, int((self.idle_seconds - (now - oldest.last_used)) * 1000)))

    def __contains__(self, sid: str) -> bool:
        with self._meta:
            return sid in self._sessions

    def __len__(self) -> int:
        with self._meta:
            return len(self._sessions)

    def session_ids(self):
        """least recently used first"""
        with self._meta:
            return list(self._sessions)

    def reset(self, sid: str) -> bool:
        """/reset of one session; False when there is no such session"""
        with self._meta:
            s = self._get(sid, create=False)
        if s is None:
            return False
        with self.lock:
            s.detector.reset()
        return True

    def stats(self, sid: str) -> Optional[dict]:
        """/stats of one session (without 'device'), or None"""
        with self._meta:
            s = self._get(sid, create=False)
        if s is None:
            return None
        with self.lock:
            d, t = s.detector, s.detector.temporal_tracker
            return {'frame_count': d.frame_count, 'temporal_average': float(t.get_temporal_average()),
                    'stability_score': float(t.get_stability_score()), 'confidence_level': t.get_confidence_level(),
                    'history_length': len(t.score_history), 'voting': t.get_voting_stats()}

    def close(self, sid: str) -> bool:
        with self._meta:
            s = self._sessions.pop(sid, None)
        if s is None:
            return False
        s.closed = True
        with self.lock:
            s.detector.release()
        return True

    # ------------------------------------------------------------------ work
    def submit(self, sid: str, items) -> Future:
        """Queue one request of session `sid` (JPEG bytes and / or BGR frames, in stream order).  The future holds the
        list of response dicts `DeepfakeDetector.analyze_request` would return for them.  Raises SessionPoolFull."""
        items = list(items)
        if not items:
            raise ValueError("no frames")
        px = sum(_pixels(it) for it in items)   # header reads here, in the caller's thread: no lock is held
        fut: Future = Future()
        evicted: list = []
        with self._meta:
            s = self._get(sid, create=True, evicted=evicted)
            s.pending += 1
            self._queue.append((s, items, px, fut))
            if self._worker is None:
                self._worker = threading.Thread(target=self._run, name="dfd-session-pool", daemon=True)
                self._worker.start()
            self._wake.notify()
        for old in evicted:                     # idle sessions leave through release(): their device plane is reused
            with self.lock:
                old.detector.release()
        return fut

    def _take(self):
        """under self._meta: whole submissions in queue order, at most MAX_PASS_FRAMES frames and MAX_PASS_PIXELS pixels
        (always at least one)"""
        batch, frames, pixels = [], 0, 0
        while self._queue:
            s, items, px, fut = self._queue[0]
            if batch and (frames + len(items) > MAX_PASS_FRAMES or pixels + px > MAX_PASS_PIXELS):
                break
            self._queue.popleft()
            batch.append((s, items, fut))
            frames += len(items)
            pixels += px
        return batch

    def _run(self):
        while True:
            with self._meta:
                while not self._queue:
                    self._wake.wait()
            with self.lock:                     # what queued while the handle was busy goes into this pass
                with self._meta:
                    batch = self._take()
                try:
                    self._pass(batch)
                except BaseException as e:      # noqa: BLE001  (handed to every waiting request)
                    for _, _, fut in batch:
                        if not fut.done():
                            fut.set_exception(e)
                finally:
                    with self._meta:
                        for s, _, _ in batch:
                            s.pending -= 1
                            s.last_used = time.monotonic()

    def _pass(self, batch):
        """one analyze_streams_batch call over `batch`, then every session's votes in submission order (under self.lock)"""
        live = []
        for s, items, fut in batch:
            if s.closed:
                fut.set_exception(SessionClosed(s.sid))
            elif fut.set_running_or_notify_cancel():
                live.append([s, list(items), fut])
        while live:
            flat, ids, full = [], [], []
            offset = {}                         # session -> frames of it earlier in this pass
            for s, items, _ in live:
                d = s.detector
                d._open_stream()                # under self.lock: building the session (submit's thread) made no library call
                k = offset.get(s, 0)
                for i, it in enumerate(items):
                    flat.append(it)
                    ids.append(d.frame_analyzer.stream_id)
                    full.append((d.frame_count + k + i) % d.full_forensic_interval == 0)
                offset[s] = k + len(items)
            copies = self.num_tta_augmentations - 1 if self.use_tta and self.num_tta_augmentations > 1 else 0
            try:
                if copies > 0:
                    state, draws = tta_draw_table(len(flat), copies)     # max_faces = 1: at most one face per frame
                    res = None
                    try:
                        res = self.handle.analyze_streams_batch(flat, ids, full, confidence_threshold=0.5, max_faces=1,
                                                                tta=(copies, draws))
                    finally:                                             # a refused call used no draw
                        tta_commit_draws(state, 0 if res is None else sum(len(r[2]) for r in res), copies)
                else:
                    res = self.handle.analyze_streams_batch(flat, ids, full, confidence_threshold=0.5, max_faces=1)
            except DfdError as e:
                # a refusal of one part (its headers, or its scan while decoding), raised before any stream state has
                # moved: that part is decoded with Pillow (as the server does for /analyze) or its submission alone fails,
                # and the call is made again - never a retry of a failed GPU step.  Anything else (no part to blame) is
                # raised to every submission of the pass.
                bad = getattr(e, 'bad_index', -1)
                if e.code not in (-7, -1) or bad < 0:
                    raise
                pos = 0
                for j, (s, items, fut) in enumerate(live):
                    if bad < pos + len(items):
                        k = bad - pos
                        frame = _pillow_bgr(items[k]) if isinstance(items[k], (bytes, bytearray, memoryview)) else None
                        if frame is None:
                            fut.set_exception(InvalidFrame(k))
                            del live[j]
                        else:
                            items[k] = frame
                        break
                    pos += len(items)
                continue
            self.passes += 1
            self.frames += len(flat)
            pos = 0
            done = {}                           # session -> frames of it replayed so far
            for s, items, fut in live:
                d = s.detector
                n_s = offset[s]
                first_number = d.frame_analyzer.frame_count - n_s + 1 + done.get(s, 0)
                out = []
                for i in range(len(items)):
                    scores, fprob, faces, logits, n_detected, shape = res[pos + i]
                    small = shape[0] < 30 or shape[1] < 30
                    d.last_frame_forensic_result = {'scores': scores, 'fake_probability': fprob,
                                                    'analysis_type': 'frame_forensic' if full[pos + i] else 'frame_forensic_fast',
                                                    'frame_number': first_number + i}
                    out.append(d._request_response(fprob, [] if small else faces, logits, 0 if small else n_detected))
                done[s] = done.get(s, 0) + len(items)
                pos += len(items)
                fut.set_result(out)
            return

"""CPU: the fixtures of tests/test_forensic_sized_fused_gpu.py sit away from every threshold of the reference at the
sizes that test compares scores at (so a statistic within its bar cannot flip a score), and the Python surface of the
sized detector refuses bad sizes without a GPU."""
import io

import numpy as np
import pytest
from PIL import Image

import forensic_fused_frames as X
import forensic_sized_oracle as Z
from oracle.forensics_ref import ForensicsRef


def _assert_margin(stats, what):
    rel, cnt = Z.margin(stats)
    assert rel >= 10 * Z.STAT_RTOL and cnt >= 1, (what, rel, cnt, stats)


@pytest.mark.parametrize("S", X.SIZES)
def test_moving_sequence_sits_away_from_every_threshold(S):
    ref = ForensicsRef((S, S))
    for i, (f, full) in enumerate(zip(X.moving(), X.PATTERN)):
        (ref.analyze if full else ref.analyze_fast)(f)
        _assert_margin(ref.stats, (S, i))


def test_decoded_jpeg_sequence_sits_away_from_every_threshold():
    """the frames of the fused JPEG test as libjpeg decodes them (the device decoder is bit-identical to it)"""
    ref = ForensicsRef((80, 80))
    for i, (f, full) in enumerate(zip(X.moving(), X.PATTERN)):
        dec = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(X.jpeg(f))).convert("RGB"))[..., ::-1])
        assert dec.shape == f.shape
        (ref.analyze if full else ref.analyze_fast)(dec)
        _assert_margin(ref.stats, ("jpeg", i))


def test_sources_and_streams():
    assert {f.shape[:2] for k in range(5) for f in X.stream_frames(k, 3)} == set(X.SOURCES)
    a, b = X.stream_frames(3, 2)
    assert a.shape != b.shape or (a != b).any()
    assert all(f.dtype == np.uint8 and f.shape[2] == 3 for f in X.moving())


def test_forensic_size_surface_without_a_gpu(monkeypatch):
    import rtdfd_amd

    DeepfakeDetector = rtdfd_amd.deepfake_detection.DeepfakeDetector             # (attribute access: one copy of the modules)
    forensic_size_from_env = rtdfd_amd.deepfake_detection.forensic_size_from_env

    monkeypatch.delenv("DFD_FORENSIC_SIZE", raising=False)
    assert forensic_size_from_env() is None
    monkeypatch.setenv("DFD_FORENSIC_SIZE", " 512 ")
    assert forensic_size_from_env() == 512
    d = DeepfakeDetector(use_tta=False, forensic_size=512)
    assert d.frame_analyzer.analysis_size == (512, 512) and d.frame_analyzer.any_size and d.frame_analyzer.sized
    assert DeepfakeDetector(use_tta=False).frame_analyzer.analysis_size == (256, 256)
    assert not DeepfakeDetector(use_tta=False, forensic_size=256).frame_analyzer.sized
    for bad in (100, 16, 2048):
        with pytest.raises(ValueError, match="multiple of 16"):
            DeepfakeDetector(use_tta=False, forensic_size=bad)
        monkeypatch.setenv("DFD_FORENSIC_SIZE", str(bad))
        with pytest.raises(ValueError, match="multiple of 16"):
            rtdfd_amd.sessions.SessionPool()
    monkeypatch.setenv("DFD_FORENSIC_SIZE", "large")
    with pytest.raises(ValueError, match="multiple of 16"):
        forensic_size_from_env()
    monkeypatch.setenv("DFD_FORENSIC_SIZE", "128")
    assert rtdfd_amd.sessions.SessionPool().forensic_size == 128
    assert rtdfd_amd.sessions.SessionPool(forensic_size=64).forensic_size == 64


class _LockCheckingStub:
    """stands in for the handle of a session pool: every call must come while the pool's lock is held"""

    has_detector, has_haar = True, False

    def __init__(self, lock):
        self.lock, self.opened, self.violations, self.counts = lock, [], [], {}

    def _check(self, what):
        if not self.lock.locked():
            self.violations.append(what)

    def forensics_open(self, stream_id, size):
        self._check("forensics_open")
        self.opened.append((stream_id, size))

    def forensics_state(self, stream_id=0):
        self._check("forensics_state")
        return self.counts.get(stream_id, 0), 0, stream_id in self.counts

    def forensics_release(self, stream_id):
        self._check("forensics_release")

    def analyze_streams_batch(self, items, stream_ids, full_flags, **kw):
        self._check("analyze_streams_batch")
        out = []
        for it, sid in zip(items, stream_ids):
            self.counts[sid] = self.counts.get(sid, 0) + 1
            out.append(({'frequency': 0.1, 'temporal': 0.0, 'edge': 0.2}, 0.25, [], np.zeros(0, np.float32), 0, it.shape[:2]))
        return out


def test_building_a_sized_session_makes_no_library_call():
    """a session is built in the submitting thread, which does not hold the pool's lock: its stream is opened by the
    worker inside the pass"""
    import threading

    import rtdfd_amd

    lock = threading.Lock()
    stub = _LockCheckingStub(lock)
    pool = rtdfd_amd.sessions.SessionPool(handle=stub, lock=lock, forensic_size=80)
    f = np.zeros((40, 40, 3), np.uint8)
    futs = [pool.submit(f"s{i}", [f]) for i in range(4)]           # the worker runs freely meanwhile
    futs += [pool.submit("s0", [f, f])]
    assert [len(fu.result(timeout=10)) for fu in futs] == [1, 1, 1, 1, 2]
    assert stub.violations == []
    assert len({sid for sid, _ in stub.opened}) == 4 and {size for _, size in stub.opened} == {80}
    d = rtdfd_amd.deepfake_detection.DeepfakeDetector(use_tta=False, handle=stub, forensic_size=80)
    assert len({sid for sid, _ in stub.opened}) == 4               # ... nor does building a detector
    for i in range(4):
        pool.close(f"s{i}")
    assert stub.violations == [] and d.frame_analyzer.sized

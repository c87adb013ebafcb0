"""CPU: the session surface of the server and the session pool, against a stub handle (no GPU).

The stub stands in for `Handle.analyze_streams_batch`: it records every call, keeps a frame counter per stream id and
returns frames without faces, so the pool's scheduling, the routes' validation, limiters and status codes are checked
without the library."""
import io
import threading
import time

import numpy as np
import pytest
from PIL import Image


class StubHandle:
    def __init__(self):
        self.calls = []                  # (stream ids, full flags) per analyze_streams_batch call
        self.counts = {}
        self.released = []
        self.reset_ids = []

    def analyze_streams_batch(self, items, stream_ids, full_flags, confidence_threshold=0.5, max_faces=1, apply_clahe=True):
        self.calls.append((list(stream_ids), list(full_flags)))
        out = []
        for it, sid in zip(items, stream_ids):
            self.counts[sid] = self.counts.get(sid, 0) + 1
            shape = it.shape[:2] if isinstance(it, np.ndarray) else (405, 720)
            out.append(({'frequency': 0.1, 'temporal': 0.0, 'edge': 0.2}, 0.25, [], np.zeros(0, np.float32), 0, shape))
        return out

    def forensics_state(self, stream_id=0):
        return self.counts.get(stream_id, 0), 0, stream_id in self.counts

    def forensics_reset(self, stream_id=0):
        self.reset_ids.append(stream_id)
        self.counts.pop(stream_id, None)

    def forensics_release(self, stream_id):
        self.released.append(stream_id)
        self.counts.pop(stream_id, None)


def _png(h=40, w=48):
    buf = io.BytesIO()
    Image.fromarray(np.full((h, w, 3), 90, np.uint8)).save(buf, format="PNG")
    return buf.getvalue()


@pytest.fixture()
def srv(pkg, monkeypatch):
    s = pkg.backend_server
    s.app.config["TESTING"] = True
    stub = StubHandle()
    monkeypatch.setattr(s, "_session_pool", pkg.sessions.SessionPool(handle=stub, lock=s._detector_lock))
    monkeypatch.setattr(s, "_session_last", {})
    s._last_request_time = 0.0
    s.stub = stub
    yield s
    s._last_request_time = 0.0


def _post(client, payload, session=None, route="/analyze"):
    url = route if session is None else f"{route}?session={session}"
    return client.post(url, data={"frame": (io.BytesIO(payload), "f.png")}, content_type="multipart/form-data")


def test_session_id_is_validated(srv):
    with srv.app.test_client() as c:
        for bad in ("has space", "x" * 65, "semi;colon", ""):
            r = _post(c, _png(), session=bad)
            assert r.status_code == 400 and "error" in r.get_json(), bad
            assert c.get("/stats", query_string={"session": bad}).status_code == 400
            assert c.post("/reset", query_string={"session": bad}).status_code == 400
        assert _post(c, _png(), session="A-z_09" + "x" * 58).status_code == 200         # 64 characters


def test_session_limiters_are_independent_of_each_other_and_of_the_global_one(srv):
    with srv.app.test_client() as c:
        assert _post(c, b"junk", session="a").status_code == 400
        assert _post(c, b"junk", session="b").status_code == 400                       # not 429: its own limiter
        assert _post(c, b"junk").status_code == 400                                    # the global one is untouched
        r = _post(c, b"junk", session="a")                                              # < 100 ms after a's first
        assert r.status_code == 429
        body = r.get_json()
        assert body["error"] == "Rate limited" and 0 <= body["retry_after_ms"] <= 100
        assert _post(c, b"junk").status_code == 429                                    # global limiter as before


def test_session_routes_stats_reset_and_responses(srv, pkg):
    with srv.app.test_client() as c:
        assert c.get("/stats?session=nobody").status_code == 404
        assert "error" in c.get("/stats?session=nobody").get_json()
        before = srv.detector.frame_count
        r = _post(c, _png(), session="s1")
        assert r.status_code == 200, r.get_data()
        b = r.get_json()
        want_keys = ['success', 'analysis_mode', 'faces_detected', 'fake_probability', 'frame_forensic_probability',
                     'real_probability', 'confidence_level', 'temporal_average', 'stability_score', 'frame_count',
                     'processing_time_ms']
        assert set(b) == set(want_keys) and b["frame_count"] == 1 and b["analysis_mode"] == "frame_only"
        s = c.get("/stats?session=s1").get_json()
        assert s["frame_count"] == 1 and s["history_length"] == 1 and s["voting"]["total_frames"] == 1 and "device" in s
        assert srv.detector.frame_count == before                                      # session traffic stays out of it
        time.sleep(0.11)
        r = c.post("/analyze_batch?session=s1", data={"frame": [(io.BytesIO(_png(40, 48)), "a.png"), (io.BytesIO(_png(64, 32)), "b.png")]},
                   content_type="multipart/form-data")
        assert r.status_code == 200, r.get_data()
        res = r.get_json()["results"]
        assert [x["frame_count"] for x in res] == [2, 3]                                # frames of two sizes in one request
        assert c.post("/reset?session=s1").status_code == 200
        assert c.get("/stats?session=s1").get_json()["frame_count"] == 0
        assert c.post("/reset?session=unknown").status_code == 200


def test_full_pool_answers_503(srv, pkg, monkeypatch):
    pool = pkg.sessions.SessionPool(handle=srv.stub, lock=srv._detector_lock, max_sessions=1, idle_seconds=60)
    monkeypatch.setattr(srv, "_session_pool", pool)
    pool.submit("busy", [np.zeros((40, 40, 3), np.uint8)]).result(timeout=10)
    with srv.app.test_client() as c:
        r = _post(c, _png(), session="other")
        assert r.status_code == 503
        body = r.get_json()
        assert set(body) == {"error", "retry_after_ms"} and 0 < body["retry_after_ms"] <= 60_000
    assert pool.session_ids() == ["busy"]


def test_idle_sessions_are_evicted_least_recently_used_first(pkg):
    stub = StubHandle()
    pool = pkg.sessions.SessionPool(handle=stub, max_sessions=2, idle_seconds=0)
    frame = np.zeros((40, 40, 3), np.uint8)
    pool.submit("a", [frame]).result(timeout=10)
    pool.submit("b", [frame]).result(timeout=10)
    sid_a = pool._sessions["a"].detector.frame_analyzer.stream_id
    sid_b = pool._sessions["b"].detector.frame_analyzer.stream_id
    assert pool.stats("a")["frame_count"] == 1                                          # touches a: b is now the oldest
    pool.submit("c", [frame]).result(timeout=10)
    assert pool.session_ids() == ["a", "c"] and stub.released == [sid_b]
    pool.submit("d", [frame]).result(timeout=10)
    assert pool.session_ids() == ["c", "d"] and stub.released == [sid_b, sid_a]
    assert pool.stats("b") is None
    assert pool.close("c") and not pool.close("c") and pool.session_ids() == ["d"]


def test_worker_drains_the_queue_in_submission_order_in_one_pass(pkg):
    stub = StubHandle()
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=stub, lock=lock)
    f = np.zeros((40, 40, 3), np.uint8)
    with lock:                                    # the handle is busy: everything below queues for the next pass
        futs = [pool.submit("s1", [f, f]), pool.submit("s2", [f]), pool.submit("s1", [f]), pool.submit("s3", [f, f, f])]
        ids = {k: pool._sessions[k].detector.frame_analyzer.stream_id for k in ("s1", "s2", "s3")}
    res = [fu.result(timeout=10) for fu in futs]
    assert pool.passes == 1 and len(stub.calls) == 1
    sids, full = stub.calls[0]
    assert sids == [ids["s1"], ids["s1"], ids["s2"], ids["s1"], ids["s3"], ids["s3"], ids["s3"]]
    assert full == [True, False, True, False, True, False, False]                      # each session's own schedule
    assert [r["frame_count"] for r in res[0]] == [1, 2] and [r["frame_count"] for r in res[2]] == [3]
    assert [r["frame_count"] for r in res[1]] == [1] and [r["frame_count"] for r in res[3]] == [1, 2, 3]
    assert pool.stats("s1")["frame_count"] == 3


class RefusingStub(StubHandle):
    """refuses (like the library does for a scan that is cut off) every part equal to `bad`, with its index"""

    def __init__(self, bad):
        super().__init__()
        self.bad = bad

    def analyze_streams_batch(self, items, stream_ids, full_flags, **kw):
        for i, it in enumerate(items):
            if isinstance(it, bytes) and it == self.bad:
                from rtdfd_amd import _lib

                e = _lib.DfdError(-1, "decode_jpeg: corrupt or truncated entropy-coded data")
                e.bad_index = i
                raise e
        return super().analyze_streams_batch(items, stream_ids, full_flags, **kw)


def test_a_part_that_does_not_decode_fails_only_its_own_request(pkg):
    bad = b"\xff\xd8 not really a jpeg"
    stub = RefusingStub(bad)
    lock = threading.Lock()
    pool = pkg.sessions.SessionPool(handle=stub, lock=lock)
    f = np.zeros((40, 40, 3), np.uint8)
    with lock:
        futs = [pool.submit("a", [f]), pool.submit("b", [f, bad]), pool.submit("c", [f, f]), pool.submit("b", [f])]
    assert [r["frame_count"] for r in futs[0].result(timeout=10)] == [1]
    with pytest.raises(pkg.sessions.InvalidFrame) as e:
        futs[1].result(timeout=10)
    assert e.value.index == 1
    assert [r["frame_count"] for r in futs[2].result(timeout=10)] == [1, 2]
    assert [r["frame_count"] for r in futs[3].result(timeout=10)] == [1]              # b's refused request moved nothing
    assert pool.passes == 1 and len(stub.calls) == 1                                   # the call made again without it


def test_routes_answer_400_for_undecodable_parts_and_410_for_closed_sessions(srv, pkg, monkeypatch):
    bad = b"\xff\xd8 not really a jpeg"
    stub = RefusingStub(bad)
    monkeypatch.setattr(srv, "_session_pool", pkg.sessions.SessionPool(handle=stub, lock=srv._detector_lock))
    monkeypatch.setattr(srv, "image_size", lambda data: (40, 40))                       # headers that read fine
    with srv.app.test_client() as c:
        r = _post(c, bad, session="x")
        assert r.status_code == 400 and r.get_json() == {"error": "Invalid image format"}
    pool = srv._session_pool
    f = np.zeros((40, 40, 3), np.uint8)
    with srv._detector_lock:
        fu = pool.submit("gone", [f])
        pool._sessions["gone"].closed = True                                            # closed while queued
    with pytest.raises(pkg.sessions.SessionClosed):
        fu.result(timeout=10)
    monkeypatch.setattr(pool, "submit", lambda sid, items: fu)
    with srv.app.test_client() as c:
        r = _post(c, _png(), session="gone")
        assert r.status_code == 410 and "error" in r.get_json()

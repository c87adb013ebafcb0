"""Serving capacity with sessions: S concurrent sessions each posting 720x405 JPEGs (the extension's size for 16:9 video)
through `sessions.SessionPool` (one batched device pass per drain of the queue), against the session-less loop that
serves the same requests one at a time (`DeepfakeDetector.analyze_request`, one library call each).

One JSON line per run: S = 1, 8, 32, 64, plus one mixed-size run (720x405, 720x540, 405x720).  Every session is a client
thread that posts its next frame as soon as the previous answer arrived (closed loop, no think time).  Host clock around
synchronised work (every call returns after its last stream wait); every shape is warmed up first.

    python profiles/sessions_probe.py [--frames 24]
"""
import argparse
import io
import json
import os
import sys
import threading
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frames as F  # noqa: E402
import rtdfd_amd  # noqa: E402


def _jpeg(fr):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(fr[..., ::-1])).save(buf, format="JPEG", quality=85)
    return buf.getvalue()


def _payloads(S, n, sizes):
    return [[_jpeg(F.natural_like(*sizes[(s + t) % len(sizes)], seed=1000 * s + t)) for t in range(n)] for s in range(S)]


def run_pool(h, work):
    pool = rtdfd_amd.sessions.SessionPool(handle=h)
    lat = []
    lk = threading.Lock()

    def client(s):
        for p in work[s]:
            t = time.perf_counter()
            pool.submit(f"p{s}", [p]).result()
            with lk:
                lat.append(time.perf_counter() - t)

    passes0, frames0 = pool.passes, pool.frames
    t0 = time.perf_counter()
    th = [threading.Thread(target=client, args=(s,)) for s in range(len(work))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    wall = time.perf_counter() - t0
    for s in range(len(work)):
        pool.close(f"p{s}")
    return wall, lat, (pool.frames - frames0) / max(1, pool.passes - passes0)


def run_loop(h, work):
    """session-less: the same requests, one at a time (round robin over the sessions, one detector each)"""
    D = rtdfd_amd.deepfake_detection.DeepfakeDetector
    dets = [D(use_tta=False, num_tta_augmentations=1, detection_threshold=0.55, handle=h) for _ in work]
    lat = []
    t0 = time.perf_counter()
    for t in range(len(work[0])):
        for s, d in enumerate(dets):
            a = time.perf_counter()
            d.analyze_request(jpeg=work[s][t])
            lat.append(time.perf_counter() - a)
    wall = time.perf_counter() - t0
    for d in dets:
        d.release()
    return wall, lat


def _ms(v, q):
    return round(float(np.percentile(np.array(v) * 1e3, q)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames per session")
    args = ap.parse_args()
    W = rtdfd_amd.weights
    blob = W.pack_all(W.seeded_state_dict(0), W.seeded_ssd_state_dict(0))
    h = rtdfd_amd._lib.Handle(blob, device=0, max_batch=64)
    runs = [(S, [(405, 720)]) for S in (1, 8, 32, 64)] + [(32, [(405, 720), (540, 720), (720, 405)])]
    for S, sizes in runs:
        work = _payloads(S, args.frames, sizes)
        run_pool(h, [w[:2] for w in work])                      # warm-up: every shape and pass size met below
        run_loop(h, [w[:2] for w in work])
        wall, lat, per_pass = run_pool(h, work)
        lwall, llat = run_loop(h, work)
        n = S * args.frames
        print(json.dumps({"sessions": S, "sizes": ["x".join(map(str, s[::-1])) for s in sizes], "frames": n,
                          "pool": {"frames_per_s": round(n / wall, 1), "p50_ms": _ms(lat, 50), "p99_ms": _ms(lat, 99),
                                   "frames_per_pass": round(per_pass, 2)},
                          "one_at_a_time": {"frames_per_s": round(n / lwall, 1), "p50_ms": _ms(llat, 50), "p99_ms": _ms(llat, 99)},
                          "speedup": round(lwall / wall, 2)}), flush=True)
    h.close()


if __name__ == "__main__":
    main()

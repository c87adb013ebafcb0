"""Serving capacity of sized forensic streams: N concurrent sessions each posting 720x405 JPEGs through
`sessions.SessionPool` built at forensic analysis size S (one batched device pass per drain of the queue, the general
forensic chain grouped and chunked inside it), against the same requests served one at a time

  * through the separate entries a sized analyzer needed before the fused entries took sized streams: device JPEG decode
    to the host, `forensics_sized`, `detect_faces`, `classify_crops` on the first box (four library calls, three uploads
    of the frame), and
  * through the fused single-frame entry (`DeepfakeDetector(forensic_size=S).analyze_request(jpeg=...)`, one call).

One JSON line per (S, N): S = 128, 512 and N = 16, 64.  Every session is a client thread that posts its next frame as soon
as the previous answer arrived (closed loop, no think time).  Host clock around synchronised work (every call returns
after its last stream wait).  Every shape is warmed up first; the three routes are timed in turn, `--repeats` times, and
the median rate is reported with the lowest and highest of the repeats.

    python profiles/forensic_sized_pool_probe.py [--frames 24] [--repeats 3]
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


def run_pool(h, work, size):
    pool = rtdfd_amd.sessions.SessionPool(handle=h, forensic_size=size)
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


def _detectors(h, n, size):
    D = rtdfd_amd.deepfake_detection.DeepfakeDetector
    return [D(use_tta=False, num_tta_augmentations=1, detection_threshold=0.55, handle=h, forensic_size=size) for _ in range(n)]


def run_separate(h, work, size):
    """one at a time, the separate entries (round robin over the sessions, one detector's votes and stream each)"""
    dets = _detectors(h, len(work), size)
    lat = []
    t0 = time.perf_counter()
    for t in range(len(work[0])):
        for s, d in enumerate(dets):
            a = time.perf_counter()
            frame = h.decode_jpeg(work[s][t])
            full = d.frame_count % d.full_forensic_interval == 0
            _, prob, _ = h.forensics_sized(frame, size, full=full, stream_id=d.frame_analyzer.stream_id)
            boxes = h.detect_faces(frame, confidence_threshold=0.5)
            logits = h.classify_crops(frame, boxes[:1], apply_clahe=True)[:, 0] if boxes else []
            d._request_response(prob, boxes[:1], logits, len(boxes))
            lat.append(time.perf_counter() - a)
    wall = time.perf_counter() - t0
    for d in dets:
        d.release()
    return wall, lat


def run_fused(h, work, size):
    """one at a time, the fused single-frame entry"""
    dets = _detectors(h, len(work), size)
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


def _rate(n, walls):
    r = sorted(n / w for w in walls)
    return {"frames_per_s": round(r[len(r) // 2], 1), "low": round(r[0], 1), "high": round(r[-1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames per session")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--sessions", type=int, nargs="+", default=[16, 64])
    args = ap.parse_args()
    W = rtdfd_amd.weights
    blob = W.pack_all(W.seeded_state_dict(0), W.seeded_ssd_state_dict(0))
    h = rtdfd_amd._lib.Handle(blob, device=0, max_batch=64)
    payloads = [[_jpeg(F.natural_like(405, 720, seed=1000 * s + t)) for t in range(args.frames)] for s in range(max(args.sessions))]
    for size in args.sizes:
        for N in args.sessions:
            work = payloads[:N]
            warm = [w[:2] for w in work]                            # every shape and pass size met below
            run_pool(h, warm, size), run_separate(h, warm, size), run_fused(h, warm, size)
            pw, sw, fw, plat, slat, flat, per_pass = [], [], [], [], [], [], []
            for _ in range(args.repeats):                          # the routes in turn: drift hits all three alike
                w, lat, pp = run_pool(h, work, size)
                pw.append(w), plat.extend(lat), per_pass.append(pp)
                w, lat = run_separate(h, work, size)
                sw.append(w), slat.extend(lat)
                w, lat = run_fused(h, work, size)
                fw.append(w), flat.extend(lat)
            n = N * args.frames
            pool, sep, fused = _rate(n, pw), _rate(n, sw), _rate(n, fw)
            pool.update(p50_ms=_ms(plat, 50), p99_ms=_ms(plat, 99), frames_per_pass=round(float(np.mean(per_pass)), 2))
            sep.update(p50_ms=_ms(slat, 50), p99_ms=_ms(slat, 99))
            fused.update(p50_ms=_ms(flat, 50), p99_ms=_ms(flat, 99))
            print(json.dumps({"forensic_size": size, "sessions": N, "frames": n, "repeats": args.repeats, "pool": pool,
                              "one_at_a_time_separate_entries": sep, "one_at_a_time_fused": fused,
                              "pool_over_separate": round(pool["frames_per_s"] / sep["frames_per_s"], 2)}), flush=True)
    h.close()


if __name__ == "__main__":
    main()

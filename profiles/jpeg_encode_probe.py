"""Device JPEG encode against Pillow on 16 host threads.

Two workloads: 64 x 1080p natural-texture frames at q90 4:2:0, and 256 x 160 x 160 crops at q75.  Each is timed
  device: pixels resident in HBM -> JPEG bytes on the host (Handle.encode_jpegs_device, wall clock around the call), and
  host:   the raw D2H of the same pixels plus Pillow's encode of them on a pool of 16 threads.
Warm-up calls first, then the median and the spread of `--repeats` timed calls.  Prints one JSON line.

    python profiles/jpeg_encode_probe.py [--repeats 7] [--small]
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def _pillow(args):
    from PIL import Image

    bgr, q = args
    buf = io.BytesIO()
    Image.fromarray(bgr[..., ::-1]).save(buf, format="JPEG", quality=q, subsampling=2, optimize=False)
    return buf.getvalue()


def _timed(fn, warm, repeats):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="8 frames / 32 crops (a quick check of the probe itself)")
    a = ap.parse_args()
    import frames
    import rtdfd_amd

    h = rtdfd_amd._lib.Handle(rtdfd_amd.weights.pack_b0(rtdfd_amd.weights.seeded_state_dict(0)), device=0, max_batch=1)
    pool = ThreadPoolExecutor(16)
    out = {}
    for name, n, hh, ww, q in (("1080p_q90", 8 if a.small else 64, 1080, 1920, 90), ("crops160_q75", 32 if a.small else 256, 160, 160, 75)):
        distinct = [frames.natural_like(hh, ww, seed=s) for s in range(4)]
        imgs = [distinct[i % 4] for i in range(n)]
        buf = h.alloc(n * hh * ww * 3).upload(np.stack(imgs))
        srcs = [(buf.ptr + i * hh * ww * 3, hh, ww, ww * 3, 3) for i in range(n)]
        files = h.encode_jpegs_device(srcs, quality=q)
        want = list(pool.map(_pillow, [(im, q) for im in distinct]))
        assert all(files[i] == want[i % 4] for i in range(n)), "device bytes differ from Pillow's"

        def host():
            raw = buf.download((n, hh, ww, 3), np.uint8)
            return list(pool.map(_pillow, [(raw[i], q) for i in range(n)]))

        out[name] = {"images": n, "jpeg_bytes_per_image": int(np.mean([len(f) for f in files])),
                     "device": _timed(lambda: h.encode_jpegs_device(srcs, quality=q), 3, a.repeats),
                     "pillow16_plus_d2h": _timed(host, 1, max(3, a.repeats // 2))}
        buf.free()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

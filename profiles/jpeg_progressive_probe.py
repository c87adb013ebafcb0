"""Frames per second from PROGRESSIVE JPEG bytes: natural-texture frames (tests/frames.natural_like, as
profiles/jpeg_gpu_probe.py makes them) at 720 x 405 and 1920 x 1080, quality 85, 4:2:0, in batches of 1, 32 and 256, three
ways:

  (a) pillow   what the server did before option "jpeg_progressive": Pillow decodes each file on one host thread, the raw
               BGR frames are uploaded (dfd_memcpy_h2d into a device buffer, as the analysing entries upload a frame);
  (b) host     dfd_decode_jpeg_batch with "jpeg_progressive" = 1: the scans on the host pool, coefficients uploaded;
  (c) device   the same call with "jpeg_device_progressive" = 1: the bytes cross, the scans run on the device.

Every way ends with the decoded frames in device memory and the stream idle.  Per cell: 2 warm-up calls, then JP_REPEATS
(default 5) timed calls, wall clock around the call; the row holds the median and the min - max spread.  The frames of (b)
and (c) are checked against Pillow's once before timing.  Writes profiles/jpeg_progressive.json and prints the rows as a
markdown table.  env: JP_SIZES ("720x405,1920x1080"), JP_BATCHES ("1,32,256"), JP_REPEATS."""
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from PIL import Image

import frames as F
import rtdfd_amd

L = rtdfd_amd._lib
W = rtdfd_amd.weights
sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("JP_SIZES", "720x405,1920x1080").split(",")]
batches = [int(b) for b in os.environ.get("JP_BATCHES", "1,32,256").split(",")]
repeats = int(os.environ.get("JP_REPEATS", "5"))
h = L.Handle(W.pack_b0(W.seeded_state_dict(0)), device=0, max_batch=8)
h.set_option("jpeg_progressive", 1)


def pillow_bgr(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def timed(call):
    for _ in range(2):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


rows = []
for width, height in sizes:
    files = []
    for i in range(8):
        fr = F.natural_like(height, width, seed=9 + i)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(fr[..., ::-1])).save(buf, format="JPEG", quality=85, subsampling=2, progressive=True)
        files.append(buf.getvalue())
    want = [pillow_bgr(f) for f in files]
    for device in (0, 1):
        h.set_option("jpeg_device_progressive", device)
        got = h.decode_jpeg_batch(files)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), ("frames differ from Pillow's", width, height, device)
    for n in batches:
        datas = [files[i % len(files)] for i in range(n)]
        dev = L.DeviceBuffer(h, n * height * width * 3)

        def pillow_route():
            frames = np.stack([pillow_bgr(d) for d in datas])
            dev.upload(frames)
            h.sync()

        # one library call takes at most 2^27 pixels: a larger batch goes in as few calls as that allows
        per_call = max(1, min(n, (1 << 27) // (width * height)))
        bufs = [(C.c_char * len(d)).from_buffer_copy(d) for d in datas]
        calls = []
        for first in range(0, n, per_call):
            part = bufs[first:first + per_call]
            calls.append((len(part), (C.c_void_p * len(part))(*[C.addressof(b) for b in part]), (C.c_size_t * len(part))(*[len(b) for b in part])))
        hh, ww = C.c_int(), C.c_int()

        def library(device):
            def call():                                             # bgr_out = NULL: the frames stay on the device
                h.set_option("jpeg_device_progressive", device)
                for k, ptrs, lens in calls:
                    h._check(h._lib.dfd_decode_jpeg_batch(h._p, k, ptrs, lens, None, 0, C.byref(hh), C.byref(ww)))
            return call

        cells = {"pillow": timed(pillow_route), "host": timed(library(0)), "device": timed(library(1))}
        dev.free()
        row = {"width": width, "height": height, "batch": n, "bytes_per_file": int(np.mean([len(d) for d in datas])), "repeats": repeats,
               "library_calls": len(calls)}
        for k, (med, lo, hi) in cells.items():
            row[k] = {"median_ms": round(med * 1e3, 3), "min_ms": round(lo * 1e3, 3), "max_ms": round(hi * 1e3, 3), "frames_per_s": round(n / med, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(os.path.join(ROOT, "profiles", "jpeg_progressive.json"), "w") as f:
            json.dump({"gpu": "MI355X", "quality": 85, "subsampling": "4:2:0", "frames": "tests/frames.natural_like", "rows": rows}, f, indent=1)

print("\n| frames | batch | (a) Pillow + upload | (b) host pool | (c) device |\n|---|---|---|---|---|")
for r in rows:
    cell = lambda c: f"{c['frames_per_s']:.0f} frames/s, {c['median_ms']:.2f} ms ({c['min_ms']:.2f} - {c['max_ms']:.2f})"
    print(f"| {r['width']} x {r['height']} ({r['bytes_per_file'] // 1024} KB) | {r['batch']} | {cell(r['pillow'])} | {cell(r['host'])} | {cell(r['device'])} |")

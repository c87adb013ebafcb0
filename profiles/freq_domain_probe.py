"""Milliseconds per call of the any-size frequency-domain path (csrc/freq_domain.hip).

  - `frequency_domain` on a resident 1080p BGR frame (`dfd_frequency_domain_device`: gather, two DFT passes, the sums and
    the 16 n-byte read-back; no frame upload) for 1, 4 and 64 boxes of 96 x 96 and of 300 x 260 (w x h), at seeded
    positions;
  - `frequency_features` at 224 on a 640 x 480 frame through the 224 entry (`dfd_frequency_features`, the VALU kernels of
    freq_kernels.hip) and through the any-size entry (`dfd_frequency_features_sized`), upload and read-back included.

Each call is timed between HIP events on the handle's stream; the calls are alternated after three warm-up calls each
and the median of `--steps` is reported.  One JSON line per measurement.
    python profiles/freq_domain_probe.py [--steps 30]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtdfd_amd  # noqa: E402

H, W = 1080, 1920
BOX_SIZES = ((96, 96), (300, 260))
COUNTS = (1, 4, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    wt = rtdfd_amd.weights
    h = rtdfd_amd._lib.Handle(wt.pack_all(wt.seeded_state_dict(0), wt.seeded_ssd_state_dict(0)), device=0, max_batch=1)
    rs = np.random.RandomState(1)
    frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    small = rs.randint(0, 256, (480, 640, 3)).astype(np.uint8)
    buf = rtdfd_amd._lib.DeviceBuffer(h, frame.nbytes).upload(frame)
    calls = {}
    for bw, bh in BOX_SIZES:
        for n in COUNTS:
            boxes = [(int(rs.randint(0, W - bw + 1)), int(rs.randint(0, H - bh + 1)), bw, bh) for _ in range(n)]
            calls[f"frequency_domain_{n}x_{bw}x{bh}"] = lambda b=boxes: h.frequency_domain_device(buf.ptr, H, W, frame.strides[0], 3, b)
    calls["frequency_features_224_own_kernels"] = lambda: h.frequency_features(small)
    calls["frequency_features_224_any_size"] = lambda: h.frequency_features(small, 224, sized=True)
    for f in calls.values():
        for _ in range(3):
            f()
    h.sync()
    ms = {k: [] for k in calls}
    for _ in range(args.steps):
        for k, f in calls.items():
            h.timer_begin()
            f()
            ms[k].append(h.timer_end())
    for k, v in ms.items():
        print(json.dumps({"call": k, "steps": args.steps, "ms_per_call": round(float(np.median(v)), 4),
                          "ms_min": round(float(np.min(v)), 4), "ms_max": round(float(np.max(v)), 4)}))
    buf.free()
    h.close()


if __name__ == "__main__":
    main()

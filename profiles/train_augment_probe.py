"""Cost of the train-time augmentation path on 256 crops of 224 x 224, full default policy with Mixup:

  resident    `train_augment_features` on uint8 crops that stay in HBM (`on_device = 1`)
  host_u8     the same call from a host uint8 array (38 MB uploaded per call)
  parent      the route before the chain existed: `extract_features` from host float32 NCHW (154 MB uploaded per call),
              un-augmented
  backbone    the classifier forward alone on a resident float32 batch (`classify_device`, device events)

Each figure is the median over `--rounds` rounds of the mean over `--calls` calls; the four routes alternate inside a
round.  Host-side routes are wall clock around the synchronous calls; `resident` is also bracketed by
`dfd_timer_begin` / `_end`.  The chain's share is reported as 1 - backbone / resident (device events both): everything
`train_augment_features` does before its first backbone launch, plus the feature download.  Prints one JSON line.
    python profiles/train_augment_probe.py [--calls 5] [--rounds 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtdfd_amd  # noqa: E402
from rtdfd_amd import train_augment as TA  # noqa: E402

N = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    W = rtdfd_amd.weights
    h = rtdfd_amd._lib.Handle(W.pack_b0(W.seeded_state_dict(0)), device=0, max_batch=N)
    h.warmup(n_crops=N)
    rs = np.random.RandomState(0)
    crops = rs.randint(0, 256, (N, 224, 224, 3)).astype(np.uint8)
    nchw = rs.randn(N, 3, 224, 224).astype(np.float32)
    rows, batch = TA.draw_batch(TA.AugmentPolicy(), rs, N, 224, 224, mix=(TA.MIX_MIXUP, 0.7, rs.permutation(N)))
    resident = h.alloc(crops.nbytes).upload(crops)
    x_dev, z_dev = h.alloc(nchw.nbytes).upload(nchw), h.alloc(N * 4)

    def timed_resident():
        h.timer_begin()
        h.train_augment_features(resident, rows, batch, shape=crops.shape[:3])
        return h.timer_end()

    def timed_backbone():
        h.timer_begin()
        h.classify_device(x_dev.ptr, N, z_dev.ptr)
        return h.timer_end()

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    routes = {
        "resident_wall_ms": lambda: wall(lambda: h.train_augment_features(resident, rows, batch, shape=crops.shape[:3])),
        "resident_event_ms": timed_resident,
        "host_u8_wall_ms": lambda: wall(lambda: h.train_augment_features(crops, rows, batch)),
        "parent_wall_ms": lambda: wall(lambda: h.extract_features(nchw)),
        "backbone_event_ms": timed_backbone,
    }
    for fn in routes.values():                       # first calls allocate the work memory
        fn()
        fn()
    samples = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            samples[k].append(float(np.mean([fn() for _ in range(args.calls)])))
    out = {"crops": N, "calls": args.calls, "rounds": args.rounds}
    for k, v in samples.items():
        out[k] = round(float(np.median(v)), 3)
        out[k.replace("_ms", "_spread")] = [round(min(v), 3), round(max(v), 3)]
    out["chain_share_of_resident"] = round(1.0 - out["backbone_event_ms"] / out["resident_event_ms"], 3)
    out["flags_on"] = {name: int(((rows["flags"] & bit) != 0).sum()) for name, bit in
                       (("jpeg", TA.F_JPEG), ("gray", TA.F_GRAY), ("perspective", TA.F_PERSPECTIVE), ("blur", TA.F_BLUR),
                        ("erase", TA.F_ERASE), ("noise", TA.F_NOISE))}
    print(json.dumps(out))
    for b in (resident, x_dev, z_dev):
        b.free()
    h.close()


if __name__ == "__main__":
    main()

"""Cost of a Grad-CAM call against a classify call at batch 256 (DESIGN sections 4 / 5), fp32 and bf16 activations.

Warmed shapes (dfd_warmup at 256), device inputs, HIP events on the handle's stream around each call, the two calls
alternated in one process (classify, gradcam heat only, gradcam heat + overlay).  Prints one JSON line.
    python profiles/gradcam_probe.py [--steps 30]
Per-kernel times: the same script under rocprofv3 --kernel-trace --stats (a run of its own)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtdfd_amd  # noqa: E402

N = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    W = rtdfd_amd.weights
    h = rtdfd_amd._lib.Handle(W.pack_b0(W.seeded_state_dict(0)), device=0, max_batch=N)
    x = np.random.RandomState(1).randn(N, 3, 224, 224).astype(np.float32)
    xd = h.alloc(x.nbytes).upload(x)
    ld, hd, od = h.alloc(N * 4), h.alloc(N * 224 * 224 * 4), h.alloc(N * 224 * 224 * 3)
    calls = {
        "classify": lambda: h.classify_device(xd.ptr, N, ld.ptr),
        "gradcam_heat": lambda: h.gradcam_device(xd.ptr, N, ld.ptr, None, hd.ptr, None),
        "gradcam_heat_overlay": lambda: h.gradcam_device(xd.ptr, N, ld.ptr, None, hd.ptr, od.ptr),
    }
    out = {"batch": N, "steps": args.steps}
    for mode in ("fp32", "bf16"):
        h.set_option("bf16_activations", int(mode == "bf16"))
        h.warmup(N, 0)
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
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out[mode] = {k + "_ms": round(v, 4) for k, v in med.items()}
        out[mode]["ratio_heat"] = round(med["gradcam_heat"] / med["classify"], 4)
        out[mode]["ratio_heat_overlay"] = round(med["gradcam_heat_overlay"] / med["classify"], 4)
    print(json.dumps(out))
    for b in (xd, ld, hd, od):
        b.free()
    h.close()


if __name__ == "__main__":
    main()

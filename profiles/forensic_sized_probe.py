"""Milliseconds per frame of the general forensic chain (csrc/forensic_kernels.hip, run-time edge) at n = 16 frames for
S in 128, 256, 512, 1024, and of the specialised 256x256 chain in the same run (DESIGN sections 4f / 5).

What is timed: one `forensic_tap_sized(..., "stats")` call (full mode) between HIP events on the handle's stream - the
upload of the 16 already-resized S x S frames, every kernel of the chain and the 1 KB read-back; the resize from 1080p
is NOT included (the library has no entry that runs the general chain on device-resident frames; the resize is the
generic `dfd_resize` kernel either way).  The 256x256 chain is timed the same way through `forensic_tap`.  Calls are
alternated after three warm-up calls each; the median of `--steps` is reported.  Prints one JSON line.
    python profiles/forensic_sized_probe.py [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtdfd_amd  # noqa: E402

N = 16
SIZES = (128, 256, 512, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    W = rtdfd_amd.weights
    h = rtdfd_amd._lib.Handle(W.pack_all(W.seeded_state_dict(0), W.seeded_ssd_state_dict(0)), device=0, max_batch=1)
    rs = np.random.RandomState(1)
    stacks = {S: rs.randint(0, 256, (N, S, S, 3)).astype(np.uint8) for S in SIZES}
    calls = {f"general_{S}": (lambda S=S: h.forensic_tap_sized(stacks[S], S, "stats")) for S in SIZES}
    calls["specialised_256"] = lambda: h.forensic_tap(stacks[256], "stats")
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
    out = {"frames": N, "steps": args.steps}
    out.update({k + "_ms_per_frame": round(float(np.median(v)) / N, 4) for k, v in ms.items()})
    out["ratio_256"] = round(float(np.median(ms["general_256"]) / np.median(ms["specialised_256"])), 3)
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()

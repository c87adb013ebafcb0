"""One optimizer step (accumulate + apply) of the head trainer at n = 32 crops at three depths: with
blocks 14..15 ("depth14", section 4o's trainer), blocks 13..15 ("depth13") and blocks 12..15 ("depth12") unfrozen in front
of the conv stage and the head, drop-connect at the reference's rates, on the same machine in the same process.

Wall clock around whole steps ending in a device synchronise, medians of `--rounds` rounds of `--steps` steps with the
three trainers alternated inside every round (one trainer hangs off a handle at a time); the spread printed with every
median is the min .. max over the rounds of the same code in the same process.  Prints one JSON line.

    python profiles/block12_train_probe.py [--steps 20] [--rounds 5] [--n 32]

The depth-14 figure is the one profiles/block14_train_probe.py prints as "block14_ms": the unchanged path."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtdfd_amd  # noqa: E402
from rtdfd_amd import head_training as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=32)
    args = ap.parse_args()
    W = rtdfd_amd.weights
    sd = W.seeded_state_dict(0)
    n = args.n
    rs = np.random.RandomState(n)
    xb, y = rs.randn(n, 7, 7, 192).astype(np.float32), (rs.rand(n) < 0.5).astype(np.float32)
    h = rtdfd_amd._lib.Handle(W.pack_b0(sd), device=0, max_batch=1)
    variants = (("depth14", dict(train_block14=True)), ("depth13", dict(train_block13=True)), ("depth12", dict(train_block12=True)))
    ms = {name: [] for name, _ in variants}
    for rnd in range(-1, args.rounds):                          # round -1: warm-up, not recorded
        for name, kw in variants:
            with T.HeadTrainer(h, sd, max_n=n, **kw) as tr:
                def step():
                    tr.accumulate(xb, y)
                    tr.apply(3e-4)
                for _ in range(3):
                    step()
                h.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                h.sync()
                ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        if rnd < 0:
            ms = {k: [] for k in ms}
    row = {"n": n, "steps": args.steps, "rounds": args.rounds}
    for k, v in ms.items():
        row[k + "_ms"] = round(float(np.median(v)), 3)
        row[k + "_ms_min_max"] = [round(float(min(v)), 3), round(float(max(v)), 3)]
    row["block13_adds_ms"] = round(row["depth13_ms"] - row["depth14_ms"], 3)
    row["block12_adds_ms"] = round(row["depth12_ms"] - row["depth13_ms"], 3)
    print(json.dumps(row))
    h.close()


if __name__ == "__main__":
    main()

"""One optimizer step (accumulate + apply) of the head trainer at n = 32 crops at two depths: with
blocks 12..15 ("depth12", section 4p's trainer) and blocks 11..15 ("depth11") unfrozen in front of the conv stage and the
head, drop-connect of the skip blocks at the reference's rates, on the same machine in the same process.  The depth-11
trainer takes rows of block 10's output, (n, 14, 14, 112); the depth-12 trainer rows of block 11's, (n, 7, 7, 192).

Wall clock around whole steps ending in a device synchronise, medians of `--rounds` rounds of `--steps` steps with the two
trainers alternated inside every round (one trainer hangs off a handle at a time); the spread printed with every median is
the min .. max over the rounds of the same code in the same process.  Prints one JSON line.

    python profiles/block11_train_probe.py [--steps 20] [--rounds 5] [--n 32]

The depth-12 figure is the one profiles/block12_train_probe.py prints as "depth12_ms": the unchanged path."""
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
    rows = {"depth12": rs.randn(n, 7, 7, 192).astype(np.float32), "depth11": rs.randn(n, 14, 14, 112).astype(np.float32)}
    y = (rs.rand(n) < 0.5).astype(np.float32)
    h = rtdfd_amd._lib.Handle(W.pack_b0(sd), device=0, max_batch=1)
    variants = (("depth12", dict(train_block12=True)), ("depth11", dict(train_block11=True)))
    ms = {name: [] for name, _ in variants}
    for rnd in range(-1, args.rounds):                          # round -1: warm-up, not recorded
        for name, kw in variants:
            xb = rows[name]
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
    row["block11_adds_ms"] = round(row["depth11_ms"] - row["depth12_ms"], 3)
    print(json.dumps(row))
    h.close()


if __name__ == "__main__":
    main()

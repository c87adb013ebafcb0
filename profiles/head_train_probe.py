"""Optimizer steps per second of the head trainer (DESIGN sections 4g / 5) at n = 32 and n = 256 rows, grad_accum 1 and 2,
next to the same step written in torch eager on the same GPU (nn.Linear / BatchNorm1d / Dropout / FocalLoss formula /
clip_grad_norm_ / AdamW / EMA, fp32, host features uploaded per batch as the library call does).

Wall clock around whole steps (host calls included: a step is launch-bound), medians of `--rounds` rounds of `--steps`
steps, the two implementations alternated in one process.  Prints one JSON line.  torch is initialised before the
library's handle is created: seen once, on the measuring host, the other order left torch without a device (cause not
looked into); without torch on the GPU the comparison column is reported as not measured.
    python profiles/head_train_probe.py [--steps 50] [--rounds 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtdfd_amd  # noqa: E402
from rtdfd_amd import head_training as T  # noqa: E402


def torch_stepper(sd, n, accum):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    dev = torch.device("cuda:0")
    net = nn.Sequential(nn.Dropout(0.5), nn.Linear(1280, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.35),
                        nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.25), nn.Linear(256, 1))
    net.load_state_dict({k[len("net._fc."):]: torch.from_numpy(np.array(v)) for k, v in sd.items() if k.startswith("net._fc.")})
    net = net.to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=3e-4, weight_decay=0.05)
    shadow = [p.detach().clone() for p in net.parameters()]

    def focal(z, t):
        t = t * 0.9 + 0.05
        bce = F.binary_cross_entropy_with_logits(z, t, reduction="none")
        p = torch.sigmoid(z)
        p_t = p * t + (1 - p) * (1 - t)
        return ((0.25 * t + 0.75 * (1 - t)) * (1 - p_t) ** 2.0 * bce).mean()

    def step(x, y):
        for _ in range(accum):
            xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
            loss = focal(net(xd).squeeze(1), yd) / accum
            loss.backward()
            loss.item()                                      # the library call returns the loss too
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
        with torch.no_grad():
            for s, p in zip(shadow, net.parameters()):
                s.mul_(0.999).add_(p, alpha=0.001)

    return step, lambda: torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    W = rtdfd_amd.weights
    sd = W.seeded_state_dict(0)
    out = {"steps": args.steps, "rounds": args.rounds, "rows": []}
    try:                                                    # torch first (module docstring)
        import torch

        torch.zeros(1, device="cuda:0")
        have_torch = True
    except Exception as e:                                  # the comparison column is then reported as not measured
        have_torch, out["torch_eager"] = False, f"not measured: {e}"
    h = rtdfd_amd._lib.Handle(W.pack_b0(sd), device=0, max_batch=1)
    for n in (32, 256):
        rs = np.random.RandomState(n)
        x = rs.uniform(0, 2, (n, 1280)).astype(np.float32)
        y = (rs.rand(n) < 0.5).astype(np.float32)
        for accum in (1, 2):
            tstep, tsync = torch_stepper(sd, n, accum) if have_torch else ((lambda *_a: None), (lambda: None))
            with T.HeadTrainer(h, sd, max_n=n) as tr:
                def hstep():
                    for _ in range(accum):
                        tr.accumulate(x, y, None, 1.0, 1.0 / accum)
                    tr.apply(3e-4)

                for _ in range(5):
                    hstep()
                    tstep(x, y)
                tsync()
                rates = {"hip": [], "torch": []}
                for _ in range(args.rounds):
                    for name, fn, sync in (("hip", hstep, h.sync), ("torch", lambda: tstep(x, y), tsync)):
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            fn()
                        sync()
                        rates[name].append(args.steps / (time.perf_counter() - t0))
            row = {"n": n, "grad_accum": accum, "hip_steps_per_s": round(float(np.median(rates["hip"])), 1),
                   "torch_eager_steps_per_s": round(float(np.median(rates["torch"])), 1) if have_torch else None}
            row["ratio"] = round(row["hip_steps_per_s"] / row["torch_eager_steps_per_s"], 3) if have_torch else None
            out["rows"].append(row)
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()

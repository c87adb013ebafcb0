"""One optimizer step (accumulate + apply) of the head trainer with block 15 unfrozen (DESIGN sections 4j / 5) at n = 32
and n = 256 crops, next to
  * the conv-stage trainer's step on trunk rows and the head-only trainer's step on pooled rows, and
  * the same block + conv + head written with torch.nn modules and autograd in fp32 on the same GPU (Conv2d / BatchNorm2d /
    ZeroPad2d + depthwise Conv2d / the squeeze-excite pair / x * sigmoid(x) / mean / the head of
    profiles/head_train_probe.py, AdamW with the backbone group at 0.1 x lr, clip_grad_norm_, EMA; host rows uploaded per
    batch as the library call does).

Wall clock around whole steps ending in a device synchronise, medians of `--rounds` rounds of `--steps` steps with the
four implementations alternated inside every round; the spread printed with every median is the min .. max over the
rounds of the same code in the same process.  torch is initialised before the library's handle is created (see
head_train_probe.py); without torch on the GPU the comparison is reported as not measured.  Prints one JSON line.

    python profiles/block15_train_probe.py [--steps 20] [--rounds 5]

Per kernel: run `--trace N` (N crops; 3 warm-up + `--steps` steps of the library alone, no torch) under
`rocprofv3 --kernel-trace --stats`, in a run of its own, then `--kernel-table <kernel_stats.csv> --n N` turns the
statistics into the table of section 5: average time per launch of every kernel of the step, slowest first."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtdfd_amd  # noqa: E402
from rtdfd_amd import head_training as T  # noqa: E402

TAGS = ("bk_", "hc_", "ht_", "ht64")


def torch_stepper(sd, n):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    dev = torch.device("cuda:0")
    p = "net._blocks.15."
    t = lambda k: torch.from_numpy(np.array(sd[k]))
    bn2d = lambda c: nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)

    def load_bn(m, prefix):
        m.load_state_dict({k: t(prefix + "." + k) for k in ("weight", "bias", "running_mean", "running_var")}, strict=False)
        return m

    expand, bn0 = nn.Conv2d(192, 1152, 1, bias=False), load_bn(bn2d(1152), p + "_bn0")
    dw, bn1 = nn.Conv2d(1152, 1152, 3, groups=1152, bias=False), load_bn(bn2d(1152), p + "_bn1")
    se1, se2 = nn.Conv2d(1152, 48, 1), nn.Conv2d(48, 1152, 1)
    proj, bn2 = nn.Conv2d(1152, 320, 1, bias=False), load_bn(bn2d(320), p + "_bn2")
    conv, bn = nn.Conv2d(320, 1280, 1, bias=False), load_bn(bn2d(1280), "net._bn1")
    expand.load_state_dict({"weight": t(p + "_expand_conv.weight")})
    dw.load_state_dict({"weight": t(p + "_depthwise_conv.weight")})
    se1.load_state_dict({"weight": t(p + "_se_reduce.weight"), "bias": t(p + "_se_reduce.bias")})
    se2.load_state_dict({"weight": t(p + "_se_expand.weight"), "bias": t(p + "_se_expand.bias")})
    proj.load_state_dict({"weight": t(p + "_project_conv.weight")})
    conv.load_state_dict({"weight": t("net._conv_head.weight")})
    head = nn.Sequential(nn.Dropout(0.5), nn.Linear(1280, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.35),
                         nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.25), nn.Linear(256, 1))
    head.load_state_dict({k[len("net._fc."):]: torch.from_numpy(np.array(v)) for k, v in sd.items() if k.startswith("net._fc.")})
    backbone = nn.ModuleList([expand, bn0, dw, bn1, se1, se2, proj, bn2, conv, bn])
    net = nn.ModuleList([backbone, head]).to(dev).train()
    opt = torch.optim.AdamW([{"params": head.parameters(), "lr": 3e-4}, {"params": backbone.parameters(), "lr": 3e-5}], weight_decay=0.05)
    shadow = [q.detach().clone() for q in net.parameters()]
    sw = lambda a: a * torch.sigmoid(a)

    def focal(z, tg):
        tg = tg * 0.9 + 0.05
        bce = F.binary_cross_entropy_with_logits(z, tg, reduction="none")
        pr = torch.sigmoid(z)
        p_t = pr * tg + (1 - pr) * (1 - tg)
        return ((0.25 * tg + 0.75 * (1 - tg)) * (1 - p_t) ** 2.0 * bce).mean()

    def step(x, y):
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        a = sw(bn0(expand(xd.view(n, 7, 7, 192).permute(0, 3, 1, 2))))   # NHWC rows as a channels-last NCHW view: no copy
        d = sw(bn1(dw(F.pad(a, (1, 1, 1, 1)))))
        g = torch.sigmoid(se2(sw(se1(d.mean(dim=(2, 3), keepdim=True)))))
        a = bn(conv(bn2(proj(d * g))))
        loss = focal(head(sw(a).mean(dim=(2, 3))).squeeze(1), yd)
        loss.backward()
        loss.item()                                              # the library call returns the loss too
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
        with torch.no_grad():
            for s, q in zip(shadow, net.parameters()):
                s.mul_(0.999).add_(q, alpha=0.001)

    return step, lambda: torch.cuda.synchronize()


def kernel_table(path, n):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if not any(tag in name for tag in TAGS):
                continue
            start = min(name.index(tag) for tag in TAGS if tag in name)
            short = name[start:].split("(")[0].strip()
            calls = int(float(r.get("Calls") or r.get("Count") or 0))
            avg_ns = float(r.get("AverageNs") or r.get("Average") or 0.0)
            rows.append({"kernel": short, "calls": calls, "avg_us": round(avg_ns / 1e3, 2), "total_ms": round(calls * avg_ns / 1e6, 3)})
    rows.sort(key=lambda r: -r["total_ms"])
    return {"n": n, "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0, help="crops: run the library's step alone (for rocprofv3)")
    ap.add_argument("--kernel-table", default=None, help="rocprofv3 kernel_stats.csv -> the per-kernel table")
    ap.add_argument("--n", type=int, default=256)
    args = ap.parse_args()
    if args.kernel_table:
        print(json.dumps(kernel_table(args.kernel_table, args.n)))
        return
    W = rtdfd_amd.weights
    sd = W.seeded_state_dict(0)
    if args.trace:
        n = args.trace
        rs = np.random.RandomState(n)
        xb, y = rs.randn(n, 7, 7, 192).astype(np.float32), (rs.rand(n) < 0.5).astype(np.float32)
        h = rtdfd_amd._lib.Handle(W.pack_b0(sd), device=0, max_batch=1)
        with T.HeadTrainer(h, sd, train_block15=True, max_n=n) as tr:
            for _ in range(3 + args.steps):
                tr.accumulate(xb, y)
                tr.apply(3e-4)
        h.sync()
        h.close()
        print(json.dumps({"traced_steps": 3 + args.steps, "n": n}))
        return
    out = {"steps": args.steps, "rounds": args.rounds, "rows": []}
    try:                                                    # torch first (head_train_probe.py's docstring)
        import torch

        torch.zeros(1, device="cuda:0")
        have_torch = True
    except Exception as e:                                  # the comparison is then reported as not measured
        have_torch, out["torch"] = False, f"not measured: {e}"
    h = rtdfd_amd._lib.Handle(W.pack_b0(sd), device=0, max_batch=1)
    for n in (32, 256):
        rs = np.random.RandomState(n)
        xb = rs.randn(n, 7, 7, 192).astype(np.float32)
        xt = rs.randn(n, 7, 7, 320).astype(np.float32)
        xf = rs.uniform(0, 2, (n, 1280)).astype(np.float32)
        y = (rs.rand(n) < 0.5).astype(np.float32)
        tstep, tsync = torch_stepper(sd, n) if have_torch else ((lambda *_a: None), (lambda: None))
        ms = {"block": [], "conv": [], "head": [], "torch": []}

        def timed(name, fn, sync):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            sync()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)

        # one trainer hangs off a handle at a time: the three library variants take turns inside every round
        variants = (("block", dict(train_block15=True), xb), ("conv", dict(train_conv_head=True), xt), ("head", {}, xf))
        for rnd in range(-1, args.rounds):                  # round -1: warm-up of every shape, not recorded
            for name, kw, rows in variants:
                with T.HeadTrainer(h, sd, max_n=n, **kw) as tr:
                    def lstep():
                        tr.accumulate(rows, y)
                        tr.apply(3e-4)
                    for _ in range(3):
                        lstep()
                    h.sync()
                    timed(name, lstep, h.sync)
            if have_torch:
                for _ in range(3):
                    tstep(xb, y)
                tsync()
                timed("torch", lambda: tstep(xb, y), tsync)
            if rnd < 0:
                ms = {k: [] for k in ms}
        row = {"n": n}
        for k, v in ms.items():
            if v:
                row[k + "_ms"] = round(float(np.median(v)), 3)
                row[k + "_ms_min_max"] = [round(float(min(v)), 3), round(float(max(v)), 3)]
        if have_torch:
            row["torch_over_block"] = round(row["torch_ms"] / row["block_ms"], 3)
        row["block_adds_ms"] = round(row["block_ms"] - row["conv_ms"], 3)
        out["rows"].append(row)
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()

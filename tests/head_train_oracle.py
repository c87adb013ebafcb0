"""Test-side oracle of the head trainer (csrc/head_train.hip): one training step and one apply written with
torch.nn.Linear / BatchNorm1d / autograd / torch.optim.AdamW / clip_grad_norm_ and the reference's FocalLoss formula
(train.py:380-392), EMA as train.py:411-416.  `Oracle(..., dtype=torch.float64)` is the reference, `torch.float32` on
the CPU the yardstick.  Dropout is a multiplication by a given mask (head_training.dropout_keep_mask of the trainer's
(seed, accumulate counter)), not nn.Dropout.

Bars are the project's: `bar_ratio` applies b0_layer_oracle's RMS_FACTOR / MAX_FACTOR to the float32 yardstick's own
rms(d) / rms(ref) and max|d| / max|ref| against the float64 reference, floored at RMS_FLOOR / MAX_FLOOR.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import b0_layer_oracle as B
import rtdfd_amd
from rtdfd_amd import head_training as T

FIELDS = rtdfd_amd._lib.HEAD_FIELDS
STAT_FIELDS = ("rm1", "rv1", "rm2", "rv2")
GRAD_FIELDS = tuple(f for f in FIELDS if f not in STAT_FIELDS)


def config_values(cfg) -> Dict[str, float]:
    """the library's settings as it holds them (float32 values as Python floats)"""
    return {name: getattr(cfg, name) for name, _ in type(cfg)._fields_}


def default_params(seed: int) -> Dict[str, np.ndarray]:
    """default-initialised torch layers (the reference's `_fc` after construction), float32 arrays by field"""
    torch.manual_seed(seed)
    fc1, bn1, fc2, bn2, fc3 = nn.Linear(1280, 512), nn.BatchNorm1d(512), nn.Linear(512, 256), nn.BatchNorm1d(256), nn.Linear(256, 1)
    t = {"w1": fc1.weight, "b1": fc1.bias, "g1": bn1.weight, "be1": bn1.bias, "rm1": bn1.running_mean, "rv1": bn1.running_var,
         "w2": fc2.weight, "b2": fc2.bias, "g2": bn2.weight, "be2": bn2.bias, "rm2": bn2.running_mean, "rv2": bn2.running_var,
         "w3": fc3.weight, "b3": fc3.bias}
    return {k: v.detach().numpy().astype(np.float32).copy() for k, v in t.items()}


def features(seed: int, n: int) -> np.ndarray:
    """uniform [0, 2): pooled swish outputs are mostly positive"""
    return np.random.RandomState(seed).uniform(0.0, 2.0, (n, 1280)).astype(np.float32)


def focal(logits, targets, gamma, alpha, ls):
    """train.py:380-392, verbatim"""
    if ls > 0:
        targets = targets * (1 - ls) + 0.5 * ls
    bce = F.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    probs = torch.sigmoid(logits)
    p_t = probs * targets + (1 - probs) * (1 - targets)
    alpha_t = alpha * targets + (1 - alpha) * (1 - targets)
    return (alpha_t * (1 - p_t) ** gamma * bce).mean()


class Oracle:
    """The trainer's state and calls in torch; same call surface as head_training.HeadTrainer where fit_loop needs it."""

    def __init__(self, params: Dict[str, np.ndarray], cfg: Dict[str, float], dtype=torch.float64):
        self.dtype, self.cfg = dtype, dict(cfg)
        self.max_n = int(cfg["max_n"])
        self.loss_settings = (cfg["focal_gamma"], cfg["focal_alpha"], cfg["label_smoothing"])
        mom = cfg["bn_momentum"]
        self.fc1, self.bn1 = nn.Linear(1280, 512), nn.BatchNorm1d(512, eps=1e-5, momentum=mom)
        self.fc2, self.bn2 = nn.Linear(512, 256), nn.BatchNorm1d(256, eps=1e-5, momentum=mom)
        self.fc3 = nn.Linear(256, 1)
        self.mods = nn.ModuleList([self.fc1, self.bn1, self.fc2, self.bn2, self.fc3]).to(dtype)
        self.tensors = {"w1": self.fc1.weight, "b1": self.fc1.bias, "g1": self.bn1.weight, "be1": self.bn1.bias,
                        "rm1": self.bn1.running_mean, "rv1": self.bn1.running_var, "w2": self.fc2.weight, "b2": self.fc2.bias,
                        "g2": self.bn2.weight, "be2": self.bn2.bias, "rm2": self.bn2.running_mean, "rv2": self.bn2.running_var,
                        "w3": self.fc3.weight, "b3": self.fc3.bias}
        with torch.no_grad():
            for k, t in self.tensors.items():
                t.copy_(torch.from_numpy(np.asarray(params[k], np.float32)).to(dtype).reshape(t.shape))
        self.trainable = [self.tensors[k] for k in GRAD_FIELDS]
        self.opt = torch.optim.AdamW(self.trainable, lr=1e-3, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"],
                                     weight_decay=cfg["weight_decay"])
        self.opt.zero_grad(set_to_none=False)
        for p in self.trainable:
            p.grad = torch.zeros_like(p)
        self.shadow = {k: self.tensors[k].detach().clone() for k in GRAD_FIELDS}
        self.rates = T.dropout_rates(cfg["dropout"])
        self.counter = 0
        self.taps: Dict[str, torch.Tensor] = {}

    # -- forward
    def _forward(self, x, masks):
        self.mods.train(masks is not None)
        if masks is not None:
            x = x * masks[0]
        z1 = self.bn1(self.fc1(x))
        a1 = F.relu(z1)
        if masks is not None:
            a1 = a1 * masks[1]
        z2 = self.bn2(self.fc2(a1))
        a2 = F.relu(z2)
        if masks is not None:
            a2 = a2 * masks[2]
        return self.fc3(a2).squeeze(1), z1, z2

    def masks(self, n: int, counter: Optional[int] = None):
        """the three multipliers (keep / (1 - p)) of accumulate number `counter`"""
        c = self.counter if counter is None else counter
        out = []
        for layer, (w, p) in enumerate(zip(T.LAYER_WIDTHS, self.rates)):
            keep = T.dropout_keep_mask(int(self.cfg["seed"]), c, layer, n, w, p)
            out.append(torch.from_numpy(keep.astype(np.float64) / (1.0 - p)).to(self.dtype))
        return out

    def accumulate(self, feat, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        x = torch.from_numpy(np.asarray(feat, np.float32)).to(self.dtype)
        ya = torch.from_numpy(np.asarray(labels_a, np.float32)).to(self.dtype)
        z, z1, z2 = self._forward(x, self.masks(x.shape[0]))
        g, a, ls = self.loss_settings
        loss = focal(z, ya, g, a, ls)
        if labels_b is not None:
            yb = torch.from_numpy(np.asarray(labels_b, np.float32)).to(self.dtype)
            loss = lam * loss + (1 - lam) * focal(z, yb, g, a, ls)
        (loss * loss_scale).backward()
        self.counter += 1
        self.taps = {"z1": z1.detach(), "z2": z2.detach()}
        return float(loss.detach()), z.detach().numpy().copy()

    def apply(self, lr: float) -> float:
        for grp in self.opt.param_groups:
            grp["lr"] = lr
        norm = torch.nn.utils.clip_grad_norm_(self.trainable, max_norm=self.cfg["clip_norm"])
        self.opt.step()
        for p in self.trainable:
            p.grad.zero_()
        d = self.cfg["ema_decay"]
        with torch.no_grad():
            for k in GRAD_FIELDS:
                self.shadow[k].mul_(d).add_(self.tensors[k].detach(), alpha=1 - d)
        return float(norm)

    @torch.no_grad()
    def evaluate(self, feat, use_ema: bool = False) -> np.ndarray:
        """eval-mode logits; the BatchNorm outputs of this forward are kept in `taps` as `accumulate` keeps its own"""
        x = torch.from_numpy(np.asarray(feat, np.float32)).to(self.dtype)
        backup = None
        if use_ema:
            backup = {k: self.tensors[k].detach().clone() for k in GRAD_FIELDS}
            for k in GRAD_FIELDS:
                self.tensors[k].copy_(self.shadow[k])
        z, z1, z2 = self._forward(x, None)
        z = z.numpy().copy()
        self.taps = {"z1": z1.detach().clone(), "z2": z2.detach().clone()}
        if backup is not None:
            for k in GRAD_FIELDS:
                self.tensors[k].copy_(backup[k])
        return z

    @torch.no_grad()
    def force_from(self, other: "Oracle"):
        """Teacher-force this oracle's whole state (parameters, running statistics, EMA shadow, Adam moments and step)
        from `other`, rounded to this dtype.  A float32 oracle forced from the float64 one after every apply never
        drifts: the difference of the two in the next forward is float32 rounding of that forward alone."""
        for k in FIELDS:
            self.tensors[k].copy_(other.tensors[k].to(self.dtype))
        for k in GRAD_FIELDS:
            self.shadow[k].copy_(other.shadow[k].to(self.dtype))
            src = other.opt.state.get(other.tensors[k], {})
            dst = self.opt.state[self.tensors[k]]
            for name, v in src.items():
                dst[name] = v.detach().clone().to(self.dtype) if torch.is_tensor(v) and v.is_floating_point() and v.ndim else (
                    v.detach().clone() if torch.is_tensor(v) else v)
        self.counter = other.counter

    def export(self, use_ema: bool = False) -> Dict[str, np.ndarray]:
        src = {k: (self.shadow[k] if use_ema and k in self.shadow else self.tensors[k]) for k in FIELDS}
        return {k: v.detach().numpy().copy() for k, v in src.items()}

    def grads(self) -> Dict[str, np.ndarray]:
        return {k: self.tensors[k].grad.detach().numpy().copy() for k in GRAD_FIELDS}

    def set_grads(self, g: Dict[str, np.ndarray]):
        for k in GRAD_FIELDS:
            self.tensors[k].grad = torch.from_numpy(np.asarray(g[k], np.float32)).to(self.dtype).reshape(self.tensors[k].shape).clone()


def pair(params, cfg):
    """(float64 reference, float32 yardstick) from the same start"""
    return Oracle(params, cfg, torch.float64), Oracle(params, cfg, torch.float32)


# --------------------------------------------------------------------------- bars
def metrics(got, ref) -> Dict[str, float]:
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    d = got - ref
    rr, dd = float(np.sqrt(np.mean(ref ** 2))), float(np.sqrt(np.mean(d ** 2)))
    mr, md = float(np.abs(ref).max()), float(np.abs(d).max())
    return {"rms": dd / rr if rr > 0 else (0.0 if dd == 0 else float("inf")),
            "max": md / mr if mr > 0 else (0.0 if md == 0 else float("inf"))}


def bar_ratio(got, ref64, yard32) -> Dict[str, float]:
    """the device tensor against the project's bar: "ratio" <= 1 passes; the metrics of both for the record"""
    m, y = metrics(got, ref64), metrics(yard32, ref64)
    ratio = max(m["rms"] / (B.RMS_FACTOR * y["rms"] + B.RMS_FLOOR), m["max"] / (B.MAX_FACTOR * y["max"] + B.MAX_FLOOR))
    return {"ratio": ratio, "rms": m["rms"], "max": m["max"], "yard_rms": y["rms"], "yard_max": y["max"]}


def gate_margin(o64: Oracle, o32: Oracle) -> float:
    """min over both BN outputs of min|z64| / (8 max|z32 - z64|): >= 1 means no ReLU gate sits within rounding of zero.
    0 when the two oracles disagree on the sign of any pre-activation."""
    out = float("inf")
    for k in ("z1", "z2"):
        z64, z32 = o64.taps[k].double(), o32.taps[k].double()
        if bool(((z64 > 0) != (z32 > 0)).any()):
            return 0.0
        out = min(out, float(z64.abs().min()) / (8.0 * float((z32 - z64).abs().max())))
    return out

"""Test-side oracle of the head trainer's conv stage (csrc/head_train_conv.hip): net._conv_head + net._bn1 + swish + the
average pool in front of head_train_oracle.Oracle's head, written with torch.nn.Conv2d(320, 1280, 1, bias=False),
BatchNorm2d(1280, eps=1e-3, momentum=0.01), x * sigmoid(x), the mean over H, W and autograd; one torch.optim.AdamW with
two parameter groups (head at lr, conv at lr * lr_scale), one clip_grad_norm_ over all parameters, EMA over all
parameters.  `ConvOracle(..., dtype=torch.float64)` is the reference, `torch.float32` on the CPU the yardstick; bars
are head_train_oracle.bar_ratio's.

Trunk rows are NHWC (n, 7, 7, 320) or (n, 15680), as `Handle.extract_trunk` returns them.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn as nn

import b0_layer_oracle as B
import head_train_oracle as O
import rtdfd_amd
from rtdfd_amd import head_training as T

CONV_FIELDS = rtdfd_amd._lib.CONV_FIELDS
CONV_STAT_FIELDS = ("rm", "rv")
CONV_GRAD_FIELDS = ("w", "g", "be")
HW, C_IN, C_OUT = 49, 320, 1280


def conv_params(sd) -> Dict[str, np.ndarray]:
    """the five `dfd_headconv_params` arrays of a reference state dict"""
    sd = {(k if k.startswith("net.") else "net." + k): v for k, v in sd.items()}
    return {f: np.asarray(sd[k], np.float32).reshape(rtdfd_amd._lib.CONV_SHAPES[f]).copy() for k, f in T.CONV_KEYS.items()}


def synthetic_trunk(seed: int, n: int) -> np.ndarray:
    """standard normals: block 15 ends in a BatchNorm without activation, its output has both signs"""
    return np.random.RandomState(seed).randn(n, 7, 7, C_IN).astype(np.float32)


def nchw(trunk, dtype) -> torch.Tensor:
    a = np.asarray(trunk, np.float32)
    return torch.from_numpy(a.reshape(a.shape[0], 7, 7, C_IN)).to(dtype).permute(0, 3, 1, 2).contiguous()


class ConvOracle:
    """conv stage + head; the call surface of head_training.HeadTrainer where fit_loop needs it"""

    row_width = HW * C_IN

    def __init__(self, conv: Dict[str, np.ndarray], head: Dict[str, np.ndarray], cfg: Dict[str, float], dtype=torch.float64,
                 lr_scale: float = 0.1, bn_momentum: float = 0.01, bn_eps: float = 1e-3):
        self.dtype = dtype
        self.head = O.Oracle(head, cfg, dtype)                 # modules, masks and loss settings; its optimizer is not used
        self.cfg, self.max_n, self.loss_settings = self.head.cfg, self.head.max_n, self.head.loss_settings
        self.lr_scale = float(np.float32(lr_scale))            # the library holds the float
        self.conv = nn.Conv2d(C_IN, C_OUT, 1, bias=False).to(dtype)
        self.bn = nn.BatchNorm2d(C_OUT, eps=bn_eps, momentum=bn_momentum).to(dtype)
        self.ctensors = {"w": self.conv.weight, "g": self.bn.weight, "be": self.bn.bias, "rm": self.bn.running_mean,
                         "rv": self.bn.running_var}
        with torch.no_grad():
            for k, t in self.ctensors.items():
                t.copy_(torch.from_numpy(np.asarray(conv[k], np.float32)).to(dtype).reshape(t.shape))
        self.ctrainable = [self.ctensors[k] for k in CONV_GRAD_FIELDS]
        self.opt = torch.optim.AdamW([{"params": self.head.trainable}, {"params": self.ctrainable}], lr=1e-3,
                                     betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], weight_decay=cfg["weight_decay"])
        for p in self.ctrainable:
            p.grad = torch.zeros_like(p)
        self.cshadow = {k: self.ctensors[k].detach().clone() for k in CONV_GRAD_FIELDS}
        self.taps: Dict[str, torch.Tensor] = {}

    @property
    def counter(self):
        return self.head.counter

    # -- forward
    def features(self, trunk, train: bool):
        """-> (pooled features (n, 1280), BatchNorm output NCHW)"""
        self.conv.train(train)
        self.bn.train(train)
        y = self.bn(self.conv(nchw(trunk, self.dtype)))
        return (y * torch.sigmoid(y)).mean(dim=(2, 3)), y

    def accumulate(self, trunk, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        feat, y = self.features(trunk, True)
        feat.retain_grad()
        ya = torch.from_numpy(np.asarray(labels_a, np.float32)).to(self.dtype)
        z, z1, z2 = self.head._forward(feat, self.head.masks(feat.shape[0]))
        g, a, ls = self.loss_settings
        loss = O.focal(z, ya, g, a, ls)
        if labels_b is not None:
            yb = torch.from_numpy(np.asarray(labels_b, np.float32)).to(self.dtype)
            loss = lam * loss + (1 - lam) * O.focal(z, yb, g, a, ls)
        (loss * loss_scale).backward()
        self.head.counter += 1
        self.head.taps = {"z1": z1.detach(), "z2": z2.detach()}
        self.taps = {"cfeat": feat.detach(), "dfeat": feat.grad.detach().clone(), "z": z.detach(),
                     "cz": y.detach().permute(0, 2, 3, 1).reshape(y.shape[0], HW, C_OUT)}
        return float(loss.detach()), z.detach().numpy().copy()

    def group_rates(self, lr: float):
        """what dfd_head_train_apply documents: the head at lr, the conv at lr * lr_scale (product in double)"""
        return float(lr), float(lr) * self.lr_scale

    def apply(self, lr: float) -> float:
        for grp, rate in zip(self.opt.param_groups, self.group_rates(lr)):
            grp["lr"] = rate
        every = self.head.trainable + self.ctrainable
        norm = torch.nn.utils.clip_grad_norm_(every, max_norm=self.cfg["clip_norm"])
        self.opt.step()
        for p in every:
            p.grad.zero_()
        d = self.cfg["ema_decay"]
        with torch.no_grad():
            for k in O.GRAD_FIELDS:
                self.head.shadow[k].mul_(d).add_(self.head.tensors[k].detach(), alpha=1 - d)
            for k in CONV_GRAD_FIELDS:
                self.cshadow[k].mul_(d).add_(self.ctensors[k].detach(), alpha=1 - d)
        return float(norm)

    @torch.no_grad()
    def evaluate(self, trunk, use_ema: bool = False) -> np.ndarray:
        backup = None
        if use_ema:
            backup = {k: self.ctensors[k].detach().clone() for k in CONV_GRAD_FIELDS}
            for k in CONV_GRAD_FIELDS:
                self.ctensors[k].copy_(self.cshadow[k])
        feat, _ = self.features(trunk, False)
        z = self._head_eval(feat, use_ema)
        if backup is not None:
            for k in CONV_GRAD_FIELDS:
                self.ctensors[k].copy_(backup[k])
        return z

    def _head_eval(self, feat: torch.Tensor, use_ema: bool) -> np.ndarray:
        """head_train_oracle.Oracle.evaluate on a tensor of this dtype (its own takes float32 arrays)"""
        h = self.head
        backup = None
        if use_ema:
            backup = {k: h.tensors[k].detach().clone() for k in O.GRAD_FIELDS}
            for k in O.GRAD_FIELDS:
                h.tensors[k].copy_(h.shadow[k])
        z, z1, z2 = h._forward(feat, None)
        h.taps = {"z1": z1.detach().clone(), "z2": z2.detach().clone()}
        if backup is not None:
            for k in O.GRAD_FIELDS:
                h.tensors[k].copy_(backup[k])
        return z.numpy().copy()

    # -- state
    def export(self, use_ema: bool = False) -> Dict[str, np.ndarray]:
        """head fields as head_train_oracle.Oracle.export, conv fields under "conv." + name"""
        out = self.head.export(use_ema)
        for k in CONV_FIELDS:
            t = self.cshadow[k] if use_ema and k in self.cshadow else self.ctensors[k]
            out["conv." + k] = t.detach().numpy().reshape(rtdfd_amd._lib.CONV_SHAPES[k]).copy()
        return out

    def grads(self) -> Dict[str, np.ndarray]:
        out = self.head.grads()
        for k in CONV_GRAD_FIELDS:
            out["conv." + k] = self.ctensors[k].grad.detach().numpy().reshape(rtdfd_amd._lib.CONV_SHAPES[k]).copy()
        return out

    def set_grads(self, g: Dict[str, np.ndarray]):
        self.head.set_grads(g)
        for k in CONV_GRAD_FIELDS:
            t = self.ctensors[k]
            t.grad = torch.from_numpy(np.asarray(g["conv." + k], np.float32)).to(self.dtype).reshape(t.shape).clone()

    def state_dict(self, base, use_ema: bool = False) -> Dict[str, np.ndarray]:
        """`base` with this oracle's conv and head tensors under the reference's names (float32)"""
        e = self.export(use_ema)
        sd = dict(base)
        sd.update({k: e[f].astype(np.float32) for k, f in T.KEYS.items()})
        sd.update({k: (e["conv." + f].reshape(C_OUT, C_IN, 1, 1) if f == "w" else e["conv." + f]).astype(np.float32)
                   for k, f in T.CONV_KEYS.items()})
        return sd


def pair(conv, head, cfg, **kw):
    """(float64 reference, float32 yardstick) from the same start"""
    return ConvOracle(conv, head, cfg, torch.float64, **kw), ConvOracle(conv, head, cfg, torch.float32, **kw)


def gate_margin(o64: ConvOracle, o32: ConvOracle) -> float:
    """head_train_oracle.gate_margin on the two heads behind the conv stage"""
    return O.gate_margin(o64.head, o32.head)


@torch.no_grad()
def rounding_share(o64: ConvOracle, labels_a, labels_b=None, lam: float = 1.0) -> float:
    """Conditioning of the last accumulate, from the float64 oracle alone.  The pooled features are a float32 tensor on
    the device ("cfeat"; the head trainer's input), so the best any implementation can hand the head is the float64
    oracle's cfeat rounded to float32.  This feeds the float64 head exactly that and returns how far the logits and the
    loss move, in units of the bar's floor (`O.metrics` against b0_layer_oracle.RMS_FLOOR / MAX_FLOOR; the larger of the
    four): <= 1 means half an ulp on cfeat stays inside the part of the bar that does not depend on the float32
    yardstick's luck.  BatchNorm1d over a few rows divides by sqrt(var + 1e-5) of columns whose variance can lie below
    that eps; there this figure reaches 100 and the case measures the conditioning of the head, not a kernel."""
    h = o64.head
    n = o64.taps["cfeat"].shape[0]
    keep = {k: h.tensors[k].detach().clone() for k in O.STAT_FIELDS}
    tracked = [m.num_batches_tracked.clone() for m in (h.bn1, h.bn2)]
    z, _, _ = h._forward(o64.taps["cfeat"].float().to(o64.dtype), h.masks(n, h.counter - 1))
    for k, v in keep.items():
        h.tensors[k].copy_(v)
    for m, t in zip((h.bn1, h.bn2), tracked):
        m.num_batches_tracked.copy_(t)

    def loss_of(zz):
        g, a, ls = o64.loss_settings
        loss = O.focal(zz, torch.from_numpy(np.asarray(labels_a, np.float32)).to(zz.dtype), g, a, ls)
        if labels_b is not None:
            loss = lam * loss + (1 - lam) * O.focal(zz, torch.from_numpy(np.asarray(labels_b, np.float32)).to(zz.dtype), g, a, ls)
        return [float(loss)]

    z64 = o64.taps["z"]
    out = 0.0
    for got, ref in ((z.numpy(), z64.numpy()), (loss_of(z), loss_of(z64))):
        m = O.metrics(got, ref)
        out = max(out, m["rms"] / B.RMS_FLOOR, m["max"] / B.MAX_FLOOR)
    return out


def closed_form_backward(trunk, w, gamma, beta, dfeat, eps: float = 1e-3):
    """The backward the kernels implement, numpy float64, from the gradient of the pooled features:
      dA = dfeat / 49, dy = dA s (1 + y (1 - s)), dgamma = sum dy xhat, dbeta = sum dy,
      dZ = gamma istd (dy - dbeta / m - xhat dgamma / m), dW = dZ^T X.   -> (dW (1280, 320), dgamma, dbeta)"""
    x = np.asarray(trunk, np.float64).reshape(-1, C_IN)
    m = x.shape[0]
    z = x @ np.asarray(w, np.float64).reshape(C_OUT, C_IN).T
    mean, var = z.mean(0), z.var(0)
    istd = 1.0 / np.sqrt(var + eps)
    xh = (z - mean) * istd
    y = xh * gamma + beta
    s = 1.0 / (1.0 + np.exp(-y))
    dy = np.repeat(np.asarray(dfeat, np.float64) / HW, HW, axis=0) * (s * (1.0 + y * (1.0 - s)))
    dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
    dz = gamma * istd * (dy - dbeta / m - xh * dgamma / m)
    return dz.T @ x, dgamma, dbeta

"""Test-side oracle of the head trainer with block 11 unfrozen below block 12 (csrc/head_train_block.hip): the chain
11 -> 12 -> 13 -> 14 -> 15 -> conv -> head, built on block12_train_oracle.Block12Oracle at depth 12.  net._blocks.11 is the
MBConv that takes the 14 x 14 maps to 7 x 7: expand 112 -> 672, depthwise 5 x 5 at stride 2 behind
`ZeroPad2d((1, 2, 1, 2))` (TF-"SAME": 1 before, 2 after, on both axes), squeeze-excite 28, projection 672 -> 192, no skip
and so no drop-connect.  torch modules and autograd in train mode; one torch.optim.AdamW with seven parameter groups (head
at lr; conv and every block at lr * lr_scale), one clip_grad_norm_ over all parameters, EMA over all parameters.
`dtype=torch.float64` is the reference, `torch.float32` on the CPU the yardstick; bars are head_train_oracle.bar_ratio's.

Rows are block 10's output, NHWC (n, 14, 14, 112) or (n, 21952), as `Handle.extract_block_rows(x, 11)` returns them.

Taps of block 11: "b11.out" (n, 49, 192) - block 12's input -, "b11.gate" (n, 672), "b11.ad" (n, 49, 672), "b11.dout"
(n, 49, 192) - what block 12 hands down, dOut12 + dZe12 . We12 -, "b11.dae" (n, 196, 672).  There is no "b11.keep".

`store=True` rounds to float32, inside the float64 oracle, every tensor the device keeps in fp32 between two launches:
what block12_train_oracle rounds, and of block 11 Ze, ae, Zd, ad, the pooled s, gate, Zp and the output in the forward, its
dOut, dt, dZd and dae in the backward.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

import block12_train_oracle as B2
import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
import rtdfd_amd
from rtdfd_amd import head_training as T

L = rtdfd_amd._lib
BLOCK_FIELDS, BLOCK_STAT_FIELDS, BLOCK_GRAD_FIELDS = BO.BLOCK_FIELDS, BO.BLOCK_STAT_FIELDS, BO.BLOCK_GRAD_FIELDS
H_IN, H_OUT, HW_IN, HW, C_IN, C_EXP, C_SE, C_OUT, KS, STRIDE = 14, 7, 196, 49, 112, 672, 28, 192, 5, 2
PAD = (1, 2, 1, 2)                       # left, right, top, bottom: same_pad(14, 5, 2) = 3 in all, the smaller half first
TAPS = ("b11.out", "b11.gate", "b11.ad", "b11.dout", "b11.dae")
_swish = BO._swish


def block11_params(sd) -> Dict[str, np.ndarray]:
    """the 19 `dfd_mbconv_params` arrays of block 11 of a reference state dict"""
    sd = {(k if k.startswith("net.") else "net." + k): v for k, v in sd.items()}
    return {f: np.asarray(sd[k], np.float32).reshape(L.BLOCK11_SHAPES[f]).copy() for k, f in T.BLOCK11_KEYS.items() if f in L.BLOCK11_SHAPES}


def synthetic_rows(seed: int, n: int) -> np.ndarray:
    """standard normals: block 10 ends in a BatchNorm plus a skip, its output has both signs"""
    return np.random.RandomState(seed).randn(n, H_IN, H_IN, C_IN).astype(np.float32)


def nchw(rows, dtype) -> torch.Tensor:
    a = np.asarray(rows, np.float32)
    return torch.from_numpy(a.reshape(a.shape[0], H_IN, H_IN, C_IN)).to(dtype).permute(0, 3, 1, 2).contiguous()


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.detach().permute(0, 2, 3, 1).reshape(t.shape[0], t.shape[2] * t.shape[3], t.shape[1])


class _Block11:
    """the modules, tensors and EMA shadow of block 11; `pad`, `pool` and `skip` exist so that a test can corrupt them"""

    def __init__(self, params: Dict[str, np.ndarray], dtype, bn_momentum: float, bn_eps: float):
        bn = lambda c: nn.BatchNorm2d(c, eps=bn_eps, momentum=bn_momentum)
        self.expand, self.bn0 = nn.Conv2d(C_IN, C_EXP, 1, bias=False), bn(C_EXP)
        self.pad, self.dw, self.bn1 = nn.ZeroPad2d(PAD), nn.Conv2d(C_EXP, C_EXP, KS, stride=STRIDE, groups=C_EXP, bias=False), bn(C_EXP)
        self.se_reduce, self.se_expand = nn.Conv2d(C_EXP, C_SE, 1), nn.Conv2d(C_SE, C_EXP, 1)
        self.project, self.bn2 = nn.Conv2d(C_EXP, C_OUT, 1, bias=False), bn(C_OUT)
        self.mods = nn.ModuleList([self.expand, self.bn0, self.dw, self.bn1, self.se_reduce, self.se_expand, self.project, self.bn2]).to(dtype)
        self.tensors = {"exp_w": self.expand.weight, "dw_w": self.dw.weight, "se_w1": self.se_reduce.weight, "se_b1": self.se_reduce.bias,
                        "se_w2": self.se_expand.weight, "se_b2": self.se_expand.bias, "proj_w": self.project.weight}
        for l, m in enumerate((self.bn0, self.bn1, self.bn2)):
            self.tensors.update({f"g{l}": m.weight, f"be{l}": m.bias, f"rm{l}": m.running_mean, f"rv{l}": m.running_var})
        with torch.no_grad():
            for k, t in self.tensors.items():
                t.copy_(torch.from_numpy(np.asarray(params[k], np.float32)).to(dtype).reshape(t.shape))
        self.trainable = [self.tensors[k] for k in BLOCK_GRAD_FIELDS]
        for p in self.trainable:
            p.grad = torch.zeros_like(p)
        self.shadow = {k: self.tensors[k].detach().clone() for k in BLOCK_GRAD_FIELDS}
        self.pool_positions: Optional[int] = None              # None: the mean over the 49 output positions
        self.skip = False


class Block11Oracle(B2.Block12Oracle):
    """blocks 11..15 + conv stage + head; the call surface of head_training.HeadTrainer where fit_loop needs it.
    `below` = {13: params, 12: params}; `drops` = {13: rate, 12: rate}, `drop_connect` stays block 14's."""

    row_width = HW_IN * C_IN

    def __init__(self, block11, below, block14, block15, conv, head, cfg, dtype=torch.float64, lr_scale: float = 0.1,
                 bn_momentum: float = 0.01, bn_eps: float = 1e-3, store: bool = False, drop_connect: float = 0.0,
                 drops: Optional[Dict[int, float]] = None):
        super().__init__(below, block14, block15, conv, head, cfg, dtype, lr_scale, bn_momentum, bn_eps, store, drop_connect, drops)
        assert self.depth == 12
        self.b11 = _Block11(block11, dtype, bn_momentum, bn_eps)
        self.opt = torch.optim.AdamW([{"params": self.head.trainable}, {"params": self.co.ctrainable}, {"params": self.btrainable}]
                                     + [{"params": self.skips[b].trainable} for b in self.skips] + [{"params": self.b11.trainable}],
                                     lr=1e-3, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], weight_decay=cfg["weight_decay"])

    # -- forward
    def forward_block11(self, x: torch.Tensor, train: bool):
        """-> (block 11's output NCHW (n, 192, 7, 7), ae (n, 672, 14, 14), ad (n, 672, 7, 7), gate (n, 672))"""
        k = self.b11
        k.mods.train(train)
        S = self._st
        ze = S(k.expand(x), True, False)
        ae = S(_swish(k.bn0(ze)), True, True)
        zd = S(k.dw(k.pad(ae)), True, True)
        ad = S(_swish(k.bn1(zd)), True, False)
        s = ad.mean(dim=(2, 3), keepdim=True)
        if k.pool_positions is not None:
            s = s * (float(HW) / float(k.pool_positions))
        s = S(s, True, False)
        gate = S(torch.sigmoid(k.se_expand(_swish(k.se_reduce(s)))), True, False)
        t = S(ad * gate, False, True)
        zp = S(k.project(t), True, False)
        y = k.bn2(zp)
        if k.skip:                                             # a defect a test plants: block 11 has none
            y = y + x[:, :1, ::2, ::2]
        return S(y, True, True), ae, ad, gate.flatten(1)

    def accumulate(self, rows, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        n = np.asarray(rows).shape[0]
        x11, ae11, ad11, gate11 = self.forward_block11(nchw(rows, self.dtype), True)
        x11.retain_grad()
        ae11.retain_grad()
        x, held = x11, {}
        for b in range(12, 15):
            x, ae, ad, gate, factor = self.forward_skip(b, x, True, self.keep_of(b, n))
            x.retain_grad()
            ae.retain_grad()
            held[b] = (x, ae, ad, gate, factor)
        x15, ae, ad, gate = self.forward_block15(x, True)
        x15.retain_grad()
        ae.retain_grad()
        feat, y = self.features(x15, True)
        feat.retain_grad()
        h = self.head
        ya = torch.from_numpy(np.asarray(labels_a, np.float32)).to(self.dtype)
        z, z1, z2 = h._forward(feat, h.masks(feat.shape[0]))
        g, a, ls = self.loss_settings
        loss = O.focal(z, ya, g, a, ls)
        if labels_b is not None:
            yb = torch.from_numpy(np.asarray(labels_b, np.float32)).to(self.dtype)
            loss = lam * loss + (1 - lam) * O.focal(z, yb, g, a, ls)
        (loss * loss_scale).backward()
        h.counter += 1
        h.taps = {"z1": z1.detach(), "z2": z2.detach()}
        self.co.taps = {"cfeat": feat.detach(), "dfeat": feat.grad.detach().clone(), "z": z.detach(),
                        "cz": y.detach().permute(0, 2, 3, 1).reshape(y.shape[0], HW, CO.C_OUT)}
        self.taps = dict(self.co.taps)
        self.taps.update({"b15.out": nhwc(x15), "b15.gate": gate.detach(), "b15.ad": nhwc(ad), "b15.dout": nhwc(x15.grad),
                          "b15.dae": nhwc(ae.grad)})
        for b, (xb, aeb, adb, gateb, factor) in held.items():
            self.taps.update({f"b{b}.out": nhwc(xb), f"b{b}.gate": gateb.detach(), f"b{b}.ad": nhwc(adb), f"b{b}.keep": factor.detach(),
                              f"b{b}.dout": nhwc(xb.grad), f"b{b}.dae": nhwc(aeb.grad)})
        self.taps.update({"b11.out": nhwc(x11), "b11.gate": gate11.detach(), "b11.ad": nhwc(ad11), "b11.dout": nhwc(x11.grad),
                          "b11.dae": nhwc(ae11.grad)})
        return float(loss.detach()), z.detach().numpy().copy()

    def group_rates(self, lr: float):
        return super().group_rates(lr) + (float(lr) * self.lr_scale,)

    def every(self):
        return super().every() + self.b11.trainable

    def _groups(self):
        return super()._groups() + ((self.b11.shadow, self.b11.tensors),)

    @torch.no_grad()
    def evaluate(self, rows, use_ema: bool = False) -> np.ndarray:
        swaps = self._groups()[1:] if use_ema else ()
        backup = [{k: t[k].detach().clone() for k in sh} for sh, t in swaps]
        for sh, t in swaps:
            for k in sh:
                t[k].copy_(sh[k])
        x = self.forward_block11(nchw(rows, self.dtype), False)[0]
        for b in range(12, 15):
            x = self.forward_skip(b, x, False)[0]
        x15 = self.forward_block15(x, False)[0]
        feat, _ = self.features(x15, False)
        z = self.co._head_eval(feat, use_ema)
        for (sh, t), b in zip(swaps, backup):
            for k in sh:
                t[k].copy_(b[k])
        return z

    # -- state
    def export(self, use_ema: bool = False) -> Dict[str, np.ndarray]:
        """as Block12Oracle.export, block 11's fields under "b11." + name"""
        out = super().export(use_ema)
        for k in BLOCK_FIELDS:
            t = self.b11.shadow[k] if use_ema and k in self.b11.shadow else self.b11.tensors[k]
            out["b11." + k] = t.detach().numpy().reshape(L.BLOCK11_SHAPES[k]).copy()
        return out

    def grads(self) -> Dict[str, np.ndarray]:
        out = super().grads()
        for k in BLOCK_GRAD_FIELDS:
            out["b11." + k] = self.b11.tensors[k].grad.detach().numpy().reshape(L.BLOCK11_SHAPES[k]).copy()
        return out

    def set_grads(self, g: Dict[str, np.ndarray]):
        super().set_grads(g)
        for k in BLOCK_GRAD_FIELDS:
            t = self.b11.tensors[k]
            t.grad = torch.from_numpy(np.asarray(g["b11." + k], np.float32)).to(self.dtype).reshape(t.shape).clone()

    def state_dict(self, base, use_ema: bool = False) -> Dict[str, np.ndarray]:
        e = self.export(use_ema)
        sd = super().state_dict(base, use_ema)
        sd.update({k: e["b11." + f].reshape(T.BLOCK11_SD_SHAPES.get(f, e["b11." + f].shape)).astype(np.float32)
                   for k, f in T.BLOCK11_KEYS.items() if f in L.BLOCK11_SHAPES})
        return sd


def pair(block11, below, block14, block15, conv, head, cfg, **kw):
    """(float64 reference, float32 yardstick) from the same start"""
    return (Block11Oracle(block11, below, block14, block15, conv, head, cfg, torch.float64, **kw),
            Block11Oracle(block11, below, block14, block15, conv, head, cfg, torch.float32, **kw))


def triple(block11, below, block14, block15, conv, head, cfg, **kw):
    """`pair` and the float64 oracle with the device's storage (`store=True`) from the same start"""
    return pair(block11, below, block14, block15, conv, head, cfg, **kw) + (
        Block11Oracle(block11, below, block14, block15, conv, head, cfg, torch.float64, store=True, **kw),)


gate_margin = BO.gate_margin
rounding_share = BO.rounding_share


def float_taps():
    """every float tap of a depth-11 trainer the device serves (the keep factors are compared exactly, elsewhere)"""
    return TAPS + B2.float_taps(12)


def storage_share(o64: Block11Oracle, o32: Block11Oracle, ost: Block11Oracle, losses) -> Dict[str, float]:
    """block12_train_oracle.storage_share (logits, loss, every gradient - block 11's included through `grads` - and the taps
    of blocks 12..15) extended over block 11's taps, each in units of `O.bar_ratio`'s bar, and the largest under "max"."""
    out = B2.storage_share(o64, o32, ost, losses)
    for k in TAPS:
        out["tap " + k] = O.bar_ratio(ost.taps[k].numpy(), o64.taps[k].numpy(), o32.taps[k].numpy())["ratio"]
    out["max"] = max(v for k, v in out.items() if k != "max")
    return out


# --------------------------------------------------------------------------- the closed form of the depthwise input gradient
def depthwise_input_gradient(dzd, wd) -> np.ndarray:
    """dae of the stride-2 depthwise conv as the kernel gathers it, numpy float64: input (iy, ix) collects the taps with
    2 oy - 1 + ky = iy - an even iy takes ky in {1, 3}, an odd one ky in {0, 2, 4} - in (ky, kx) order, outputs outside the
    7 x 7 left out.  dzd (n, 7, 7, 672), wd (672, 5, 5) -> (n, 14, 14, 672)"""
    dzd, wd = np.asarray(dzd, np.float64), np.asarray(wd, np.float64).reshape(C_EXP, KS, KS)
    out = np.zeros((dzd.shape[0], H_IN, H_IN, C_EXP))
    for iy in range(H_IN):
        kys = (1, 3) if iy % 2 == 0 else (0, 2, 4)
        for ix in range(H_IN):
            kxs = (1, 3) if ix % 2 == 0 else (0, 2, 4)
            for ky in kys:
                oy = (iy + 1 - ky) // 2
                if not 0 <= oy < H_OUT:
                    continue
                for kx in kxs:
                    ox = (ix + 1 - kx) // 2
                    if 0 <= ox < H_OUT:
                        out[:, iy, ix] += dzd[:, oy, ox] * wd[:, ky, kx]
    return out

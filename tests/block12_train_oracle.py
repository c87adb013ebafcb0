"""Test-side oracle of the head trainer with blocks 13 and 12 unfrozen below block 14 (csrc/head_train_block.hip): the chain
12 -> 13 -> 14 -> 15 -> conv -> head at depth 13 (blocks 13..15) or depth 12 (blocks 12..15), built on
block14_train_oracle.Block14Oracle.  net._blocks.13 and net._blocks.12 have block 14's geometry (MBConv k5, pad 2,
192 -> 1152 -> 192, squeeze-excite 48, the identity skip with efficientnet_pytorch's per-crop drop_connect); torch modules
and autograd in train mode; one torch.optim.AdamW with five or six parameter groups (head at lr; conv and every block at
lr * lr_scale), one clip_grad_norm_ over all parameters, EMA over all parameters.  `dtype=torch.float64` is the reference,
`torch.float32` on the CPU the yardstick; bars are head_train_oracle.bar_ratio's.

Rows are the input rows of the deepest block, NHWC (n, 7, 7, 192) or (n, 9408), as `Handle.extract_block_input(x, depth)`
returns them.

Drop-connect: block b's out = x_(b-1) + y / keep_prob_b * b_i with b_i = head_training.drop_connect_keep(seed, counter, n,
p_b, block=b): layer 17 - b of the trainer's hash, so the blocks drop independently.  `masks` ({block: bool (n,)}) replaces
the hash for a CPU check with given masks.  Eval applies none.

The gradient a skip block hands down is autograd's sum at the block's input, dX_b = dOut_b + dZe_b . We_b: the taps
"b{b-1}.dout" for the blocks that have a trained block below, "b{depth}.dx" for the deepest (the device forms none there).
`skip_input_gradient` restates the sum in closed form.

`store=True` rounds to float32, inside the float64 oracle, every tensor the device keeps in fp32 between two launches:
what block14_train_oracle rounds, and of each new block what it rounds of block 14 (Ze, ae, Zd, ad, the pooled s, gate, Zp,
the output after the skip; its dOut, dt, dZd, dae).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

import block14_train_oracle as B4
import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
import rtdfd_amd
from rtdfd_amd import head_training as T

L = rtdfd_amd._lib
BLOCK_FIELDS, BLOCK_STAT_FIELDS, BLOCK_GRAD_FIELDS = BO.BLOCK_FIELDS, BO.BLOCK_STAT_FIELDS, BO.BLOCK_GRAD_FIELDS
HW, C_IN, C_EXP, C_SE, C_OUT, KS = B4.HW, B4.C_IN, B4.C_EXP, B4.C_SE, B4.C_OUT, B4.KS
TAP_NAMES = ("out", "gate", "ad", "keep", "dout", "dae")
KEYS_OF = {14: T.BLOCK14_KEYS, 13: T.BLOCK13_KEYS, 12: T.BLOCK12_KEYS}
SD_SHAPES_OF = {14: T.BLOCK14_SD_SHAPES, 13: T.BLOCK13_SD_SHAPES, 12: T.BLOCK12_SD_SHAPES}
nchw, nhwc, _swish = BO.nchw, BO.nhwc, BO._swish
synthetic_rows = BO.synthetic_rows       # block 11 and block 12 end as block 14 does: BatchNorm (plus a skip), both signs


def taps_of(block: int):
    return tuple(f"b{block}.{k}" for k in TAP_NAMES)


def skip_block_params(sd, block: int) -> Dict[str, np.ndarray]:
    """the 19 `dfd_mbconv_params` arrays of block 14, 13 or 12 of a reference state dict"""
    sd = {(k if k.startswith("net.") else "net." + k): v for k, v in sd.items()}
    return {f: np.asarray(sd[k], np.float32).reshape(L.BLOCK14_SHAPES[f]).copy() for k, f in KEYS_OF[block].items() if f in L.BLOCK14_SHAPES}


class _SkipBlock:
    """the modules, tensors and EMA shadow of one k5 skip block"""

    def __init__(self, params: Dict[str, np.ndarray], dtype, bn_momentum: float, bn_eps: float, drop_connect: float):
        self.p = float(np.float32(drop_connect))               # the double of the float32 argument
        bn = lambda c: nn.BatchNorm2d(c, eps=bn_eps, momentum=bn_momentum)
        self.expand, self.bn0 = nn.Conv2d(C_IN, C_EXP, 1, bias=False), bn(C_EXP)
        self.pad, self.dw, self.bn1 = nn.ZeroPad2d(2), nn.Conv2d(C_EXP, C_EXP, KS, groups=C_EXP, bias=False), bn(C_EXP)
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


class _Block14View:
    """Block14Oracle's own block 14 under _SkipBlock's names"""

    def __init__(self, o: B4.Block14Oracle):
        self.p = o.p
        self.expand, self.bn0, self.pad, self.dw, self.bn1 = o.expand14, o.bn0_14, o.pad14, o.dw14, o.bn1_14
        self.se_reduce, self.se_expand, self.project, self.bn2 = o.se_reduce14, o.se_expand14, o.project14, o.bn2_14
        self.mods, self.tensors, self.trainable, self.shadow = o.mods14, o.b14tensors, o.b14trainable, o.b14shadow


class Block12Oracle(B4.Block14Oracle):
    """blocks `depth`..15 + conv stage + head; the call surface of head_training.HeadTrainer where fit_loop needs it.
    `below` = {13: params} (depth 13) or {13: params, 12: params} (depth 12); `drops` = {block: rate} for the new blocks,
    `drop_connect` stays block 14's."""

    def __init__(self, below: Dict[int, Dict[str, np.ndarray]], block14, block15, conv, head, cfg, dtype=torch.float64,
                 lr_scale: float = 0.1, bn_momentum: float = 0.01, bn_eps: float = 1e-3, store: bool = False,
                 drop_connect: float = 0.0, drops: Optional[Dict[int, float]] = None):
        super().__init__(block14, block15, conv, head, cfg, dtype, lr_scale, bn_momentum, bn_eps, store, drop_connect)
        assert set(below) in ({13}, {13, 12})
        self.depth = min(below)
        drops = drops or {}
        self.skips = {14: _Block14View(self)}                  # block -> its modules, top down
        for b in sorted(below, reverse=True):
            self.skips[b] = _SkipBlock(below[b], dtype, bn_momentum, bn_eps, drops.get(b, 0.0))
        self.opt = torch.optim.AdamW([{"params": self.head.trainable}, {"params": self.co.ctrainable}, {"params": self.btrainable}]
                                     + [{"params": self.skips[b].trainable} for b in self.skips],
                                     lr=1e-3, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], weight_decay=cfg["weight_decay"])
        self.masks: Optional[Dict[int, np.ndarray]] = None

    # -- forward
    def keep_of(self, block: int, n: int, counter=None) -> np.ndarray:
        """bool (n,): the crops whose branch block `block` keeps in accumulate number `counter`"""
        if self.masks is not None:
            return np.asarray(self.masks[block], bool).reshape(n)
        return T.drop_connect_keep(int(self.cfg["seed"]), self.counter if counter is None else counter, n, self.skips[block].p, block=block)

    def forward_skip(self, block: int, x: torch.Tensor, train: bool, keep=None):
        """Block14Oracle.forward_block14 of block `block` on a tensor -> (output NCHW, ae, ad, gate (n, 1152), factors (n,))"""
        k = self.skips[block]
        k.mods.train(train)
        S = self._st
        ze = S(k.expand(x), True, False)
        ae = S(_swish(k.bn0(ze)), True, True)
        zd = S(k.dw(k.pad(ae)), True, True)
        ad = S(_swish(k.bn1(zd)), True, False)
        s = S(ad.mean(dim=(2, 3), keepdim=True), True, False)
        gate = S(torch.sigmoid(k.se_expand(_swish(k.se_reduce(s)))), True, False)
        t = S(ad * gate, False, True)
        zp = S(k.project(t), True, False)
        y = k.bn2(zp)
        if keep is None:
            factor = torch.ones(x.shape[0], dtype=self.dtype)
        else:                                                  # efficientnet_pytorch.utils.drop_connect
            keep_prob = 1.0 - k.p
            b = torch.from_numpy(np.asarray(keep, np.float64)).to(self.dtype)
            y = y / keep_prob * b.reshape(-1, 1, 1, 1)
            factor = b / keep_prob
        return S(x + y, True, True), ae, ad, gate.flatten(1), factor

    def accumulate(self, rows, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        n = np.asarray(rows).shape[0]
        x0 = nchw(rows, self.dtype).requires_grad_(True)
        x, held = x0, {}
        for b in range(self.depth, 15):
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
        self.taps[f"b{self.depth}.dx"] = nhwc(x0.grad)
        return float(loss.detach()), z.detach().numpy().copy()

    def group_rates(self, lr: float):
        """what dfd_head_train_apply documents: the head at lr; conv and every block at lr * lr_scale"""
        return (float(lr),) + (float(lr) * self.lr_scale,) * (2 + len(self.skips))

    def every(self):
        out = self.head.trainable + self.co.ctrainable + self.btrainable
        for b in self.skips:
            out = out + self.skips[b].trainable
        return out

    def _groups(self):
        return ((self.head.shadow, self.head.tensors), (self.co.cshadow, self.co.ctensors), (self.bshadow, self.btensors)) + tuple(
            (self.skips[b].shadow, self.skips[b].tensors) for b in self.skips)

    @torch.no_grad()
    def evaluate(self, rows, use_ema: bool = False) -> np.ndarray:
        swaps = self._groups()[1:] if use_ema else ()
        backup = [{k: t[k].detach().clone() for k in sh} for sh, t in swaps]
        for sh, t in swaps:
            for k in sh:
                t[k].copy_(sh[k])
        x = nchw(rows, self.dtype)
        for b in range(self.depth, 15):
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
        """as Block14Oracle.export, the new blocks' fields under "b13." / "b12." + name"""
        out = super().export(use_ema)
        for b in range(self.depth, 14):
            k_ = self.skips[b]
            for k in BLOCK_FIELDS:
                t = k_.shadow[k] if use_ema and k in k_.shadow else k_.tensors[k]
                out[f"b{b}." + k] = t.detach().numpy().reshape(L.BLOCK14_SHAPES[k]).copy()
        return out

    def grads(self) -> Dict[str, np.ndarray]:
        out = super().grads()
        for b in range(self.depth, 14):
            for k in BLOCK_GRAD_FIELDS:
                out[f"b{b}." + k] = self.skips[b].tensors[k].grad.detach().numpy().reshape(L.BLOCK14_SHAPES[k]).copy()
        return out

    def set_grads(self, g: Dict[str, np.ndarray]):
        super().set_grads(g)
        for b in range(self.depth, 14):
            for k in BLOCK_GRAD_FIELDS:
                t = self.skips[b].tensors[k]
                t.grad = torch.from_numpy(np.asarray(g[f"b{b}." + k], np.float32)).to(self.dtype).reshape(t.shape).clone()

    def state_dict(self, base, use_ema: bool = False) -> Dict[str, np.ndarray]:
        e = self.export(use_ema)
        sd = super().state_dict(base, use_ema)
        for b in range(self.depth, 14):
            sd.update({k: e[f"b{b}." + f].reshape(SD_SHAPES_OF[b].get(f, e[f"b{b}." + f].shape)).astype(np.float32)
                       for k, f in KEYS_OF[b].items() if f in L.BLOCK14_SHAPES})
        return sd


def pair(below, block14, block15, conv, head, cfg, **kw):
    """(float64 reference, float32 yardstick) from the same start"""
    return (Block12Oracle(below, block14, block15, conv, head, cfg, torch.float64, **kw),
            Block12Oracle(below, block14, block15, conv, head, cfg, torch.float32, **kw))


def triple(below, block14, block15, conv, head, cfg, **kw):
    """`pair` and the float64 oracle with the device's storage (`store=True`) from the same start"""
    return pair(below, block14, block15, conv, head, cfg, **kw) + (
        Block12Oracle(below, block14, block15, conv, head, cfg, torch.float64, store=True, **kw),)


gate_margin = BO.gate_margin
rounding_share = BO.rounding_share


def float_taps(depth: int):
    """every float tap of a trainer of this depth the device serves (the keep factors are compared exactly, elsewhere)"""
    out = ()
    for b in range(depth, 15):
        out += tuple(k for k in taps_of(b) if not k.endswith(".keep"))
    return out + BO.TAPS + ("cfeat", "dfeat")


def storage_share(o64: Block12Oracle, o32: Block12Oracle, ost: Block12Oracle, losses) -> Dict[str, float]:
    """block15_train_oracle.storage_share (logits, loss and every gradient, every block's included through `grads`)
    extended over the taps of every block: how far the float64 oracle with the device's storage lies from the plain float64
    oracle, each in units of `O.bar_ratio`'s bar, by name, and the largest under "max"."""
    out = BO.storage_share(o64, o32, ost, losses)
    for k in float_taps(o64.depth):
        out["tap " + k] = O.bar_ratio(ost.taps[k].numpy(), o64.taps[k].numpy(), o32.taps[k].numpy())["ratio"]
    out["max"] = max(v for k, v in out.items() if k != "max")
    return out


# --------------------------------------------------------------------------- the closed form of the skip gradient
def skip_input_gradient(rows, p: Dict[str, np.ndarray], dout, dae, eps: float = 1e-3) -> np.ndarray:
    """dX_b = dOut_b + dZe_b . We_b of one skip block, numpy float64: from the block's input rows (m, 192), its parameters,
    the gradient arriving at its output dOut_b (m, 192) and dae (m, 1152), the gradient of its expanded activation.  dZe is
    BN0's backward of dae swish'(ye) with the batch statistics of Ze = X We^T.  -> (m, 192)"""
    f = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(rows, np.float64).reshape(-1, C_IN)
    we = f["exp_w"].reshape(C_EXP, C_IN)
    xh0, istd0, ye = B4._bn_fwd(x @ we.T, f["g0"], f["be0"], eps)
    dze = B4._bn_bwd(np.asarray(dae, np.float64).reshape(-1, C_EXP) * B4._dswish(ye), xh0, istd0, f["g0"])[0]
    return np.asarray(dout, np.float64).reshape(-1, C_OUT) + dze @ we

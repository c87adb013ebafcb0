"""Test-side oracle of block 14's stage of the head trainer (csrc/head_train_block.hip): net._blocks.14 (MBConv k5, pad 2,
192 -> 1152 -> 192, squeeze-excite 48, the identity skip with efficientnet_pytorch's per-crop drop_connect) in train mode,
chained into block15_train_oracle.BlockOracle's block 15, the conv stage and the head, with torch modules and autograd; one
torch.optim.AdamW with four parameter groups (head at lr; conv, block 15 and block 14 at lr * lr_scale), one
clip_grad_norm_ over all parameters, EMA over all parameters.  `Block14Oracle(..., dtype=torch.float64)` is the reference,
`torch.float32` on the CPU the yardstick; bars are head_train_oracle.bar_ratio's.

Rows are block 13's output, NHWC (n, 7, 7, 192) or (n, 9408), as `Handle.extract_block(x, 13)` returns them.

Drop-connect: out = x13 + y / keep_prob * b_i with b_i = head_training.drop_connect_keep(seed, counter, n, p), p the double
of the float32 rate.  Eval applies none.

`store=True` rounds to float32, inside the float64 oracle, every tensor the device keeps in fp32 between two launches:
what block15_train_oracle rounds, and of block 14 Ze, ae, Zd, ad, the pooled s, gate, Zp and the output after the skip in
the forward, dOut14, dt, dZd and dae in the backward.  BN2's output y before the skip is never stored.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn as nn

import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
import rtdfd_amd
from rtdfd_amd import head_training as T

L = rtdfd_amd._lib
BLOCK_FIELDS, BLOCK_STAT_FIELDS, BLOCK_GRAD_FIELDS = BO.BLOCK_FIELDS, BO.BLOCK_STAT_FIELDS, BO.BLOCK_GRAD_FIELDS
HW, C_IN, C_EXP, C_SE, C_OUT, KS = 49, 192, 1152, 48, 192, 5
TAPS = ("b14.out", "b14.gate", "b14.ad", "b14.keep", "b14.dout", "b14.dae")
nchw, nhwc, _swish = BO.nchw, BO.nhwc, BO._swish


def block14_params(sd) -> Dict[str, np.ndarray]:
    """the 19 `dfd_mbconv_params` arrays of block 14 of a reference state dict"""
    sd = {(k if k.startswith("net.") else "net." + k): v for k, v in sd.items()}
    return {f: np.asarray(sd[k], np.float32).reshape(L.BLOCK14_SHAPES[f]).copy() for k, f in T.BLOCK14_KEYS.items() if f in L.BLOCK14_SHAPES}


synthetic_rows = BO.synthetic_rows       # block 13 ends as block 14 does: BatchNorm plus a skip, both signs


class Block14Oracle(BO.BlockOracle):
    """block 14 + block 15 + conv stage + head; the call surface of head_training.HeadTrainer where fit_loop needs it"""

    def __init__(self, block14: Dict[str, np.ndarray], block15: Dict[str, np.ndarray], conv: Dict[str, np.ndarray],
                 head: Dict[str, np.ndarray], cfg: Dict[str, float], dtype=torch.float64, lr_scale: float = 0.1,
                 bn_momentum: float = 0.01, bn_eps: float = 1e-3, store: bool = False, drop_connect: float = 0.0):
        super().__init__(block15, conv, head, cfg, dtype, lr_scale, bn_momentum, bn_eps, store)
        self.p = float(np.float32(drop_connect))               # the double of the float32 argument
        bn = lambda c: nn.BatchNorm2d(c, eps=bn_eps, momentum=bn_momentum)
        self.expand14, self.bn0_14 = nn.Conv2d(C_IN, C_EXP, 1, bias=False), bn(C_EXP)
        self.pad14, self.dw14, self.bn1_14 = nn.ZeroPad2d(2), nn.Conv2d(C_EXP, C_EXP, KS, groups=C_EXP, bias=False), bn(C_EXP)
        self.se_reduce14, self.se_expand14 = nn.Conv2d(C_EXP, C_SE, 1), nn.Conv2d(C_SE, C_EXP, 1)
        self.project14, self.bn2_14 = nn.Conv2d(C_EXP, C_OUT, 1, bias=False), bn(C_OUT)
        self.mods14 = nn.ModuleList([self.expand14, self.bn0_14, self.dw14, self.bn1_14, self.se_reduce14, self.se_expand14,
                                     self.project14, self.bn2_14]).to(dtype)
        self.b14tensors = {"exp_w": self.expand14.weight, "dw_w": self.dw14.weight, "se_w1": self.se_reduce14.weight,
                           "se_b1": self.se_reduce14.bias, "se_w2": self.se_expand14.weight, "se_b2": self.se_expand14.bias,
                           "proj_w": self.project14.weight}
        for l, m in enumerate((self.bn0_14, self.bn1_14, self.bn2_14)):
            self.b14tensors.update({f"g{l}": m.weight, f"be{l}": m.bias, f"rm{l}": m.running_mean, f"rv{l}": m.running_var})
        with torch.no_grad():
            for k, t in self.b14tensors.items():
                t.copy_(torch.from_numpy(np.asarray(block14[k], np.float32)).to(dtype).reshape(t.shape))
        self.b14trainable = [self.b14tensors[k] for k in BLOCK_GRAD_FIELDS]
        self.opt = torch.optim.AdamW([{"params": self.head.trainable}, {"params": self.co.ctrainable}, {"params": self.btrainable},
                                      {"params": self.b14trainable}],
                                     lr=1e-3, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], weight_decay=cfg["weight_decay"])
        for p in self.b14trainable:
            p.grad = torch.zeros_like(p)
        self.b14shadow = {k: self.b14tensors[k].detach().clone() for k in BLOCK_GRAD_FIELDS}

    # -- forward
    def keep(self, n: int, counter=None) -> np.ndarray:
        """bool (n,): the crops whose branch accumulate number `counter` keeps"""
        return T.drop_connect_keep(int(self.cfg["seed"]), self.counter if counter is None else counter, n, self.p)

    def forward_block14(self, rows, train: bool, keep=None):
        """-> (block 14's output NCHW, ae, ad, gate (n, 1152), the factor of each crop's branch (n,)); `keep` (bool (n,)):
        the drop-connect mask of a train-mode forward, None = every crop kept at keep_prob 1 (eval)"""
        self.mods14.train(train)
        S = self._st
        x = nchw(rows, self.dtype)
        ze = S(self.expand14(x), True, False)
        ae = S(_swish(self.bn0_14(ze)), True, True)
        zd = S(self.dw14(self.pad14(ae)), True, True)
        ad = S(_swish(self.bn1_14(zd)), True, False)
        s = S(ad.mean(dim=(2, 3), keepdim=True), True, False)
        gate = S(torch.sigmoid(self.se_expand14(_swish(self.se_reduce14(s)))), True, False)
        t = S(ad * gate, False, True)
        zp = S(self.project14(t), True, False)
        y = self.bn2_14(zp)
        if keep is None:
            factor = torch.ones(x.shape[0], dtype=self.dtype)
        else:                                                  # efficientnet_pytorch.utils.drop_connect
            keep_prob = 1.0 - self.p
            b = torch.from_numpy(np.asarray(keep, np.float64)).to(self.dtype)
            y = y / keep_prob * b.reshape(-1, 1, 1, 1)
            factor = b / keep_prob
        return S(x + y, True, True), ae, ad, gate.flatten(1), factor

    def forward_block15(self, x14: torch.Tensor, train: bool):
        """BlockOracle.forward_block on a tensor"""
        self.mods.train(train)
        S = self._st
        ze = S(self.expand(x14), True, False)
        ae = S(_swish(self.bn0(ze)), True, True)
        zd = S(self.dw(self.pad(ae)), True, True)
        ad = S(_swish(self.bn1(zd)), True, False)
        s = S(ad.mean(dim=(2, 3), keepdim=True), True, False)
        gate = S(torch.sigmoid(self.se_expand(_swish(self.se_reduce(s)))), True, False)
        t = S(ad * gate, False, True)
        zp = S(self.project(t), True, False)
        return S(self.bn2(zp), True, True), ae, ad, gate.flatten(1)

    def accumulate(self, rows, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        n = np.asarray(rows).shape[0]
        x14, ae14, ad14, gate14, factor = self.forward_block14(rows, True, self.keep(n))
        x14.retain_grad()
        ae14.retain_grad()
        x15, ae, ad, gate = self.forward_block15(x14, True)
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
        self.taps.update({"b14.out": nhwc(x14), "b14.gate": gate14.detach(), "b14.ad": nhwc(ad14), "b14.keep": factor.detach(),
                          "b14.dout": nhwc(x14.grad), "b14.dae": nhwc(ae14.grad)})
        return float(loss.detach()), z.detach().numpy().copy()

    def group_rates(self, lr: float):
        """what dfd_head_train_apply documents: the head at lr; conv, block 15 and block 14 at lr * lr_scale"""
        return super().group_rates(lr) + (float(lr) * self.lr_scale,)

    def every(self):
        return super().every() + self.b14trainable

    def _groups(self):
        return ((self.head.shadow, self.head.tensors), (self.co.cshadow, self.co.ctensors), (self.bshadow, self.btensors),
                (self.b14shadow, self.b14tensors))

    def apply(self, lr: float) -> float:
        for grp, rate in zip(self.opt.param_groups, self.group_rates(lr)):
            grp["lr"] = rate
        norm = torch.nn.utils.clip_grad_norm_(self.every(), max_norm=self.cfg["clip_norm"])
        self.opt.step()
        for p in self.every():
            p.grad.zero_()
        d = self.cfg["ema_decay"]
        with torch.no_grad():
            for shadow, tensors in self._groups():
                for k, s in shadow.items():
                    s.mul_(d).add_(tensors[k].detach(), alpha=1 - d)
        return float(norm)

    @torch.no_grad()
    def evaluate(self, rows, use_ema: bool = False) -> np.ndarray:
        swaps = self._groups()[1:] if use_ema else ()
        backup = [{k: t[k].detach().clone() for k in sh} for sh, t in swaps]
        for sh, t in swaps:
            for k in sh:
                t[k].copy_(sh[k])
        x14 = self.forward_block14(rows, False)[0]
        x15 = self.forward_block15(x14, False)[0]
        feat, _ = self.features(x15, False)
        z = self.co._head_eval(feat, use_ema)
        for (sh, t), b in zip(swaps, backup):
            for k in sh:
                t[k].copy_(b[k])
        return z

    # -- state
    def export(self, use_ema: bool = False) -> Dict[str, np.ndarray]:
        """as BlockOracle.export, block 14's fields under "b14." + name"""
        out = super().export(use_ema)
        for k in BLOCK_FIELDS:
            t = self.b14shadow[k] if use_ema and k in self.b14shadow else self.b14tensors[k]
            out["b14." + k] = t.detach().numpy().reshape(L.BLOCK14_SHAPES[k]).copy()
        return out

    def grads(self) -> Dict[str, np.ndarray]:
        out = super().grads()
        for k in BLOCK_GRAD_FIELDS:
            out["b14." + k] = self.b14tensors[k].grad.detach().numpy().reshape(L.BLOCK14_SHAPES[k]).copy()
        return out

    def set_grads(self, g: Dict[str, np.ndarray]):
        super().set_grads(g)
        for k in BLOCK_GRAD_FIELDS:
            t = self.b14tensors[k]
            t.grad = torch.from_numpy(np.asarray(g["b14." + k], np.float32)).to(self.dtype).reshape(t.shape).clone()

    def state_dict(self, base, use_ema: bool = False) -> Dict[str, np.ndarray]:
        e = self.export(use_ema)
        sd = super().state_dict(base, use_ema)
        sd.update({k: e["b14." + f].reshape(T.BLOCK14_SD_SHAPES.get(f, e["b14." + f].shape)).astype(np.float32)
                   for k, f in T.BLOCK14_KEYS.items() if f in L.BLOCK14_SHAPES})
        return sd


def pair(block14, block15, conv, head, cfg, **kw):
    """(float64 reference, float32 yardstick) from the same start"""
    return (Block14Oracle(block14, block15, conv, head, cfg, torch.float64, **kw),
            Block14Oracle(block14, block15, conv, head, cfg, torch.float32, **kw))


def triple(block14, block15, conv, head, cfg, **kw):
    """`pair` and the float64 oracle with the device's storage (`store=True`) from the same start"""
    return pair(block14, block15, conv, head, cfg, **kw) + (Block14Oracle(block14, block15, conv, head, cfg, torch.float64, store=True, **kw),)


gate_margin = BO.gate_margin
rounding_share = BO.rounding_share


def storage_share(o64: Block14Oracle, o32: Block14Oracle, ost: Block14Oracle, losses) -> Dict[str, float]:
    """block15_train_oracle.storage_share (logits, loss and every gradient, block 14's included through `grads`) extended
    over the taps of both blocks: how far the float64 oracle with the device's storage lies from the plain float64 oracle,
    each in units of `O.bar_ratio`'s bar, by name, and the largest under "max"."""
    out = BO.storage_share(o64, o32, ost, losses)
    for k in TAPS + BO.TAPS + ("cfeat", "dfeat"):
        out["tap " + k] = O.bar_ratio(ost.taps[k].numpy(), o64.taps[k].numpy(), o32.taps[k].numpy())["ratio"]
    out["max"] = max(v for k, v in out.items() if k != "max")
    return out


# --------------------------------------------------------------------------- the closed form
_sig, _dswish, _bn_fwd, _bn_bwd, _shift = BO._sig, BO._dswish, BO._bn_fwd, BO._bn_bwd, BO._shift


def closed_form_backward(rows, p: Dict[str, np.ndarray], dout, factor, eps: float = 1e-3) -> Dict[str, np.ndarray]:
    """The backward the kernels implement for block 14, numpy float64, from dOut14 (m, 192) = dLoss / d(the block's output)
    and the crops' drop-connect factors (n,) (0 or 1 / keep_prob):
      BN2's gradient source is dOut14 * factor (per crop);  BN2 backward -> dZp;  dWp = dZp^T t;  dt = dZp . Wp
      the squeeze-excite and BN1 steps of block15_train_oracle.closed_form_backward
      dWd[c][ky][kx] = sum of dZd * (ae shifted by (ky - 2, kx - 2), zeros outside the 7 x 7)
      dae = dZd correlated with the flipped 5 x 5 kernel, pad 2;  dye = dae swish'(ye);  BN0 backward -> dZe;  dWe = dZe^T X
    No gradient with respect to the rows: block 13 is frozen.
    -> the 13 gradients by `dfd_mbconv_params` field, "dae" (m, 1152) and "out" (m, 192), the forward's output"""
    f = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(rows, np.float64).reshape(-1, C_IN)
    m, n = x.shape[0], x.shape[0] // HW
    fac = np.repeat(np.asarray(factor, np.float64).reshape(n), HW)[:, None]
    we, wd, wp = f["exp_w"].reshape(C_EXP, C_IN), f["dw_w"].reshape(C_EXP, KS, KS), f["proj_w"].reshape(C_OUT, C_EXP)
    w1, w2 = f["se_w1"].reshape(C_SE, C_EXP), f["se_w2"].reshape(C_EXP, C_SE)
    taps = [(ky, kx) for ky in range(KS) for kx in range(KS)]
    # forward
    xh0, istd0, ye = _bn_fwd(x @ we.T, f["g0"], f["be0"], eps)
    ae = (ye * _sig(ye)).reshape(n, 7, 7, C_EXP)
    zd = sum(_shift(ae, ky - 2, kx - 2) * wd[:, ky, kx] for ky, kx in taps).reshape(m, C_EXP)
    xh1, istd1, yd = _bn_fwd(zd, f["g1"], f["be1"], eps)
    ad = yd * _sig(yd)
    s = ad.reshape(n, HW, C_EXP).mean(1)
    r = s @ w1.T + f["se_b1"]
    q = r * _sig(r)
    gate = _sig(q @ w2.T + f["se_b2"])
    t = (ad.reshape(n, HW, C_EXP) * gate[:, None, :]).reshape(m, C_EXP)
    xh2, istd2, y2 = _bn_fwd(t @ wp.T, f["g2"], f["be2"], eps)
    # backward
    out = {"out": x + y2 * fac}
    dzp, out["g2"], out["be2"] = _bn_bwd(np.asarray(dout, np.float64).reshape(m, C_OUT) * fac, xh2, istd2, f["g2"])
    out["proj_w"] = dzp.T @ t
    dt = dzp @ wp
    dgate = (dt * ad).reshape(n, HW, C_EXP).sum(1)
    du = dgate * gate * (1.0 - gate)
    out["se_w2"], out["se_b2"] = du.T @ q, du.sum(0)
    dr = (du @ w2) * _dswish(r)
    out["se_w1"], out["se_b1"] = dr.T @ s, dr.sum(0)
    ds = dr @ w1
    dad = (dt.reshape(n, HW, C_EXP) * gate[:, None, :] + ds[:, None, :] / HW).reshape(m, C_EXP)
    dzd, out["g1"], out["be1"] = _bn_bwd(dad * _dswish(yd), xh1, istd1, f["g1"])
    dzd4 = dzd.reshape(n, 7, 7, C_EXP)
    out["dw_w"] = np.stack([np.stack([(dzd4 * _shift(ae, ky - 2, kx - 2)).sum((0, 1, 2)) for kx in range(KS)], -1) for ky in range(KS)], -2)
    dae = sum(_shift(dzd4, 2 - ky, 2 - kx) * wd[:, ky, kx] for ky, kx in taps).reshape(m, C_EXP)
    dze, out["g0"], out["be0"] = _bn_bwd(dae * _dswish(ye), xh0, istd0, f["g0"])
    out["exp_w"] = dze.T @ x
    out["dae"] = dae
    return out

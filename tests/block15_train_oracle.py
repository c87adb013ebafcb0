"""Test-side oracle of block 15's stage of the head trainer (csrc/head_train_block.hip): net._blocks.15 in train mode in
front of headconv_train_oracle.ConvOracle's pieces, written with torch modules - Conv2d(192, 1152, 1), three
BatchNorm2d(eps=1e-3, momentum=0.01), ZeroPad2d(1) + a depthwise Conv2d(1152, 1152, 3, groups=1152), the squeeze-excite
pair Conv2d(1152, 48, 1) / Conv2d(48, 1152, 1), Conv2d(1152, 320, 1) - and autograd; one torch.optim.AdamW with three
parameter groups (head at lr, conv and block at lr * lr_scale), one clip_grad_norm_ over all parameters, EMA over all
parameters.  `BlockOracle(..., dtype=torch.float64)` is the reference, `torch.float32` on the CPU the yardstick; bars
are head_train_oracle.bar_ratio's.

Rows are block 14's output, NHWC (n, 7, 7, 192) or (n, 9408), as `Handle.extract_trunk(x, block=14)` returns them.

`store=True` rounds to float32, inside the float64 oracle, every tensor the device keeps in fp32 between two launches
(DESIGN 4j): forward Ze, ae, Zd, ad, the pooled s, gate, Zp, x15, the conv stage's z, y and cfeat; backward dfeat, dX15,
dt, dZd and dae.  ye, yd, t = ad * gate, the three dZ and the small squeeze-excite vectors are never stored in fp32 and
are not rounded.  `storage_share` measures with it how much of the bar the storage format alone takes.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn as nn

import b0_layer_oracle as B
import head_train_oracle as O
import headconv_train_oracle as CO
import rtdfd_amd
from rtdfd_amd import head_training as T

L = rtdfd_amd._lib
BLOCK_FIELDS = L.BLOCK_FIELDS
BLOCK_STAT_FIELDS = L.BLOCK_STAT_FIELDS
BLOCK_GRAD_FIELDS = tuple(f for f in BLOCK_FIELDS if f not in BLOCK_STAT_FIELDS)
HW, C_IN, C_EXP, C_SE, C_OUT = 49, 192, 1152, 48, 320
TAPS = ("b15.out", "b15.gate", "b15.ad", "b15.dout", "b15.dae")


def block_params(sd) -> Dict[str, np.ndarray]:
    """the 19 `dfd_mbconv_params` arrays of a reference state dict"""
    sd = {(k if k.startswith("net.") else "net." + k): v for k, v in sd.items()}
    return {f: np.asarray(sd[k], np.float32).reshape(L.BLOCK_SHAPES[f]).copy() for k, f in T.BLOCK_KEYS.items() if f in L.BLOCK_SHAPES}


def synthetic_rows(seed: int, n: int) -> np.ndarray:
    """standard normals: block 14 ends in a BatchNorm (plus a skip) without activation, its output has both signs"""
    return np.random.RandomState(seed).randn(n, 7, 7, C_IN).astype(np.float32)


def nchw(rows, dtype) -> torch.Tensor:
    a = np.asarray(rows, np.float32)
    return torch.from_numpy(a.reshape(a.shape[0], 7, 7, C_IN)).to(dtype).permute(0, 3, 1, 2).contiguous()


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.detach().permute(0, 2, 3, 1).reshape(t.shape[0], HW, t.shape[1])


class _Store(torch.autograd.Function):
    """a tensor kept in fp32: its value (fwd) and / or its gradient (bwd) rounded to float32"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return x.float().to(x.dtype) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.float().to(g.dtype) if ctx.bwd else g), None, None


def _swish(x):
    return x * torch.sigmoid(x)


class BlockOracle:
    """block 15 + conv stage + head; the call surface of head_training.HeadTrainer where fit_loop needs it"""

    row_width = HW * C_IN

    def __init__(self, block: Dict[str, np.ndarray], conv: Dict[str, np.ndarray], head: Dict[str, np.ndarray], cfg: Dict[str, float],
                 dtype=torch.float64, lr_scale: float = 0.1, bn_momentum: float = 0.01, bn_eps: float = 1e-3, store: bool = False):
        self.dtype, self.store = dtype, bool(store)
        self.co = CO.ConvOracle(conv, head, cfg, dtype, lr_scale, bn_momentum, bn_eps)      # its optimizer is not used
        self.head = self.co.head
        self.cfg, self.max_n, self.loss_settings, self.lr_scale = self.co.cfg, self.co.max_n, self.co.loss_settings, self.co.lr_scale
        bn = lambda c: nn.BatchNorm2d(c, eps=bn_eps, momentum=bn_momentum)
        self.expand, self.bn0 = nn.Conv2d(C_IN, C_EXP, 1, bias=False), bn(C_EXP)
        self.pad, self.dw, self.bn1 = nn.ZeroPad2d(1), nn.Conv2d(C_EXP, C_EXP, 3, groups=C_EXP, bias=False), bn(C_EXP)
        self.se_reduce, self.se_expand = nn.Conv2d(C_EXP, C_SE, 1), nn.Conv2d(C_SE, C_EXP, 1)
        self.project, self.bn2 = nn.Conv2d(C_EXP, C_OUT, 1, bias=False), bn(C_OUT)
        self.mods = nn.ModuleList([self.expand, self.bn0, self.dw, self.bn1, self.se_reduce, self.se_expand, self.project, self.bn2]).to(dtype)
        self.btensors = {"exp_w": self.expand.weight, "dw_w": self.dw.weight, "se_w1": self.se_reduce.weight, "se_b1": self.se_reduce.bias,
                         "se_w2": self.se_expand.weight, "se_b2": self.se_expand.bias, "proj_w": self.project.weight}
        for l, m in enumerate((self.bn0, self.bn1, self.bn2)):
            self.btensors.update({f"g{l}": m.weight, f"be{l}": m.bias, f"rm{l}": m.running_mean, f"rv{l}": m.running_var})
        with torch.no_grad():
            for k, t in self.btensors.items():
                t.copy_(torch.from_numpy(np.asarray(block[k], np.float32)).to(dtype).reshape(t.shape))
        self.btrainable = [self.btensors[k] for k in BLOCK_GRAD_FIELDS]
        self.opt = torch.optim.AdamW([{"params": self.head.trainable}, {"params": self.co.ctrainable}, {"params": self.btrainable}],
                                     lr=1e-3, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], weight_decay=cfg["weight_decay"])
        for p in self.btrainable:
            p.grad = torch.zeros_like(p)
        self.bshadow = {k: self.btensors[k].detach().clone() for k in BLOCK_GRAD_FIELDS}
        self.taps: Dict[str, torch.Tensor] = {}

    @property
    def counter(self):
        return self.head.counter

    def _st(self, x, fwd, bwd):
        return _Store.apply(x, fwd, bwd) if self.store else x

    # -- forward
    def forward_block(self, rows, train: bool):
        """-> (x15 NCHW, ae, ad, gate (n, 1152)); every tensor the device stores goes through `_st`"""
        self.mods.train(train)
        S = self._st
        ze = S(self.expand(nchw(rows, self.dtype)), True, False)
        ae = S(_swish(self.bn0(ze)), True, True)
        zd = S(self.dw(self.pad(ae)), True, True)
        ad = S(_swish(self.bn1(zd)), True, False)
        s = S(ad.mean(dim=(2, 3), keepdim=True), True, False)
        gate = S(torch.sigmoid(self.se_expand(_swish(self.se_reduce(s)))), True, False)
        t = S(ad * gate, False, True)
        zp = S(self.project(t), True, False)
        return S(self.bn2(zp), True, True), ae, ad, gate.flatten(1)

    def features(self, x15: torch.Tensor, train: bool):
        """ConvOracle.features on a tensor -> (pooled features, BatchNorm output NCHW)"""
        co, S = self.co, self._st
        co.conv.train(train)
        co.bn.train(train)
        y = S(co.bn(S(co.conv(x15), True, False)), True, False)
        return S(_swish(y).mean(dim=(2, 3)), True, True), y

    def accumulate(self, rows, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        x15, ae, ad, gate = self.forward_block(rows, True)
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
        return float(loss.detach()), z.detach().numpy().copy()

    def group_rates(self, lr: float):
        """what dfd_head_train_apply documents: the head at lr, conv and block at lr * lr_scale (product in double)"""
        return float(lr), float(lr) * self.lr_scale, float(lr) * self.lr_scale

    def every(self):
        return self.head.trainable + self.co.ctrainable + self.btrainable

    def apply(self, lr: float) -> float:
        for grp, rate in zip(self.opt.param_groups, self.group_rates(lr)):
            grp["lr"] = rate
        norm = torch.nn.utils.clip_grad_norm_(self.every(), max_norm=self.cfg["clip_norm"])
        self.opt.step()
        for p in self.every():
            p.grad.zero_()
        d = self.cfg["ema_decay"]
        with torch.no_grad():
            for shadow, tensors in ((self.head.shadow, self.head.tensors), (self.co.cshadow, self.co.ctensors), (self.bshadow, self.btensors)):
                for k, s in shadow.items():
                    s.mul_(d).add_(tensors[k].detach(), alpha=1 - d)
        return float(norm)

    @torch.no_grad()
    def evaluate(self, rows, use_ema: bool = False) -> np.ndarray:
        swaps = ((self.bshadow, self.btensors), (self.co.cshadow, self.co.ctensors)) if use_ema else ()
        backup = [{k: t[k].detach().clone() for k in sh} for sh, t in swaps]
        for sh, t in swaps:
            for k in sh:
                t[k].copy_(sh[k])
        x15, _, _, _ = self.forward_block(rows, False)
        feat, _ = self.features(x15, False)
        z = self.co._head_eval(feat, use_ema)
        for (sh, t), b in zip(swaps, backup):
            for k in sh:
                t[k].copy_(b[k])
        return z

    # -- state
    def export(self, use_ema: bool = False) -> Dict[str, np.ndarray]:
        """head and conv fields as ConvOracle.export, block fields under "b15." + name"""
        out = self.co.export(use_ema)
        for k in BLOCK_FIELDS:
            t = self.bshadow[k] if use_ema and k in self.bshadow else self.btensors[k]
            out["b15." + k] = t.detach().numpy().reshape(L.BLOCK_SHAPES[k]).copy()
        return out

    def grads(self) -> Dict[str, np.ndarray]:
        out = self.co.grads()
        for k in BLOCK_GRAD_FIELDS:
            out["b15." + k] = self.btensors[k].grad.detach().numpy().reshape(L.BLOCK_SHAPES[k]).copy()
        return out

    def set_grads(self, g: Dict[str, np.ndarray]):
        self.co.set_grads(g)
        for k in BLOCK_GRAD_FIELDS:
            t = self.btensors[k]
            t.grad = torch.from_numpy(np.asarray(g["b15." + k], np.float32)).to(self.dtype).reshape(t.shape).clone()

    def state_dict(self, base, use_ema: bool = False) -> Dict[str, np.ndarray]:
        """`base` with this oracle's block, conv and head tensors under the reference's names (float32)"""
        e = self.export(use_ema)
        sd = self.co.state_dict(base, use_ema)
        sd.update({k: e["b15." + f].reshape(T.BLOCK_SD_SHAPES.get(f, e["b15." + f].shape)).astype(np.float32)
                   for k, f in T.BLOCK_KEYS.items() if f in L.BLOCK_SHAPES})
        return sd


def pair(block, conv, head, cfg, **kw):
    """(float64 reference, float32 yardstick) from the same start"""
    return BlockOracle(block, conv, head, cfg, torch.float64, **kw), BlockOracle(block, conv, head, cfg, torch.float32, **kw)


def gate_margin(o64: BlockOracle, o32: BlockOracle) -> float:
    """head_train_oracle.gate_margin on the two heads behind the stages"""
    return O.gate_margin(o64.head, o32.head)


def rounding_share(o64: BlockOracle, labels_a, labels_b=None, lam: float = 1.0) -> float:
    """headconv_train_oracle.rounding_share of the last accumulate: the head's conditioning on its float32 input"""
    return CO.rounding_share(o64.co, labels_a, labels_b, lam)


def triple(block, conv, head, cfg, **kw):
    """`pair` and the float64 oracle with the device's storage (`store=True`) from the same start"""
    return pair(block, conv, head, cfg, **kw) + (BlockOracle(block, conv, head, cfg, torch.float64, store=True, **kw),)


def storage_share(o64: BlockOracle, o32: BlockOracle, ost: BlockOracle, losses) -> Dict[str, float]:
    """Conditioning of the accumulates so far, from the oracles alone.  `ost` runs in float64 with every tensor the
    device stores as fp32 rounded to float32 where it is stored (`store=True`): the best any implementation with that
    storage can do.  All three have run the same accumulates from the same start; `losses` = the last one's
    (float64, float32, stored).  Returns how far the stored oracle's logits, loss and every gradient lie from the plain
    float64 oracle's, each in units of `O.bar_ratio`'s bar (so against the float32 yardstick's own error), by name, and
    the largest under "max": <= 0.5 means the storage format alone takes at most half of any bar."""
    assert ost.store and not o64.store and o64.counter == o32.counter == ost.counter
    l64, l32, lst = losses
    out = {"loss": O.bar_ratio([lst], [l64], [l32])["ratio"],
           "logits": O.bar_ratio(ost.taps["z"].numpy(), o64.taps["z"].numpy(), o32.taps["z"].numpy())["ratio"]}
    g, g64, g32 = ost.grads(), o64.grads(), o32.grads()
    for k in g64:
        out["grad " + k] = O.bar_ratio(g[k], g64[k], g32[k])["ratio"]
    out["max"] = max(out.values())
    return out


# --------------------------------------------------------------------------- the closed form
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _dswish(y):
    s = _sig(y)
    return s * (1.0 + y * (1.0 - s))


def _bn_fwd(z, gamma, beta, eps):
    mean, var = z.mean(0), z.var(0)
    istd = 1.0 / np.sqrt(var + eps)
    xh = (z - mean) * istd
    return xh, istd, xh * gamma + beta


def _bn_bwd(dy, xh, istd, gamma):
    m = dy.shape[0]
    sdy, sdx = dy.sum(0), (dy * xh).sum(0)
    return gamma * istd * (dy - sdy / m - xh * sdx / m), sdx, sdy


def _shift(a, dy, dx):
    """a (n, 7, 7, c) -> b with b[y][x] = a[y + dy][x + dx], zeros outside"""
    b = np.zeros_like(a)
    ys, xs = slice(max(0, -dy), 7 - max(0, dy)), slice(max(0, -dx), 7 - max(0, dx))
    yd, xd = slice(max(0, dy), 7 + min(0, dy)), slice(max(0, dx), 7 + min(0, dx))
    b[:, ys, xs] = a[:, yd, xd]
    return b


def conv_input_gradient(trunk, w, gamma, beta, dfeat, eps: float = 1e-3):
    """dX15 = dZh . Wh of the conv stage (headconv_train_oracle.closed_form_backward's dZ), numpy float64 -> (m, 320)"""
    x = np.asarray(trunk, np.float64).reshape(-1, CO.C_IN)
    w = np.asarray(w, np.float64).reshape(CO.C_OUT, CO.C_IN)
    xh, istd, y = _bn_fwd(x @ w.T, gamma, beta, eps)
    dy = np.repeat(np.asarray(dfeat, np.float64) / HW, HW, axis=0) * _dswish(y)
    dz, _, _ = _bn_bwd(dy, xh, istd, gamma)
    return dz @ w


def closed_form_backward(rows, p: Dict[str, np.ndarray], dx15, eps: float = 1e-3) -> Dict[str, np.ndarray]:
    """The backward the kernels implement, numpy float64, from dX15 (m, 320) = dLoss / d(BN2's output):
      BN2 backward -> dZp;  dWp = dZp^T t;  dt = dZp . Wp
      dgate = sum over 49 of dt * ad;  du = dgate gate (1 - gate);  dW2 = du^T q, db2 = sum du;  dq = du . W2
      dr = dq swish'(r);  dW1 = dr^T s, db1 = sum dr;  ds = dr . W1
      dad = dt * gate + ds / 49;  dyd = dad swish'(yd);  BN1 backward -> dZd
      dWd[c][ky][kx] = sum of dZd * (ae shifted);  dae = dZd correlated with the flipped kernel, pad 1
      dye = dae swish'(ye);  BN0 backward -> dZe;  dWe = dZe^T X
    -> the 13 gradients by `dfd_mbconv_params` field, and "dae" (m, 1152)"""
    f = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(rows, np.float64).reshape(-1, C_IN)
    m, n = x.shape[0], x.shape[0] // HW
    we, wd, wp = f["exp_w"].reshape(C_EXP, C_IN), f["dw_w"].reshape(C_EXP, 3, 3), f["proj_w"].reshape(C_OUT, C_EXP)
    w1, w2 = f["se_w1"].reshape(C_SE, C_EXP), f["se_w2"].reshape(C_EXP, C_SE)
    # forward
    xh0, istd0, ye = _bn_fwd(x @ we.T, f["g0"], f["be0"], eps)
    ae = (ye * _sig(ye)).reshape(n, 7, 7, C_EXP)
    zd = sum(_shift(ae, ky - 1, kx - 1) * wd[:, ky, kx] for ky in range(3) for kx in range(3)).reshape(m, C_EXP)
    xh1, istd1, yd = _bn_fwd(zd, f["g1"], f["be1"], eps)
    ad = yd * _sig(yd)
    s = ad.reshape(n, HW, C_EXP).mean(1)
    r = s @ w1.T + f["se_b1"]
    q = r * _sig(r)
    gate = _sig(q @ w2.T + f["se_b2"])
    t = (ad.reshape(n, HW, C_EXP) * gate[:, None, :]).reshape(m, C_EXP)
    xh2, istd2, _ = _bn_fwd(t @ wp.T, f["g2"], f["be2"], eps)
    # backward
    out = {}
    dzp, out["g2"], out["be2"] = _bn_bwd(np.asarray(dx15, np.float64).reshape(m, C_OUT), xh2, istd2, f["g2"])
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
    out["dw_w"] = np.stack([np.stack([(dzd4 * _shift(ae, ky - 1, kx - 1)).sum((0, 1, 2)) for kx in range(3)], -1) for ky in range(3)], -2)
    dae = sum(_shift(dzd4, 1 - ky, 1 - kx) * wd[:, ky, kx] for ky in range(3) for kx in range(3)).reshape(m, C_EXP)
    dze, out["g0"], out["be0"] = _bn_bwd(dae * _dswish(ye), xh0, istd0, f["g0"])
    out["exp_w"] = dze.T @ x
    out["dae"] = dae
    return out

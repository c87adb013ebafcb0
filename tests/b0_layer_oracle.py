"""Test-side float64 per-layer oracle of the B0 classifier, teacher-forced by the HIP path's own taps.

Each layer's reference is evaluated from the HIP path's own input to that layer (a tap), so what remains of the
difference is that kernel's own arithmetic, and it can be held to the precision the kernel claims:

  * float64 reference - `layer(cfg, name, get, to_torch(sd))`: oracle.b0_ref's pieces (`_same_conv`, `_bn`, `head`)
    on a float64 copy of the state dict, BatchNorm unfolded;
  * fp32 yardstick - the same call on float32 inputs and the float32 state dict: torch's plain fp32 evaluation of the
    same op, which is what "fp32-accurate" means for it;
  * bf16 mirror - `layer(cfg, name, get, kernel_state_dict(sd, cfg), MIRROR)`: float64 arithmetic on the weights as
    the device holds them, rounded to bf16 exactly where the bf16-activation path rounds.

Which tap feeds which op follows `b0_forward_t` (csrc/b0_plan.hip):
  stem <- x;  b{i}.exp <- b{i-1}.out (block 1: b0.out);  b{i}.dw <- b{i}.exp, or - expand fused into the depthwise
  launch (`Config.expand_fused`) - <- b{i-1}.out through expand, or - block 0 - <- stem, or - "fuse_stem": the stem
  computed inside stem_dw_kernel - <- x through the stem;  b{i}.gate <- b{i}.dw;  b{i}.out <- b{i}.dw, b{i}.gate and,
  on skip blocks, the block input;  head <- b15.out;  feat <- head;  logit <- feat.

bf16 rounding points of the "bf16_activations" path, read from the kernels (every fp32 -> bf16 conversion there is
`(__bf16)` / v_cvt_pk_bf16_f32: round to nearest even):
  * stem, unfused (stem_kernel): fp32 conv + bias + swish, rounded at the store.
  * stem, fused (stem_dw_kernel): written to the depthwise LDS tile as fp32, NOT rounded; block 0's depthwise reads
    the unrounded value.  The "stem" tap is a rounded side copy.
  * expand, unfused (split GEMM, pointwise_t<bf16_t>): bf16 activations times the weight planes, fp32 accumulation,
    bias, swish, rounded at the store (s6_epilogue).
  * expand, fused (mbconv2_kernel, blocks 1-5; mbconv_late_kernel, blocks 6-15): the swish output goes to the LDS tile
    as fp32 and is NOT rounded.  These launches always multiply with the three weight planes (fp32-exact weights),
    also when "bf16_weight_planes" = 1.
  * depthwise (dw_compute, and the 7 x 7 path of mbconv_late_kernel): fp32 taps + bias + swish, rounded at the store.
    The squeeze-excite pool partials (`psum` -> `red[]` -> P) sum the fp32 values BEFORE that rounding, so with bf16
    storage the gate's reference recomputes the unrounded depthwise output from the depthwise input.
  * gate: `h->gate` is fp32, and so is the squeeze-excite MLP.
  * projection: the gated operand is bf16(fp32(x_bf16 * gate)) (bf16x8_gate: one fp32 multiply, then rounded), times
    the three weight planes (the fp32 folded weights exactly) or - planes = 1 - the first plane, bf16(fold32(w)) with
    fold32 = weights._fold; fp32 accumulation, + bias + the bf16 residual as loaded, rounded at the store.
  * head: as an unfused expand (weight planes as for the projection).  feat: fp32 mean of the bf16 head tensor.  The
    MLP runs on fp32 activations and fp32 weights.

The comparison helpers return metrics and never assert; `check` applies the bars to one tap.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Mapping

import numpy as np
import torch
import torch.nn.functional as F

from oracle import b0_ref

EPS = b0_ref._BN_EPS
BLOCKS = b0_ref.block_list()                               # (kernel, stride, expand, c_in, c_out) per block
# the blocks mbconv_late_kernel has an instance for (DFD_MB_LATE_TABLE): every 14 x 14 and 7 x 7 block except the
# stride-2 block 11
LATE_BLOCKS = frozenset(i for i in range(6, 16) if i != 11)
DEFAULT_LATE_SKIP = (1 << 8) | (1 << 9)


# --------------------------------------------------------------------------- configurations
@dataclasses.dataclass(frozen=True)
class Config:
    """One set of handle options (dfd_set_option names) and the launch plan it implies."""
    name: str
    bf16: bool = False
    planes: int = 3
    fuse_expand: int = 1
    fuse_stem: int = 1
    fuse_late: int = 1
    fuse_late_skip: int = DEFAULT_LATE_SKIP
    split_gemm: int = 1

    def options(self) -> Dict[str, int]:
        return {"bf16_activations": int(self.bf16), "bf16_weight_planes": self.planes, "fuse_expand": self.fuse_expand,
                "fuse_stem": self.fuse_stem, "fuse_late": self.fuse_late, "fuse_late_skip": self.fuse_late_skip,
                "split_gemm": self.split_gemm}

    def expand_fused(self, i: int) -> bool:
        """b0_forward_t: expand runs inside the depthwise launch when "fuse_expand" is on and a front kernel exists for
        the block (mbconv_tiles > 0): blocks 1-5 always, blocks 6-15 through mbconv_late_kernel when "fuse_late" is on
        and the block's bit of "fuse_late_skip" is clear."""
        if BLOCKS[i][2] == 1 or not self.fuse_expand:
            return False
        if 1 <= i <= 5:
            return True
        return i in LATE_BLOCKS and bool(self.fuse_late) and not (self.fuse_late_skip >> i) & 1

    def taps(self):
        names = ["stem"]
        for i, b in enumerate(BLOCKS):
            if b[2] != 1 and not self.expand_fused(i):
                names.append(f"b{i}.exp")
            names += [f"b{i}.dw", f"b{i}.gate", f"b{i}.out"]
        return names + ["head", "feat", "logit"]

    def rounds(self, name: str) -> bool:
        """True where the bf16 path stores the tap as bf16; gate, feat and logit stay fp32 there"""
        return self.bf16 and not (name.endswith(".gate") or name in ("feat", "logit"))


DEFAULT = Config("default")
FP32_CONFIGS = (
    Config("fuse0", fuse_expand=0, fuse_stem=0, fuse_late=0),
    Config("fuse1", fuse_late=0),
    DEFAULT,                                               # fuse = 2: the shipped defaults
    Config("late_all", fuse_late_skip=0),
    Config("split_gemm0", split_gemm=0),
)
BF16_CONFIGS = (
    Config("bf16_p3_fused", bf16=True, planes=3),
    Config("bf16_p3_unfused", bf16=True, planes=3, fuse_expand=0, fuse_stem=0),
    Config("bf16_p1_fused", bf16=True, planes=1),
    Config("bf16_p1_unfused", bf16=True, planes=1, fuse_expand=0, fuse_stem=0),
)


# --------------------------------------------------------------------------- tap layout
def parse(name: str):
    i, kind = name[1:].split(".")
    return int(i), kind


def tap_shape(name: str, n: int):
    """NCHW shape, or (n, C), of a tap (the device returns 4-d taps as NHWC)"""
    if name == "stem":
        return (n, 32, 112, 112)
    if name == "head":
        return (n, 1280, 7, 7)
    if name == "feat":
        return (n, 1280)
    if name == "logit":
        return (n, 1)
    i, kind = parse(name)
    _, s, e, ci, co = BLOCKS[i]
    hi = 112
    for b in BLOCKS[:i]:
        hi = -(-hi // b[1])
    ho = -(-hi // s)
    return {"exp": (n, ci * e, hi, hi), "dw": (n, ci * e, ho, ho), "gate": (n, ci * e), "out": (n, co, ho, ho)}[kind]


def tap_size(name: str, n: int) -> int:
    return int(np.prod(tap_shape(name, n)))


def from_tap(flat: np.ndarray, name: str, n: int) -> torch.Tensor:
    """device tap (NHWC, flattened) -> float64 NCHW tensor"""
    shp = tap_shape(name, n)
    a = torch.from_numpy(np.array(flat, np.float32))
    if len(shp) == 4:
        a = a.reshape(shp[0], shp[2], shp[3], shp[1]).permute(0, 3, 1, 2)
    return a.reshape(shp).double().contiguous()


def block_input(i: int) -> str:
    return "stem" if i == 0 else f"b{i - 1}.out"


def has_skip(i: int) -> bool:
    _, s, _, ci, co = BLOCKS[i]
    return s == 1 and ci == co


# --------------------------------------------------------------------------- rounding
def round_bits(t: torch.Tensor, bits: int, toward_zero: bool = False) -> torch.Tensor:
    """Round to `bits` significand bits (bf16: 8) in ONE rounding from t's precision, to nearest even or toward zero.
    Exponent range as bf16's (subnormals below 2^-126)."""
    a = t.detach().double().numpy()
    _, e = np.frexp(a)
    ulp = np.ldexp(1.0, np.maximum(e - bits, -133))
    q = a / ulp
    return torch.from_numpy((np.trunc(q) if toward_zero else np.rint(q)) * ulp).to(t.dtype)


def rne_bf16(t: torch.Tensor) -> torch.Tensor:
    return round_bits(t, 8)


def rtz_bf16(t: torch.Tensor) -> torch.Tensor:
    return round_bits(t, 8, toward_zero=True)


def bf16_ulp(t: torch.Tensor) -> torch.Tensor:
    """one bf16 ulp at |t| (float64)"""
    _, e = np.frexp(t.detach().double().numpy())
    return torch.from_numpy(np.ldexp(1.0, np.maximum(e - 8, -133)))


# --------------------------------------------------------------------------- numerics of one evaluation
def _ident(t):
    return t


@dataclasses.dataclass(frozen=True)
class Numerics:
    """What one evaluation does at the points a kernel could get wrong: the store of a tensor that reaches HBM, the
    gated projection operand, sigmoid, and the operands of the 1x1 convs.  PLAIN is exact arithmetic in the tensors'
    dtype; MIRROR the bf16 storage; the tests' mutants replace one hook."""
    store: Callable = _ident
    gated: Callable = _ident
    sigmoid: Callable = torch.sigmoid
    operand: Callable = _ident


PLAIN = Numerics()
MIRROR = Numerics(store=rne_bf16, gated=lambda t: rne_bf16(t.float().double()))


# --------------------------------------------------------------------------- the ops
def _net(sd):
    return {(k if k.startswith("net.") else "net." + k): v for k, v in sd.items()}


def _swish(x, num):
    return x * num.sigmoid(x)


def _bn(x, sd, p):
    return b0_ref._bn(x, sd, p, EPS)


def _pw(x, w, num):
    return F.conv2d(num.operand(x), num.operand(w))


def op_stem(sd, x, num=PLAIN):
    return _swish(_bn(b0_ref._same_conv(x, sd["net._conv_stem.weight"], 2), sd, "net._bn0"), num)


def op_expand(sd, i, a, num=PLAIN):
    p = f"net._blocks.{i}"
    return _swish(_bn(_pw(a, sd[p + "._expand_conv.weight"], num), sd, p + "._bn0"), num)


def op_dw(sd, i, a, num=PLAIN):
    p = f"net._blocks.{i}"
    y = b0_ref._same_conv(a, sd[p + "._depthwise_conv.weight"], BLOCKS[i][1], groups=a.shape[1])
    return _swish(_bn(y, sd, p + "._bn1"), num)


def mean_hw(t: torch.Tensor) -> torch.Tensor:
    """mean over H, W.  float32: a pairwise sum with every add in fp32 - torch's CPU reductions accumulate float32 in
    float64, which is no fp32 yardstick for the device's fp32 pooling."""
    if t.dtype != torch.float32:
        return t.mean(dim=(2, 3))
    s = t.reshape(t.shape[0], t.shape[1], -1)
    while s.shape[-1] > 1:
        if s.shape[-1] % 2:
            s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0] / float(t.shape[2] * t.shape[3])


def op_gate(sd, i, d, num=PLAIN):
    p = f"net._blocks.{i}"
    q = mean_hw(d)[:, :, None, None]
    q = _swish(F.conv2d(q, sd[p + "._se_reduce.weight"], sd[p + "._se_reduce.bias"]), num)
    q = F.conv2d(q, sd[p + "._se_expand.weight"], sd[p + "._se_expand.bias"])
    return num.sigmoid(q).flatten(1)


def op_out(sd, i, d, g, skip, num=PLAIN):
    p = f"net._blocks.{i}"
    y = _bn(_pw(num.gated(d * g[:, :, None, None]), sd[p + "._project_conv.weight"], num), sd, p + "._bn2")
    return y if skip is None else y + skip


def op_head(sd, a, num=PLAIN):
    return _swish(_bn(_pw(a, sd["net._conv_head.weight"], num), sd, "net._bn1"), num)


def _dw_unrounded(cfg, sd, i, get, num):
    """b{i}.dw before its store, from what the depthwise launch reads (module docstring)"""
    if BLOCKS[i][2] == 1:
        a = op_stem(sd, get("x"), num) if cfg.fuse_stem else get("stem")
    elif cfg.expand_fused(i):
        a = op_expand(sd, i, get(block_input(i)), num)
    else:
        a = get(f"b{i}.exp")
    return op_dw(sd, i, a, num)


@torch.no_grad()
def layer(cfg: Config, name: str, get: Callable[[str], torch.Tensor], sd, num: Numerics = PLAIN) -> torch.Tensor:
    """Reference of tap `name` from the taps it reads: `get(tap)` -> NCHW tensor in sd's dtype ("x": the input)."""
    sd = _net(sd)
    if name == "stem":
        return num.store(op_stem(sd, get("x"), num))
    if name == "head":
        return num.store(op_head(sd, get("b15.out"), num))
    if name == "feat":
        return mean_hw(get("head"))
    if name == "logit":
        return b0_ref.head(sd, get("feat"))
    i, kind = parse(name)
    if kind == "exp":
        return num.store(op_expand(sd, i, get(block_input(i)), num))
    if kind == "dw":
        return num.store(_dw_unrounded(cfg, sd, i, get, num))
    if kind == "gate":
        d = _dw_unrounded(cfg, sd, i, get, num) if cfg.bf16 else get(f"b{i}.dw")
        return op_gate(sd, i, d, num)
    if kind == "out":
        skip = get(block_input(i)) if has_skip(i) else None
        return num.store(op_out(sd, i, get(f"b{i}.dw"), get(f"b{i}.gate"), skip, num))
    raise KeyError(name)


# --------------------------------------------------------------------------- state dicts
def conv_bn_pairs():
    """(conv weight key, BatchNorm prefix) of every backbone conv that BN follows"""
    out = [("net._conv_stem.weight", "net._bn0")]
    for i, b in enumerate(BLOCKS):
        p = f"net._blocks.{i}"
        if b[2] != 1:
            out.append((p + "._expand_conv.weight", p + "._bn0"))
        out += [(p + "._depthwise_conv.weight", p + "._bn1"), (p + "._project_conv.weight", p + "._bn2")]
    return out + [("net._conv_head.weight", "net._bn1")]


def to_torch(sd: Mapping[str, np.ndarray], dtype=torch.float64):
    """torch copy of a numpy state dict, floating tensors in `dtype`"""
    return {k: torch.from_numpy(np.array(v)).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.array(v))
            for k, v in _net(sd).items()}


def kernel_state_dict(sd: Mapping[str, np.ndarray], cfg: Config):
    """float64 state dict of the weights as the device holds them - weights._fold (BN folded in float64, stored as
    fp32), with bf16_weight_planes = 1 the 1x1 convs of the split GEMM rounded to bf16 - and BN reduced to `+ bias`."""
    import rtdfd_amd

    sd = _net({k: np.asarray(v) for k, v in sd.items()})
    out = to_torch(sd)
    gemm_1x1 = {"net._conv_head.weight"}
    for i, b in enumerate(BLOCKS):
        gemm_1x1.add(f"net._blocks.{i}._project_conv.weight")
        if b[2] != 1 and not cfg.expand_fused(i):          # a fused expand always multiplies with the three planes
            gemm_1x1.add(f"net._blocks.{i}._expand_conv.weight")
    for wk, bn in conv_bn_pairs():
        w, bias = rtdfd_amd.weights._fold(sd[wk], None, sd, bn, EPS)
        w = torch.from_numpy(w).double()
        out[wk] = rne_bf16(w) if cfg.planes == 1 and wk in gemm_1x1 else w
        c = w.shape[0]
        out[bn + ".weight"] = torch.ones(c, dtype=torch.float64)
        out[bn + ".bias"] = torch.from_numpy(bias).double()
        out[bn + ".running_mean"] = torch.zeros(c, dtype=torch.float64)
        out[bn + ".running_var"] = torch.full((c,), 1.0 - EPS, dtype=torch.float64)
    return out


def stress_state_dict(seed: int = 0) -> Dict[str, np.ndarray]:
    """seeded_state_dict(seed) moved to the ranges trained EfficientNet weights have:
      * BN running_var log-uniform over 1e-3 .. 20 (over four decades, down to the BN eps; two channels per layer at
        1e-3); each channel's conv weights scaled by sqrt(var) times a log-uniform 0.4 .. 1.6 spread (wider spreads
        make the 16 blocks blow the activations up or wash the input out), running_mean ~ N(0, var): folded scales up
        to ~45, with the folded bias cancelling part of the conv;
      * gamma of both signs, |gamma| in 0.5 .. 1.5, exact zeros on 1/32 of the channels (at least one per layer);
        beta ~ N(0, 1);
      * squeeze-excite expand bias -15 on a tenth of the channels and +15 on another tenth: gates saturated below 1e-3
        and above 0.999."""
    import rtdfd_amd

    sd = _net(rtdfd_amd.weights.seeded_state_dict(seed))
    rs = np.random.RandomState(seed + 77)
    for wk, bn in conv_bn_pairs():
        c = sd[wk].shape[0]
        var = 10.0 ** rs.uniform(-3.0, 1.3, c)
        var[rs.choice(c, 2, replace=False)] = 1e-3
        spread = 10.0 ** rs.uniform(-0.4, 0.2, c)
        sd[wk] = (sd[wk] * (np.sqrt(var) * spread).reshape(-1, 1, 1, 1)).astype(np.float32)
        g = rs.uniform(0.5, 1.5, c) * np.where(rs.rand(c) < 0.5, -1.0, 1.0)
        g[rs.choice(c, max(1, c // 32), replace=False)] = 0.0
        sd[bn + ".weight"] = g.astype(np.float32)
        sd[bn + ".bias"] = rs.randn(c).astype(np.float32)
        sd[bn + ".running_mean"] = (rs.randn(c) * np.sqrt(var)).astype(np.float32)
        sd[bn + ".running_var"] = var.astype(np.float32)
    for i in range(len(BLOCKS)):
        k = f"net._blocks.{i}._se_expand.bias"
        b = sd[k].copy()
        pick = rs.permutation(b.size)
        tenth = max(1, b.size // 10)
        b[pick[:tenth]] = -15.0
        b[pick[tenth:2 * tenth]] = 15.0
        sd[k] = b
    return sd


# --------------------------------------------------------------------------- inputs
IMG_HI = (1.0 - 0.406) / 0.225          # 2.64: the top of the ImageNet-normalised pixel range (blue)
IMG_LO = (0.0 - 0.485) / 0.229          # -2.12: its bottom (red)
EDGE_NAMES = ("zeros", "const_hi", "const_lo", "hot_pixels", "checkerboard", "pm30", "random")


def edge_crops(seed: int = 0) -> np.ndarray:
    """(7, 3, 224, 224) float32: all zeros; the two ends of the normalised range; hot pixels on a dark crop at the four
    corners and the four edge midpoints, at even and odd coordinates (the TF-SAME (0, 1) padding of the stride-2
    convs); a Nyquist checkerboard; +-30 (swish / sigmoid tails, exp overflow); one random crop."""
    rs = np.random.RandomState(seed)
    x = np.zeros((7, 3, 224, 224), np.float32)
    x[1] = IMG_HI
    x[2] = IMG_LO
    x[3] = IMG_LO
    for y, xx in ((0, 0), (0, 223), (223, 0), (223, 223), (0, 112), (112, 0), (223, 111), (111, 223)):
        x[3, :, y, xx] = IMG_HI
    yy, xx = np.mgrid[0:224, 0:224]
    x[4] = np.where((yy + xx) % 2 == 0, IMG_HI, IMG_LO)
    x[5] = np.where(rs.rand(3, 224, 224) < 0.5, -30.0, 30.0)
    x[6] = rs.randn(3, 224, 224)
    return x


def random_crops(n: int, seed: int = 42) -> np.ndarray:
    """random normals at spread scales and offsets"""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, 3, 224, 224).astype(np.float32)
    scale = np.linspace(0.3, 2.0, n, dtype=np.float32).reshape(n, 1, 1, 1)
    shift = np.linspace(-1.0, 1.0, n, dtype=np.float32).reshape(n, 1, 1, 1)
    return x * scale + shift


@torch.no_grad()
def forward_taps(sd_torch, x: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Plain forward (no teacher forcing) in sd_torch's dtype: every tap in tap_shape's layout, "feat", "logit" and
    the input "x"."""
    taps: Dict[str, torch.Tensor] = {"x": x}
    taps["feat"] = b0_ref.extract_features(sd_torch, x, taps)
    taps["logit"] = b0_ref.head(sd_torch, taps["feat"])
    return {k: v.flatten(1) if k.endswith(".gate") else v for k, v in taps.items()}


# --------------------------------------------------------------------------- fp32 conditioning scale
def _bn_mag(c, sd, p):
    """|BN(conv)| bound from |conv| bound c: |a| c + |a mu| + |beta|, a = gamma / sqrt(var + eps)"""
    a = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + EPS)
    sh = (1, -1, 1, 1)
    return a.abs().reshape(sh) * c + ((a * sd[p + ".running_mean"]).abs() + sd[p + ".bias"].abs()).reshape(sh)


def _swish_mag(pre, m):
    """scale of swish(pre) when pre carries errors of scale m: |swish'(pre)| m + |swish(pre)|"""
    s = torch.sigmoid(pre)
    return (s + pre * s * (1 - s)).abs() * m + (pre * s).abs()


def _conv_swish_mag(sd, a, ma, wk, bn, stride=1, groups=1):
    """(swish(BN(conv(a))), its scale) for an input a of scale ma"""
    w = sd[wk]
    pre = _bn(b0_ref._same_conv(a, w, stride, groups=groups), sd, bn)
    return _swish(pre, PLAIN), _swish_mag(pre, _bn_mag(b0_ref._same_conv(ma, w.abs(), stride, groups=groups), sd, bn))


def _dw_mag(cfg, sd, i, get):
    """(b{i}.dw before its store, its scale), from what the depthwise launch reads"""
    p = f"net._blocks.{i}"
    if BLOCKS[i][2] == 1 and cfg.fuse_stem:
        x = get("x")
        a, ma = _conv_swish_mag(sd, x, x.abs(), "net._conv_stem.weight", "net._bn0", 2)
    elif cfg.expand_fused(i):
        b = get(block_input(i))
        a, ma = _conv_swish_mag(sd, b, b.abs(), p + "._expand_conv.weight", p + "._bn0")
    else:
        a = get("stem" if BLOCKS[i][2] == 1 else f"b{i}.exp")
        ma = a.abs()
    return _conv_swish_mag(sd, a, ma, p + "._depthwise_conv.weight", p + "._bn1", BLOCKS[i][1], a.shape[1])


@torch.no_grad()
def scale(cfg: Config, name: str, get: Callable[[str], torch.Tensor], sd) -> torch.Tensor:
    """fp32 conditioning scale u of every element of tap `name` (float64, from the same inputs as `layer`): the op
    evaluated on magnitudes - |weights| times |inputs| plus |biases| through each conv, BN and linear map, and through
    each activation its slope times that plus the activation's own value.  One fp32 evaluation of the op is off by a
    few eps * u; where terms cancel, u is far above |result|, and an fp32 result can be no closer than that."""
    sd = _net(sd)
    if name == "stem":
        x = get("x")
        return _conv_swish_mag(sd, x, x.abs(), "net._conv_stem.weight", "net._bn0", 2)[1]
    if name == "head":
        a = get("b15.out")
        return _conv_swish_mag(sd, a, a.abs(), "net._conv_head.weight", "net._bn1")[1]
    if name == "feat":
        return mean_hw(get("head").abs())
    if name == "logit":
        f = get("feat")
        m = f.abs()
        for lin, bn in (("net._fc.1", "net._fc.2"), ("net._fc.5", "net._fc.6")):
            w, b = sd[lin + ".weight"], sd[lin + ".bias"]
            g, beta, mu, var = (sd[bn + k] for k in (".weight", ".bias", ".running_mean", ".running_var"))
            a = g / torch.sqrt(var + 1e-5)
            m = a.abs() * (F.linear(m, w.abs(), b.abs()) + mu.abs()) + beta.abs()
            f = F.relu(a * (F.linear(f, w, b) - mu) + beta)
        return F.linear(m, sd["net._fc.9.weight"].abs(), sd["net._fc.9.bias"].abs())
    i, kind = parse(name)
    p = f"net._blocks.{i}"
    if kind == "exp":
        a = get(block_input(i))
        return _conv_swish_mag(sd, a, a.abs(), p + "._expand_conv.weight", p + "._bn0")[1]
    if kind == "dw":
        return _dw_mag(cfg, sd, i, get)[1]
    if kind == "gate":
        d, md = _dw_mag(cfg, sd, i, get) if cfg.bf16 else (get(f"b{i}.dw"), get(f"b{i}.dw").abs())
        w1, b1 = sd[p + "._se_reduce.weight"].flatten(1), sd[p + "._se_reduce.bias"]
        w2, b2 = sd[p + "._se_expand.weight"].flatten(1), sd[p + "._se_expand.bias"]
        zp = F.linear(mean_hw(d), w1, b1)
        uz = _swish_mag(zp, F.linear(mean_hw(md), w1.abs(), b1.abs()))
        sg = torch.sigmoid(F.linear(zp * torch.sigmoid(zp), w2, b2))
        return sg * (1 - sg) * F.linear(uz, w2.abs(), b2.abs()) + sg
    if kind == "out":
        xg = get(f"b{i}.dw") * get(f"b{i}.gate")[:, :, None, None]
        m = _bn_mag(F.conv2d(xg.abs(), sd[p + "._project_conv.weight"].abs()), sd, p + "._bn2")
        return m + get(block_input(i)).abs() if has_skip(i) else m
    raise KeyError(name)


# --------------------------------------------------------------------------- metrics
FLOOR_REL = 1e-6        # scales below 1e-6 of the tensor's largest are measured against that floor


def fp32_metrics(got: torch.Tensor, ref: torch.Tensor, u: torch.Tensor) -> Dict[str, float]:
    """rms: rms(d) / rms(ref).  max: the largest |d| / u over the elements, u = `scale` (floored at FLOOR_REL of its
    max): each element - and so each (image, channel) slice - is measured against its own scale, so neither a
    small-scale channel nor a small element is hidden by the tensor's max, and an element whose terms cancel is held
    to what fp32 can do with those terms."""
    ref = ref.double()
    d = got.double() - ref
    rr, dd = float(ref.pow(2).mean().sqrt()), float(d.pow(2).mean().sqrt())
    rms = dd / rr if rr > 0 else (0.0 if dd == 0 else float("inf"))
    floor = max(FLOOR_REL * float(u.max()), 1e-30)
    return {"rms": rms, "max": float((d.abs() / u.clamp_min(floor)).max())}


BF16_FLOOR = 2.0 ** -8  # elements below 1/256 of their scale u are counted in ulps at 2^-8 u


def bf16_metrics(got: torch.Tensor, mirror: torch.Tensor, u: torch.Tensor) -> Dict[str, float]:
    """diff: fraction of elements that are not bit-identical; ulp: the largest |d| in bf16 ulps of the larger magnitude,
    floored at BF16_FLOOR of the element's scale u: a result far below the terms it was summed from (a cancellation,
    a swish tail) carries the fp32 sum's error, a few eps * u, which no bf16 ulp of its own magnitude bounds"""
    got, mirror = got.double(), mirror.double()
    d = (got - mirror).abs()
    floor = torch.maximum(BF16_FLOOR * u, torch.full_like(u, FLOOR_REL * float(u.max())))
    ulp = bf16_ulp(torch.maximum(torch.maximum(got.abs(), mirror.abs()), floor))
    return {"diff": float((d > 0).double().mean()), "ulp": float((d / ulp).max())}


# --------------------------------------------------------------------------- bars
RMS_FACTOR, MAX_FACTOR = 4.0, 8.0
RMS_FLOOR, MAX_FLOOR = 2.0 ** -23, 2.0 ** -21       # for yardsticks that happen to be exact: 1 and 4 fp32 ulps
BF16_MAX_ULP, BF16_MAX_DIFF = 1.0, 0.01


def fp32_ratio(m: Dict[str, float], yard: Dict[str, float]) -> float:
    """the worse of the two metrics over its bar: <= 1 passes"""
    return max(m["rms"] / (RMS_FACTOR * yard["rms"] + RMS_FLOOR), m["max"] / (MAX_FACTOR * yard["max"] + MAX_FLOOR))


def yard_ratio(m: Dict[str, float], yard: Dict[str, float]) -> float:
    """HIP error / yardstick error, the worse of the two metrics (the yardstick floored as in the bar)"""
    return max(m["rms"] / max(yard["rms"], RMS_FLOOR), m["max"] / max(yard["max"], MAX_FLOOR))


def bf16_ratio(m: Dict[str, float]) -> float:
    return max(m["ulp"] / BF16_MAX_ULP, m["diff"] / BF16_MAX_DIFF)


# taps with one value per crop: a rms over one batch is too few draws for a ratio of two of them (the logit's
# conditioning scale is loose: a sum that cancels through two BN layers); their rms bar is applied to the errors of
# several batches pooled (`pooled_rms_ratio`), their max bar per batch
POOLED = ("logit",)


def pooled_rms_ratio(sqs) -> Dict[str, float]:
    """rms bar over several evaluations of one op, pooled: sqs = the "sq" entries of `check` (sum d^2, sum d_yard^2,
    sum ref^2) -> {"ratio": <= 1 passes, "vs_yard"}"""
    d, y, r = (sum(q[k] for q in sqs) for k in range(3))
    hip, yard = (d / r) ** 0.5, (y / r) ** 0.5
    return {"ratio": hip / (RMS_FACTOR * yard + RMS_FLOOR), "vs_yard": hip / max(yard, RMS_FLOOR)}


def check(cfg: Config, name: str, get64, get32, sd64, sd32, ksd) -> Dict[str, float]:
    """One tap against its bar -> {"kind": "fp32" | "bf16", "ratio": <= 1 passes, metrics, "vs_yard" and "sq" for
    fp32}.  get64 / get32: the HIP taps as float64 / float32; sd64 / sd32: to_torch(sd) in both dtypes; ksd:
    kernel_state_dict(sd, cfg) (bf16 configs).  POOLED taps: "ratio" is the max bar's only."""
    got = get64(name)
    u = scale(cfg, name, get64, sd64)
    if cfg.rounds(name):
        m = bf16_metrics(got, layer(cfg, name, get64, ksd, MIRROR), u)
        return {"kind": "bf16", "ratio": bf16_ratio(m), **m}
    ref = layer(cfg, name, get64, sd64)
    y = layer(cfg, name, get32, sd32).double()
    yard, m = fp32_metrics(y, ref, u), fp32_metrics(got, ref, u)
    ratio = m["max"] / (MAX_FACTOR * yard["max"] + MAX_FLOOR) if name in POOLED else fp32_ratio(m, yard)
    sq = (float((got - ref).pow(2).sum()), float((y - ref).pow(2).sum()), float(ref.pow(2).sum()))
    return {"kind": "fp32", "ratio": ratio, "vs_yard": yard_ratio(m, yard), "sq": sq, **m}

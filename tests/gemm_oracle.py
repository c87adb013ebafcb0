"""Test-side oracle of ONE split-GEMM call (csrc/gemm_split.hip, gemm_split_impl.h), for dfd_gemm_tap.

  * float64 reference - `evaluate(case, inp, torch.float64)`: pointwise act((x * g) W^T + b [+ R]) [+ R] with torch
    matmuls, conv mode with torch.nn.functional.conv2d on the NHWC data;
  * fp32 yardstick - the same call in float32 on the CPU;
  * conditioning scale u - `scale(case, inp)`: the op on magnitudes, |x g| |W|^T + |b| (+ |R| in front of the
    activation), through the activation as b0_layer_oracle._swish_mag does it (|slope| times that plus the activation's own
    value; relu / PReLU: slope bound max(1, |a|), which also covers an element the error carries across zero), + |R|
    behind it;
  * bf16 mirror - `mirror(case, inp)`: float64 arithmetic on the operands as the bf16 path holds them - x as stored,
    bf16(fp32(x g)) after the gate (bf16x8_gate), W whole (planes = 3) or bf16(W) (planes = 1), R as stored - and the
    result rounded to bf16 once;
  * `emulate(case, inp, mutant)` - the kernel's arithmetic in float64: x and W split into three bf16 terms, the six
    products with i + j <= 2 summed, the sum rounded to fp32, the epilogue in fp32.  Its mutants are the mistakes the GPU
    assertions must catch (tests/test_gemm_oracle.py proves that they do, and where).

The bars are b0_layer_oracle's (fp32_metrics / fp32_ratio, bf16_metrics / bf16_ratio); `check` applies them.

Input families (`make_inputs`, seeded):
  random   normal x with per-row scales over two decades, normal W / sqrt(K) with per-channel scales as
           b0_layer_oracle.stress_state_dict draws them, gates from saturated-low to saturated-high
  exact_x  |x| integers in [2^(b-1), 2^b), 2^b = 2^24 / (4K) (18 bits at K = 16: all three bf16 terms of x carry bits; 17
           at K = 32: the signed terms of round-to-nearest hold 8 + 9 bits in two), W in {+-1, +-2}, small integer bias,
           no activation: every partial sum of every term product is an integer below 2^24, so the result equals float64
           bit for bit whatever the accumulation order
  exact_w  the mirror image: wide integer W, x in {+-1, +-2}
  cancel   w[k+1] = -w[k], x[k+1] = x[k] (1 + d), d in 2^-20 .. 2^-12: the output lives in the low-order terms

CASES lists every call tests/test_gemm_direct_gpu.py makes; both test files read it.
"""
from __future__ import annotations

import dataclasses
import zlib
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import b0_layer_oracle as B

FAMILIES = ("random", "exact_x", "exact_w", "cancel")


@dataclasses.dataclass(frozen=True)
class Case:
    group: str                     # "pointwise" | "pw8" | "pw9" | "gated" | "conv" | "bf16" | "exact"
    M: int
    K: int
    N: int
    HW: int = 1
    act: Optional[str] = None      # None | "swish" | "relu" | "prelu"
    res: Optional[str] = None      # None | "after" | "first"
    gated: bool = False
    bf16: bool = False
    planes: int = 3
    family: str = "random"
    conv: Optional[Tuple[int, ...]] = None      # (n_img, H, W, Cin, ksize, stride, pad, dil)
    expect: str = ""               # "pw8" / "pw9": the case was built for that kernel, which must be among its candidates

    @property
    def name(self) -> str:
        c = "" if self.conv is None else "-conv" + "x".join(str(v) for v in self.conv)
        return (f"{self.group}-M{self.M}-K{self.K}-N{self.N}-HW{self.HW}-{self.act or 'none'}-res{self.res or 'none'}"
                f"{'-gated' if self.gated else ''}{'-bf16p%d' % self.planes if self.bf16 else ''}-{self.family}{c}")

    @property
    def seed(self) -> int:
        return zlib.crc32(self.name.encode()) & 0x7FFFFFFF

    def conv_dict(self):
        return dict(zip(("n_img", "H", "W", "Cin", "ksize", "stride", "pad", "dil"), self.conv))


def conv_case(n_img, H, W, Cin, ksize, stride, pad, dil, Cout, act, res) -> Case:
    span = dil * (ksize - 1) + 1
    ho, wo = (H + 2 * pad - span) // stride + 1, (W + 2 * pad - span) // stride + 1
    return Case("conv", n_img * ho * wo, ksize * ksize * Cin, Cout, ho * wo, act, res,
                conv=(n_img, H, W, Cin, ksize, stride, pad, dil))


# --------------------------------------------------------------------------- the case list
ACTS = (None, "swish", "relu", "prelu")
RESIDUALS = (None, "after", "first")
PW_M = (1, 17, 127, 129, 300)
PW_KN = ((16, 2), (24, 10), (40, 30), (72, 64), (104, 100), (264, 196))      # N % 4 != 0 first, then N % 4 == 0
PW8_N = (16, 24, 40, 48)
PW8_K = (16, 32, 72, 96, 144, 160, 232, 256)
PW8_M = (1, 15, 33, 8200)
PW9_KN = ((72, 192), (80, 480), (112, 672), (128, 196))
PW9_M = (1, 127, 129, 588)
GATED_HW = (1, 49, 196)
GATED_KN = ((96, 24), (240, 40), (104, 30))


def _pointwise_cases():
    """every (M, (K, N)); the twelve act x residual pairings cycle so that each appears at an N % 4 != 0 and at an
    N % 4 == 0 shape (15 calls each)"""
    pairs = [(a, r) for a in ACTS for r in RESIDUALS]
    out = []
    for i, (k, n) in enumerate(PW_KN):
        for j, m in enumerate(PW_M):
            a, r = pairs[(i * len(PW_M) + j) % len(pairs)]
            out.append(Case("pointwise", m, k, n, act=a, res=r))
    return out


def _pw8_cases():
    """every K x every M ungated (N cycles, residual on every other call, activations none / swish / relu), every K
    x HW in {16, 64} gated with M = 5 HW; a bf16 subset of both (planes 3 and 1); five gated calls at HW = 80 / 144"""
    acts = (None, "swish", "relu")
    out = []
    for i, k in enumerate(PW8_K):
        for j, m in enumerate(PW8_M):
            n = PW8_N[(i + j) % 4]
            out.append(Case("pw8", m, k, n, act=acts[(i + j) % 3], res="after" if (i + j) % 2 else None, expect="pw8"))
            if j == (i % 4):
                out.append(Case("pw8", m, k, n, act=acts[i % 3], res="after" if i % 2 == 0 else None, bf16=True,
                                planes=3 if i % 2 else 1, expect="pw8"))
        for j, hw in enumerate((16, 64)):
            n = PW8_N[(i + 2 * j + 1) % 4]
            out.append(Case("pw8", 5 * hw, k, n, hw, act=acts[(i + j) % 3], res="after" if (i + j) % 2 == 0 else None, gated=True,
                            expect="pw8"))
            if (i + j) % 4 == 0:
                out.append(Case("pw8", 5 * hw, k, n, hw, res="after", gated=True, bf16=True, planes=3 if j else 1, expect="pw8"))
    # HW = 16 and 64 give a block whole images (tiles per image <= tiles per block): a block that STARTS inside one image
    # and ends in the next - both staged gate rows, `tsplit` - needs more tiles per image than waves and no multiple of them
    for i, (k, hw) in enumerate(((16, 80), (72, 80), (144, 80), (256, 144))):
        out.append(Case("pw8", 5 * hw, k, PW8_N[i], hw, act=acts[i % 3], res="after" if i % 2 else None, gated=True, expect="pw8"))
    out.append(Case("pw8", 5 * 80, 96, 24, 80, res="after", gated=True, bf16=True, planes=3, expect="pw8"))
    return out


def _pw9_cases():
    return [Case("pw9", m, k, n, act="swish" if (i + j) % 2 else None, expect="pw9")
            for i, (k, n) in enumerate(PW9_KN) for j, m in enumerate(PW9_M)]


def _gated_cases():
    """HW x {3 HW, 3 HW - 5} x (K, N); HW = 1 has no 3 HW - 5"""
    out = []
    for i, hw in enumerate(GATED_HW):
        for m in (3 * hw, 3 * hw - 5):
            for j, (k, n) in enumerate(GATED_KN):
                if m > 0:
                    out.append(Case("gated", m, k, n, hw, act=(None, "swish")[(i + j) % 2], res=(None, "after")[j % 2], gated=True))
    return out


def _conv_cases():
    """3 images; sixteen calls: Cin, stride, pad and dil walk all sixteen combinations, ksize cycles through 1, 2, 3, the
    image size, Cout, the activation and the side of the residual are mixed in from those bits
    (tests/test_gemm_oracle.py asserts every value, every activation x residual pairing and dilation on a k x k kernel)"""
    out = []
    for i in range(16):
        b = [(i >> s) & 1 for s in range(4)]
        cin, stride, pad, dil = (32, 64)[b[0]], (1, 2)[b[1]], (0, 1)[b[2]], (1, 2)[b[3]]
        h, w = ((5, 7), (9, 6))[b[0] ^ b[1] ^ b[2]]
        cout = (10, 64)[b[1] ^ b[3]]
        act = ("prelu", "relu")[b[0] ^ b[3]]
        res = ("first", "after")[b[2] ^ b[3] ^ b[1]]
        out.append(conv_case(3, h, w, cin, (1, 2, 3)[(i + i // 3) % 3], stride, pad, dil, cout, act, res))
    return out


def _bf16_cases():
    """the bf16-activation path on a subset of the pointwise and gated cases, planes 3 and 1 (pw8's subset is in its group)"""
    out = []
    for i, (k, n) in enumerate(PW_KN):
        out.append(Case("bf16", PW_M[(i + 1) % 5], k, n, act=ACTS[i % 4], res=RESIDUALS[i % 3], bf16=True, planes=(3, 1)[i % 2]))
    for i, hw in enumerate((49, 196)):
        for j, (k, n) in enumerate(GATED_KN[:2]):
            out.append(Case("bf16", 3 * hw - 5 * j, k, n, hw, act=(None, "swish")[j], res=(None, "after")[i], gated=True, bf16=True,
                            planes=(3, 1)[(i + j) % 2]))
    return out


def _exact_cases():
    """both exact families at K = 16 and 32 on one shape per kernel family: pw6 / pw7 (N % 4 != 0), pw8; pw9 has no
    instance below K = 72, so it gets K = 72 (x below 2^24 / 288: two terms carry bits there)"""
    out = []
    for fam in ("exact_x", "exact_w"):
        for k in (16, 32):
            out.append(Case("exact", 129, k, 30, family=fam))
            out.append(Case("exact", 33, k, 24, family=fam, expect="pw8"))
        out.append(Case("exact", 127, 72, 192, family=fam, expect="pw9"))
    return out


# the witnesses of tests/test_gemm_oracle.py's mutants (cancel / random at K = 16 and 24, the gated and tail cases are
# in the groups above)
def _witness_cases():
    return [Case("pointwise", 129, 16, 2, family="cancel"), Case("pointwise", 129, 24, 10, family="cancel")]


CASES = (_pointwise_cases() + _witness_cases() + _pw8_cases() + _pw9_cases() + _gated_cases() + _conv_cases() + _bf16_cases() +
         _exact_cases())
GROUPS = ("pointwise", "pw8", "pw9", "gated", "conv", "bf16", "exact")
# refused shapes: (K, N) pointwise at M = 17, and one conv with Cin = 16
REFUSED_POINTWISE = ((12, 16), (20, 16))
REFUSED_CONV = dict(n_img=1, H=5, W=7, Cin=16, ksize=3, stride=1, pad=1, dil=1)


# --------------------------------------------------------------------------- inputs
def _bf16_round(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def to_bits(a: np.ndarray) -> np.ndarray:
    """bf16-valued float32 -> uint16 bit patterns"""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _wide_ints(rs, shape, k):
    """+- integers in [2^(b-1), 2^b) with random low bits, 2^b = 2^24 / (4K) rounded down to a power of two"""
    b = int(np.floor(np.log2(2 ** 24 / (4 * k))))
    mag = (1 << (b - 1)) + rs.randint(0, 1 << (b - 1), shape)
    return (mag * rs.choice([-1, 1], shape)).astype(np.float32)


def _small_ints(rs, shape):
    return rs.choice([-2.0, -1.0, 1.0, 2.0], shape).astype(np.float32)


def make_inputs(case: Case) -> Dict[str, np.ndarray]:
    """-> x (M, K) - conv: (n_img, H, W, Cin) -, w (N, K) - conv: (N, ksize, ksize, Cin) -, bias (N,) or (2N,) = bias,
    slopes, gate (images, K) or None, res (M, N) or None; all float32 (bf16 cases: x and res hold bf16 values)"""
    rs = np.random.RandomState(case.seed)
    m, k, n = case.M, case.K, case.N
    xshape = (m, k) if case.conv is None else (case.conv[0] * case.conv[1] * case.conv[2], case.conv[3])
    fam = case.family
    if fam == "exact_x":
        x, w = _wide_ints(rs, xshape, k), _small_ints(rs, (n, k))
        bias = rs.randint(-8, 9, n).astype(np.float32)
    elif fam == "exact_w":
        x, w = _small_ints(rs, xshape), _wide_ints(rs, (n, k), k)
        bias = rs.randint(-8, 9, n).astype(np.float32)
    else:
        x = (rs.randn(*xshape) * 10.0 ** rs.uniform(-1.0, 1.0, (xshape[0], 1))).astype(np.float32)
        var = 10.0 ** rs.uniform(-3.0, 1.3, n)
        cs = np.sqrt(var) * 10.0 ** rs.uniform(-0.4, 0.2, n)
        w = (rs.randn(n, k) / np.sqrt(k) * cs[:, None]).astype(np.float32)
        bias = (rs.randn(n) * cs).astype(np.float32)
        if fam == "cancel":
            d = (2.0 ** rs.uniform(-20.0, -12.0, (xshape[0], k // 2))).astype(np.float32)
            x[:, 1::2] = x[:, 0::2] * (np.float32(1.0) + d)
            w[:, 1::2] = -w[:, 0::2]
            bias = (bias * np.float32(2.0 ** -14)).astype(np.float32)
    if case.bf16:
        x = _bf16_round(x)
    inp = {"x": x.reshape((m, k) if case.conv is None else case.conv[:4]),
           "w": w if case.conv is None else w.reshape(n, case.conv[4], case.conv[4], case.conv[3])}
    if case.act == "prelu":
        bias = np.concatenate([bias, rs.uniform(-0.5, 1.5, n).astype(np.float32)])
    inp["bias"] = bias
    inp["gate"] = None
    if case.gated:
        g = 1.0 / (1.0 + np.exp(-3.0 * rs.randn(-(-m // case.HW), k)))
        pick = rs.rand(*g.shape)
        g = np.where(pick < 0.1, 1e-3 * rs.rand(*g.shape), np.where(pick > 0.9, 1.0 - 1e-3 * rs.rand(*g.shape), g))
        inp["gate"] = g.astype(np.float32)
    inp["res"] = None
    if case.res:
        r = (rs.randn(m, n) * (np.abs(w).reshape(n, -1).sum(1) * np.abs(x).mean() + np.abs(bias[:n]))).astype(np.float32)
        if fam.startswith("exact"):
            r = rs.randint(-64, 65, (m, n)).astype(np.float32)
        inp["res"] = _bf16_round(r) if case.bf16 else r
    return inp


# --------------------------------------------------------------------------- the op
def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _act(pre, act, slopes):
    if act == "swish":
        return pre * torch.sigmoid(pre)
    if act == "relu":
        return torch.relu(pre)
    if act == "prelu":
        return torch.where(pre >= 0, pre, pre * slopes)
    return pre


def _linear(case, x, w, b):
    """x (gated already) and w in one dtype -> (M, N) pre-activation without residual"""
    if case.conv is None:
        return x @ w.t() + b
    _, _, _, _, _, stride, pad, dil = case.conv
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, stride=stride, padding=pad, dilation=dil)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def _gate_rows(case, gate, shift=0):
    img = torch.arange(case.M) // case.HW + shift
    return gate[img.clamp(0, gate.shape[0] - 1)]


def _finish(case, pre, bias, res):
    n = case.N
    if res is not None and case.res == "first":
        pre = pre + res
    y = _act(pre, case.act, bias[n:] if case.act == "prelu" else None)
    return y + res if res is not None and case.res == "after" else y


@torch.no_grad()
def evaluate(case: Case, inp, dtype, gated=B._ident, wop=B._ident) -> torch.Tensor:
    """the call in `dtype` (float64: the reference, float32: the yardstick); gated / wop: hooks of the bf16 mirror"""
    x, w, bias, gate, res = (_t(inp[k], dtype) for k in ("x", "w", "bias", "gate", "res"))
    if gate is not None:
        x = gated(x * _gate_rows(case, gate))
    return _finish(case, _linear(case, x, wop(w), bias[:case.N]), bias, res)


@torch.no_grad()
def scale(case: Case, inp) -> torch.Tensor:
    x, w, bias, gate, res = (_t(inp[k], torch.float64) for k in ("x", "w", "bias", "gate", "res"))
    if gate is not None:
        x = x * _gate_rows(case, gate)
    n = case.N
    m = _linear(case, x.abs(), w.abs(), bias[:n].abs())
    pre = _linear(case, x, w, bias[:n])
    if res is not None and case.res == "first":
        m, pre = m + res.abs(), pre + res
    if case.act == "swish":
        m = B._swish_mag(pre, m)
    elif case.act == "relu":
        m = m + torch.relu(pre)
    elif case.act == "prelu":
        a = bias[n:]
        m = a.abs().clamp_min(1.0) * m + torch.where(pre >= 0, pre, pre * a).abs()
    return m + res.abs() if res is not None and case.res == "after" else m


@torch.no_grad()
def mirror(case: Case, inp) -> torch.Tensor:
    y = evaluate(case, inp, torch.float64, gated=B.MIRROR.gated, wop=B.rne_bf16 if case.planes == 1 else B._ident)
    return B.rne_bf16(y)


# --------------------------------------------------------------------------- the kernel's arithmetic
PRODUCTS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))      # (weight term, activation term), s6_products' order
MUTANTS = tuple(f"drop_w{j}x{i}" for j, i in PRODUCTS) + ("gate_prev", "gate_next", "tail", "res_side", "dup_row")


def split3(a: torch.Tensor):
    """fp32 values (as float64) -> three bf16 terms whose sum is exact (split8 / split_weights_kernel)"""
    a0 = B.rne_bf16(a)
    r1 = a - a0
    a1 = B.rne_bf16(r1)
    return a0, a1, B.rne_bf16(r1 - a1)


@torch.no_grad()
def emulate(case: Case, inp, mutant: Optional[str] = None) -> torch.Tensor:
    """pointwise fp32 calls: the six products in float64, the sum rounded to fp32, the epilogue in fp32 -> float32.
    mutant: one of MUTANTS - a dropped product, the gate row of the neighbouring image, the re-read activations of the K
    tail (k >= K up to the next multiple of 32: every octet past the row end re-reads the row's last eight values) met by
    non-zero weights, the residual on the other side of the activation, the last row stored over its neighbour."""
    assert case.conv is None and not case.bf16
    x, w, bias, gate, res = (_t(inp[k], torch.float32) for k in ("x", "w", "bias", "gate", "res"))
    if gate is not None:
        x = x * _gate_rows(case, gate, {"gate_prev": -1, "gate_next": 1}.get(mutant, 0))      # one fp32 multiply
    xs, ws = split3(x.double()), split3(w.double())
    acc = torch.zeros(case.M, case.N, dtype=torch.float64)
    for j, i in PRODUCTS:
        if mutant != f"drop_w{j}x{i}":
            acc += xs[i] @ ws[j].t()
    if mutant == "tail" and case.K % 32:
        octets = (32 - case.K % 32) // 8
        acc += octets * (x[:, -8:].double() @ w[:, -8:].double().t())
    pre = acc.float() + bias[:case.N]
    if mutant == "res_side" and res is not None:
        case = dataclasses.replace(case, res="first" if case.res == "after" else "after")
    y = _finish(case, pre, bias, res)
    if mutant == "dup_row" and case.M > 1:
        y[-2] = y[-1]
    return y


# --------------------------------------------------------------------------- bars
class Reference:
    """reference, yardstick metrics and scale of one case, computed once"""

    def __init__(self, case: Case, inp=None):
        self.case, self.inp = case, make_inputs(case) if inp is None else inp
        self.u = scale(case, self.inp)
        if case.bf16:
            self.mirror = mirror(case, self.inp)
        else:
            self.ref = evaluate(case, self.inp, torch.float64)
            self.yard = B.fp32_metrics(evaluate(case, self.inp, torch.float32).double(), self.ref, self.u)

    def check(self, got: np.ndarray) -> Dict[str, float]:
        """{"ratio": <= 1 passes, "vs_yard" (fp32), the metrics, "exact": bit-equal to float64 (exact families)}"""
        if self.case.bf16:
            m = B.bf16_metrics(torch.from_numpy(from_bits(got)), self.mirror, self.u)
            return {"ratio": B.bf16_ratio(m), **m}
        g = torch.from_numpy(np.ascontiguousarray(got, np.float32)).double()
        m = B.fp32_metrics(g, self.ref, self.u)
        out = {"ratio": B.fp32_ratio(m, self.yard), "vs_yard": B.yard_ratio(m, self.yard), **m}
        if self.case.family.startswith("exact"):
            out["exact"] = bool(torch.equal(g, self.ref))
        return out

    def passes(self, got: np.ndarray) -> bool:
        c = self.check(got)
        return c["ratio"] <= 1.0 and c.get("exact", True)

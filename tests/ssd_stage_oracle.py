"""Test-side per-launch oracle of the SSD face detector, teacher-forced by the HIP path's own taps (dfd_ssd_tap), and the
seeded inputs of its tail (dfd_ssd_detection_tap).  Modelled on tests/mtcnn_stage_oracle.py.

  * float64 references - `layer(name, get, sd64, arch)`: the op that writes one tensor of `arch.LAYERS` (or one
    "<source>.head"), from its input tap(s): convolution with dilation / stride / residual before the ReLU, ceil-mode
    max pool, L2 normalise (1e-10 inside the root), per-channel affine, add; "conv1" from the resized u8 image
    (`get("data")`: the u8 values) through x * IN_SCALE + IN_SHIFT with zero padding of the TRANSFORMED blob;
  * fp32 yardstick - the same call on float32 taps and the float32 state dict: torch's plain fp32 evaluation;
  * `scale(name, get, sd64, arch)` - the op on magnitudes: conv(|x|, |w|) + |b| (+ |res|), the max of the window's
    scales through a pool, |x| / root * |scale| through the normalise, |x| |scale| + |shift|, |x| + |other|;
  * `check` - the classifier suite's metrics and bar (tests/b0_layer_oracle.py), nothing of its own;
  * decode - `decode64` (float64) / `decode32` (numpy float32, oracle.ssd_ref's own arithmetic: the yardstick) with the
    boxes' magnitude scale |v0 l0 pw| + |pcx| + 0.5 exp(v2 l2) pw (likewise in y); the probability's scale is 1: the
    thresholds on it are absolute;
  * DetectionOutput is exact: oracle.ssd_ref.detection_output, whose float32 arithmetic is the kernel's;
    `detection_output_brute` restates it independently (vectorised all-pairs overlaps) for tests/test_ssd_stage_oracle.py.

Case builders (all seeded): `variant_arch` (non-integer input transform, affine / add layers, optionally a second reader
of conv1), `head_case` (injected head tensors), `nms_cases` (injected (boxes, prob) sets; each states what it is for).
"""
from __future__ import annotations

import types
from typing import Callable, Dict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import imgproc_ref, ssd_ref
from tests.b0_layer_oracle import MAX_FACTOR, MAX_FLOOR, RMS_FACTOR, RMS_FLOOR, fp32_metrics, fp32_ratio, yard_ratio  # noqa: F401

P = 8732
TOPK = 400
F32 = np.float32


# --------------------------------------------------------------------------- geometry
def shapes(arch) -> Dict[str, tuple]:
    """tensor name -> (channels, edge), heads included, for any arch (affine / add keep their input's shape)"""
    out = {"data": (3, arch.INPUT)}
    for name, kind, a in arch.LAYERS:
        if kind == "conv":
            src, ci, co, k, s, p, d, _, _ = a
            out[name] = (co, (out[src][1] + 2 * p - d * (k - 1) - 1) // s + 1)
        elif kind == "maxpool":
            src, k, s = a
            out[name] = (out[src][0], -(-(out[src][1] - k) // s) + 1)
        else:
            out[name] = out[a[0]]
    for src, c, m, _, _, ars, _ in arch.SOURCES:
        out[src + ".head"] = (arch.priors_per_cell(ars) * 6, m)
    return out


def to_nchw(tap: np.ndarray, dtype) -> torch.Tensor:
    """device tap (n, h, w, c) -> torch (n, c, h, w)"""
    return torch.from_numpy(np.ascontiguousarray(tap)).to(dtype).permute(0, 3, 1, 2).contiguous()


def data_u8(frame: np.ndarray, arch) -> np.ndarray:
    """(1, 300, 300, 3) uint8: the resized image conv1 reads (bit-exact with the device's resize)"""
    return imgproc_ref.resize_linear_u8(frame, arch.INPUT, arch.INPUT)[None]


def _kinds(arch):
    return {name: (kind, a) for name, kind, a in arch.LAYERS}


def _head_wb(sd, src):
    return torch.cat([sd[src + "_loc.weight"], sd[src + "_conf.weight"]], 0), torch.cat([sd[src + "_loc.bias"], sd[src + "_conf.bias"]])


def inputs_of(name: str, arch):
    """names of the taps the launch that writes `name` reads"""
    if name.endswith(".head"):
        return (name[:-5],)
    kind, a = _kinds(arch)[name]
    if kind == "conv":
        return (a[0],) if a[8] is None else (a[0], a[8])
    if kind == "add":
        return (a[0], a[1])
    return (a[0],)


def _blob(x_u8: torch.Tensor, arch) -> torch.Tensor:
    """u8 values -> the transformed blob x * IN_SCALE + IN_SHIFT (the float32 constants the device receives)"""
    sc = torch.from_numpy(np.asarray(arch.IN_SCALE, F32)).to(x_u8.dtype).view(1, 3, 1, 1)
    sh = torch.from_numpy(np.asarray(arch.IN_SHIFT, F32)).to(x_u8.dtype).view(1, 3, 1, 1)
    return x_u8 * sc + sh


def _eval(name: str, get: Callable[[str], torch.Tensor], sd, arch, mag: bool):
    """the op (mag = False) or the op on magnitudes (mag = True)"""
    ab = (lambda t: t.abs()) if mag else (lambda t: t)
    if name.endswith(".head"):
        src = name[:-5]
        w, b = _head_wb(sd, src)
        return F.conv2d(ab(get(src)), ab(w), ab(b), padding=1)
    kind, a = _kinds(arch)[name]
    if kind == "conv":
        src, ci, co, k, s, p, d, relu, res = a
        x = get(src)
        if src == "data":
            x = _blob(x, arch)                                # zero padding applies to the transformed blob
        y = F.conv2d(ab(x), ab(sd[name + ".weight"]), ab(sd[name + ".bias"]), stride=s, padding=p, dilation=d)
        if res is not None:
            y = y + ab(get(res))
        return y if mag or not relu else F.relu(y)
    if kind == "maxpool":
        src, k, s = a
        return F.max_pool2d(ab(get(src)), k, s, 0, ceil_mode=True)
    if kind == "l2norm":
        v = get(a[0])
        return ab(v) / torch.sqrt((v * v).sum(1, keepdim=True) + 1e-10) * ab(sd[name + ".scale"]).view(1, -1, 1, 1)
    if kind == "affine":
        src, c, relu = a
        y = ab(get(src)) * ab(sd[name + ".scale"]).view(1, -1, 1, 1) + ab(sd[name + ".shift"]).view(1, -1, 1, 1)
        return y if mag or not relu else F.relu(y)
    if kind == "add":
        src, other, c, relu = a
        y = ab(get(src)) + ab(get(other))
        return y if mag or not relu else F.relu(y)
    raise KeyError(name)


@torch.no_grad()
def layer(name: str, get, sd, arch) -> torch.Tensor:
    """One launch from its input taps get(input name), in the dtype of sd: a name of arch.LAYERS or "<source>.head"
    ((1, p * 6, m, m): p * 4 loc channels, then p * 2 logits, as the fused head convolution writes them)"""
    return _eval(name, get, sd, arch, False)


@torch.no_grad()
def scale(name: str, get, sd, arch) -> torch.Tensor:
    return _eval(name, get, sd, arch, True)


@torch.no_grad()
def pooled_conv1(get, sd, arch, pool: str = "pool1"):
    """the fused launch conv1 + ReLU + pool1 from the image -> (value, scale)"""
    src, k, s = _kinds(arch)[pool][1]
    return (F.max_pool2d(layer(src, get, sd, arch), k, s, 0, ceil_mode=True),
            F.max_pool2d(scale(src, get, sd, arch), k, s, 0, ceil_mode=True))


def compare(name: str, got: torch.Tensor, ref: torch.Tensor, yard: torch.Tensor, u: torch.Tensor) -> dict:
    """HIP result, float64 reference, fp32 yardstick and scale -> {"tap", "ratio": <= 1 passes, "vs_yard", "yard", metrics}"""
    assert got.shape == ref.shape == yard.shape == u.shape, (name, got.shape, ref.shape, yard.shape, u.shape)
    ym, m = fp32_metrics(yard.double(), ref, u), fp32_metrics(got.double(), ref, u)
    return {"tap": name, "ratio": fp32_ratio(m, ym), "vs_yard": yard_ratio(m, ym), "yard": ym, **m}


def check(name: str, got: torch.Tensor, get64, get32, sd64, sd32, arch) -> dict:
    """One floating launch against the classifier suite's bar.  got: the HIP tap as float64 NCHW."""
    return compare(name, got, layer(name, get64, sd64, arch), layer(name, get32, sd32, arch), scale(name, get64, sd64, arch))


def order(arch):
    """every launch: the layers in plan order, then the six heads"""
    return [n for n, _, _ in arch.LAYERS] + [s[0] + ".head" for s in arch.SOURCES]


@torch.no_grad()
def chain(frame: np.ndarray, sd, arch) -> Dict[str, torch.Tensor]:
    """every tap from the image, each launch fed by the previous one's result, in the dtype of sd"""
    dtype = next(iter(sd.values())).dtype
    taps = {"data": to_nchw(data_u8(frame, arch), dtype)}
    for name in order(arch):
        taps[name] = layer(name, taps.__getitem__, sd, arch)
    return taps


def sds(pkg, sd):
    t32 = pkg.weights.to_torch(sd)
    return t32, {k: v.double() for k, v in t32.items()}


# --------------------------------------------------------------------------- decode
def split_heads(heads, arch, n: int):
    """the six head arrays [(n, cells, p * 6)] -> loc (n, P, 4), conf (n, P, 2) in prior order"""
    locs, confs = [], []
    for h, (src, c, m, _, _, ars, _) in zip(heads, arch.SOURCES):
        p = arch.priors_per_cell(ars)
        h = np.asarray(h).reshape(n, m * m, p * 6)
        locs.append(h[:, :, :p * 4].reshape(n, m * m * p, 4))
        confs.append(h[:, :, p * 4:].reshape(n, m * m * p, 2))
    return np.concatenate(locs, 1), np.concatenate(confs, 1)


def decode64(priors: np.ndarray, loc: np.ndarray, conf: np.ndarray, variances):
    """float64 CENTER_SIZE decode and two-way softmax of float32 inputs -> boxes (P, 4), prob (P,), box scale (P, 4)"""
    pr, l, c = priors.astype(np.float64), loc.astype(np.float64), conf.astype(np.float64)
    v = np.asarray(variances, F32).astype(np.float64)
    pw, ph = pr[:, 2] - pr[:, 0], pr[:, 3] - pr[:, 1]
    pcx, pcy = (pr[:, 0] + pr[:, 2]) * 0.5, (pr[:, 1] + pr[:, 3]) * 0.5
    cx, cy = v[0] * l[:, 0] * pw + pcx, v[1] * l[:, 1] * ph + pcy
    w, h = np.exp(v[2] * l[:, 2]) * pw, np.exp(v[3] * l[:, 3]) * ph
    boxes = np.stack([cx - w * 0.5, cy - h * 0.5, cx + w * 0.5, cy + h * 0.5], 1)
    ux, uy = np.abs(v[0] * l[:, 0] * pw) + np.abs(pcx) + 0.5 * w, np.abs(v[1] * l[:, 1] * ph) + np.abs(pcy) + 0.5 * h
    m = c.max(1, keepdims=True)
    e = np.exp(c - m)
    return boxes, e[:, 1] / e.sum(1), np.stack([ux, uy, ux, uy], 1)


def decode32(priors: np.ndarray, loc: np.ndarray, conf: np.ndarray, variances):
    """the yardstick: oracle.ssd_ref's float32 decode and softmax"""
    e = np.exp(conf - conf.max(1, keepdims=True))
    return ssd_ref.decode(priors, loc, variances), (e[:, 1] / e.sum(1)).astype(F32)


# --------------------------------------------------------------------------- DetectionOutput, restated independently
def detection_output_brute(boxes: np.ndarray, prob: np.ndarray, conf_thr, nms_thr, top_k, keep_top_k):
    """All-pairs restatement: stable order by (score desc, index asc), the top_k x top_k float32 overlap matrix with
    Caffe's rule (0 unless the intersection has positive width and height), then the greedy walk over the matrix."""
    boxes, prob = np.asarray(boxes, F32), np.asarray(prob, F32)
    valid = np.nonzero(prob > F32(conf_thr))[0]
    cand = valid[np.lexsort((valid, -prob[valid].astype(np.float64)))][:top_k]
    b = boxes[cand]
    n = len(cand)
    if n == 0:
        return []
    with np.errstate(invalid="ignore", divide="ignore"):
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        area = np.where((w < 0) | (h < 0), F32(0), w * h).astype(F32)
        ix = np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0])
        iy = np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1])
        inter = (ix * iy).astype(F32)
        iou = inter / ((area[:, None] + area[None, :]).astype(F32) - inter)
    over = np.where((ix > 0) & (iy > 0), iou.astype(np.float64), 0.0) > nms_thr
    alive = np.ones(n, bool)
    keep = []
    for i in range(n):
        if alive[i]:
            keep.append(i)
            alive[i + 1:] &= ~over[i, i + 1:]
    return [(float(prob[cand[i]]),) + tuple(float(v) for v in b[i]) for i in keep[:keep_top_k]]


def rows_array(rows, keep_top_k: int = 200) -> np.ndarray:
    out = np.zeros((keep_top_k, 5), F32)
    if len(rows):
        out[:len(rows)] = np.asarray(rows, F32)
    return out


# the kernel's two-level histogram, mirrored in float32 (csrc/ssd_kernels.hip nms_bin / nms_sub)
def nms_bin(p):
    return np.clip((np.asarray(p, F32) * F32(2048)).astype(np.int64), 0, 2047)


def nms_sub(p, b):
    return np.clip(((np.asarray(p, F32) * F32(2048) - np.asarray(b, F32)) * F32(2048)).astype(np.int64), 0, 2047)


# --------------------------------------------------------------------------- variant arch
def variant_arch(base, second_reader: bool):
    """A copy of `base` (ssd_arch) with a non-integer input transform (the non-EXACT conv1 kernels), an affine + ReLU
    after pool1, an add + ReLU in front of res2a and one around res2b; every source keeps its shape.  second_reader:
    "bn1" (affine) also reads conv1, so conv1 is materialised (ssd_conv1_mfma_kernel<false>) and pool1 / pool1b are
    separate 150 -> 75 max-pool launches; without it conv1 + pool1 is the fused ssd_conv1_pool_kernel<false>."""
    A = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    A.IN_SCALE = (0.9837, 1.0173, 0.9911)
    A.IN_SHIFT = (-103.37, -176.62, -122.81)
    head = [base.LAYERS[0], base.LAYERS[1]]                                       # conv1, pool1
    if second_reader:
        head += [("bn1", "affine", ("conv1", 32, True)), ("pool1b", "maxpool", ("bn1", 3, 2))]
    head += [("aff1", "affine", ("pool1", 32, True)),
             ("sum1", "add", ("aff1", "pool1b" if second_reader else "pool1", 32, True)),
             ("res2a", "conv", ("sum1", 32, 32, 3, 1, 1, 1, True, None)),
             ("res2b", "conv", ("res2a", 32, 32, 3, 1, 1, 1, True, "sum1")),
             ("sum2", "add", ("res2b", "aff1", 32, True)),
             ("res3p", "conv", ("sum2", 32, 128, 1, 2, 0, 1, False, None)),
             ("res3a", "conv", ("sum2", 32, 128, 3, 2, 1, 1, True, None))]
    assert [n for n, _, _ in base.LAYERS[2:6]] == ["res2a", "res2b", "res3p", "res3a"]
    A.LAYERS = head + list(base.LAYERS[6:])
    return A


def variant_state_dict(sd: Dict[str, np.ndarray], arch, seed: int = 5) -> Dict[str, np.ndarray]:
    """the seeded detector weights plus scale / shift of the variant's affine layers (both signs, so the ReLU cuts)"""
    rs = np.random.RandomState(seed)
    out = dict(sd)
    for name, kind, a in arch.LAYERS:
        if kind == "affine":
            out[name + ".scale"] = (rs.uniform(0.5, 1.5, a[1]) * rs.choice([-1.0, 1.0], a[1], p=[0.25, 0.75])).astype(F32)
            out[name + ".shift"] = (rs.randn(a[1]) * 0.3).astype(F32)
    return out


# --------------------------------------------------------------------------- injected heads
LN99 = float(np.log(99.0))                   # c0 - c1 at which the face probability is 0.01
HEAD_SEED = 15                               # picked: no probability of the case within 1e-6 of 0.01 but the planted pair's
# planted logit pairs (background, face) of image 0, at these priors (one per source map and a few more)
PLANTED = {
    "half": (17, (1.25, 1.25)),              # p = 0.5 exactly
    "sat_hi30": (5800, (-15.0, 15.0)), "sat_lo30": (7400, (15.0, -15.0)),
    "sat_hi100": (8300, (-50.0, 50.0)), "sat_lo100": (8650, (50.0, -50.0)),     # p = 1.0; exp underflows: p = 0
    "thr_above": (8720, (2.0 + LN99 - 2e-4, 2.0)), "thr_below": (8731, (2.0 + LN99 + 2e-4, 2.0)),   # p = 0.01 -+ 2e-6
}


def head_case(arch, n: int = 3, seed: int = HEAD_SEED):
    """n images of head tensors [(n, cells, p * 6)] x 6: loc in +-4, logits in +-6, every value of a call distinct
    (a stratified permutation: the k-th smallest value lies in the k-th of N equal slots of the range), so no wrong
    (image, source, cell, prior, component) index reads the right number; then the PLANTED logits into image 0."""
    rs = np.random.RandomState(seed)
    nl, nc = n * P * 4, n * P * 2
    loc = ((rs.permutation(nl) + rs.uniform(0.25, 0.75, nl)) / nl * 8.0 - 4.0).astype(F32).reshape(n, P, 4)
    conf = ((rs.permutation(nc) + rs.uniform(0.25, 0.75, nc)) / nc * 12.0 - 6.0).astype(F32).reshape(n, P, 2)
    for _, (i, c) in PLANTED.items():
        conf[0, i] = c
    heads, first = [], 0
    for src, c, m, _, _, ars, _ in arch.SOURCES:
        p = arch.priors_per_cell(ars)
        k = m * m * p
        h = np.concatenate([loc[:, first:first + k].reshape(n, m * m, p * 4), conf[:, first:first + k].reshape(n, m * m, p * 2)], 2)
        heads.append(np.ascontiguousarray(h))
        first += k
    return heads, loc, conf


def flat_heads(heads, images=None) -> np.ndarray:
    """the call's one array: source after source, each [img][cell][p * 6]; images: the subset to send"""
    return np.concatenate([(h if images is None else h[list(images)]).ravel() for h in heads])


# --------------------------------------------------------------------------- injected (boxes, prob)
THR32 = F32(0.01)
NMS32 = F32(0.45)


def _clusters(rs, k: int, n_clusters: int = 30):
    """k boxes around n_clusters centres: neighbours overlap above and below the threshold, so suppression chains occur"""
    cen = rs.uniform(0.15, 0.85, (n_clusters, 2))
    c = cen[rs.randint(0, n_clusters, k)] + rs.normal(0, 0.02, (k, 2))
    wh = rs.uniform(0.06, 0.14, (k, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)


def _distinct_scores(rs, k: int, lo: float = 0.02, hi: float = 0.995):
    """k distinct float32 scores in (lo, hi), in random order (stratified: spacing far above a float32 ulp)"""
    return (lo + (rs.permutation(k) + 0.5) / max(k, 1) * (hi - lo)).astype(F32)


def _grid(k: int, cols: int = 20, cell: float = 0.05, size: float = 0.04):
    """k pairwise disjoint boxes on a grid"""
    i = np.arange(k)
    x, y = (i % cols) * cell, (i // cols) * cell
    return np.stack([x, y, x + size, y + size], 1).astype(F32)


def _place(rs, boxes_k, prob_k, background=None):
    """k (box, score) entries at random prior indices of an otherwise invalid image (prob 0; boxes: clusters, so a read
    of a wrong index finds a plausible box)"""
    k = len(prob_k)
    boxes = _clusters(rs, P) if background is None else background
    prob = np.zeros(P, F32)
    idx = np.sort(rs.choice(P, k, replace=False)) if k < P else np.arange(P)
    order_ = rs.permutation(k)
    boxes[idx] = np.asarray(boxes_k, F32)[order_]
    prob[idx] = np.asarray(prob_k, F32)[order_]
    return boxes, prob


def _ranked(k: int, lo: float = 0.3, hi: float = 0.9):
    """k distinct descending scores: entry r has rank r"""
    return np.linspace(hi, lo, k).astype(F32)


def nms_cases() -> Dict[str, dict]:
    """name -> {"boxes" (P, 4), "prob" (P,), and the properties tests/test_ssd_stage_oracle.py verifies:
    "n_valid", optionally "count" (rows expected), "kept_before_cut", "why"}"""
    cases: Dict[str, dict] = {}

    def add(name, boxes, prob, **meta):
        cases[name] = dict(boxes=np.ascontiguousarray(boxes, F32), prob=np.ascontiguousarray(prob, F32), **meta)

    # n_valid on both sides of top_k = 400 (cut_bin == -1 up to 400: every valid key sorted) and of the sort widths 512 / 4096
    for k in (0, 1, 2, 399, 400, 401, 512, 513, 4096, 8732):
        rs = np.random.RandomState(100 + k % 97)
        b, p = _place(rs, _clusters(rs, k), _distinct_scores(rs, k))
        add(f"valid_{k}", b, p, n_valid=k, **({"count": k} if k < 2 else {}))
    # all scores equal: the cut selects everything (nsel = 8732, the 16384-wide sort); order = index order
    rs = np.random.RandomState(201)
    add("all_equal", _clusters(rs, P), np.full(P, 0.5, F32), n_valid=P)
    # 1000 equal scores straddling the 400th rank
    rs = np.random.RandomState(202)
    sc = np.concatenate([_distinct_scores(rs, 150, 0.6, 0.99), np.full(1000, 0.5, F32), _distinct_scores(rs, 500, 0.02, 0.45)])
    b, p = _place(rs, _clusters(rs, len(sc)), sc)
    add("ties_straddle", b, p, n_valid=1650, tie=(0.5, 150, 1000))
    # crowded cut bin: 3000 scores in bin 1536 = [0.75, 0.75 + 2^-11): 2000 in sub-bin 1000 (4 distinct floats: ties),
    # 150 in higher sub-bins, 850 in lower ones; 100 scores above the bin, 500 below: rank 400 lies in the crowded sub-bin
    rs = np.random.RandomState(203)
    bin0, sub0 = 1536, 1000
    crowded = (0.75 + sub0 * 2.0 ** -22 + rs.randint(0, 4, 2000) * 2.0 ** -24)
    hi_sub = 0.75 + (rs.choice(np.arange(sub0 + 1, 2048), 150, replace=False) + rs.randint(0, 4, 150) / 4.0) * 2.0 ** -22
    lo_sub = 0.75 + (rs.choice(np.arange(0, sub0), 850, replace=True) + rs.randint(0, 4, 850) / 4.0) * 2.0 ** -22
    sc = np.concatenate([_distinct_scores(rs, 100, 0.8, 0.99), crowded, hi_sub, lo_sub, _distinct_scores(rs, 500, 0.02, 0.7)])
    b, p = _place(rs, _clusters(rs, len(sc)), sc)
    add("crowded_bin", b, p, n_valid=3600, crowded=(bin0, sub0, 100, 150, 2000))
    # the confidence test is strict: 50 scores equal to the threshold (invalid), 50 one ulp above (valid), 20 others
    rs = np.random.RandomState(204)
    sc = np.concatenate([np.full(50, THR32), np.full(50, np.nextafter(THR32, F32(1))), _distinct_scores(rs, 20)])
    b, p = _place(rs, _grid(120), sc)
    add("conf_threshold", b, p, n_valid=70, count=70)
    # a score of exactly 1.0 (bin 2048 clamps to 2047), alone in a small set and among > 400 with ties at 1.0
    rs = np.random.RandomState(205)
    b, p = _place(rs, _clusters(rs, 10), np.concatenate([[1.0], _distinct_scores(rs, 9)]))
    add("one_small", b, p, n_valid=10)
    sc = np.concatenate([np.full(3, 1.0), 1.0 - rs.randint(1, 4000, 300) * 2.0 ** -24, _distinct_scores(rs, 300)])
    b, p = _place(rs, _clusters(rs, len(sc)), sc)
    add("one_large", b, p, n_valid=603)
    # 400 pairwise disjoint boxes: all survive, the cut to keep_top_k = 200 is taken
    rs = np.random.RandomState(206)
    b, p = _place(rs, _grid(400), _distinct_scores(rs, 400))
    add("disjoint_400", b, p, n_valid=400, count=200, kept_before_cut=400)
    # 250 disjoint boxes + 150 duplicates of them: 250 kept, cut to 200
    g = _grid(250)
    b, p = _place(rs, np.concatenate([g, g[rs.choice(250, 150, replace=False)]]), _distinct_scores(rs, 400))
    add("disjoint_250_dup_150", b, p, n_valid=400, count=200, kept_before_cut=250)
    # word boundaries of the 64-candidate overlap words.  Literal form: 400 disjoint boxes by rank, the suppressor (rank s)
    # copied to the victim ranks - nothing else overlaps; 393 kept, cut to 200 (the later ranks are not in the rows).
    # Visible form: every rank that is neither suppressor, victim nor "lone" is a copy of the filler (its first copy keeps,
    # and suppresses its copies in all seven words), so few rows are kept and every victim and lone rank shows.
    victims = (63, 64, 127, 128, 383, 384, 399)
    lone = (62, 65, 126, 129, 255, 256, 382, 385, 398)
    for s in (0, 63, 64):
        rs = np.random.RandomState(210 + s)
        v = [r for r in victims if r > s]
        g = _grid(400)
        for r in v:
            g[r] = g[s]
        b, p = _place(rs, g, _ranked(400))
        add(f"words_literal_{s}", b, p, n_valid=400, count=200, kept_before_cut=400 - len(v))
        g = _grid(400)
        f = 1 if s == 0 else 0                                                      # the filler's first rank
        for r in range(400):
            if r in v:
                g[r] = g[s]
            elif r != s and r not in lone:
                g[r] = g[f]
        b, p = _place(rs, g, _ranked(400))
        add(f"words_visible_{s}", b, p, n_valid=400, count=2 + len(lone), kept_ranks=sorted({s, f} | set(lone)))
    # chains: A > B > C in score, IoU(A,B) = IoU(B,C) = 0.7 / 1.3 > thr, IoU(A,C) = 0.4 / 1.6 < thr: C is kept (B, removed,
    # removes nothing).  90 triples at random ranks (every word) + 130 copies of one filler box: 181 kept
    rs = np.random.RandomState(220)
    g = _grid(91)
    tb, ts = [], []
    for t in range(90):
        x1, y1, x2, y2 = g[t]
        w = F32(0.02)
        s3 = np.sort(rs.uniform(0.05, 0.95, 3))[::-1]
        for j in range(3):
            tb.append((x1 + F32(0.3 * j) * w, y1, x1 + F32(0.3 * j) * w + w, y2))
            ts.append(s3[j])
    tb += [tuple(g[90])] * 130
    ts += list(rs.uniform(0.05, 0.95, 130))
    ts = (np.asarray(ts) + np.arange(400) * 1e-6).astype(F32)                      # distinct
    b, p = _place(rs, np.asarray(tb, F32), ts)
    add("chains", b, p, n_valid=400, count=181)
    # 200 isolated pairs whose IoU is within a few float32 ulps of the threshold on both sides (and exactly (float)0.45):
    # columns at x = i 2^-8 of 20 different widths w in [2^-10, 2^-9) (so the quotient's operands differ from pair to pair),
    # the tall box [0, 0.5], the short one [0, t / 2]: IoU = t up to the rounding of area_a + area_b.  160 pairs
    # t = (float)0.45 + k ulp, k = -3 .. 4 (inside the 1e-5 band of jaccard_above, where inter * rcp(union) and
    # inter / union can fall on different sides), 40 pairs outside the band
    rs = np.random.RandomState(230)
    ulp = float(np.spacing(NMS32))
    ts_ = [float(NMS32) + (i % 8 - 3) * ulp for i in range(160)] + [float(NMS32) + sgn * d for sgn in (-1, 1) for d in np.geomspace(2e-5, 1e-2, 20)]
    pb, ps = [], []
    for i, t in enumerate(ts_):
        x, w = i * 2.0 ** -8, (2 ** 14 + rs.randint(0, 2 ** 14)) * 2.0 ** -24         # x + w is exact in float32
        pb += [(x, 0.0, x + w, 0.5), (x, 0.0, x + w, float(F32(F32(t) * F32(0.5))))]
        ps += [0.9 - i * 1e-3, 0.45 - i * 1e-3]
    b, p = _place(rs, np.asarray(pb, F32), np.asarray(ps, F32))
    add("near_threshold", b, p, n_valid=400, pairs=len(ts_))
    # zero-area boxes: identical vertical segments, identical points, segments touching end to end, segments inside and on
    # the edge of ordinary boxes: overlap 0 (Caffe), so every one survives.  Non-finite boxes are out of scope.
    rs = np.random.RandomState(240)
    zb = [(0.1, 0.1, 0.1, 0.3)] * 10 + [(0.5, 0.5, 0.5, 0.5)] * 10 + [(0.2 + 0.05 * j, 0.7, 0.25 + 0.05 * j, 0.7) for j in range(10)]
    zb += [(0.05, 0.05, 0.35, 0.35), (0.1, 0.1, 0.4, 0.3), (0.45, 0.45, 0.55, 0.55), (0.6, 0.1, 0.8, 0.3), (0.8, 0.1, 0.8, 0.3)]
    b, p = _place(rs, np.asarray(zb, F32), _distinct_scores(rs, len(zb)))
    add("zero_area", b, p, n_valid=len(zb), zero_area=31)
    return cases


BATCH3 = ("valid_8732", "valid_0", "crowded_bin")          # one call of three images: a 0-valid image between two full ones

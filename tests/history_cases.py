"""The table behind tests/test_call_history_gpu.py: does any device path's output depend on what the handle did before?

A CASE is one public call of `_lib.Handle`, or a short fixed sequence that belongs together, with everything the call
returns or lets a test read.  A HISTORY is a sequence of public calls on the same handle that ends just before the
case.  The reference is the same case on a handle made for it with nothing run before; the comparison (`compare`) is
bit for bit, on every element, with no tolerance.

Every case is a function `run(h, dirty)`: it calls `dirty()` - the history - immediately in front of EVERY call whose
output it records (as the MTCNN stale-scratch test does), so that no output is taken from a forward whose workspaces
the case's own earlier calls have already put right.  On the fresh handle `dirty` does nothing.  A case that is one
sequence (a trainer session, a stream's frames) calls it in front of the sequence, or of each of its parts.  Every array
a `large` or `grow` history hands over differs from every case input in every element position the two share
(`unlike`, `history_inputs`; test_history_cases.py walks every history of every family).

Histories, per family (`HISTORIES`):
  repeat     the case itself, once: run-to-run non-determinism shows here and not as history dependence
  large      the family's largest shapes with other content (other seed, scale and offset) at the handle's full
             max_batch, in configurations that materialise every workspace; the classifier: fuse_expand = fuse_stem =
             fuse_late = 0 and the case's own configuration, in fp32 storage, then both again in bf16 storage - the
             front halves of the activation buffers then hold bf16 leftovers, the back halves fp32 ones
  grow       a small call, then a larger one that makes ensure() re-allocate, then the case
  nonfinite  as large, with NaN and +-Inf wherever the API takes floats from the caller; families that take 8-bit
             input only have no such history (their `large` holds all-255 and checkerboard frames instead)
  cross      one call of every other family on the handle, at its largest shape

Persistent state is outside the property and each case resets it through the public API: forensic stream state (a stream
id the history used and then released), the trainer's step counter and dropout seed (begin again, same seed), TTA
arming, options (every case sets its own), counters.  No history commits weights and none calls warmup().

This module imports without a GPU; tests/test_history_cases.py checks the table, the inputs and the comparison there.
"""
from __future__ import annotations

import dataclasses
import functools
import io
import struct
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

import b0_layer_oracle as B
import rtdfd_amd
from rtdfd_amd import _lib as L

MAX_BATCH = 16
HISTORY_NAMES = ("repeat", "large", "grow", "nonfinite", "cross")


# ------------------------------------------------------------------------------------------------ the comparison
@dataclasses.dataclass(frozen=True)
class Diff:
    name: str          # the first output that differs, in the order the case produced them
    count: int         # how many of its elements differ (-1: the shapes, types or lengths themselves differ)
    first: tuple       # index of the first differing element
    detail: str

    def __str__(self):
        return f"{self.name}: {self.count} elements differ, first at {self.first} ({self.detail})"


def _leaves(prefix: str, v, out: List[Tuple[str, object]]):
    if isinstance(v, dict):
        for k in v:                                     # insertion order = the order the case produced them
            _leaves(f"{prefix}.{k}" if prefix else str(k), v[k], out)
    elif isinstance(v, (list, tuple)):
        out.append((prefix + ".len", len(v)))
        for i, e in enumerate(v):
            _leaves(f"{prefix}[{i}]", e, out)
    else:
        out.append((prefix, v))


def bits(a: np.ndarray) -> np.ndarray:
    """an array as the unsigned integers of its bytes: float32 -> uint32, bf16 / float16 -> uint16, float64 -> uint64,
    complex64 -> (.., 2) uint32; integer and bool arrays as they are"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(np.float32 if a.dtype == np.complex64 else np.float64).reshape(a.shape + (2,))
    if a.dtype.kind == "f":
        return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    if a.dtype.kind == "V":
        return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return a


def _nan_count(a) -> int:
    a = np.asarray(a)
    return int(np.isnan(a).sum()) if a.dtype.kind in "fc" else 0


def _leaf_diff(name: str, r, g) -> Optional[Diff]:
    if isinstance(r, np.ndarray) or isinstance(g, np.ndarray):
        if not (isinstance(r, np.ndarray) and isinstance(g, np.ndarray)) or r.dtype != g.dtype or r.shape != g.shape:
            return Diff(name, -1, (), f"fresh {getattr(r, 'dtype', type(r))} {getattr(r, 'shape', '')}, "
                                      f"after the history {getattr(g, 'dtype', type(g))} {getattr(g, 'shape', '')}")
        rb, gb = bits(r), bits(g)
        ne = rb != gb
        if ne.any():
            at = tuple(int(i) for i in np.argwhere(ne)[0])
            extra = _nan_count(g) - _nan_count(r)
            return Diff(name, int(ne.sum()), at, f"fresh {rb[at]:#x}, after the history {gb[at]:#x}"
                        + (f"; {extra} more NaN than the fresh handle" if extra > 0 else ""))
        return None
    if isinstance(r, float) or isinstance(g, float):
        if not (isinstance(r, float) and isinstance(g, float)) or struct.pack("<d", r) != struct.pack("<d", g):
            return Diff(name, 1, (), f"fresh {r!r}, after the history {g!r}")
        return None
    if type(r) is not type(g) or r != g:
        if isinstance(r, (bytes, bytearray)) and isinstance(g, (bytes, bytearray)):
            n = min(len(r), len(g))
            ne = np.frombuffer(r[:n], np.uint8) != np.frombuffer(g[:n], np.uint8)
            first = int(np.argmax(ne)) if ne.any() else n
            return Diff(name, int(ne.sum()) + abs(len(r) - len(g)), (first,), f"{len(r)} bytes fresh, {len(g)} after the history")
        return Diff(name, 1 if not name.endswith(".len") else -1, (), f"fresh {r!r}, after the history {g!r}")
    return None


def compare(ref, got) -> List[Diff]:
    """every difference between two results of one case, in output order; [] = bit for bit equal.  Floats are compared as
    their bit patterns (a NaN against a number, or against a NaN of other bits, differs), byte strings as bytes, rows,
    counts and lengths exactly; an output only one side has is a difference."""
    a, b = [], []
    _leaves("", ref, a)
    _leaves("", got, b)
    db = dict(b)
    out = []
    for name, r in a:
        if name not in db:
            out.append(Diff(name, -1, (), "missing after the history"))
            continue
        d = _leaf_diff(name, r, db[name])
        if d is not None:
            out.append(d)
    da = dict(a)
    out += [Diff(name, -1, (), "only after the history") for name, _ in b if name not in da]
    return out


def report(diffs: List[Diff]) -> str:
    if not diffs:
        return "bit for bit equal"
    return f"{len(diffs)} outputs differ; first: {diffs[0]}" + "".join(f"\n  then {d}" for d in diffs[1:6])


# ------------------------------------------------------------------------------------------------ cases and blobs
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str
    run: Callable                  # run(h, dirty) -> {output name: array / bytes / number / list}
    reaches: Tuple[str, ...]       # the exports of _lib.SIGNATURES this case calls
    histories: Tuple[str, ...] = HISTORY_NAMES
    blob: str = "full"
    arg: object = None             # what the family's histories need to know of the case (the classifier: its options)
    thinnable: bool = False        # run(h, dirty, thin=True) records every fourth tap only (used under "cross")


def _noop():
    pass


_BLOBS: Dict[str, bytes] = {}


def blob(kind: str = "full") -> bytes:
    """"full": the stress classifier weights (saturated gates, zero gammas, a four-decade BN variance), the seeded SSD
    detector, the dense seeded MTCNN cascade and the toy Haar cascade in one blob; "ssd_variant0/1": the classifier and
    ssd_stage_oracle's variant detector architectures"""
    if kind not in _BLOBS:
        W = rtdfd_amd.weights
        if kind == "full":
            import haar_cases

            _BLOBS[kind] = W.pack_all(B.stress_state_dict(0), W.seeded_ssd_state_dict(0), W.seeded_mtcnn_state_dict(0),
                                      haar=haar_cases.toy())
        elif kind.startswith("ssd_variant"):
            import ssd_stage_oracle as S
            from rtdfd_amd import ssd_arch

            arch = S.variant_arch(ssd_arch, bool(int(kind[-1])))
            sd = S.variant_state_dict(W.seeded_ssd_state_dict(0), arch)
            _BLOBS[kind] = W.pack_all(W.seeded_state_dict(0), sd, ssd_arch=arch)
        else:
            raise KeyError(kind)
    return _BLOBS[kind]


def new_handle(kind: str = "full"):
    return L.Handle(blob(kind), device=0, max_batch=MAX_BATCH)


# ------------------------------------------------------------------------------------------------ inputs, fixed seeds
def nonfinite_like(a: np.ndarray) -> np.ndarray:
    """float32 array of a's shape with NaN, +Inf and -Inf in turn: no finite element"""
    v = np.array([np.nan, np.inf, -np.inf], np.float32)
    return v[np.arange(a.size) % 3].reshape(a.shape)


@functools.lru_cache(maxsize=None)
def case_crops(n: int) -> np.ndarray:
    return B.random_crops(n)                            # seed 42


@functools.lru_cache(maxsize=None)
def history_crops(nonfinite: bool = False, n: int = MAX_BATCH) -> np.ndarray:
    x = B.random_crops(n, seed=7) * np.float32(1.7) + np.float32(0.4)
    return nonfinite_like(x) if nonfinite else x


@functools.lru_cache(maxsize=None)
def noise_frame(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def white_frame(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


@functools.lru_cache(maxsize=None)
def checker_frame(h: int, w: int) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def shared(hist: np.ndarray, case: np.ndarray):
    """the element positions two inputs share: both cut to their common leading corner (a gray case image against a
    colour history frame: against each channel)"""
    if case.ndim == hist.ndim - 1:
        case = case[..., None]
    assert case.ndim == hist.ndim, (case.shape, hist.shape)
    gray = case.shape[-1] == 1 and hist.shape[-1] != 1
    cut = tuple(slice(0, min(a, b)) for a, b in zip(hist.shape[:-1], case.shape[:-1]))
    cut += (slice(None),) if gray else (slice(0, min(hist.shape[-1], case.shape[-1])),)
    return hist[cut], np.broadcast_to(case[cut[:-1]], hist[cut].shape) if gray else case[cut]


def unlike(hist: np.ndarray, *cases: np.ndarray) -> np.ndarray:
    """`hist` (uint8) with every element that equals the element of a case input at the same position moved on by one:
    two noise frames agree in one position of 256 otherwise"""
    hist = hist.copy()
    for _ in range(8):
        again = False
        for c in cases:
            hv, cv = shared(hist, c)
            eq = hv == cv
            if eq.any():
                hv[eq] += np.uint8(1)                   # (hv is a view of hist; uint8 wraps)
                again = True
        if not again:
            return hist
    raise AssertionError("unlike: did not settle")


# ------------------------------------------------------------------------------------------------ the classifier
CLS_RESET = dict(B.DEFAULT.options(), fuse_late_skip=-1, fuse_k5=1, fuse_k5_min=0, fuse_proj0=1)     # the handle's defaults
CLS_UNFUSED = dict(CLS_RESET, fuse_expand=0, fuse_stem=0, fuse_late=0)
THIN_TAPS = ("b0.dw", "b1.dw", "b6.dw", "b8.gate", "b11.dw", "b15.out")
CLS_N = (1, 3, 5)


def _set(h, options):
    for k, v in options.items():
        h.set_option(k, v)


def _per_image_taps():
    """the taps of the per-image kernels forced on at small batch: every expand of blocks 1-15 runs inside a depthwise
    launch there (block 11 too, which has no form in the 4-image late launch), so no b{i}.exp is materialised"""
    return tuple(t for t in B.Config("late_all", fuse_late_skip=0).taps() if not t.endswith(".exp"))


def classifier_configs():
    """(name, options, taps at n = 3): b0_layer_oracle's nine configurations, and the per-image kernels forced on at
    small batch ("fuse_k5_min" = 1) with "fuse_late_skip" unset and 0, "fuse_proj0" on and off"""
    out = [(c.name, dict(CLS_RESET, **c.options()), tuple(c.taps())) for c in B.FP32_CONFIGS + B.BF16_CONFIGS]
    for skip in (-1, 0):
        for proj0 in (1, 0):
            out.append((f"per_image_skip{skip}_proj0{proj0}",
                        dict(CLS_RESET, fuse_k5=1, fuse_k5_min=1, fuse_late_skip=skip, fuse_proj0=proj0), _per_image_taps()))
    return out


def classifier_large(h, options, nonfinite=False):
    """16 crops of other content through the unfused plan and the case's own, fp32 storage and then bf16 storage, and
    through Grad-CAM (whose buffers ensure() sizes by the batch)"""
    x = history_crops(nonfinite)
    for bf in (0, 1):
        for opt in (CLS_UNFUSED, options):
            _set(h, dict(opt, bf16_activations=bf))
            h.classify(x)
        h.gradcam(x, overlay=True, raw=True)
    _set(h, CLS_RESET)


def classifier_grow(h, options):
    _set(h, options)
    for n in (1, MAX_BATCH):
        x = history_crops(n=n)
        h.classify(x)
        h.extract_trunk(x, block=14)
        h.gradcam(x, overlay=True, raw=True)
    _set(h, CLS_RESET)


def classifier_case(cfg_name: str, options: dict, taps: Tuple[str, ...], n: int) -> Case:
    names = taps if n == 3 else THIN_TAPS
    absent = tuple(f"b{i}.exp" for i in range(1, 16) if f"b{i}.exp" not in taps)

    def run(h, dirty=_noop, thin=False):
        x = case_crops(n)
        xd = h.alloc(x.nbytes).upload(x)
        out = {}

        def call(fn):
            dirty()
            _set(h, options)
            return fn()

        try:
            for t in (names[::4] if thin else names):
                out[t] = call(lambda: h.tap(xd.ptr, n, t, B.tap_size(t, n)).copy())
            out["feat"] = call(lambda: h.extract_features(x))
            out["logits"] = call(lambda: h.classify(x))
            out["trunk14"] = call(lambda: h.extract_trunk(x, block=14))
            out["trunk15"] = call(lambda: h.extract_trunk(x, block=15))
            lg, heat = call(lambda: h.gradcam(x))
            out["gradcam.logits"], out["gradcam.heat"] = lg, heat
            for t in (absent if n == 3 and not thin else ()):        # the plan is the one the configuration names: these expands ran fused
                try:
                    call(lambda: h.tap(xd.ptr, n, t, B.tap_size(t, n)))
                    out["refused." + t] = 0
                except L.DfdError as e:
                    out["refused." + t] = e.code
            if n == 3:                                  # the device-pointer entries: the same launches, no host copies
                od = h.alloc(n * 4 + n * 224 * 224 * 4)

                def device_entries():
                    h.classify_device(xd.ptr, n, od.ptr)
                    h.sync()
                    a = od.download((n,))
                    h.gradcam_device(xd.ptr, n, od.ptr, None, od.ptr + n * 4, None)
                    h.sync()
                    return a, od.download((n + n * 224 * 224,))
                out["device.logits"], out["device.gradcam"] = call(device_entries)
                od.free()
        finally:
            _set(h, CLS_RESET)
            xd.free()
        return out

    return Case(f"classifier-{cfg_name}-n{n}", "classifier", run,
                ("dfd_b0_tap", "dfd_extract_features", "dfd_classify_nchw", "dfd_extract_trunk", "dfd_extract_trunk_at",
                 "dfd_gradcam_nchw", "dfd_classify_nchw_device", "dfd_gradcam_nchw_device"), arg=options, thinnable=n == 3)


def logit_check(out: dict) -> dict:
    """the fresh handle's logits against float64 at the suite's bar for that tap (b0_layer_oracle.check of "logit" from
    the handle's own "feat": the max bar per batch; "sq" feeds the rms bar pooled over a configuration's batches)"""
    import torch

    sd = B.stress_state_dict(0)
    taps = {"feat": torch.from_numpy(np.array(out["feat"])).double(), "logit": torch.from_numpy(np.array(out["logits"])).double()}
    return B.check(B.DEFAULT, "logit", lambda k: taps[k], lambda k: taps[k].float(), B.to_torch(sd), B.to_torch(sd, torch.float32), None)


@functools.lru_cache(maxsize=None)
def _stress_torch():
    import torch

    sd = B.stress_state_dict(0)
    return sd, B.to_torch(sd), B.to_torch(sd, torch.float32)


def layer_checks(cfg: "B.Config", out: dict, n: int = 3) -> dict:
    """every tap of a fresh n = 3 result against its float64 layer reference at the bars of test_b0_layers_gpu.py (teacher
    forcing from the result's own taps) -> {tap: b0_layer_oracle.check result}: the whole chain from the crops to the logit"""
    import torch

    sd, sd64, sd32 = _stress_torch()
    ksd = B.kernel_state_dict(sd, cfg) if cfg.bf16 else None
    cache = {"x": torch.from_numpy(case_crops(n)).double()}

    def get64(name):
        if name not in cache:
            cache[name] = B.from_tap(np.array(out[name]).reshape(-1), name, n)
        return cache[name]

    return {name: B.check(cfg, name, get64, lambda k: get64(k).float(), sd64, sd32, ksd) for name in cfg.taps()}


# the form whose bits a per-image configuration must reproduce (b0_plan.hip: "neither the option nor the batch size changes a result")
PER_IMAGE_FORM = {"per_image_skip-1_proj01": "default", "per_image_skip-1_proj00": "default",
                  "per_image_skip0_proj01": "late_all", "per_image_skip0_proj00": "late_all"}


def classifier_cases() -> List[Case]:
    return [classifier_case(name, opt, taps, n) for name, opt, taps in classifier_configs() for n in CLS_N]


# ------------------------------------------------------------------------------------------------ the split GEMM, direct
@functools.lru_cache(maxsize=None)
def gemm_picks():
    """one ragged shape per kernel family from gemm_oracle.CASES (the tile each call took is part of its result)"""
    import gemm_oracle as G

    def first(group, pred):
        return next(c for c in G.CASES if c.group == group and c.family == "random" and pred(c))

    return [first("pointwise", lambda c: c.M == 127 and c.N % 4 != 0),                  # pw6 / pw7, N % 4 != 0
            first("pointwise", lambda c: c.M == 129 and c.N % 4 == 0 and c.K >= 72),
            first("pw8", lambda c: c.M == 33 and not c.bf16 and not c.gated),
            first("pw8", lambda c: c.gated and c.HW == 80 and not c.bf16),
            first("pw8", lambda c: c.bf16 and c.gated),
            first("pw9", lambda c: c.M == 127),
            first("gated", lambda c: c.HW == 49 and c.M == 3 * 49 - 5),
            first("conv", lambda c: c.conv[4] == 3 and c.conv[7] == 2),
            first("bf16", lambda c: not c.gated and c.M > 1),
            first("bf16", lambda c: c.gated)]


@functools.lru_cache(maxsize=None)
def gemm_history_shapes():
    """the largest M (8200), K (264) and N (672) of gemm_oracle's list, every operand kind, fp32 and bf16, and a convolution"""
    import gemm_oracle as G

    return [G.Case("pointwise", 8200, 264, 196, act="swish", res="after"),
            G.Case("pw9", 8200, 112, 672, act="swish"),
            G.Case("pw8", 8200, 256, 48, 82, res="after", gated=True),
            G.Case("bf16", 8200, 264, 196, 82, act="relu", res="first", gated=True, bf16=True),
            G.conv_case(16, 9, 6, 64, 3, 1, 1, 1, 64, "prelu", "after")]


@functools.lru_cache(maxsize=None)
def gemm_inputs(case, history=False, nonfinite=False):
    import gemm_oracle as G

    inp = G.make_inputs(case)
    if history:
        inp["x"] = inp["x"] * np.float32(-1.5) + np.float32(0.25)
        if case.bf16:
            inp["x"] = G._bf16_round(inp["x"])
        # bf16 values are few: where one meets a case operand's value at the same position it is doubled (exact)
        for _ in range(4):
            for pick in gemm_picks():
                pin = G.make_inputs(pick)
                for k in ("x", "gate", "res"):
                    if inp[k] is not None and pin[k] is not None and inp[k].ndim == pin[k].ndim:
                        hv, cv = shared(inp[k], pin[k])
                        hv[hv == cv] *= np.float32(2.0)
    if nonfinite:
        for k in ("x", "gate", "res"):
            if inp[k] is not None:
                inp[k] = nonfinite_like(inp[k])
    return inp


def gemm_call(h, case, inp):
    import gemm_oracle as G

    x = inp["x"] if not case.bf16 else G.to_bits(inp["x"])
    res = inp["res"] if inp["res"] is None or not case.bf16 else G.to_bits(inp["res"])
    return h.gemm_tap(x, inp["w"], inp["bias"], act=case.act, gate=inp["gate"], res=res, res_first=case.res == "first", hw=case.HW,
                      bf16=case.bf16, planes=case.planes, conv=case.conv_dict() if case.conv is not None else None)


def gemm_large(h, nonfinite=False):
    h.set_option("gemm_tile", -1)
    for c in gemm_history_shapes():
        gemm_call(h, c, gemm_inputs(c, True, nonfinite))


def gemm_grow(h):
    import gemm_oracle as G

    for m in (17, 8200):
        c = G.Case("pointwise", m, 264, 196, act="swish", res="after")
        gemm_call(h, c, gemm_inputs(c, True))


def _gemm_run(h, dirty=_noop):
    out = {}
    for c in gemm_picks():
        dirty()
        h.set_option("gemm_tile", -1)
        r = gemm_call(h, c, gemm_inputs(c))
        out[c.name] = {k: (np.asarray(r[k]) if k == "tile" else r[k]) for k in ("rc", "launches", "tile", "before", "y", "after")}
    return out


# ------------------------------------------------------------------------------------------------ Grad-CAM, launch by launch
@functools.lru_cache(maxsize=None)
def gradcam_inputs(n: int, seed: int, nonfinite=False):
    rs = np.random.RandomState(seed)
    z = (rs.randn(n, 49, 1280) * 2.0).astype(np.float32)
    fc1 = np.maximum(rs.randn(n, 512), 0).astype(np.float32)
    fc2 = np.maximum(rs.randn(n, 256), 0).astype(np.float32)
    if seed != 70:                                  # the histories: no zero where the case's ReLU outputs have theirs
        fc1, fc2 = fc1 + np.float32(0.5), fc2 + np.float32(0.5)
    if nonfinite:
        z, fc1, fc2 = nonfinite_like(z), nonfinite_like(fc1), nonfinite_like(fc2)
    return z, fc1, fc2


def gradcam_large(h, nonfinite=False):
    z, fc1, fc2 = gradcam_inputs(MAX_BATCH, 71, nonfinite)
    x = history_crops(nonfinite)
    h.gradcam_tap(x=x, z=z, fc1=fc1, fc2=fc2, overlay=True)
    h.gradcam_tap(x=x, overlay=True)


def gradcam_grow(h):
    for n in (1, MAX_BATCH):
        z, fc1, fc2 = gradcam_inputs(n, 72)
        h.gradcam_tap(x=history_crops(n=n), z=z, fc1=fc1, fc2=fc2, overlay=True)


def _gradcam_run(h, dirty=_noop):
    import gemm_oracle as G

    z, fc1, fc2 = gradcam_inputs(3, 70)
    x = case_crops(3)
    out = {}
    dirty()
    out["z_fp32"] = h.gradcam_tap(x=x, z=z.copy(), fc1=fc1.copy(), fc2=fc2.copy(), overlay=True)      # (the result holds its inputs)
    dirty()
    out["z_bf16"] = h.gradcam_tap(x=x, z=G.to_bits(G._bf16_round(z)), fc1=fc1.copy(), fc2=fc2.copy(), overlay=True)
    dirty()
    out["x"] = h.gradcam_tap(x=x, overlay=True)
    return out


# ------------------------------------------------------------------------------------------------ the 8-bit face path
FACE_FRAME = (100, 100, 11)
FACE_BOXES = [(10, 10, 1, 1), (40, 30, 8, 8), (60, 70, 40, 30)]                 # 1 x 1, 8 x 8, one touching the border
FACE_HISTORY_FRAME = (1080, 1920, 12)


@functools.lru_cache(maxsize=None)
def face_history_boxes(n: int = MAX_BATCH):
    return [(40 + 90 * i, 20 + 37 * i, 300 + 10 * i, 460 - 7 * i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def tta_draw_list(rows: int, copies: int):
    return [(i % 2, 0.8 + 0.1 * (i % 5), -10.0 + 5.0 * (i % 5)) for i in range(rows * copies)]


@functools.lru_cache(maxsize=None)
def face_history_frame():
    return unlike(noise_frame(*FACE_HISTORY_FRAME), noise_frame(*FACE_FRAME))


def face_large(h):
    h.set_option("mtcnn", 0)
    boxes = face_history_boxes()
    for frame in (face_history_frame(), white_frame(1080, 1920), checker_frame(1080, 1920)):
        h.preprocess_crops(frame, boxes, True)
        h.classify_crops(frame, boxes, True)
        h.classify_crops_tta(frame, boxes[:4], 3, tta_draw_list(4, 3), True)
        h.gradcam_crops(frame, boxes, True, overlay=True, raw=True)
        h.tta_augment(np.ascontiguousarray(frame[:480, :640]), True, 1.2, 9.0)
        h.preprocess_face_quality(np.ascontiguousarray(frame[:480, :640]))
        h.resize_bgr(frame, 300, 300)
    h.set_option("mtcnn", 1)


def face_grow(h):
    h.set_option("mtcnn", 0)
    frame = face_history_frame()
    for n in (1, MAX_BATCH):
        h.classify_crops(frame, face_history_boxes(n), True)
        h.gradcam_crops(frame, face_history_boxes(n), True, overlay=True)
    h.set_option("mtcnn", 1)


def _face_run(h, dirty=_noop):
    frame = noise_frame(*FACE_FRAME)
    out = {}

    def call(fn):
        dirty()
        h.set_option("mtcnn", 0)                  # the crops go to the classifier as they are (no cascade in front)
        try:
            return fn()
        finally:
            h.set_option("mtcnn", 1)

    out["preprocess_clahe"] = call(lambda: h.preprocess_crops(frame, FACE_BOXES, True))
    out["preprocess_plain"] = call(lambda: h.preprocess_crops(frame, FACE_BOXES, False))
    out["classify_crops"] = call(lambda: h.classify_crops(frame, FACE_BOXES, True))
    out["classify_crops_tta"] = call(lambda: h.classify_crops_tta(frame, FACE_BOXES, 3, tta_draw_list(3, 3), True))
    out["tta_augment_crops"] = call(lambda: h.tta_augment_crops(frame, FACE_BOXES, 3, tta_draw_list(3, 3)))
    for name, (x, y, w, hh) in zip(("1x1", "8x8", "border"), FACE_BOXES):
        face = np.ascontiguousarray(frame[y:y + hh, x:x + w])
        out["tta_augment_" + name] = call(lambda: h.tta_augment(face, True, 1.1, 7.0))
    out["face_quality"] = call(lambda: h.preprocess_face_quality(np.ascontiguousarray(frame[70:100, 60:100])))
    out["resize_bgr"] = call(lambda: h.resize_bgr(frame, 37, 53))
    out["gradcam_crops"] = call(lambda: h.gradcam_crops(frame, FACE_BOXES, True, overlay=True, raw=True))
    return out


# ------------------------------------------------------------------------------------------------ the SSD detector
SSD_THRESHOLDS = (0.5, 0.05)


@functools.lru_cache(maxsize=None)
def ssd_case_frame():
    import frames

    return frames.noisy_image((240, 320), 9)


@functools.lru_cache(maxsize=None)
def ssd_history_frames():
    import frames

    return [unlike(frames.face_frame(1280, 720, 3), ssd_case_frame()), white_frame(720, 1280), checker_frame(720, 1280)]


def ssd_tap_names(arch):
    import ssd_stage_oracle as S

    shp = S.shapes(arch)
    return [(n, shp[n][0] * shp[n][1] ** 2) for n in S.order(arch)] + [("prob", S.P), ("boxes", S.P * 4), ("rows", 200 * 5)]


def ssd_large(h):
    for f in ssd_history_frames():
        h.detect_faces(f, 0.01, with_conf=True)


@functools.lru_cache(maxsize=None)
def ssd_grow_frames():
    return [unlike(noise_frame(48, 64, 13), ssd_case_frame()), ssd_history_frames()[0]]


def ssd_grow(h):
    for f in ssd_grow_frames():
        h.detect_faces(f, 0.5)


def _ssd_run_for(arch_of):
    def run(h, dirty=_noop):
        frame = ssd_case_frame()
        out = {}
        for thr in SSD_THRESHOLDS:
            dirty()
            boxes, conf = h.detect_faces(frame, thr, with_conf=True)
            out[f"detect_{thr}"] = {"boxes": boxes, "conf": conf}
        for name, size in ssd_tap_names(arch_of()):
            dirty()
            out[name] = h.ssd_tap(frame, name, size).copy()
        return out
    return run


def _default_arch():
    from rtdfd_amd import ssd_arch

    return ssd_arch


def _variant_arch(k):
    import ssd_stage_oracle as S

    return lambda: S.variant_arch(_default_arch(), bool(k))


@functools.lru_cache(maxsize=None)
def ssd_one_prior():
    """(boxes (1, P, 4), prob (1, P)): one prior above the confidence threshold"""
    import ssd_stage_oracle as S

    rs = np.random.RandomState(21)
    lo = rs.uniform(0.0, 0.6, (1, S.P, 2))
    boxes = np.concatenate([lo, lo + rs.uniform(0.05, 0.4, (1, S.P, 2))], 2).astype(np.float32)
    prob = np.zeros((1, S.P), np.float32)
    prob[0, 4321] = 0.875
    return boxes, prob


@functools.lru_cache(maxsize=None)
def ssd_many_priors(nonfinite=False):
    """the flat head tensors of three images (ssd_stage_oracle.head_case): several thousand valid priors each"""
    import ssd_stage_oracle as S

    heads = S.flat_heads(S.head_case(_default_arch(), 3)[0])
    return nonfinite_like(heads) if nonfinite else heads


@functools.lru_cache(maxsize=None)
def ssd_case_heads():
    """one image of head tensors: image 1 of a two-image draw (image 0 carries head_case's planted logits, as the history's does)"""
    import ssd_stage_oracle as S

    return S.flat_heads(S.head_case(_default_arch(), 2, seed=16)[0], images=[1])


def ssd_detection_large(h, nonfinite=False):
    h.ssd_detection_tap(heads=ssd_many_priors(nonfinite))
    if nonfinite:
        b, p = ssd_one_prior()
        h.ssd_detection_tap(boxes=nonfinite_like(np.repeat(b, 3, 0)), prob=nonfinite_like(np.repeat(p, 3, 0)))


def _ssd_detection_run(h, dirty=_noop):
    import ssd_stage_oracle as S

    b, p = ssd_one_prior()
    dirty()
    rows, count = h.ssd_detection_tap(boxes=b, prob=p)
    out = {"one_prior": {"rows": rows, "count": count}}
    dirty()
    bo, po, rows, count = h.ssd_detection_tap(heads=ssd_case_heads())
    out["heads"] = {"boxes": bo, "prob": po, "rows": rows, "count": count}
    return out


# ------------------------------------------------------------------------------------------------ MTCNN
def _bgr(rgb):
    return np.ascontiguousarray(rgb[..., ::-1])


@functools.lru_cache(maxsize=None)
def mtcnn_images():
    import mtcnn_stage_oracle as M

    small = _bgr(M.image(M.STALE_SMALL))
    return small, unlike(_bgr(M.image(M.STALE_BIG)), small, mtcnn_edge_image())


MTCNN_CASE_THRESHOLDS = (0.3, 0.3, 0.3)      # the dense seeded cascade puts the small image's P-Net probabilities at 0.34 .. 0.48


def mtcnn_case_params():
    return L.mtcnn_params(keep_all=True, min_face_size=20, thresholds=MTCNN_CASE_THRESHOLDS)


@functools.lru_cache(maxsize=None)
def mtcnn_windows(nonfinite=False, seed=31):
    rs = np.random.RandomState(seed)
    r, o = (rs.rand(300, 24, 24, 3) * 255).astype(np.float32), (rs.rand(600, 48, 48, 3) * 255).astype(np.float32)
    return (nonfinite_like(r), nonfinite_like(o)) if nonfinite else (r, o)


def mtcnn_large(h, nonfinite=False):
    small, big = mtcnn_images()
    p = L.mtcnn_params(keep_all=True, min_face_size=20)
    h.mtcnn_extract([big, _bgr(noise_frame(300, 280, 32)), big, white_frame(200, 200)], p, landmarks=True)
    h.mtcnn_align(big)
    r, o = mtcnn_windows(nonfinite, 34)
    h.mtcnn_net_tap("onet", o, "onet.prob")
    h.mtcnn_net_tap("rnet", r, "rnet.dense4")


@functools.lru_cache(maxsize=None)
def mtcnn_grow_images():
    small, big = mtcnn_images()
    return [unlike(_bgr(noise_frame(24, 24, 33)), small, mtcnn_edge_image()), big]


def mtcnn_grow(h):
    tiny, big = mtcnn_grow_images()
    h.mtcnn_align(tiny)
    h.mtcnn_extract([big, big, big], L.mtcnn_params(keep_all=True), landmarks=True)


MTCNN_EDGE = (47, 58, 24)       # mtcnn_stage_oracle.EDGE_CASES: three levels, no map width a multiple of the MFMA tile; seven
#                                 P-Net candidates at the default thresholds (the small image has none there)


@functools.lru_cache(maxsize=None)
def mtcnn_edge_image():
    import mtcnn_stage_oracle as M

    return _bgr(M.image(MTCNN_EDGE))


def _mtcnn_run(h, dirty=_noop):
    small, big = mtcnn_images()
    edge = mtcnn_edge_image()
    p = mtcnn_case_params()
    out = {}
    dirty()
    out["detect"] = [list(r[:2]) for r in h.mtcnn_detect([small], p, landmarks=True)]
    dirty()
    out["extract"] = [list(r) for r in h.mtcnn_extract([small], p, landmarks=True)]
    dirty()
    face, box = h.mtcnn_align(small)
    out["align"] = {"found": face is not None, "face": face, "box": box}
    for name in ("pnet.conv2.0", "pnet.prob.0"):
        dirty()
        out["tap." + name] = h.mtcnn_tap(small, name).copy()
    dirty()
    out["detect_edge"] = [list(r[:2]) for r in h.mtcnn_detect([edge, small], landmarks=True)]
    dirty()
    rec, counter = h.mtcnn_tap_batch([small, edge], 1, "pnet.cand")
    rec = np.ascontiguousarray(rec).view(np.uint32)
    out["tap_batch.pnet.cand"] = {"records": rec[np.lexsort(rec.T[::-1])], "counter": counter}      # the launch's atomics order them
    dirty()
    out["tap_batch.rnet.prob"] = h.mtcnn_tap_batch([small, edge], 1, "rnet.prob").copy()
    r, o = mtcnn_windows()
    dirty()
    out["net_tap.rnet"] = h.mtcnn_net_tap("rnet", r[:5], "rnet.reg").copy()
    dirty()
    out["net_tap.onet"] = h.mtcnn_net_tap("onet", o[:5], "onet.pts").copy()
    return out


# ------------------------------------------------------------------------------------------------ the Haar fallback
@functools.lru_cache(maxsize=None)
def haar_frames():
    import haar_cases as C

    small = C.noise_frame(64, 64, [(30, 34, 9)], 35)
    return small, [unlike(C.noise_frame(720, 1280, [(300, 300, 40), (900, 400, 70)], 36), small), white_frame(720, 1280),
                   checker_frame(720, 1280)]


def haar_large(h):
    for f in haar_frames()[1]:
        h.detect_faces_haar(f, 1.1, 0, 0, max_out=4096, with_candidates=True)


@functools.lru_cache(maxsize=None)
def haar_grow_frames():
    import haar_cases as C

    small, big = haar_frames()
    return [unlike(C.noise_frame(40, 40, [(20, 18, 7)], 37), small), big[0]]


def haar_grow(h):
    tiny, big = haar_grow_frames()
    h.detect_faces_haar(tiny, 1.1, 0, 0)
    h.detect_faces_haar(big, 1.1, 0, 0, max_out=4096)


def _haar_run(h, dirty=_noop):
    frame = haar_frames()[0]
    out = {}
    for mn in (0, 2):
        dirty()
        boxes, ncand = h.detect_faces_haar(frame, 1.1, mn, 0, max_out=4096, with_candidates=True)
        out[f"detect_min_neighbors_{mn}"] = {"boxes": boxes, "candidates": ncand}
    dirty()
    n_scales = h.haar_tap(frame, 1.1, 0, names=())["n_scales"]
    out["n_scales"] = n_scales
    for k in range(n_scales):
        for name in ("gray", "scaled", "sum", "sqsum", "result"):
            dirty()
            t = h.haar_tap(frame, 1.1, k, names=(name,))
            out[f"scale{k}.{name}"] = {"buf": t[name], "factor": t["factor"], "step": t["step"], "window": list(t["window"])}
    return out


# ------------------------------------------------------------------------------------------------ forensics
FORENSIC_STREAMS = (5, 6)               # the ids every history uses and releases; the cases use them again
FORENSIC_SIZES = (64, 208)              # the issue names 64 and 200; 200 is no multiple of 16 and the entry refuses it (asserted)


@functools.lru_cache(maxsize=None)
def forensic_frames(n: int, size: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, (n, size, size, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def forensic_case_data(size: int) -> np.ndarray:
    return forensic_frames(2, size, 48 if size == 256 else 49 + size)


@functools.lru_cache(maxsize=None)
def forensic_history_data(size: int) -> np.ndarray:
    return unlike(forensic_frames(14, size, 42 if size == 512 else 43), *[forensic_case_data(s) for s in (256,) + FORENSIC_SIZES])


@functools.lru_cache(maxsize=None)
def forensic_history_frame():
    return unlike(noise_frame(1080, 1920, 41), *[np.ascontiguousarray(f) for f in _forensic_stream_frames()])


def forensic_large(h):
    big = [forensic_history_frame(), white_frame(1080, 1920), checker_frame(1080, 1920)]
    for f in big:
        h.forensics(f, True, stream_id=FORENSIC_STREAMS[0])
        h.forensics_sized(f, 512, True, stream_id=FORENSIC_STREAMS[1])
    data = np.concatenate([forensic_history_data(512), white_frame(512, 512)[None], checker_frame(512, 512)[None]])
    h.forensic_tap_sized(data, 512, "stats")
    h.forensic_tap(np.concatenate([forensic_history_data(256), white_frame(256, 256)[None], checker_frame(256, 256)[None]]), "stats")
    for s in FORENSIC_STREAMS:
        h.forensics_release(s)


@functools.lru_cache(maxsize=None)
def forensic_grow_inputs():
    """(tap data at 32, tap data at 512, a 64 x 64 frame, a 1080p frame), none equal to a case input where they share a position"""
    data = [forensic_case_data(s) for s in (256,) + FORENSIC_SIZES]
    stream = [np.ascontiguousarray(f) for f in _forensic_stream_frames()]
    return [unlike(forensic_frames(1, 32, 44), *data), unlike(forensic_frames(16, 512, 45), *data),
            unlike(noise_frame(64, 64, 46), *stream), unlike(noise_frame(1080, 1920, 47), *stream)]


def forensic_grow(h):
    d32, d512, f64, f1080 = forensic_grow_inputs()
    h.forensic_tap_sized(d32, 32, "stats")
    h.forensic_tap_sized(d512, 512, "stats")
    h.forensics(f64, True, stream_id=FORENSIC_STREAMS[0])
    h.forensics(f1080, True, stream_id=FORENSIC_STREAMS[0])
    h.forensics_release(FORENSIC_STREAMS[0])


def _forensic_tap_run(h, dirty=_noop):
    out = {}
    data = forensic_case_data(256)
    for name in L.Handle.FORENSIC_TAPS:
        dirty()
        out[f"256.{name}"] = h.forensic_tap(data, name).copy()
    for size in FORENSIC_SIZES:
        data = forensic_case_data(size)
        for name in L.Handle.forensic_taps_sized(size)[0]:
            dirty()
            out[f"{size}.{name}"] = h.forensic_tap_sized(data, size, name).copy()
    dirty()
    try:
        h.forensic_tap_sized(forensic_frames(1, 200, 50), 200, "stats")
        out["refused_200"] = 0
    except L.DfdError as e:
        out["refused_200"] = e.code
    return out


@functools.lru_cache(maxsize=None)
def _forensic_stream_frames():
    import forensic_fused_frames as FF

    return FF.moving(3, 120, 160, 7)


def _forensic_stream_run(h, dirty=_noop):
    """forensics / forensics_sized on stream ids the history used and released; forensic_signals_device; the batched
    pass with two streams of two sizes"""
    seq = [np.ascontiguousarray(f) for f in _forensic_stream_frames()]
    a, b = FORENSIC_STREAMS
    out = {}
    dirty()
    for s in (a, b):
        h.forensics_release(s)
    out["state_before"] = list(h.forensics_state(a))
    out["forensics"] = [list(h.forensics(f, i != 1, stream_id=a)) for i, f in enumerate(seq)]
    out["forensics_sized"] = [list(h.forensics_sized(f, 64, i != 1, stream_id=b)) for i, f in enumerate(seq)]
    out["state_after"] = list(h.forensics_state(a)) + list(h.forensics_state(b))
    h.forensics_reset(a)
    out["state_reset"] = list(h.forensics_state(a))
    out["after_reset"] = list(h.forensics(seq[0], True, stream_id=a))
    for s in (a, b):
        h.forensics_release(s)
    dirty()
    frames = np.stack(seq)
    d = h.alloc(frames.nbytes).upload(frames)
    sc, md = h.forensic_signals_device(d.ptr, 3, 120, 160, [-1, 0, 1])
    d.free()
    out["signals_device"] = {"scores": sc, "mean_diff": md}
    dirty()
    for s in (a, b):
        h.forensics_release(s)
    h.forensics_open(b, 64)
    small = [np.ascontiguousarray(f[:90, :144]) for f in seq]
    out["streams_batch"] = [list(r) for r in h.analyze_streams_batch([seq[0], small[0], seq[1], small[1], seq[2]], [a, b, a, b, a],
                                                                     [True, True, False, True, True], max_faces=2)]
    for s in (a, b):
        h.forensics_release(s)
    return out


def _forensic_sensitivity_run(h, dirty=_noop):
    """the one case whose output legitimately depends on the history: the stream is NOT released, so the temporal signal
    and the frame counter carry the history's frames"""
    dirty()
    return {"forensics": list(h.forensics(np.ascontiguousarray(_forensic_stream_frames()[0]), True, stream_id=FORENSIC_STREAMS[0]))}


def forensic_unreleased(h):
    for f in (noise_frame(270, 480, 51), noise_frame(270, 480, 52)):
        h.forensics(f, True, stream_id=FORENSIC_STREAMS[0])


# ------------------------------------------------------------------------------------------------ frequency features
@functools.lru_cache(maxsize=None)
def freq_images():
    return noise_frame(16, 16, 53)[:, :, 0].copy(), noise_frame(200, 200, 54)


@functools.lru_cache(maxsize=None)
def freq_history_frame():
    return unlike(noise_frame(1080, 1920, 55), *freq_images())


def freq_large(h):
    for f in (freq_history_frame(), white_frame(1080, 1920), checker_frame(1080, 1920)):
        h.frequency_features(f)


@functools.lru_cache(maxsize=None)
def freq_grow_frames():
    return [unlike(noise_frame(8, 8, 56), *freq_images()), freq_history_frame()]


def freq_grow(h):
    for f in freq_grow_frames():
        h.frequency_features(f)


def _freq_run(h, dirty=_noop):
    gray, colour = freq_images()
    out = {}
    dirty()
    out["gray16"] = h.frequency_features(gray)
    dirty()
    out["colour200"] = h.frequency_features(colour)
    return out


# ------------------------------------------------------------------------------------------------ JPEG
def pillow_jpeg(img: np.ndarray, quality: int, subsampling=None, **kw) -> bytes:
    """Pillow's file of a BGR (or gray) image"""
    from PIL import Image

    im = Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[..., ::-1]))
    buf = io.BytesIO()
    if subsampling is not None:
        kw["subsampling"] = subsampling
    im.save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_decode(data: bytes) -> np.ndarray:
    from PIL import Image

    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


_JPEG_FILES: Dict[str, list] = {}


@functools.lru_cache(maxsize=None)
def jpeg_sources(kind: str) -> List[np.ndarray]:
    """the pixels behind the files Pillow writes here"""
    if kind == "420":
        return [noise_frame(16, 16, 60 + i) for i in range(2)]
    if kind == "gray":
        return [noise_frame(13, 17, 62 + i)[:, :, 0].copy() for i in range(2)]
    seed = {"history": 64, "history_restart": 74}[kind]
    return [unlike(noise_frame(512, 512, seed + i), *(jpeg_sources("420") + jpeg_sources("gray"))) for i in range(8)]


def jpeg_files(kind: str) -> List[bytes]:
    if kind not in _JPEG_FILES:
        if kind == "420":
            v = [pillow_jpeg(a, 85, 2) for a in jpeg_sources(kind)]
        elif kind == "gray":
            v = [pillow_jpeg(a, 85) for a in jpeg_sources(kind)]
        elif kind == "history":
            v = [pillow_jpeg(a, 100, 0) for a in jpeg_sources(kind)]
        elif kind == "restart":
            import jpeg_stream_cases as J

            v = [f.data for f in J.files("dri_beyond")[:2]] + [pillow_jpeg(noise_frame(40, 56, 72), 85, 2, restart_marker_blocks=2)]
        elif kind == "history_restart":
            v = [pillow_jpeg(a, 100, 0, restart_marker_blocks=8) for a in jpeg_sources(kind)]
        _JPEG_FILES[kind] = v
    return _JPEG_FILES[kind]


def jpeg_decode_large(h, restart=False):
    h.set_option("jpeg_device_entropy", 1)
    h.set_option("jpeg_device_restart", int(restart))
    files = jpeg_files("history_restart" if restart else "history")
    h.decode_jpeg_batch(files)
    h.decode_jpeg(files[0])
    h.set_option("jpeg_device_entropy", 2)
    h.set_option("jpeg_device_restart", 0)


@functools.lru_cache(maxsize=None)
def jpeg_grow_source():
    return unlike(noise_frame(8, 8, 80), *(jpeg_sources("420") + jpeg_sources("gray")))


def jpeg_decode_grow(h):
    h.set_option("jpeg_device_entropy", 1)
    h.decode_jpeg_batch([pillow_jpeg(jpeg_grow_source(), 50, 0)])
    h.decode_jpeg_batch(jpeg_files("history"))
    h.set_option("jpeg_device_entropy", 2)


def _jpeg_decode_run_for(restart: bool):
    def run(h, dirty=_noop):
        out = {}

        def call(fn):
            dirty()
            h.set_option("jpeg_device_entropy", 1)
            h.set_option("jpeg_device_restart", int(restart))
            try:
                return fn()
            finally:
                h.set_option("jpeg_device_entropy", 2)
                h.set_option("jpeg_device_restart", 0)

        kinds = ("restart",) if restart else ("420", "gray")
        for kind in kinds:
            files = jpeg_files(kind)
            for i, f in enumerate(files):
                out[f"{kind}.single{i}"] = call(lambda: h.decode_jpeg(f))
            same = files[:2]

            def counted():                          # the batch went through the device entropy decoder, not the host pool
                before = h.jpeg_decode_counts()
                pixels = h.decode_jpeg_batch(same)
                now = h.jpeg_decode_counts()
                return pixels, [now[0] - before[0], now[1] - before[1]]
            out[f"{kind}.batch"], out[f"{kind}.batch_counts"] = call(counted)
            if restart:
                out[f"{kind}.batch_pillow"] = call(lambda: h.decode_jpeg_batch(files[2:]))
        return out
    return run


def jpeg_decode_expected(restart: bool) -> dict:
    """Pillow's decode of the same files, in the layout of the case's result"""
    out = {}
    for kind in (("restart",) if restart else ("420", "gray")):
        files = jpeg_files(kind)
        for i, f in enumerate(files):
            out[f"{kind}.single{i}"] = pillow_decode(f)
        out[f"{kind}.batch"] = np.stack([pillow_decode(f) for f in files[:2]])
        out[f"{kind}.batch_counts"] = [2, 0]                    # (frames decoded on the device, frames decoded on the host)
        if restart:
            out[f"{kind}.batch_pillow"] = np.stack([pillow_decode(f) for f in files[2:]])
    return out


@functools.lru_cache(maxsize=None)
def jpeg_encode_images():
    return [noise_frame(1, 1, 81), noise_frame(13, 17, 82)]


@functools.lru_cache(maxsize=None)
def jpeg_encode_history_image():
    return unlike(noise_frame(512, 512, 83), *jpeg_encode_images())


def jpeg_encode_large(h):
    big = jpeg_encode_history_image()
    h.encode_jpegs([big, white_frame(512, 512), checker_frame(512, 512)], quality=100, subsampling=0)
    h.encode_jpegs([big], quality=100, subsampling=2, restart_blocks=4)


@functools.lru_cache(maxsize=None)
def jpeg_encode_grow_image():
    return unlike(noise_frame(8, 8, 84), *jpeg_encode_images())


def jpeg_encode_grow(h):
    h.encode_jpegs([jpeg_encode_grow_image()], quality=50)
    h.encode_jpegs([jpeg_encode_history_image()], quality=100, subsampling=0)


def _jpeg_encode_run(h, dirty=_noop):
    import ctypes as C

    imgs = jpeg_encode_images()
    out = {}
    dirty()
    out["batch"] = h.encode_jpegs(imgs, quality=75, subsampling=2)
    dirty()
    out["gray"] = h.encode_jpegs([imgs[1][:, :, 0].copy()], quality=90)
    # dfd_encode_jpeg, the one-image export: Handle.encode_jpeg goes through the batch entry, so it has no wrapper to call
    a = imgs[1]
    buf = np.zeros(int(h._lib.dfd_encode_jpeg_bound(a.shape[0], a.shape[1], 0)), np.uint8)
    n = C.c_size_t()
    dirty()
    h._check(h._lib.dfd_encode_jpeg(h._p, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1], a.shape[1] * 3, 0, 75, 0, 0,
                                    buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)))
    out["single_444"] = buf[: n.value].tobytes()
    d = h.alloc(a.nbytes).upload(a)
    dirty()
    out["device"] = h.encode_jpegs_device([(d.ptr, a.shape[0], a.shape[1], a.shape[1] * 3, 3)], quality=75, subsampling=2)
    d.free()
    return out


def jpeg_encode_expected() -> dict:
    import jpeg_encode_oracle as JO

    imgs = jpeg_encode_images()
    return {"batch": [JO.pillow_bytes(a, 75, 2) for a in imgs], "gray": [JO.pillow_bytes(imgs[1][:, :, 0].copy(), 90)],
            "single_444": JO.pillow_bytes(imgs[1], 75, 0), "device": [JO.pillow_bytes(imgs[1], 75, 2)]}


# ------------------------------------------------------------------------------------------------ train-time augmentation
AUG_CASE = dict(n=1, h=32, w=48, t=32, seed=91)
AUG_HISTORY = dict(n=8, h=96, w=128, t=224, seed=92)


@functools.lru_cache(maxsize=None)
def aug_inputs(n, h, w, t, seed):
    import test_train_augment_gpu as TG

    rgb = TG._sources(n, h, w, seed)
    if seed != AUG_CASE["seed"]:
        rgb = unlike(rgb, TG._sources(AUG_CASE["n"], AUG_CASE["h"], AUG_CASE["w"], AUG_CASE["seed"]))
    rows, batch = TG._tables(n, h, w, t, seed + 1)            # image 0: every stage on
    return rgb, rows, batch


def aug_large(h):
    p = AUG_HISTORY
    rgb, rows, batch = aug_inputs(**p)
    h.train_augment(rgb, rows, batch, p["t"])
    h.train_augment_trunk(rgb, rows, batch, block=14)
    for extra in (np.full_like(rgb, 255), np.stack([checker_frame(p["h"], p["w"])] * p["n"])):
        h.train_augment(extra, rows, batch, p["t"])


def aug_grow(h):
    rgb, rows, batch = aug_inputs(1, 32, 32, 32, 93)
    h.train_augment(rgb, rows, batch, 32)
    p = AUG_HISTORY
    rgb, rows, batch = aug_inputs(**p)
    h.train_augment(rgb, rows, batch, p["t"])


def _aug_run(h, dirty=_noop):
    p = AUG_CASE
    rgb, rows, batch = aug_inputs(**p)
    out = {}
    for stage in ("jpeg", "resize") + L.Handle.AUG_U8_STAGES[2:] + L.Handle.AUG_F32_STAGES:
        dirty()
        out["tap." + stage] = h.train_augment_tap(rgb, rows, batch, stage, p["t"])
    dirty()
    out["train_augment"] = h.train_augment(rgb, rows, batch, p["t"])
    dirty()
    out["trunk14"] = h.train_augment_trunk(rgb, rows, batch, block=14)
    dirty()
    out["trunk15"] = h.train_augment_trunk(rgb, rows, batch, block=15)
    dirty()
    out["features"] = h.train_augment_features(rgb, rows, batch)
    src, dst = h.alloc(rgb.nbytes * 2).upload(np.concatenate([rgb[::-1], rgb])), h.alloc(rgb.nbytes)
    dirty()
    h.train_augment_gather(src, (2 * p["n"], p["h"], p["w"]), [p["n"]], dst)
    out["gathered_features"] = h.train_augment_features(dst, rows, batch, shape=(p["n"], p["h"], p["w"]))
    src.free()
    dst.free()
    return out


# ------------------------------------------------------------------------------------------------ the three trainers
TRAIN_LEVELS = ("head", "conv", "block")
# of seeds 0..39 the one with the largest smaller gate margin of the two accumulates, on the oracles alone (head 813 / 164,
# conv 253 / 80, block 2275 / 76); test_history_cases.py asserts them
TRAIN_SEED = {"head": 35, "conv": 39, "block": 25}
TRAIN_N = (2, 5)
TRAIN_HISTORY_N = 64
HEAD_TAPS = ("mask0", "mask1", "mask2", "z1", "z2")
CONV_TAPS = ("cfeat", "dfeat", "cz")


@functools.lru_cache(maxsize=None)
def train_params(level: str):
    """(head, conv, block) parameter dicts the level begins with (conv / block: None below their level)"""
    import block15_train_oracle as BO
    import head_train_oracle as HO
    import headconv_train_oracle as CO

    sd = B.stress_state_dict(0)
    return (HO.default_params(TRAIN_SEED[level]), CO.conv_params(sd) if level != "head" else None,
            BO.block_params(sd) if level == "block" else None)


@functools.lru_cache(maxsize=None)
def train_rows(level: str, n: int, seed: int, nonfinite=False) -> np.ndarray:
    import block15_train_oracle as BO
    import head_train_oracle as HO
    import headconv_train_oracle as CO

    x = {"head": HO.features, "conv": CO.synthetic_trunk, "block": BO.synthetic_rows}[level](seed, n)
    return nonfinite_like(x) if nonfinite else x


@functools.lru_cache(maxsize=None)
def train_labels(seed: int, n: int) -> np.ndarray:
    return (np.random.RandomState(seed).rand(n) < 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def train_case_batches(level: str):
    s = TRAIN_SEED[level]
    return [(train_rows(level, n, s + 100 + k), train_labels(s + 200 + k, n)) for k, n in enumerate(TRAIN_N)]


def _train_open(h, level: str, max_n: int):
    head, conv, block = train_params(level)
    h.head_train_begin(head, L.head_config(max_n=max_n, seed=TRAIN_SEED[level]))
    if conv is not None:
        h.head_train_unfreeze_conv(conv)
    if block is not None:
        h.head_train_unfreeze_block(block)


def _train_fns(h, level: str):
    acc = {"head": h.head_train_accumulate, "conv": h.head_train_accumulate_trunk, "block": h.head_train_accumulate_block}[level]
    ev = {"head": h.head_train_eval, "conv": h.head_train_eval_trunk, "block": h.head_train_eval_block}[level]
    return acc, ev


def _train_state(h, level: str, ema=False):
    out = {"grads": h.head_train_grads(), "export": h.head_train_export(ema)}
    if level != "head":
        out["conv.grads"], out["conv.export"] = h.head_train_conv_grads(), h.head_train_export_conv(ema)
    if level == "block":
        out["b15.grads"], out["b15.export"] = h.head_train_block_grads(), h.head_train_export_block(ema)
    return out


@functools.lru_cache(maxsize=None)
def _forced_gradients(level: str, nonfinite: bool, seed: int = 95):
    rs = np.random.RandomState(seed)

    def make(shapes, skip):
        g = {k: rs.randn(*s).astype(np.float32) for k, s in shapes.items() if k not in skip}
        return {k: nonfinite_like(v) for k, v in g.items()} if nonfinite else g

    out = {"head": make(L.HEAD_SHAPES, ("rm1", "rv1", "rm2", "rv2"))}
    if level != "head":
        out["conv"] = make(L.CONV_SHAPES, ("rm", "rv"))
    if level == "block":
        out["block"] = make(L.BLOCK_SHAPES, L.BLOCK_STAT_FIELDS)
    return out


def trainer_large(h, level: str, nonfinite=False):
    """a whole session at max_n = 64 on other rows: two accumulates, forced gradients, an apply, end"""
    _train_open(h, level, TRAIN_HISTORY_N)
    try:
        acc, ev = _train_fns(h, level)
        for k, n in enumerate((TRAIN_HISTORY_N, 37)):
            acc(train_rows(level, n, 300 + k, nonfinite), train_labels(310 + k, n), train_labels(320 + k, n), 0.7, 0.5)
        g = _forced_gradients(level, nonfinite)
        h.head_train_grads(set_to=g["head"])
        if "conv" in g:
            h.head_train_conv_grads(set_to=g["conv"])
        if "block" in g:
            h.head_train_block_grads(set_to=g["block"])
        h.head_train_apply(1e-2)
        ev(train_rows(level, TRAIN_HISTORY_N, 330), True)
    finally:
        h.head_train_end()


def trainer_grow(h, level: str):
    for max_n in (2, TRAIN_HISTORY_N):
        _train_open(h, level, max_n)
        try:
            _train_fns(h, level)[0](train_rows(level, max_n, 340), train_labels(341, max_n))
        finally:
            h.head_train_end()


def _trainer_run_for(level: str):
    taps = HEAD_TAPS + (CONV_TAPS if level != "head" else ()) + (("b15.out", "b15.gate", "b15.ad", "b15.dout", "b15.dae") if level == "block" else ())

    def run(h, dirty=_noop):
        dirty()                                   # one session is one case: the history ends before its begin
        out = {}
        _train_open(h, level, 8)
        try:
            acc, ev = _train_fns(h, level)
            for k, (x, y) in enumerate(train_case_batches(level)):
                loss, logits = acc(x, y)
                step = {"loss": loss, "logits": logits.copy()}
                for t in taps:
                    step["tap." + t] = h.head_train_tap(t, x.shape[0])
                step.update(_train_state(h, level))
                out[f"accumulate{k}"] = step
            out["grad_norm"] = h.head_train_apply(1e-3)
            held = train_rows(level, 5, TRAIN_SEED[level] + 400)
            out["eval_live"], out["eval_ema"] = ev(held, False).copy(), ev(held, True).copy()
            out["after_apply"] = _train_state(h, level)
            out["after_apply_ema"] = _train_state(h, level, True)
        finally:
            h.head_train_end()
        return out
    return run


def trainer_margins(level: str) -> List[float]:
    """the gate margin of the case's accumulates on the float64 / float32 oracles (>= 1: the precondition the trainer
    tests hold their inputs to; no device involved)"""
    import block15_train_oracle as BO
    import head_train_oracle as HO
    import headconv_train_oracle as CO

    head, conv, block = train_params(level)
    cfg = HO.config_values(L.head_config(max_n=8, seed=TRAIN_SEED[level]))
    if level == "head":
        o64, o32 = HO.pair(head, cfg)
        gm = HO.gate_margin
    elif level == "conv":
        o64, o32 = CO.pair(conv, head, cfg)
        gm = CO.gate_margin
    else:
        o64, o32 = BO.pair(block, conv, head, cfg)
        gm = BO.gate_margin
    out = []
    for x, y in train_case_batches(level):
        o64.accumulate(x, y, None, 1.0, 1.0)
        o32.accumulate(x, y, None, 1.0, 1.0)
        out.append(float(gm(o64, o32)))
    return out


# ------------------------------------------------------------------------------------------------ the fused entries
@functools.lru_cache(maxsize=None)
def fused_frame():
    import frames

    return frames.face_frame(320, 240, 4)


@functools.lru_cache(maxsize=None)
def fused_history_frames():
    import frames

    return [unlike(frames.face_frame(1280, 720, 5), fused_frame()), white_frame(720, 1280), checker_frame(720, 1280)]


def fused_large(h):
    s = FORENSIC_STREAMS[0]
    h.analyze_stream_batch(fused_history_frames(), [True, False, True], stream_id=s, max_faces=4)
    h.forensics_release(s)
    h.analyze_stream_batch(fused_history_frames(), [False, True, True], stream_id=s, max_faces=1, tta=(2, tta_draw_list(3, 2)))
    h.forensics_release(s)


@functools.lru_cache(maxsize=None)
def fused_grow_frame():
    return unlike(noise_frame(48, 64, 96), fused_frame())


def fused_grow(h):
    s = FORENSIC_STREAMS[0]
    h.analyze_frame(fused_grow_frame(), True, stream_id=s, max_faces=1)
    h.analyze_stream_batch(fused_history_frames(), [True, True, True], stream_id=s, max_faces=4)
    h.forensics_release(s)


def _fused_run(h, dirty=_noop):
    frame = fused_frame()
    data = pillow_jpeg(frame, 90, 2)
    s = FORENSIC_STREAMS[0]
    out = {}

    def call(fn):
        dirty()
        h.forensics_release(s)
        try:
            return fn()
        finally:
            h.forensics_release(s)

    out["analyze_frame"] = call(lambda: list(h.analyze_frame(frame, True, stream_id=s, max_faces=4)))
    out["analyze_frame_tta"] = call(lambda: list(h.analyze_frame(frame, False, stream_id=s, max_faces=4, tta=(2, tta_draw_list(4, 2)))))
    out["analyze_jpeg"] = call(lambda: list(h.analyze_jpeg(data, True, stream_id=s, max_faces=4)))
    out["analyze_stream_batch"] = call(lambda: [list(r) for r in h.analyze_stream_batch([frame, data], [True, False], stream_id=s,
                                                                                        max_faces=4)[0]])
    frames4 = np.ascontiguousarray(frame[None])
    out["analyze_frames_host"] = call(lambda: list(h.analyze_frames_host(frames4, 1, max_faces=4, with_forensics=True)))
    out["analyze_jpegs_host"] = call(lambda: list(h.analyze_jpegs_host([data], 1, max_faces=4, with_forensics=True)))

    def on_device():
        d = h.alloc(frames4.nbytes).upload(frames4)
        try:
            return list(h.analyze_batch_device(d.ptr, 1, 240, 320, max_faces=4, with_forensics=True))
        finally:
            d.free()
    out["analyze_batch_device"] = call(on_device)
    return out


# ------------------------------------------------------------------------------------------------ the table
_T = ("dfd_head_train_begin", "dfd_head_train_apply", "dfd_head_train_export", "dfd_head_train_grads", "dfd_head_train_tap",
      "dfd_head_train_end")
TRAIN_REACHES = {
    "head": _T + ("dfd_head_train_accumulate", "dfd_head_train_eval"),
    "conv": _T + ("dfd_head_train_unfreeze_conv", "dfd_head_train_accumulate_trunk", "dfd_head_train_eval_trunk",
                  "dfd_head_train_export_conv", "dfd_head_train_conv_grads"),
    "block": _T + ("dfd_head_train_unfreeze_conv", "dfd_head_train_unfreeze_block", "dfd_head_train_accumulate_block",
                   "dfd_head_train_eval_block", "dfd_head_train_export_block", "dfd_head_train_block_grads",
                   "dfd_head_train_export_conv", "dfd_head_train_conv_grads"),
}
U8_HISTORIES = ("repeat", "large", "grow", "cross")          # 8-bit input only: no non-finite history

OTHER_CASES: List[Case] = [
    Case("gemm_tap", "gemm", _gemm_run, ("dfd_gemm_tap",)),
    Case("gradcam_tap", "gradcam", _gradcam_run, ("dfd_gradcam_tap",)),
    Case("face_path", "face", _face_run,
         ("dfd_preprocess_crops", "dfd_classify_crops", "dfd_classify_crops_tta", "dfd_tta_augment", "dfd_tta_augment_crops",
          "dfd_gradcam_crops", "dfd_preprocess_face_quality", "dfd_resize_bgr"), U8_HISTORIES),
    Case("ssd", "ssd", _ssd_run_for(_default_arch), ("dfd_detect_faces", "dfd_ssd_tap"), U8_HISTORIES),
    Case("ssd_variant_fused", "ssd", _ssd_run_for(_variant_arch(0)), ("dfd_detect_faces", "dfd_ssd_tap"), ("repeat", "large"),
         blob="ssd_variant0"),
    Case("ssd_variant_two_readers", "ssd", _ssd_run_for(_variant_arch(1)), ("dfd_detect_faces", "dfd_ssd_tap"), ("repeat", "large"),
         blob="ssd_variant1"),
    Case("ssd_detection_tap", "ssd_detection", _ssd_detection_run, ("dfd_ssd_detection_tap",), ("repeat", "large", "nonfinite", "cross")),
    # tests/test_mtcnn_stages_gpu.py::test_stale_scratch_of_a_large_call_does_not_reach_a_small_one holds every P-Net tap
    # of the small image to a fresh handle's bits after non-finite R- / O-Net leftovers; this case holds the product calls
    Case("mtcnn", "mtcnn", _mtcnn_run,
         ("dfd_mtcnn_detect", "dfd_mtcnn_extract", "dfd_mtcnn_align", "dfd_mtcnn_tap", "dfd_mtcnn_tap_batch", "dfd_mtcnn_net_tap")),
    Case("haar", "haar", _haar_run, ("dfd_detect_faces_haar", "dfd_haar_tap"), U8_HISTORIES),
    Case("forensic_taps", "forensics", _forensic_tap_run, ("dfd_forensic_tap", "dfd_forensic_tap_sized"), U8_HISTORIES),
    Case("forensic_streams", "forensics", _forensic_stream_run,
         ("dfd_forensics", "dfd_forensics_sized", "dfd_forensics_reset", "dfd_forensics_release", "dfd_forensics_state",
          "dfd_forensics_open", "dfd_forensic_signals_device", "dfd_analyze_streams_batch"), U8_HISTORIES),
    Case("frequency_features", "frequency", _freq_run, ("dfd_frequency_features",), U8_HISTORIES),
    Case("jpeg_decode", "jpeg_decode", _jpeg_decode_run_for(False), ("dfd_decode_jpeg", "dfd_decode_jpeg_batch", "dfd_frame_ptr",
                                                                     "dfd_memcpy_d2h"), U8_HISTORIES),
    Case("jpeg_decode_restart", "jpeg_decode", _jpeg_decode_run_for(True), ("dfd_decode_jpeg", "dfd_decode_jpeg_batch"),
         U8_HISTORIES, arg=True),
    Case("jpeg_encode", "jpeg_encode", _jpeg_encode_run,
         ("dfd_encode_jpeg", "dfd_encode_jpeg_batch", "dfd_encode_jpeg_device", "dfd_encode_jpeg_bound"), U8_HISTORIES),
    Case("train_augment", "augment", _aug_run,
         ("dfd_train_augment_tap", "dfd_train_augment", "dfd_train_augment_trunk", "dfd_train_augment_trunk_at",
          "dfd_train_augment_features", "dfd_train_augment_gather"), U8_HISTORIES),
] + [Case(f"trainer_{lv}", "trainer", _trainer_run_for(lv), TRAIN_REACHES[lv], arg=lv) for lv in TRAIN_LEVELS] + [
    Case("fused_entries", "fused", _fused_run,
         ("dfd_analyze_frame", "dfd_analyze_jpeg", "dfd_analyze_stream_batch", "dfd_analyze_frames_host", "dfd_analyze_jpegs_host",
          "dfd_analyze_batch_device", "dfd_tta_arm", "dfd_tta_logits"), U8_HISTORIES),
]
SENSITIVITY = Case("forensics_stream_not_reset", "forensics", _forensic_sensitivity_run, ("dfd_forensics",), ("unreleased",))

CASES: List[Case] = classifier_cases() + OTHER_CASES
BY_NAME = {c.name: c for c in CASES}

# family -> {history: fn(h, case)}; "repeat" and "cross" are the same for every family (`history`)
HISTORIES = {
    "classifier": {"large": lambda h, c: classifier_large(h, c.arg), "grow": lambda h, c: classifier_grow(h, c.arg),
                   "nonfinite": lambda h, c: classifier_large(h, c.arg, True)},
    "gemm": {"large": lambda h, c: gemm_large(h), "grow": lambda h, c: gemm_grow(h), "nonfinite": lambda h, c: gemm_large(h, True)},
    "gradcam": {"large": lambda h, c: gradcam_large(h), "grow": lambda h, c: gradcam_grow(h),
                "nonfinite": lambda h, c: gradcam_large(h, True)},
    "face": {"large": lambda h, c: face_large(h), "grow": lambda h, c: face_grow(h)},
    "ssd": {"large": lambda h, c: ssd_large(h), "grow": lambda h, c: ssd_grow(h)},
    "ssd_detection": {"large": lambda h, c: ssd_detection_large(h), "nonfinite": lambda h, c: ssd_detection_large(h, True)},
    "mtcnn": {"large": lambda h, c: mtcnn_large(h), "grow": lambda h, c: mtcnn_grow(h), "nonfinite": lambda h, c: mtcnn_large(h, True)},
    "haar": {"large": lambda h, c: haar_large(h), "grow": lambda h, c: haar_grow(h)},
    "forensics": {"large": lambda h, c: forensic_large(h), "grow": lambda h, c: forensic_grow(h),
                  "unreleased": lambda h, c: forensic_unreleased(h)},
    "frequency": {"large": lambda h, c: freq_large(h), "grow": lambda h, c: freq_grow(h)},
    "jpeg_decode": {"large": lambda h, c: jpeg_decode_large(h, bool(c.arg)), "grow": lambda h, c: jpeg_decode_grow(h)},
    "jpeg_encode": {"large": lambda h, c: jpeg_encode_large(h), "grow": lambda h, c: jpeg_encode_grow(h)},
    "augment": {"large": lambda h, c: aug_large(h), "grow": lambda h, c: aug_grow(h)},
    "trainer": {"large": lambda h, c: trainer_large(h, c.arg), "grow": lambda h, c: trainer_grow(h, c.arg),
                "nonfinite": lambda h, c: trainer_large(h, c.arg, True)},
    "fused": {"large": lambda h, c: fused_large(h), "grow": lambda h, c: fused_grow(h)},
}
# one call of each family at its largest shape, for "cross" (the trainer: its deepest level)
CROSS = {
    "classifier": lambda h: classifier_large(h, CLS_RESET), "gemm": gemm_large, "gradcam": gradcam_large, "face": face_large,
    "ssd": ssd_large, "ssd_detection": ssd_detection_large, "mtcnn": mtcnn_large, "haar": haar_large, "forensics": forensic_large,
    "frequency": freq_large, "jpeg_decode": jpeg_decode_large, "jpeg_encode": jpeg_encode_large, "augment": aug_large,
    "trainer": lambda h: trainer_large(h, "block"), "fused": fused_large,
}


def cross(h, family: str):
    for name, fn in CROSS.items():
        if name != family:
            fn(h)


def history(case: Case, name: str) -> Callable:
    """the history `name` of `case` as a function of the handle ("repeat" is the case itself and is run by the caller)"""
    if name == "cross":
        return lambda h: cross(h, case.family)
    fn = HISTORIES[case.family][name]
    return lambda h: fn(h, case)


def pairs():
    """every (case, history) the GPU file runs"""
    return [(c, hname) for c in CASES for hname in c.histories]


# ------------------------------------------------------------------------------------------------ the inputs, for the CPU checks
def _pairs(hists, cases):
    """every (history array, case array) that can share element positions: one type, one rank (or a gray case image
    against a colour frame)"""
    return [(a, c) for a in hists for c in cases
            if a.dtype == c.dtype and (a.ndim == c.ndim or (a.dtype == np.uint8 and c.ndim == 2 and a.ndim == 3))]


def _gemm_pairs(history_cases_):
    out = []
    for a in history_cases_:
        for b in gemm_picks():
            for k in ("x", "gate", "res"):
                ha, cb = gemm_inputs(a, True)[k], gemm_inputs(b)[k]
                if ha is not None and cb is not None and ha.ndim == cb.ndim:
                    out.append((ha, cb))
    return out


@functools.lru_cache(maxsize=None)
def history_inputs() -> Dict[str, Dict[str, list]]:
    """family -> history -> [(history input, case input)]: every array a `large` or `grow` history hands to the library,
    paired with every case input it can share element positions with.  (The all-255 and checkerboard frames a `large`
    history adds for 8-bit paths are extra and not held to this; `nonfinite` is `large` with `nonfinite_inputs`, `cross`
    the `large` histories of the other families, `repeat` the case itself.)"""
    import gemm_oracle as G

    large = _large_inputs()
    stream = [np.ascontiguousarray(f) for f in _forensic_stream_frames()]
    data = [forensic_case_data(s) for s in (256,) + FORENSIC_SIZES]
    crops = [case_crops(n) for n in CLS_N]
    small, _ = mtcnn_images()
    trainer = [x for lv in TRAIN_LEVELS for x, _ in train_case_batches(lv)]
    grow = {
        "classifier": _pairs([history_crops(n=1), history_crops()], crops),
        "gemm": _gemm_pairs([G.Case("pointwise", m, 264, 196, act="swish", res="after") for m in (17, 8200)]),
        "gradcam": _pairs([a for n in (1, MAX_BATCH) for a in gradcam_inputs(n, 72) + (history_crops(n=n),)],
                          list(gradcam_inputs(3, 70)) + [case_crops(3)]),
        "face": _pairs([face_history_frame()], [noise_frame(*FACE_FRAME)]),
        "ssd": _pairs(ssd_grow_frames(), [ssd_case_frame()]),
        "mtcnn": _pairs(mtcnn_grow_images(), [small, mtcnn_edge_image()]),
        "haar": _pairs(haar_grow_frames(), [haar_frames()[0]]),
        "forensics": _pairs(forensic_grow_inputs(), data + stream),
        "frequency": _pairs(freq_grow_frames(), list(freq_images())),
        "jpeg_decode": _pairs([jpeg_grow_source()] + jpeg_sources("history"), jpeg_sources("420") + jpeg_sources("gray")),
        "jpeg_encode": _pairs([jpeg_encode_grow_image(), jpeg_encode_history_image()], jpeg_encode_images()),
        "augment": _pairs([aug_inputs(1, 32, 32, 32, 93)[0], aug_inputs(**AUG_HISTORY)[0]], [aug_inputs(**AUG_CASE)[0]]),
        "trainer": _pairs([train_rows(lv, n, 340) for lv in TRAIN_LEVELS for n in (2, TRAIN_HISTORY_N)], trainer),
        "fused": _pairs([fused_grow_frame(), fused_history_frames()[0]], [fused_frame()]),
    }
    return {f: {"large": large[f], **({"grow": grow[f]} if f in grow else {})} for f in large}


def _large_inputs() -> Dict[str, list]:
    import gemm_oracle as G
    import ssd_stage_oracle as S

    hp, cp = gemm_history_shapes(), gemm_picks()
    gemm = [(gemm_inputs(a, True)[k], gemm_inputs(b)[k]) for a, b in ((hp[0], cp[0]), (hp[0], cp[1]), (hp[1], cp[5]), (hp[2], cp[3]),
                                                                        (hp[3], cp[9]), (hp[4], cp[7])) for k in ("x", "gate", "res")
            if gemm_inputs(a, True)[k] is not None and gemm_inputs(b)[k] is not None]
    gh, gc = gradcam_inputs(MAX_BATCH, 71), gradcam_inputs(3, 70)
    small, big = mtcnn_images()
    hs, hb = haar_frames()
    ob, op = ssd_one_prior()
    stream = [np.ascontiguousarray(f) for f in _forensic_stream_frames()]
    trainer = [(train_rows(lv, TRAIN_HISTORY_N, 300), x) for lv in TRAIN_LEVELS for x, _ in train_case_batches(lv)]
    return {
        "classifier": [(history_crops(), case_crops(n)) for n in CLS_N],
        "gemm": gemm,
        "gradcam": list(zip(gh, gc)) + [(history_crops(), case_crops(3))],
        "face": [(face_history_frame(), noise_frame(*FACE_FRAME))],
        "ssd": [(ssd_history_frames()[0], ssd_case_frame())],
        "ssd_detection": [(ssd_many_priors()[: S.P * 6], ssd_case_heads())],
        "mtcnn": [(big, small), (big, mtcnn_edge_image())] + list(zip(mtcnn_windows(seed=34), mtcnn_windows())),
        "haar": [(hb[0], hs)],
        "forensics": [(forensic_history_data(512), forensic_case_data(s)) for s in (256,) + FORENSIC_SIZES] +
                     [(forensic_history_data(256), forensic_case_data(256))] + [(forensic_history_frame(), f) for f in stream],
        "frequency": [(freq_history_frame(), a) for a in freq_images()],
        "jpeg_decode": [(h, c) for h in jpeg_sources("history")[:2] for c in jpeg_sources("420") + jpeg_sources("gray")],
        "jpeg_encode": [(jpeg_encode_history_image(), a) for a in jpeg_encode_images()],
        "augment": [(aug_inputs(**AUG_HISTORY)[0], aug_inputs(**AUG_CASE)[0])],
        "trainer": trainer,
        "fused": [(fused_history_frames()[0], fused_frame())],
    }


@functools.lru_cache(maxsize=None)
def nonfinite_inputs() -> Dict[str, list]:
    """family -> the float arrays its `nonfinite` history hands to the library"""
    r, o = mtcnn_windows(True, 34)
    b, p = ssd_one_prior()
    gem = [gemm_inputs(c, True, True) for c in gemm_history_shapes()]
    return {
        "classifier": [history_crops(True)],
        "gemm": [i[k] for i in gem for k in ("x", "gate", "res") if i[k] is not None],
        "gradcam": list(gradcam_inputs(MAX_BATCH, 71, True)) + [history_crops(True)],
        "ssd_detection": [ssd_many_priors(True), nonfinite_like(b), nonfinite_like(p)],
        "mtcnn": [r, o],
        "trainer": [train_rows(lv, TRAIN_HISTORY_N, 300, True) for lv in TRAIN_LEVELS] +
                   [v for lv in TRAIN_LEVELS for g in _forced_gradients(lv, True).values() for v in g.values()],
    }


# ------------------------------------------------------------------------------------------------ coverage
EXEMPT = {
    "dfd_abi_version": "no handle, no device",
    "dfd_create": "create / destroy: every test makes its handles with it",
    "dfd_destroy": "create / destroy",
    "dfd_last_error": "error text",
    "dfd_max_batch": "a constant of the handle",
    "dfd_set_option": "options: part of every case that needs one, no output of its own",
    "dfd_gemm_tile_count": "a constant of the library",
    "dfd_warmup": "the tile table: neither handle warms up, both take the heuristic tile (test_gemm_tiles_gpu.py holds every tile to the same bits)",
    "dfd_tiles_export": "tiles import / export",
    "dfd_tiles_import": "tiles import / export",
    "dfd_gemm_chunk_rows": "host arithmetic, no handle",
    "dfd_device_alloc": "alloc / free",
    "dfd_device_free": "alloc / free",
    "dfd_memcpy_h2d": "a copy, used by the cases that work on device buffers",
    "dfd_sync": "waits, computes nothing",
    "dfd_wait_for": "orders two handles, computes nothing",
    "dfd_timer_begin": "timers",
    "dfd_timer_end": "timers",
    "dfd_has_detector": "a constant of the blob",
    "dfd_has_haar": "a constant of the blob",
    "dfd_has_mtcnn": "a constant of the blob",
    "dfd_last_detection_count": "counters",
    "dfd_classifier_crop_count": "counters: persistent by design",
    "dfd_jpeg_decode_counts": "counters: persistent by design",
    "dfd_mtcnn_params_default": "fills a struct on the host",
    "dfd_head_config_default": "fills a struct on the host",
    "dfd_jpeg_coefficients": "host half of the decoder, no handle",
    "dfd_train_augment_noise_words": "host test tap, no handle",
    "dfd_host_alloc": "host alloc",
    "dfd_host_free": "host alloc",
    "dfd_comm_unique_id": "comm_*: multi-GPU, out of scope",
    "dfd_comm_init": "comm_*",
    "dfd_comm_destroy": "comm_*",
    "dfd_comm_info": "comm_*",
    "dfd_vote_allgather": "comm_*",
    "dfd_vote_allgather_waves": "comm_*",
    "dfd_b0_profile_begin": "profiling",
    "dfd_b0_profile_end": "profiling",
    "dfd_head_train_commit": "committed weights are persistent state by design: no history commits, so no case can",
}


def coverage():
    """(exports neither reached nor exempt, names of the table that are no export, names both reached and exempt)"""
    reached = {n for c in CASES + [SENSITIVITY] for n in c.reaches}
    known = set(L.SIGNATURES)
    return sorted(known - reached - set(EXEMPT)), sorted((reached | set(EXEMPT)) - known), sorted(reached & set(EXEMPT))

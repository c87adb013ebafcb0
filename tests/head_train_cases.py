"""The case table of tests/test_head_train_config_gpu.py (device) and tests/test_head_train_cases.py (CPU): plain data and
helpers, no GPU.  A case is (stage, settings, n, seed, variant) with the figures its seed gave on the oracles.

Seeds.  As in test_head_train_gpu.py a comparison against float64 needs inputs whose ReLU gates do not sit within rounding
of zero: `O.gate_margin` >= 1 on the two oracles, asserted before the device is looked at.  `search` walks seeds 0..249
with `O.default_params(seed)`, `O.features(seed + 100, n)` and labels from `seed + 200` (second vector `seed + 201`,
held-out rows of an eval case `seed + 700`), keeps the seed with the largest margin among those that meet every
precondition of the case (`figures(case)["ok"]`) and counts how many of the 250 did.  RECORDED holds (seed, margin,
qualified) per case, written by `python tests/head_train_cases.py` and pasted; test_head_train_cases.py reproduces every
entry.  The float32 oracle's last bits depend on how the BLAS splits its sums (a margin moves by 20 % between one and
eight threads), so `figures` runs both oracles on one thread; what is asserted everywhere is the recorded seed's
margin >= 1 on the machine at hand.  Another machine's BLAS moves a margin too (1.27 on the authoring host was 1.36
on the MI355X host, 4.69 was 5.29, 23.24 was 35.66, and 100.3 was 64.4 in a stage case), so the CPU test holds a
recorded margin to a factor of 3, no closer.  The narrowest case is one accumulate at n = 256: 8 seeds of 250 qualify,
the best at 1.27 / 1.36.

Four cases had their inputs changed for want of (robustly) qualifying seeds: eval at n >= 129 (see ROWS_EVAL_CASES).

Preconditions beside the margin:
  * focal_gamma < 1: every |logit| of both oracles < 15 (beyond, the reference formula's own autograd is inf * 0);
  * the degenerate batch: the float64 oracle gives z1 = be1 and z2 = be2 to 1e-10 (variance 0 up to the ulp by which
    torch's two rows differ, times 1 / sqrt(eps)) and both give rv = (1 - m) rv0; the device's are compared exactly;
  * apply cases: the forced norm's side of clip_norm is the one the case names, at every step.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

import head_train_oracle as O

F32 = np.float32


def f32(v) -> float:
    return float(F32(v))


# dfd_head_config_default, as the library holds it; the device test asserts that head_config() gives exactly these
DEFAULTS = {"dropout": f32(0.5), "beta1": f32(0.9), "beta2": f32(0.999), "eps": f32(1e-8), "weight_decay": f32(0.05),
            "focal_gamma": 2.0, "focal_alpha": 0.25, "label_smoothing": f32(0.1), "clip_norm": 1.0, "ema_decay": f32(0.999),
            "bn_momentum": f32(0.1)}
BELOW_ONE = float(np.nextafter(F32(1.0), F32(0.0)))          # the largest float below 1


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str                       # "acc" one accumulate | "masks" | "eval" | "apply" | "saturated"
    settings: Tuple[Tuple[str, float], ...] = ()
    n: int = 16
    seed: int = 0
    variant: str = "plain"          # "plain" | "mix" (two label vectors with lam) | "degenerate"
    lam: float = 1.0
    loss_scale: float = 1.0
    max_n: int = 64
    steps: int = 1                  # applies of an "apply" case
    clip_side: str = ""             # "above" (never clips) | "below" (always clips) | "about" (both, step by step) | ""
    held: int = 700                 # an "eval" case: its held-out rows are O.features(seed + held, n) ...
    distinct: int = 0               # ... or, when > 0, that many distinct rows, row r of the n being row 7 r mod distinct
    stage: str = "head"
    group: str = ""
    margin: float = float("nan")    # recorded: the gate margin the seed gave
    qualified: int = -1             # recorded: seeds of 0..249 that met every precondition

    def config(self) -> Dict[str, float]:
        cfg = dict(DEFAULTS)
        cfg.update({k: f32(v) for k, v in self.settings})
        cfg.update(max_n=self.max_n, seed=self.seed)
        return cfg

    def library_kwargs(self) -> Dict[str, float]:
        return dict(self.settings, max_n=self.max_n, seed=self.seed)


def labels(seed: int, n: int) -> np.ndarray:
    return (np.random.RandomState(seed).rand(n) < 0.5).astype(np.float32)


# --------------------------------------------------------------------------- running a case on an oracle
def acc_inputs(case: Case):
    """-> (params, x, labels_a, labels_b or None, lam, loss_scale)"""
    seed, n = case.seed, case.n
    params = O.default_params(seed)
    if case.variant == "degenerate":
        rs = np.random.RandomState(seed + 300)
        params["be1"] = np.where(rs.rand(512) < 0.5, -0.5, 0.5).astype(np.float32)
        params["be2"] = np.where(rs.rand(256) < 0.5, -0.5, 0.5).astype(np.float32)
        x = np.repeat(O.features(seed + 100, 1), n, axis=0)
        ya = (np.arange(n) % 2).astype(np.float32)
    else:
        x, ya = O.features(seed + 100, n), labels(seed + 200, n)
    yb = labels(seed + 201, n) if case.variant == "mix" else None
    return params, x, ya, yb, case.lam, case.loss_scale


def acc_outputs(o, loss, logits) -> Dict[str, np.ndarray]:
    """what one accumulate is compared on: everything the device hands back"""
    out = {"loss": np.array([loss]), "logits": np.asarray(logits), "z1": o.taps["z1"].numpy(), "z2": o.taps["z2"].numpy()}
    out.update({"grad " + k: v for k, v in o.grads().items()})
    e = o.export()
    out.update({k: e[k] for k in O.STAT_FIELDS})
    return out


def run_acc(make: Callable, case: Case):
    """`make(params, cfg)` -> an oracle; -> (oracle, outputs)"""
    params, x, ya, yb, lam, scale = acc_inputs(case)
    o = make(params, case.config())
    loss, z = o.accumulate(x, ya, yb, lam, scale)
    return o, acc_outputs(o, loss, z)


def forced_grads(seed: int) -> Dict[str, np.ndarray]:
    """test_head_train_gpu._forced_grads: magnitudes log-uniform in [1e-4, 1], random signs"""
    import rtdfd_amd

    rs, out = np.random.RandomState(seed), {}
    for k in O.GRAD_FIELDS:
        shape = rtdfd_amd._lib.HEAD_SHAPES[k]
        out[k] = (10.0 ** rs.uniform(-4.0, 0.0, shape) * np.where(rs.rand(*shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    return out


APPLY_PARAM_SEED, APPLY_GRAD_SEED = 3, 50                       # as test_apply_matches_adamw_and_ema


def apply_lrs(case: Case):
    if case.name == "apply-lr-0":
        return [0.0] * case.steps
    if case.name.startswith("existing"):
        return [f32(v) for v in (3e-4, 1.2e-5, 1e-3)]
    return [f32(3e-4 * (k + 1)) for k in range(case.steps)]    # every step another rate: a late step counter cannot hide


def run_apply(make: Callable, case: Case):
    """forced gradients, `case.steps` applies -> (oracle, [outputs after step k], [float norms])"""
    o = make(O.default_params(APPLY_PARAM_SEED), case.config())
    per_step, norms = [], []
    for step, lr in enumerate(apply_lrs(case)):
        o.set_grads(forced_grads(APPLY_GRAD_SEED + step))
        norm = o.apply(lr)
        norms.append(norm)
        out = {"grad norm": np.array([norm])}
        for ema in (False, True):
            e = o.export(ema)
            out.update({("ema " if ema else "param ") + k: e[k] for k in O.GRAD_FIELDS})
        per_step.append(out)
    return o, per_step, norms


EVAL_LR = f32(1e-3)


def eval_inputs(case: Case):
    """-> (params, accumulate rows, labels, forced gradients, held-out rows)"""
    seed, n = case.seed, case.n
    if case.distinct:
        held = O.features(seed + case.held, case.distinct)[(7 * np.arange(n)) % case.distinct]
    else:
        held = O.features(seed + case.held, n)
    return O.default_params(seed), O.features(seed + 100, n), labels(seed + 200, n), forced_grads(seed + 800), held


def run_eval(make: Callable, case: Case):
    """one accumulate (running statistics move), one forced apply (live and EMA parameters part), eval of held-out rows
    on both -> (oracle, outputs, {"live": taps, "ema": taps})"""
    params, x, y, g, held = eval_inputs(case)
    o = make(params, case.config())
    o.accumulate(x, y)
    o.set_grads(g)
    o.apply(EVAL_LR)
    out, taps = {}, {}
    for ema in (False, True):
        tag = "ema" if ema else "live"
        out["eval logits, " + tag] = o.evaluate(held, ema)
        taps[tag] = dict(o.taps)
    return o, out, taps


def gate_margin(t64: Dict[str, torch.Tensor], t32: Dict[str, torch.Tensor]) -> float:
    """O.gate_margin on two tap dicts; inf where the two agree exactly (O.gate_margin would divide by zero)"""
    out = float("inf")
    for k in ("z1", "z2"):
        z64, z32 = t64[k].double(), t32[k].double()
        if bool(((z64 > 0) != (z32 > 0)).any()):
            return 0.0
        d = float((z32 - z64).abs().max())
        if d > 0:
            out = min(out, float(z64.abs().min()) / (8.0 * d))
        elif float(z64.abs().min()) == 0.0:
            return 0.0
    return out


def worst(got: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], yard: Dict[str, np.ndarray], show: Optional[Callable] = None):
    """-> (largest `O.bar_ratio` over every compared tensor, its name); `show(name, figures)` sees each one first"""
    assert set(got) == set(ref) == set(yard), (sorted(got), sorted(ref))
    top, name = 0.0, ""
    for k in ref:
        r = O.bar_ratio(got[k], ref[k], yard[k])
        if show is not None:
            show(k, r)
        if not r["ratio"] <= top:
            top, name = r["ratio"], k
    return top, name


def figures(case: Case) -> Dict[str, object]:
    """The case on both oracles -> its preconditions' figures, "ok", and the outputs of both ("ref", "yard").  The oracles
    run on one thread: the float32 one's last bits, and with them the margin, follow how the BLAS splits its sums."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _figures(case)
    finally:
        torch.set_num_threads(threads)


def _figures(case: Case) -> Dict[str, object]:
    if case.kind == "acc":
        o64, ref = run_acc(lambda p, c: O.Oracle(p, c, torch.float64), case)
        o32, yard = run_acc(lambda p, c: O.Oracle(p, c, torch.float32), case)
        fig = {"margin": gate_margin(o64.taps, o32.taps), "ref": ref, "yard": yard, "o64": o64, "o32": o32}
        fig["ok"] = fig["margin"] >= 1.0
        if dict(case.settings).get("focal_gamma", 2.0) < 1.0:
            fig["max_logit"] = max(float(np.abs(ref["logits"]).max()), float(np.abs(yard["logits"]).max()))
            fig["ok"] = fig["ok"] and fig["max_logit"] < 15.0
        if case.variant == "degenerate":
            params = acc_inputs(case)[0]
            m = case.config()["bn_momentum"]
            # torch's rows come out of its GEMM an ulp apart, and 1 / sqrt(eps) = 316 multiplies that: the float64
            # oracle must sit within 1e-10 of the exact statement (the float32 one is the yardstick, whatever it gives)
            exact = all(float(np.abs(ref[z] - params[be]).max()) < 1e-10 for z, be in (("z1", "be1"), ("z2", "be2"))) and all(
                float(np.abs(out[rv].astype(np.float64) / (1.0 - m) - 1.0).max()) < 1e-6 for out in (ref, yard) for rv in ("rv1", "rv2"))
            fig["degenerate_exact"] = exact
            fig["ok"] = fig["ok"] and exact
        return fig
    if case.kind == "eval":
        o64, ref, t64 = run_eval(lambda p, c: O.Oracle(p, c, torch.float64), case)
        o32, yard, t32 = run_eval(lambda p, c: O.Oracle(p, c, torch.float32), case)
        margin = min(gate_margin(t64[k], t32[k]) for k in ("live", "ema"))
        return {"margin": margin, "ok": margin >= 1.0, "ref": ref, "yard": yard, "o64": o64, "o32": o32}
    if case.kind == "apply":
        o64, ref, n64 = run_apply(lambda p, c: O.Oracle(p, c, torch.float64), case)
        o32, yard, n32 = run_apply(lambda p, c: O.Oracle(p, c, torch.float32), case)
        clip = case.config()["clip_norm"]
        sides = ["above" if v < clip else "below" for v in n64]          # clip_norm above / below the norm of the step
        ok = {"above": all(s == "above" for s in sides), "below": all(s == "below" for s in sides),
              "about": len(set(sides)) == 2 and all(abs(v / clip - 1.0) < 0.02 for v in n64), "": True}[case.clip_side]
        return {"margin": float("nan"), "ok": ok, "norms": n64, "ref": ref, "yard": yard, "o64": o64, "o32": o32}
    raise ValueError(case.kind)


def search(case: Case, seeds=range(250)):
    """-> (best seed, its margin, number of qualifying seeds)"""
    best, count = None, 0
    for s in seeds:
        fig = figures(dataclasses.replace(case, seed=s))
        if fig["ok"]:
            count += 1
            if best is None or fig["margin"] > best[1]:
                best = (s, fig["margin"])
    if best is None:
        raise RuntimeError(f"{case.name}: no seed of {seeds} meets the preconditions")
    return best[0], best[1], count


# --------------------------------------------------------------------------- saturated loss: the reference restated
def focal_restated(z, y, gamma: float, alpha: float, ls: float, dtype=np.float64):
    """FocalLoss (head_train_oracle.focal) per logit and its d/dz, in numpy of `dtype`, without a cancelling
    subtraction anywhere: softplus as max(z, 0) + log1p(exp(-|z|)), p and q = 1 - p each from exp(-|z|) on its own
    side (both tails explicit), 1 - p_t = p (1 - t) + q t, and p - t taken as (1 - t) - q where p is the one near 1.
    -> (loss terms, d loss terms / dz)"""
    z, y = np.asarray(z, dtype), np.asarray(y, dtype)
    one, gamma, alpha, ls = dtype(1.0), dtype(gamma), dtype(alpha), dtype(ls)
    t = y * (one - ls) + dtype(0.5) * ls if ls > 0 else y
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(z))
        pos = z >= 0
        big, small = one / (one + e), e / (one + e)
        p, q = np.where(pos, big, small), np.where(pos, small, big)
        bce = np.maximum(z, dtype(0.0)) - z * t + np.log1p(e)
        u = p * (one - t) + q * t
        at = alpha * t + (one - alpha) * (one - t)
        pmt = np.where(pos, (one - t) - q, p - t)
        if gamma == 0:
            w, dw = np.ones_like(u), np.zeros_like(u)
        else:
            w = u ** gamma
            dw = np.where(u > 0, gamma * u ** (gamma - one) * (p * q * (one - dtype(2.0) * t)), dtype(0.0))
        return (at * w * bce).astype(dtype), (at * (dw * bce + w * pmt)).astype(dtype)


def saturated_reference(logits, a2, ya, cfg, dtype=np.float64) -> Dict[str, np.ndarray]:
    """loss, grad b3 = sum dlogit and grad w3 = dlogit . a2 of one accumulate (one label vector, loss_scale 1),
    teacher-forced from the given logits [n] and fc3 inputs a2 [n][256]"""
    z, a2 = np.asarray(logits, dtype), np.asarray(a2, dtype)
    n = z.shape[0]
    terms, dz = focal_restated(z, ya, cfg["focal_gamma"], cfg["focal_alpha"], cfg["label_smoothing"], dtype)
    dlogit = dz / dtype(n)
    return {"loss": np.array([terms.sum(dtype=dtype) / dtype(n)]), "grad b3": np.array([dlogit.sum(dtype=dtype)]),
            "grad w3": (dlogit[None, :] @ a2).astype(dtype)}


SATURATED_B3 = (20.0, -20.0, 40.0, -40.0, 90.0, -90.0)
SATURATED_SEED, SATURATED_N = 5, 16


def saturated_inputs(case: Case, b3: float):
    params = O.default_params(case.seed)
    params["b3"] = np.array([b3], np.float32)
    return params, O.features(case.seed + 100, case.n), labels(case.seed + 200, case.n)


# --------------------------------------------------------------------------- the table
# (seed, gate margin, seeds of 0..249 that qualified), written by `python tests/head_train_cases.py`
RECORDED: Dict[str, Tuple[int, float, int]] = {
    "rows-eval-n129": (206, 23.89, 191),
    "rows-eval-n241": (65, 25.37, 174),
    "rows-eval-n255": (62, 19.23, 190),
    "rows-eval-n256": (29, 20.51, 175),
    "alpha-0.5-n16": (247, 37.02, 219),
    "alpha-0.5-n37": (167, 17.84, 173),
    "alpha-0.75-n16": (247, 37.02, 219),
    "alpha-0.75-n37": (167, 17.84, 173),
    "degenerate-n2": (184, 4128.25, 250),
    "dropout-0-n16": (13, 17.05, 180),
    "dropout-0-n37": (43, 7.03, 115),
    "dropout-0.2-n16": (183, 23.24, 208),
    "dropout-0.2-n37": (141, 17.86, 143),
    "dropout-0.9-n16": (189, 110.03, 232),
    "dropout-0.9-n37": (5, 27.52, 224),
    "gamma-0.5-n16": (247, 37.02, 219),
    "gamma-0.5-n37": (167, 17.84, 173),
    "gamma-1-n16": (247, 37.02, 219),
    "gamma-1-n37": (167, 17.84, 173),
    "gamma-2.5-n16": (247, 37.02, 219),
    "gamma-2.5-n37": (167, 17.84, 173),
    "gamma-3-n16": (247, 37.02, 219),
    "gamma-3-n37": (167, 17.84, 173),
    "loss-scale-1/64-n16": (247, 37.02, 219),
    "loss-scale-1/64-n37": (167, 17.84, 173),
    "mix-lam-0-n16": (247, 37.02, 219),
    "mix-lam-0-n37": (167, 17.84, 173),
    "mix-lam-1-n16": (247, 37.02, 219),
    "mix-lam-1-n37": (167, 17.84, 173),
    "momentum-0-n16": (247, 37.02, 219),
    "momentum-0-n37": (167, 17.84, 173),
    "momentum-0.01-n16": (247, 37.02, 219),
    "momentum-0.01-n37": (167, 17.84, 173),
    "momentum-1-n16": (247, 37.02, 219),
    "momentum-1-n37": (167, 17.84, 173),
    "rows-acc-n129": (57, 4.69, 76),
    "rows-acc-n15": (144, 79.96, 231),
    "rows-acc-n17": (75, 37.91, 209),
    "rows-acc-n241": (30, 2.28, 12),
    "rows-acc-n255": (69, 2.57, 18),
    "rows-acc-n256": (183, 1.27, 8),
    "rows-acc-n63": (38, 8.11, 140),
    "rows-acc-n65": (166, 12.47, 133),
    "rows-acc-n80": (125, 8.96, 105),
    "rows-eval-n15": (33, 52.98, 216),
    "rows-eval-n17": (80, 16.91, 182),
    "rows-eval-n63": (223, 6.80, 63),
    "rows-eval-n65": (236, 5.01, 49),
    "rows-eval-n80": (145, 5.01, 37),
    "smoothing-0.3-n16": (247, 37.02, 219),
    "smoothing-0.3-n37": (167, 17.84, 173),
    "smoothing-1-n16": (247, 37.02, 219),
    "smoothing-1-n37": (167, 17.84, 173),
}


def _case(name, kind, group, **kw) -> Case:
    seed, margin, qualified = RECORDED.get(name, (kw.pop("seed", 0), float("nan"), -1))
    kw.pop("seed", None)
    settings = tuple(sorted(kw.pop("settings", {}).items()))
    return Case(name=name, kind=kind, group=group, settings=settings, seed=seed, margin=margin, qualified=qualified, **kw)


def _settings_rows():
    rows = [("dropout-0", {"dropout": 0.0}, {}), ("dropout-0.2", {"dropout": 0.2}, {}), ("dropout-0.9", {"dropout": 0.9}, {}),
            ("gamma-0.5", {"focal_gamma": 0.5}, {}), ("gamma-1", {"focal_gamma": 1.0}, {}), ("gamma-3", {"focal_gamma": 3.0}, {}),
            ("gamma-2.5", {"focal_gamma": 2.5}, {}), ("alpha-0.75", {"focal_alpha": 0.75}, {}), ("alpha-0.5", {"focal_alpha": 0.5}, {}),
            ("smoothing-0.3", {"label_smoothing": 0.3}, {}), ("smoothing-1", {"label_smoothing": 1.0}, {}),
            ("mix-lam-0", {}, {"variant": "mix", "lam": 0.0}), ("mix-lam-1", {}, {"variant": "mix", "lam": 1.0}),
            ("loss-scale-1/64", {}, {"loss_scale": 1.0 / 64.0}),
            ("momentum-0", {"bn_momentum": 0.0}, {}), ("momentum-0.01", {"bn_momentum": 0.01}, {}), ("momentum-1", {"bn_momentum": 1.0}, {})]
    out = []
    for n in (16, 37):
        for name, settings, kw in rows:
            out.append(_case(f"{name}-n{n}", "acc", "settings", settings=settings, n=n, **kw))
    return out


ROWS_NS = (15, 17, 63, 65, 80, 129, 241, 255, 256)
SETTINGS_CASES = _settings_rows()
DEGENERATE_CASE = _case("degenerate-n2", "acc", "settings", settings={"dropout": 0.0}, n=2, variant="degenerate")
MASK_CASES = [_case(f"dropout-below-1-n{n}", "masks", "masks", settings={"dropout": BELOW_ONE}, n=n, seed=40 + n) for n in (16, 37)]
ROWS_ACC_CASES = [_case(f"rows-acc-n{n}", "acc", "rows", n=n, max_n=256) for n in ROWS_NS]
# An eval case asks for the margin in two forwards of n x 768 gates each.  With n independent rows that leaves 10, 3, 0 and
# 1 of the 250 seeds at n = 129, 241, 255 and 256, none with a margin above 1.5 - and the float32 oracle's last bits, so
# the margin, move by that much from one BLAS to the next.  Their inputs are changed, not the condition: from n = 129 up
# the held-out rows are 17 distinct ones, row r of the batch being row 7 r mod 17 of them.  Eval is per row, so every
# 16-row tile, row mask and tile cut-off still runs on rows that differ from those 16, 64 (and any d with 17 not
# dividing d) places away; the gates are those of 17 rows.
ROWS_EVAL_CASES = [_case(f"rows-eval-n{n}", "eval", "rows", n=n, max_n=256, distinct=17 if n >= 129 else 0) for n in ROWS_NS]

# the forced norms of the twelve steps (790 k values of one law each) lie between 206.456 and 207.358, six on either side of
FORCED_NORM_MID = 206.95


def _apply_rows():
    rows = [("apply-decay-0", {"weight_decay": 0.0}, ""), ("apply-decay-0.5", {"weight_decay": 0.5}, ""),
            ("apply-betas-0-0.999", {"beta1": 0.0}, ""), ("apply-betas-0.9-0", {"beta2": 0.0}, ""),
            ("apply-betas-0.5-0.9", {"beta1": 0.5, "beta2": 0.9}, ""), ("apply-eps-1e-3", {"eps": 1e-3}, ""),
            ("apply-ema-0", {"ema_decay": 0.0}, ""), ("apply-ema-1", {"ema_decay": 1.0}, ""), ("apply-lr-0", {}, ""),
            ("apply-clip-below", {"clip_norm": 150.0}, "below"), ("apply-clip-about", {"clip_norm": FORCED_NORM_MID}, "about"),
            ("apply-clip-above", {"clip_norm": 400.0}, "above")]
    out = []
    for name, settings, side in rows:
        settings = dict(settings)
        settings.setdefault("clip_norm", 1.0e4)                 # the norm is ~2e2: no clipping unless the case is about it
        out.append(_case(name, "apply", "apply", settings=settings, n=0, seed=APPLY_PARAM_SEED, max_n=16, steps=12,
                         clip_side=side or "above"))
    return out


APPLY_CASES = _apply_rows()
SATURATED_CASES = [_case("saturated-defaults", "saturated", "saturated", n=SATURATED_N, seed=SATURATED_SEED),
                   _case("saturated-gamma-0", "saturated", "saturated", settings={"focal_gamma": 0.0}, n=SATURATED_N, seed=SATURATED_SEED)]

SEARCHED = SETTINGS_CASES + [DEGENERATE_CASE] + ROWS_ACC_CASES + ROWS_EVAL_CASES
ALL_CASES = SEARCHED + MASK_CASES + APPLY_CASES + SATURATED_CASES

# what tests/test_head_train_gpu.py runs, restated as cases: for the record of which defects it could see
_EXISTING_GATE_SEED = {2: 0, 5: 8, 16: 11, 37: 10, 64: 2}
EXISTING_ACC = [Case(name=f"existing-{v}-n{n}", kind="acc", n=n, seed=s, variant="mix" if v == "mix" else "plain",
                     lam=0.7 if v == "mix" else 1.0,
                     settings=(("focal_gamma", 0.0), ("label_smoothing", 0.0)) if v == "bce" else ())
                for n, s in _EXISTING_GATE_SEED.items() for v in ("plain", "mix", "bce")]
EXISTING_APPLY = [Case(name=f"existing-apply-{c:g}", kind="apply", settings=(("clip_norm", c),), n=0, seed=APPLY_PARAM_SEED, max_n=16,
                       steps=3, clip_side="above" if c > 1.0 else "below") for c in (1.0e4, 1.0)]


# --------------------------------------------------------------------------- conv and block stages
# One accumulate at n = 5 on the stages' real rows and three forced applies, under the settings that reach those stages:
# the head's dropout (through ht_dfeat_kernel), lr_scale, and the stages' own bn_momentum / bn_eps.  Preconditions as in
# test_headconv_train_gpu.py / test_block15_train_gpu.py: gate margin >= 1, rounding share <= 1, and for the block stage
# storage share <= 0.5.  The shares move by a factor of 2 and more when the rows change in their last bits (0.22 against
# 0.58 for one seed between two CPU forwards of the same crops), so the seeds were searched on the rows one MI355X
# extracted, kept as a fixture (`golden_rows`); the device test asserts the conditions on the rows it extracts itself.
STAGE_N = 5
NEAR_1E_3 = float(np.nextafter(F32(1e-3), F32(1.0)))           # the float neighbour of the backbone's eps
STAGE_SETTINGS = (("dropout-0.2", {"dropout": 0.2}, {}), ("lr-scale-0", {}, {"lr_scale": 0.0}), ("lr-scale-0.5", {}, {"lr_scale": 0.5}),
                  ("lr-scale-1", {}, {"lr_scale": 1.0}), ("momentum-0.1", {}, {"bn_momentum": 0.1}),
                  ("eps-1e-5", {}, {"bn_eps": 1e-5}), ("eps-near-1e-3", {}, {"bn_eps": NEAR_1E_3}))
STAGE_APPLY_LRS = (3e-4, 1.2e-5, 1e-3)


@dataclasses.dataclass(frozen=True)
class StageCase:
    name: str
    stage: str                      # "conv" | "block"
    settings: Tuple[Tuple[str, float], ...] = ()               # dfd_head_config fields
    stage_kw: Tuple[Tuple[str, float], ...] = ()               # lr_scale, bn_momentum, bn_eps of the unfreeze calls
    n: int = STAGE_N
    seed: int = 0
    margin: float = float("nan")    # recorded, on `golden_rows`: gate margin, rounding share, storage share (block stage)
    rounding: float = float("nan")
    storage: float = float("nan")
    qualified: int = -1
    group: str = "stages"

    def config(self) -> Dict[str, float]:
        cfg = dict(DEFAULTS)
        cfg.update({k: f32(v) for k, v in self.settings})
        cfg.update(max_n=64, seed=self.seed, clip_norm=1.0e4)   # the forced norm is ~3e2: the applies do not clip
        return cfg

    def library_kwargs(self) -> Dict[str, float]:
        return dict(self.settings, max_n=64, seed=self.seed, clip_norm=1.0e4)

    def oracle_kwargs(self) -> Dict[str, float]:
        """what the oracles take: the floats the library holds (its eps is the double of the float it is given, and
        1e-3 itself where that float is (float) 1e-3)"""
        kw = {k: f32(v) for k, v in self.stage_kw}
        if "bn_eps" in kw and F32(kw["bn_eps"]) == F32(1e-3):
            kw["bn_eps"] = 1e-3
        return kw


_GOLDEN_ROWS: Dict[str, np.ndarray] = {}


def golden_rows(stage: str) -> np.ndarray:
    """tests/golden/head_train_stage_rows.npz: the first STAGE_N rows of the stage tests' real-row fixtures as one MI355X
    extracted them - `extract_trunk` ("conv": block 15's output) and `extract_trunk(block=14)` ("block") of
    b0_layer_oracle.stress_state_dict(0) weights on random_crops(37, 42)[:16], NHWC float32"""
    import os

    if not _GOLDEN_ROWS:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_train_stage_rows.npz")) as f:
            _GOLDEN_ROWS.update(conv=f["trunk"].copy(), block=f["rows"].copy())
    return _GOLDEN_ROWS[stage]


def stage_forced_grads(case: StageCase, seed: int) -> Dict[str, np.ndarray]:
    """test_headconv_train_gpu / test_block15_train_gpu._forced_grads"""
    import rtdfd_amd
    import block15_train_oracle as BO
    import headconv_train_oracle as CO

    lib, rs = rtdfd_amd._lib, np.random.RandomState(seed)
    shapes = {k: lib.HEAD_SHAPES[k] for k in O.GRAD_FIELDS}
    shapes.update({"conv." + k: lib.CONV_SHAPES[k] for k in CO.CONV_GRAD_FIELDS})
    if case.stage == "block":
        shapes.update({"b15." + k: lib.BLOCK_SHAPES[k] for k in BO.BLOCK_GRAD_FIELDS})
    return {k: (10.0 ** rs.uniform(-4.0, 0.0, sh) * np.where(rs.rand(*sh) < 0.5, -1.0, 1.0)).astype(np.float32) for k, sh in shapes.items()}


def stage_taps(case: StageCase) -> Tuple[str, ...]:
    import block15_train_oracle as BO

    return ("cfeat", "cz", "dfeat") if case.stage == "conv" else BO.TAPS + ("cfeat", "dfeat")


def stage_figures(case: StageCase, rows: np.ndarray, conv0, block0=None, applies: bool = True) -> Dict[str, object]:
    """The case on the oracles, from the given rows -> preconditions' figures, "ok", and "ref" / "yard": the outputs of the
    accumulate ("acc") and of the three forced applies after it ("apply")"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _stage_figures(case, rows, conv0, block0, applies)
    finally:
        torch.set_num_threads(threads)


def _stage_figures(case, rows, conv0, block0, applies):
    import block15_train_oracle as BO
    import headconv_train_oracle as CO

    head, ya, cfg, kw = O.default_params(case.seed), labels(case.seed + 200, case.n), case.config(), case.oracle_kwargs()
    x = rows[:case.n]
    if case.stage == "conv":
        oracles = CO.pair(conv0, head, cfg, **kw)
    else:
        oracles = BO.triple(block0, conv0, head, cfg, **kw)
    outs = [o.accumulate(x, ya) for o in oracles]
    o64, o32 = oracles[:2]
    fig = {"margin": gate_margin(o64.head.taps, o32.head.taps), "rounding": CO.rounding_share(o64 if case.stage == "conv" else o64.co, ya)}
    fig["ok"] = fig["margin"] >= 1.0 and fig["rounding"] <= 1.0
    if case.stage == "block":
        fig["storage"] = BO.storage_share(o64, o32, oracles[2], tuple(l for l, _ in outs))["max"]
        fig["ok"] = fig["ok"] and fig["storage"] <= 0.5
    for tag, o, (loss, z) in (("ref", o64, outs[0]), ("yard", o32, outs[1])):
        acc = {"loss": np.array([loss]), "logits": z}
        acc.update({k: o.taps[k].numpy() for k in stage_taps(case)})
        acc.update({"grad " + k: v for k, v in o.grads().items()})
        e = o.export()
        acc.update({k: v for k, v in e.items() if k.split(".")[-1].startswith(("rm", "rv"))})
        app = {}
        for step, lr in enumerate(STAGE_APPLY_LRS if applies else ()):
            o.set_grads(stage_forced_grads(case, 50 + step))
            app[f"grad norm, step {step}"] = np.array([o.apply(f32(lr))])
        for ema in (False, True) if applies else ():
            e = o.export(ema)
            app.update({("ema " if ema else "param ") + k: v for k, v in e.items() if not k.split(".")[-1].startswith(("rm", "rv"))})
        fig[tag] = {"acc": acc, "apply": app}
    return fig


def stage_search(case: StageCase, rows, conv0, block0=None, seeds=range(250)):
    """-> (best seed, margin, rounding share, storage share or nan, number of qualifying seeds).  The shares move when
    the rows change in their last bits (the device's against the CPU's), so of the qualifying seeds only those with half
    the allowance to spare (rounding share <= 0.5, storage share <= 0.25) compete for the largest margin."""
    best, count = None, 0
    for s in seeds:
        fig = stage_figures(dataclasses.replace(case, seed=s), rows, conv0, block0, applies=False)
        if fig["ok"]:
            count += 1
            spare = fig["rounding"] <= 0.5 and fig.get("storage", 0.0) <= 0.25
            if spare and (best is None or fig["margin"] > best[1]):
                best = (s, fig["margin"], fig["rounding"], fig.get("storage", float("nan")))
    if best is None:
        raise RuntimeError(f"{case.name}: no seed of {seeds} meets the preconditions with room to spare")
    return best + (count,)


# (seed, gate margin, rounding share, storage share, seeds of 0..249 that qualified), on `golden_rows`
# The storage share is a ratio against the float32 yardstick's own error, which for single numbers such as the loss is
# luck: seed 168 of block-eps-1e-5 has the largest margin (62.7) and a storage share of 0.077 on the authoring host, but
# 0.451 with the BLAS of the MI355X host.  Of seeds 0..63 with room to spare on both hosts, 56 has the largest margin
# (38.7 / 36.2, storage 0.134 / 0.045) and stands in the table; every other entry is `stage_search`'s.
STAGE_RECORDED: Dict[str, Tuple[int, float, float, float, int]] = {
    "block-dropout-0.2": (38, 33.96, 0.358, 0.141, 138),
    "block-eps-1e-5": (56, 38.72, 0.243, 0.134, 215),        # not 168, see above
    "block-eps-near-1e-3": (0, 109.64, 0.323, 0.053, 204),
    "block-lr-scale-0": (0, 91.88, 0.403, 0.122, 207),
    "block-lr-scale-0.5": (0, 91.88, 0.403, 0.122, 207),
    "block-lr-scale-1": (0, 91.88, 0.403, 0.122, 207),
    "block-momentum-0.1": (0, 91.88, 0.403, 0.122, 207),
    "conv-dropout-0.2": (219, 33.74, 0.458, float("nan"), 157),
    "conv-eps-1e-5": (202, 91.78, 0.244, float("nan"), 216),
    "conv-eps-near-1e-3": (96, 96.93, 0.445, float("nan"), 212),
    "conv-lr-scale-0": (96, 100.27, 0.467, float("nan"), 210),
    "conv-lr-scale-0.5": (96, 100.27, 0.467, float("nan"), 210),
    "conv-lr-scale-1": (96, 100.27, 0.467, float("nan"), 210),
    "conv-momentum-0.1": (96, 100.27, 0.467, float("nan"), 210),
}


def _stage_cases():
    out = []
    for stage in ("conv", "block"):
        for name, settings, kw in STAGE_SETTINGS:
            full = f"{stage}-{name}"
            seed, margin, rounding, storage, qualified = STAGE_RECORDED.get(full, (0, float("nan"), float("nan"), float("nan"), -1))
            out.append(StageCase(name=full, stage=stage, settings=tuple(sorted(settings.items())), stage_kw=tuple(sorted(kw.items())),
                                 seed=seed, margin=margin, rounding=rounding, storage=storage, qualified=qualified))
    return out


STAGE_CASES = _stage_cases()


if __name__ == "__main__":                                      # writes the table: python tests/head_train_cases.py [name ...]
    import sys

    wanted = sys.argv[1:]
    for case in SEARCHED:
        if wanted and case.name not in wanted:
            continue
        seed, margin, count = search(case)
        print(f'    "{case.name}": ({seed}, {margin:.2f}, {count}),', flush=True)

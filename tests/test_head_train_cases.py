"""CPU: keeps the case table of tests/head_train_cases.py honest.

1. Every case's preconditions hold on the oracles at its recorded seed, and the recorded margin reproduces to a factor
   of 3 (the float32 oracle's last bits follow the machine's BLAS, see head_train_cases.py; the assertion that matters,
   margin >= 1, is exact).
2. The float64 restatement of the loss that the saturated cases use as their reference is head_train_oracle.focal and its
   autograd to 1e-12 on logits in [-10, 10]: no second opinion about the formula.
3. Each named defect, carried by `DefectOracle` (float64, a flag on the test side), fails `O.bar_ratio` in the case meant
   for it, and the test records whether any case of test_head_train_gpu.py (restated as H.EXISTING_ACC / _APPLY) would
   have failed too.  A `DefectOracle` without a flag passes every bar by a wide margin (it is the same arithmetic).

Measured here (ratio = largest `O.bar_ratio` over every compared tensor; > 1 fails):

  defect               caught by              ratio     existing suite: its worst case   ratio
  rates_same           dropout-0.2-n16        4.2e+05   plain, n = 16                    1.8e+06
  no_backward_scale    dropout-0.9-n16        8.1e+05   bce, n = 16                      5.9e+05
  focal_no_dw          gamma-3-n16            1.7e+06   mix, n = 37                      3.1e+06
  alpha_both           alpha-0.75-n16         3.3e+06   bce, n = 64                      8.2e+06
  ls_bce_only          smoothing-0.3-n16      3.4e+05   plain, n = 64                    1.8e+05
  lam_loss_only        mix-lam-1-n16          1.9e+06   mix, n = 37                      4.8e+06
  biased_var           momentum-1-n16         8.0e+04   plain, n = 2                     1.9e+05
  momentum_reversed    momentum-0.01-n16      2.0e+08   plain, n = 64                    2.2e+07
  l2_decay             apply-decay-0.5        2.8e+05   apply, clip 1                    8.2e+05
  bias_late            apply-betas-0.5-0.9    1.7e+05   apply, clip 1e4                  3.1e+05
  eps_in_sqrt          apply-eps-1e-3         1.3e+06   apply, clip 1                    8.8e+05
  ema_before           apply-ema-0            2.7e+06   apply, clip 1e4                  1.5e+06
  stats_lost_tile      rows-acc-n65           1.2e+05   none fails                       2.1e-09
  dyw_lost_tile        rows-acc-n65           6.6e+04   none fails                       2.1e-09

So the formula defects were within the old suite's reach at its one setting each; what it could not see at all is
anything that goes wrong from row 64 on: a lost tile of the column statistics or of the dY . W product changes no
figure of any of its cases.  The new cases still matter for the first twelve: each is now caught at a second setting
where the defect has another size (a missing 1 / (1 - p) is a factor 2 at p = 0.5 and a factor 10 at 0.9; `alpha_both`
vanishes at alpha = 0.5 and `lam_loss_only` at lam = 0, which is why those rows are in the table beside 0.75 and 1).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_train_cases as H
import head_train_oracle as O

DEFECTS = {
    # name: (the case meant for it, what goes wrong)
    "rates_same": ("dropout-0.2-n16", "layers 1 and 2 dropped at layer 0's rate"),
    "no_backward_scale": ("dropout-0.9-n16", "1 / (1 - p) missing from the backward"),
    "focal_no_dw": ("gamma-3-n16", "the d(u^gamma) / dz term of the focal gradient dropped"),
    "alpha_both": ("alpha-0.75-n16", "alpha_t taken as alpha for both classes"),
    "ls_bce_only": ("smoothing-0.3-n16", "label smoothing applied to the BCE target but not to p_t"),
    "lam_loss_only": ("mix-lam-1-n16", "lam applied to the loss but not to the gradient of the second label vector"),
    "biased_var": ("momentum-1-n16", "biased running variance"),
    "momentum_reversed": ("momentum-0.01-n16", "momentum convention reversed"),
    "l2_decay": ("apply-decay-0.5", "weight decay coupled into the gradient (L2) instead of decoupled"),
    "bias_late": ("apply-betas-0.5-0.9", "bias corrections one step late (step t uses t - 1, the first step its own)"),
    "eps_in_sqrt": ("apply-eps-1e-3", "Adam's eps inside the square root"),
    "ema_before": ("apply-ema-0", "EMA taken from the parameter before the step"),
    "stats_lost_tile": ("rows-acc-n65", "rows 64 and up left out of the column statistics"),
    "dyw_lost_tile": ("rows-acc-n65", "rows 64 and up left out of the dY . W product"),
}
INVISIBLE_BEFORE = {"stats_lost_tile", "dyw_lost_tile"}
CASES = {c.name: c for c in H.ALL_CASES}


class DefectOracle(O.Oracle):
    """head_train_oracle.Oracle with its forward, loss and optimizer step written out, so that one of DEFECTS can be
    switched in.  Float64 only; without a flag it is the same arithmetic (test_carrier_without_a_defect_is_the_oracle)."""

    def __init__(self, params, cfg, defect=None):
        super().__init__(params, cfg, torch.float64)
        self.defect = defect
        if defect == "rates_same":
            self.rates = (self.rates[0],) * 3
        self.state = {k: [torch.zeros_like(self.tensors[k]), torch.zeros_like(self.tensors[k])] for k in O.GRAD_FIELDS}
        self.t = 0

    def _drop(self, x, mult, layer):
        if self.defect == "no_backward_scale":
            keep = (mult != 0).to(x.dtype)
            return x * keep + (x * (mult - keep)).detach()
        return x * mult

    def _bn(self, y, bn, train):
        if train:
            ys = y[:64] if self.defect == "stats_lost_tile" else y
            n = ys.shape[0]
            mu, var = ys.mean(0), ys.var(0, unbiased=False)
            m = self.cfg["bn_momentum"]
            if self.defect == "momentum_reversed":
                m = 1.0 - m
            with torch.no_grad():
                run_var = var if self.defect == "biased_var" else var * (n / (n - 1))
                bn.running_mean.mul_(1.0 - m).add_(mu * m)
                bn.running_var.mul_(1.0 - m).add_(run_var * m)
        else:
            mu, var = bn.running_mean, bn.running_var
        return (y - mu) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias

    def _forward(self, x, masks):
        train = masks is not None
        if train:
            x = self._drop(x, masks[0], 0)
        z1 = self._bn(self.fc1(x), self.bn1, train)
        a1 = F.relu(z1)
        if train:
            a1 = self._drop(a1, masks[1], 1)
            if self.defect == "dyw_lost_tile":
                a1 = torch.cat([a1[:64], a1[64:].detach()])
        z2 = self._bn(self.fc2(a1), self.bn2, train)
        a2 = F.relu(z2)
        if train:
            a2 = self._drop(a2, masks[2], 2)
        return self.fc3(a2).squeeze(1), z1, z2

    def _focal(self, logits, targets):
        gamma, alpha, ls = self.loss_settings
        smooth = targets * (1 - ls) + 0.5 * ls if ls > 0 else targets
        bce = F.binary_cross_entropy_with_logits(logits, smooth, reduction="none")
        probs = torch.sigmoid(logits)
        tp = targets if self.defect == "ls_bce_only" else smooth
        p_t = probs * tp + (1 - probs) * (1 - tp)
        alpha_t = torch.full_like(smooth, alpha) if self.defect == "alpha_both" else alpha * smooth + (1 - alpha) * (1 - smooth)
        w = (1 - p_t) ** gamma
        if self.defect == "focal_no_dw":
            w = w.detach()
        return (alpha_t * w * bce).mean()

    def accumulate(self, feat, labels_a, labels_b=None, lam=1.0, loss_scale=1.0):
        x = torch.from_numpy(np.asarray(feat, np.float32)).double()
        ya = torch.from_numpy(np.asarray(labels_a, np.float32)).double()
        z, z1, z2 = self._forward(x, self.masks(x.shape[0]))
        loss = self._focal(z, ya)
        if labels_b is not None:
            second = self._focal(z, torch.from_numpy(np.asarray(labels_b, np.float32)).double())
            if self.defect == "lam_loss_only":
                loss = lam * loss + (1 - lam) * second.detach() + (second - second.detach())
            else:
                loss = lam * loss + (1 - lam) * second
        (loss * loss_scale).backward()
        self.counter += 1
        self.taps = {"z1": z1.detach(), "z2": z2.detach()}
        return float(loss.detach()), z.detach().numpy().copy()

    @torch.no_grad()
    def apply(self, lr):
        c = self.cfg
        norm = torch.sqrt(sum((self.tensors[k].grad ** 2).sum() for k in O.GRAD_FIELDS))
        coef = min(1.0, c["clip_norm"] / (float(norm) + 1e-6))
        self.t += 1
        t = max(self.t - 1, 1) if self.defect == "bias_late" else self.t
        bc1, bc2 = 1.0 - c["beta1"] ** t, 1.0 - c["beta2"] ** t
        for k in O.GRAD_FIELDS:
            p, (m, v) = self.tensors[k], self.state[k]
            g = p.grad * coef
            if self.defect == "l2_decay":
                g = g + c["weight_decay"] * p
            else:
                p.mul_(1.0 - lr * c["weight_decay"])
            m.add_((g - m) * (1.0 - c["beta1"]))
            v.mul_(c["beta2"]).add_(g * g * (1.0 - c["beta2"]))
            denom = torch.sqrt(v / bc2 + c["eps"]) if self.defect == "eps_in_sqrt" else torch.sqrt(v) / bc2 ** 0.5 + c["eps"]
            before = p.clone()
            p.sub_(lr / bc1 * m / denom)
            self.shadow[k].mul_(c["ema_decay"]).add_((before if self.defect == "ema_before" else p) * (1.0 - c["ema_decay"]))
            p.grad.zero_()
        return float(norm)


def _run(case, make):
    """the outputs of one case as one dict (an apply case: every step's)"""
    if case.kind == "acc":
        return H.run_acc(make, case)[1]
    per_step = H.run_apply(make, case)[1]
    last = len(per_step) - 1 if case.name.startswith("existing") else -1      # test_apply_matches_adamw_and_ema: norms, then the end
    return {f"{k}, step {s}": v for s, out in enumerate(per_step) for k, v in out.items() if last < 0 or s == last or k == "grad norm"}


_MEMO = {}


def _oracles(case):
    """(float64 outputs, float32 outputs) of a case, computed once"""
    if case.name not in _MEMO:
        _MEMO[case.name] = (_run(case, lambda p, c: O.Oracle(p, c, torch.float64)), _run(case, lambda p, c: O.Oracle(p, c, torch.float32)))
    return _MEMO[case.name]


def _defect_ratio(case, defect):
    ref, yard = _oracles(case)
    return H.worst(_run(case, lambda p, c: DefectOracle(p, c, defect)), ref, yard)


# --------------------------------------------------------------------------- 1. the table
def test_the_table_names_every_setting_and_size():
    names = [c.name for c in H.ALL_CASES]
    assert len(names) == len(set(names))
    touched = {k for c in H.ALL_CASES for k, _ in c.settings}
    assert touched == set(H.DEFAULTS), set(H.DEFAULTS) - touched          # every float field departs from its default somewhere
    assert {c.n for c in H.ROWS_ACC_CASES} == {c.n for c in H.ROWS_EVAL_CASES} == {15, 17, 63, 65, 80, 129, 241, 255, 256}
    ends = {("dropout", 0.0), ("dropout", H.BELOW_ONE), ("beta1", 0.0), ("beta2", 0.0), ("ema_decay", 0.0), ("ema_decay", 1.0),
            ("bn_momentum", 0.0), ("bn_momentum", 1.0), ("label_smoothing", 1.0), ("weight_decay", 0.0)}
    assert ends <= {s for c in H.ALL_CASES for s in c.settings}
    for c in H.SEARCHED:
        assert c.name in H.RECORDED and c.qualified >= 1 and c.margin >= 1.0, c.name
    assert set(DEFECTS.values()) and all(case in CASES for case, _ in DEFECTS.values())


@pytest.mark.parametrize("case", H.SEARCHED + H.APPLY_CASES, ids=lambda c: c.name)
def test_preconditions_hold_and_figures_reproduce(case):
    fig = H.figures(case)
    print({k: v for k, v in fig.items() if k not in ("ref", "yard", "o64", "o32")}, "recorded margin", case.margin)
    assert fig["ok"]
    if case.kind == "apply":
        assert len(fig["norms"]) == case.steps == 12
        return
    assert fig["margin"] >= 1.0
    if np.isinf(case.margin):
        assert np.isinf(fig["margin"])
    else:
        assert case.margin / 3.0 <= fig["margin"] <= 3.0 * case.margin
    if case.name.startswith("dropout-0-") or case.variant == "degenerate":
        masks = fig["o64"].masks(case.n, 0)
        assert all(bool((m == 1.0).all()) for m in masks)                    # every mask all ones, the scale exactly 1


def test_mask_cases_keep_almost_nothing_in_layer_0():
    """the largest float below 1: thr = 2^32 - 256, scale 2^24; layers 1 and 2 at 0.7 and 0.5 of it"""
    from rtdfd_amd import head_training as T

    for case in H.MASK_CASES:
        p0, p1, p2 = T.dropout_rates(case.config()["dropout"])
        assert int(p0 * 4294967296.0) == 2 ** 32 - 256 and 1.0 / (1.0 - p0) == 2.0 ** 24
        keep = T.dropout_keep_mask(case.seed, 0, 0, case.n, 1280, p0)
        assert keep.sum() <= 3
        assert 0.25 < T.dropout_keep_mask(case.seed, 0, 1, case.n, 512, p1).mean() < 0.35
        assert 0.45 < T.dropout_keep_mask(case.seed, 0, 2, case.n, 256, p2).mean() < 0.55


@pytest.fixture(scope="module")
def stage_start():
    import b0_layer_oracle as B
    import block15_train_oracle as BO
    import headconv_train_oracle as CO

    sd = B.stress_state_dict(0)
    return CO.conv_params(sd), BO.block_params(sd)


@pytest.mark.parametrize("case", H.STAGE_CASES, ids=lambda c: c.name)
def test_stage_preconditions_hold_and_figures_reproduce(case, stage_start):
    """on the rows of tests/golden (H.golden_rows); the device test asserts the same conditions on the rows it extracts"""
    conv0, block0 = stage_start
    fig = H.stage_figures(case, H.golden_rows(case.stage), conv0, block0, applies=False)
    print({k: v for k, v in fig.items() if k not in ("ref", "yard")}, "recorded", case.margin, case.rounding, case.storage)
    assert fig["ok"] and case.qualified >= 1
    assert case.margin / 3.0 <= fig["margin"] <= 3.0 * case.margin
    assert abs(fig["rounding"] - case.rounding) <= 0.2 * case.rounding + 0.01 and fig["rounding"] <= 0.5   # float64 alone
    if case.stage == "block":
        assert fig["storage"] <= 0.5          # against the float32 yardstick's luck on single numbers: recorded, not reproducible


# --------------------------------------------------------------------------- 2. the restated loss
@pytest.mark.parametrize("gamma,alpha,ls", [(2.0, 0.25, 0.1), (0.0, 0.25, 0.1), (2.0, 0.25, 0.0), (0.0, 0.25, 0.0), (0.5, 0.75, 0.3),
                                            (3.0, 0.5, 1.0), (2.5, 0.25, 0.1), (1.0, 0.25, 0.1)])
def test_restated_loss_is_the_oracles_formula(gamma, alpha, ls):
    rs = np.random.RandomState(0)
    z = np.concatenate([rs.uniform(-10.0, 10.0, 500), [-10.0, 10.0, 0.0]])
    y = (rs.rand(z.size) < 0.5).astype(np.float64)
    zt = torch.from_numpy(z).requires_grad_(True)
    per = []
    for i in range(z.size):                                     # O.focal takes the mean: one logit at a time gives the terms
        per.append(O.focal(zt[i:i + 1], torch.from_numpy(y[i:i + 1]), gamma, alpha, ls))
    terms = torch.stack(per)
    terms.sum().backward()
    loss, dz = H.focal_restated(z, y, gamma, alpha, ls)
    # 1e-12 per element wherever labels are smoothed (the settings the saturated cases run).  Without smoothing the
    # REFERENCE formula loses digits inside [-10, 10] for a confident right answer, which is why it is restated at all:
    #   * 1 - p_t = 1 - sigmoid(|z|) cancels (u = 4.5e-5 at |z| = 10); its u carries the roundings of sigmoid, two
    #     products, a sum and the subtraction, 2^-51 absolute in all, so u^gamma and the derivative autograd takes from
    #     the same u are off by (gamma + 1) 2^-51 / u relative;
    #   * binary_cross_entropy_with_logits adds log(1 + e^-|z|) to terms of size |z| that cancel: an ulp of |z| <= 10,
    #     2^-49 absolute, on a bce of 4.5e-5.
    # Both are allowed for as what they are, per element, from u and bce; with smoothing both terms are nothing
    # (u >= ls / 2, bce >= ls |z| / 2) and the bound is 1e-12 alone.
    t = y * (1 - ls) + 0.5 * ls
    p = 1.0 / (1.0 + np.exp(-z))
    u = p * (1 - t) + (1 - p) * t
    bce = np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))
    bound = 1e-12 + (0.0 if ls > 0 else 1.0) * ((gamma + 1.0) * 2.0 ** -51 / np.maximum(u, 1e-300) + 2.0 ** -49 / bce)
    assert (np.abs(loss - terms.detach().numpy()) <= bound * np.abs(terms.detach().numpy())).all()
    # the gradient is a sum of two terms of opposite sign, at (d(u^gamma)/dz bce + u^gamma (p - t)), and crosses zero inside
    # the range: relative to the larger of itself and its second term (an exact zero, z = 0 at t = 1/2, still must be one)
    scale = np.maximum(np.abs(zt.grad.numpy()), loss / bce * np.abs(p - t))
    assert (np.abs(dz - zt.grad.numpy()) <= bound * scale).all()
    # and saturated_reference is the mean of those terms with their gradients through fc3
    a2 = rs.rand(z.size, 256)
    cfg = {"focal_gamma": gamma, "focal_alpha": alpha, "label_smoothing": ls}
    out = H.saturated_reference(z, a2, y, cfg)
    assert abs(out["loss"][0] / float(terms.detach().mean()) - 1.0) <= 1e-12
    want = (zt.grad.numpy() / z.size) @ a2
    assert float(np.abs(out["grad w3"].ravel() - want).max()) <= 1e-12 * float(np.abs(want).max())
    assert abs(out["grad b3"][0] - zt.grad.numpy().sum() / z.size) <= 1e-12 * np.abs(zt.grad.numpy()).sum() / z.size


def test_restated_loss_stays_finite_where_the_formula_saturates():
    """at +-90 torch's 1 - sigmoid(z) is 0 or 1 exactly; the restatement keeps both tails (float64, and float32 as
    denormals or zero) and nothing is NaN or infinite"""
    z = np.array([20.0, -20.0, 40.0, -40.0, 90.0, -90.0, 95.0, -95.0])
    for y in (np.zeros(8), np.ones(8)):
        for gamma in (2.0, 0.0):
            for ls in (0.1, 0.0):
                for dt in (np.float64, np.float32):
                    loss, dz = H.focal_restated(z, y, gamma, 0.25, ls, dt)
                    assert np.isfinite(loss).all() and np.isfinite(dz).all() and (loss >= 0).all()
                l64, d64 = H.focal_restated(z, y, gamma, 0.25, ls, np.float64)
                if ls == 0.0:                                   # the exact tail: a confident right answer costs ~ e^-|z| ...
                    right = (z > 0) == (y > 0.5)
                    assert (l64[right] < 1e-8).all() and (l64[right][:6] > 0).all()
                    assert (np.abs(d64[right])[:6] > 0).all()   # ... and its gradient has not rounded to zero


# --------------------------------------------------------------------------- 3. defects
def test_carrier_without_a_defect_is_the_oracle():
    for name in ("dropout-0.2-n16", "mix-lam-1-n16", "momentum-0.01-n16", "rows-acc-n65", "apply-betas-0.5-0.9", "apply-clip-about"):
        ratio, where = _defect_ratio(CASES[name], None)
        print(name, ratio, where)
        assert ratio < 1e-3, (name, where)


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_defect_fails_the_case_meant_for_it(defect):
    case = CASES[DEFECTS[defect][0]]
    ratio, where = _defect_ratio(case, defect)
    kind = "apply" if case.kind == "apply" else "acc"
    existing = H.EXISTING_APPLY if kind == "apply" else H.EXISTING_ACC
    seen = [(c.name,) + _defect_ratio(c, defect) for c in existing]
    top = max(seen, key=lambda s: s[1])
    print(f"{defect} ({DEFECTS[defect][1]}): {case.name} ratio {ratio:.3g} at {where}; existing suite: worst {top[1]:.3g} in {top[0]} at {top[2]}")
    assert ratio > 1.0
    assert (top[1] <= 1.0) == (defect in INVISIBLE_BEFORE)      # the record of what the existing suite could not see

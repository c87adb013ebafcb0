"""The cases tests/test_block11_train_gpu.py runs on the device and tests/test_block11_train_oracle.py checks on the oracles
alone: sizes, variants, drop-connect rates of the blocks above, the trainer seeds that drive their masks and the parameter
seeds, with what was measured when they were picked.

A case is (n, variant, rates) at depth 11 (blocks 11..15): n crops; variant plain / mix (two label vectors with lam 0.7) /
scaled (loss_scale 0.5); rates "zero" (every crop kept in blocks 14, 13 and 12) or "ref" (the reference's 0.2 * b / 16 per
block, the masks drawn by the trainer seed `MASK_SEED[n]`).  Block 11 has no skip and no mask.

Sizes: block 11 sees 196 n rows in front of its depthwise conv and 49 n after it.  n = 2: 392 / 98 rows, ragged against the
64-row forward tiles and under one chunk after the conv; n = 11: 2156 / 539 rows, the 512-row weight-gradient chunks, the
256-row statistic chunks and the 8-crop depthwise chunks all ragged; n = 37 and the synthetic n = 64 cross several chunks of
every kind (7252 / 1813 and 12544 / 3136 rows; 64 crops are max_n).

The trainer seeds are block12_train_cases' (the same hash, the same layers 3, 4, 5 for blocks 14, 13, 12), picked there by
enumerating the hash alone: MASK_SEED[2] gives three masks that differ pairwise, MASK_SEED[11] and MASK_SEED[37] drop one
crop in all three blocks and one in block 14 only.  DROP12_SEED (`pick_drop12_seed`: the smallest seed that qualifies) drops
both crops of block 12 at n = 2 while blocks 13 and 14 keep both: dX12 is then dOut12 element for element, so "b11.dout"
equals "b12.dout".  ACC_MASK_SEED: block12_train_cases' again (every mask mixed at counter 0 with n = 16 and counter 1 with
n = 5).  The masks themselves are RECORDED in tests/test_block11_train_oracle.py.

The parameter seed (head parameters `O.default_params(seed)` and the labels) of an (n, rates) was picked on the CPU from
seeds 0..59 (`enumerate_seeds`), rows from a float32 CPU forward of the same weights and crops: of the seeds that meet gate
margin >= 1, rounding share <= 1 and storage share <= 0.5 in all three variants, the one with the largest gate margin
(`SEEDS`, with the margin, rounding share and storage share of its worst variant and the count of seeds that qualified, in
`PICKED`).

At n = 2 the shares are conditioned badly, as block12_train_cases explains (a BatchNorm over two crops follows the low bits
of the rows, and those follow the number of threads the float32 CPU forward sums with).  The n = 2 seeds were therefore
enumerated on two sources of rows, a forward with one thread and one with eight, and picked among the seeds that qualify on
both; `PICKED` holds the worse figure of the two runs and the count of seeds that qualified in both.
tests/test_block11_train_gpu.py asserts the same conditions again on the rows the device extracts.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import b0_layer_oracle as B
import block11_train_oracle as B1
import block12_train_cases as C12
import head_train_oracle as O
from rtdfd_amd import head_training as T

SIZES = (2, 11, 37)
MAX_N = 64
VARIANTS = C12.VARIANTS
RATES = C12.RATES                        # blocks 14, 13, 12; block 11 has none
ROW_CROPS, ROW_SEED = 37, 42             # the real rows: random_crops(37, 42) up to block 11's input

MASK_SEED = dict(C12.MASK_SEED)          # {2: 44, 11: 7, 37: 2}
DROP12_SEED = 0
ACC_MASK_SEED = C12.ACC_MASK_SEED
# (n, rates) -> parameter seed;  PICKED: the same key -> (gate margin, rounding share, storage share of the worst of the three
# variants, the number of seeds 0..59 that qualified), measured on the CPU when the seed was picked
SEEDS = {(2, "zero"): 8, (11, "zero"): 3, (37, "zero"): 32, (2, "ref"): 5, (11, "ref"): 32, (37, "ref"): 13}
PICKED = {(2, "zero"): (391.99, 0.77, 0.12, 2), (11, "zero"): (13.64, 0.23, 0.08, 43), (37, "zero"): (8.32, 0.46, 0.06, 29),
          (2, "ref"): (102.18, 0.12, 0.15, 5), (11, "ref"): (44.96, 0.34, 0.08, 44), (37, "ref"): (3.87, 0.47, 0.10, 32)}
# (37, "ref"): seed 56 has the largest margin with one thread (9.89, 0.27, 0.06) but its storage share is 0.58 with eight (the
# scalar gradient of the head's last bias against a yardstick error that moves with the thread count); seed 13 is the next
# by margin and qualifies with one thread and with eight - the worse figures of the two runs are recorded
# n = 2, both sources of rows (one thread / eight): "zero" qualifies seeds 8 and 23 on both (of 8 / 6 on one), "ref" seeds 5, 6,
# 49, 53 and 54 (of 10 / 8); picked by the smaller of max(rounding share, storage share / 0.5)
# the same enumeration for the cases outside the table (plain variant): seed -> margin, rounding share, storage share (qualifying of 60)
SYN64_SEED = 57                          # synthetic n = 64, drop_connect 0: 6.78, 0.25, 0.06 (31)
DROP_SEED = 14                           # block 12 drops both crops of n = 2, both sources of rows: 4221, 0.18, 0.08 (2: seeds 14 and 59)
ACC_SEED = 6                             # two accumulates (n = 16, then 5), the worse of the two: 10.6, 0.35, 0.10 (33)
EVAL_SEED = 13                           # eval at n = 5: of seeds 0..19 the largest smaller margin of the live and the EMA forward (57.9)

labels, bits, default_cfg = C12.labels, C12.bits, C12.default_cfg


def rates_of(rates: str):
    """-> (block 14's rate, {13: rate, 12: rate}) as the oracle and the device take them"""
    return C12.rates_of(12, rates)


def masks(trainer_seed: int, counter: int, n: int):
    """{block: bool (n,)} of blocks 14, 13, 12 at the reference's rates: the specification of what the device draws"""
    return C12.masks(trainer_seed, counter, n, 12)


def pick_drop12_seed(limit: int = 4000) -> int:
    """the enumeration DROP12_SEED comes from: at n = 2 block 12 drops both crops, blocks 13 and 14 keep both"""
    def only12(s):
        m = masks(s, 0, 2)
        return not m[12].any() and m[13].all() and m[14].all()

    return next(s for s in range(limit) if only12(s))


stress_sd = C12.stress_sd


@functools.lru_cache(maxsize=None)
def start():
    """(block 11, {13, 12}, block 14, block 15, conv) of the stress weights"""
    return (B1.block11_params(stress_sd()),) + C12.start(12)


@functools.lru_cache(maxsize=None)
def cpu_rows() -> np.ndarray:
    """the real rows of the CPU checks: block 10's output from a float32 CPU forward of the stress weights, NHWC"""
    x = torch.from_numpy(B.random_crops(ROW_CROPS, ROW_SEED))
    sdt = B.to_torch(stress_sd(), torch.float32)
    out = [B.forward_taps(sdt, x[i:i + 8])["b10.out"] for i in range(0, ROW_CROPS, 8)]
    return torch.cat(out).permute(0, 2, 3, 1).contiguous().numpy()


def single_cases():
    """every single-accumulate case: (kind, n, variant, rates)"""
    return [("real", n, v, r) for r in ("zero", "ref") for n in SIZES for v in VARIANTS] + [("synthetic", MAX_N, "plain", "zero")]


def case_seeds(kind: str, n: int, rates: str):
    """-> (parameter seed, trainer seed): the cases at rate 0 use the parameter seed for both"""
    seed = SYN64_SEED if kind == "synthetic" else SEEDS[(n, rates)]
    return seed, (seed if rates == "zero" else MASK_SEED[n])


case_inputs = C12.case_inputs


def oracles(head, cfg, rates: str = "zero", n: int = 3):
    b11, below, b14, b15, conv = start()
    p14, drops = rates_of(rates)
    make = B1.triple if n == 3 else B1.pair
    return make(b11, below, b14, b15, conv, head, cfg, drop_connect=p14, drops=drops)


def run_oracles(x, seed: int, trainer_seed: int, variant: str, rates: str, cfg=None, max_n: int = MAX_N):
    """one accumulate on the three oracles -> (o64, o32, ost, losses, (ya, yb, lam, scale))"""
    head, ya, yb, lam, scale = case_inputs(seed, x.shape[0], variant)
    cfg = cfg if cfg is not None else default_cfg(max_n=max_n, seed=trainer_seed)
    os_ = oracles(head, cfg, rates)
    losses = tuple(o.accumulate(x, ya, yb, lam, scale)[0] for o in os_)
    return os_ + (losses, (ya, yb, lam, scale))


def preconditions(o64, o32, ost, losses, ya, yb=None, lam=1.0):
    """-> (gate margin, rounding share, storage share, the name of the worst storage share)"""
    share = B1.storage_share(o64, o32, ost, losses)
    worst = max((k for k in share if k != "max"), key=lambda k: share[k])
    return B1.gate_margin(o64, o32), B1.rounding_share(o64, ya, yb, lam), share["max"], worst


def figures(x, seed: int, trainer_seed: int, rates: str, variants=tuple(VARIANTS)):
    """the worst (smallest margin, largest shares) of the variants of one seed -> (margin, rounding share, storage share)"""
    out = []
    for v in variants:
        o64, o32, ost, losses, (ya, yb, lam, _) = run_oracles(x, seed, trainer_seed, v, rates)
        out.append(preconditions(o64, o32, ost, losses, ya, yb, lam)[:3])
    return min(f[0] for f in out), max(f[1] for f in out), max(f[2] for f in out)


def forced_grads(seed: int):
    """gradients for every tensor of the seven groups, magnitudes log-uniform in [1e-4, 1], random signs: Adam's
    g / (sqrt(v) + eps) is well conditioned everywhere"""
    import block15_train_oracle as BO
    import headconv_train_oracle as CO
    import rtdfd_amd

    L = rtdfd_amd._lib
    rs = np.random.RandomState(seed)
    shapes = {k: L.HEAD_SHAPES[k] for k in O.GRAD_FIELDS}
    shapes.update({"conv." + k: L.CONV_SHAPES[k] for k in CO.CONV_GRAD_FIELDS})
    for b in (15, 14, 13, 12, 11):
        shapes.update({f"b{b}." + k: L.BLOCK_SHAPES_AT[b][k] for k in BO.BLOCK_GRAD_FIELDS})
    return {k: (10.0 ** rs.uniform(-4.0, 0.0, s) * np.where(rs.rand(*s) < 0.5, -1.0, 1.0)).astype(np.float32) for k, s in shapes.items()}


def eval_margins(x, seed: int, cfg=None):
    """the eval case: one forced apply, then the gate margins of the live and the EMA eval forward -> (live, ema)"""
    cfg = cfg if cfg is not None else default_cfg(max_n=16, seed=DROP12_SEED, clip_norm=1.0e4, ema_decay=0.5)
    o64, o32 = oracles(O.default_params(seed), cfg, "ref", n=2)
    g = forced_grads(70)
    out = []
    for o in (o64, o32):
        o.set_grads(g)
        o.apply(float(np.float32(1e-3)))
    for ema in (False, True):
        o64.evaluate(x, ema), o32.evaluate(x, ema)
        out.append(B1.gate_margin(o64, o32))
    return tuple(out)


def acc_figures(rows, seed: int):
    """the two-accumulate case (n = 16, then 5, loss_scale 0.5, the reference's rates) -> the worse figures of the two"""
    os_ = oracles(O.default_params(seed), default_cfg(max_n=16, seed=ACC_MASK_SEED), "ref")
    out = []
    for k, xk in enumerate((rows[:16], rows[16:21])):
        y = labels(seed + 400 + k, xk.shape[0])
        losses = tuple(o.accumulate(xk, y, None, 1.0, 0.5)[0] for o in os_)
        out.append(preconditions(*os_, losses, y)[:3])
    return min(f[0] for f in out), max(f[1] for f in out), max(f[2] for f in out)


def enumerate_seeds(x, n: int, rates: str, seeds=range(60)):
    """the enumeration `SEEDS` comes from -> {seed: (margin, rounding share, storage share)} of the seeds that qualify"""
    out = {}
    for s in seeds:
        m, r, st = figures(x[:n], s, s if rates == "zero" else MASK_SEED[n], rates)
        if m >= 1.0 and r <= 1.0 and st <= 0.5:
            out[s] = (m, r, st)
    return out

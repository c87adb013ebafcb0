"""The cases tests/test_block12_train_gpu.py runs on the device and tests/test_block12_train_oracle.py checks on the oracles
alone: sizes, variants, drop-connect rates, the trainer seeds that drive the masks and the parameter seeds, with what was
measured when they were picked.

A case is (depth, n, variant, rates): depth 13 (blocks 13..15) or 12 (blocks 12..15); n crops; variant plain / mix (two label
vectors with lam 0.7) / scaled (loss_scale 0.5); rates "zero" (every crop kept in every block) or "ref" (the reference's
0.2 * b / 16 per block, the masks drawn by the trainer seed `MASK_SEED[n]`).

The trainer seeds were picked by enumerating the hash alone (`pick_mask_seeds`: the smallest seed that qualifies):
  MASK_SEED[11], MASK_SEED[37]: one crop dropped in blocks 14, 13 and 12 alike, one crop dropped in exactly one of blocks 14
      and 13 and kept in 12 (so both depths see a crop dropped everywhere and one dropped once), no block with every crop dropped
  MASK_SEED[2]: the three masks differ pairwise and no block drops both crops
  DROP13_SEED: at n = 2 block 13 drops both crops, blocks 14 and 12 keep both
  ACC_MASK_SEED: at counter 0 (n = 16) and counter 1 (n = 5) every block's mask is mixed and the three differ
The masks themselves are RECORDED in tests/test_block12_train_oracle.py.

The parameter seed (head parameters `O.default_params(seed)` and the labels) of a (depth, n, rates) was picked on the CPU
from seeds 0..59, rows from a float32 CPU forward of the same weights and crops: of the seeds that meet gate margin >= 1,
rounding share <= 1 and storage share <= 0.5 in all three variants, the one with the largest gate margin (`SEEDS`, with the
margin, rounding share and storage share of its worst variant and the count of seeds that qualified, in `PICKED`).

At n = 2 the shares are conditioned badly: a BatchNorm over two crops makes them move with the low bits of the rows, and
those bits move with the number of threads the float32 CPU forward sums with (the rounding share of one seed goes from 0.1
to 5 between one thread and eight; the device's rows differ again).  The n = 2 seeds were therefore enumerated twice, on
the rows of a forward with one thread and with eight, and picked among the seeds that qualify on both with the rounding
and storage shares furthest from their limits; `PICKED` holds the worse figure of the two runs and the count of seeds that
qualified in both.  tests/test_block12_train_gpu.py asserts the same conditions again on the rows the device extracts.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import b0_layer_oracle as B
import block12_train_oracle as B2
import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
from rtdfd_amd import head_training as T

DEPTHS = (13, 12)
SIZES = (2, 11, 37)
MAX_N = 64
VARIANTS = {"plain": (False, 1.0), "mix": (True, 1.0), "scaled": (False, 0.5)}     # (two label vectors with lam, loss_scale)
RATES = {14: T.DROP_CONNECT_BLOCK14, 13: T.DROP_CONNECT_BLOCK13, 12: T.DROP_CONNECT_BLOCK12}
ROW_CROPS, ROW_SEED = 37, 42             # the real rows: random_crops(37, 42) up to the deepest block's input

MASK_SEED = {2: 44, 11: 7, 37: 2}
DROP13_SEED = 17
ACC_MASK_SEED = 0
# (depth, n, rates) -> parameter seed;  PICKED: the same key -> (gate margin, rounding share, storage share of the worst of
# the three variants, the number of seeds 0..59 that qualified), measured on the CPU when the seed was picked
SEEDS = {(13, 2, "zero"): 54, (13, 11, "zero"): 21, (13, 37, "zero"): 35, (13, 2, "ref"): 51, (13, 11, "ref"): 23, (13, 37, "ref"): 19,
         (12, 2, "zero"): 6, (12, 11, "zero"): 14, (12, 37, "zero"): 28, (12, 2, "ref"): 39, (12, 11, "ref"): 13, (12, 37, "ref"): 59}
PICKED = {(13, 2, "zero"): (437.98, 0.28, 0.13, 3), (13, 11, "zero"): (26.33, 0.48, 0.08, 53), (13, 37, "zero"): (13.10, 0.38, 0.06, 38),
          (13, 2, "ref"): (788.48, 0.14, 0.09, 8), (13, 11, "ref"): (42.60, 0.29, 0.08, 52), (13, 37, "ref"): (9.89, 0.38, 0.08, 37),
          (12, 2, "zero"): (1614.15, 0.23, 0.08, 4), (12, 11, "zero"): (32.31, 0.47, 0.08, 52), (12, 37, "zero"): (9.30, 0.33, 0.06, 41),
          (12, 2, "ref"): (1763.26, 0.13, 0.08, 7), (12, 11, "ref"): (27.71, 0.34, 0.15, 53), (12, 37, "ref"): (6.79, 0.32, 0.06, 35)}
# the same enumeration for the cases outside the table (plain variant): seed -> margin, rounding share, storage share (qualifying of 60)
SYN64_SEED = {13: 42, 12: 23}            # synthetic n = 64, drop_connect 0: 8.06, 0.35, 0.06 (33) / 5.24, 0.36, 0.06 (33)
DROP_SEED = {13: 41, 12: 43}             # block 13 drops both crops of n = 2: 304, 0.04, 0.08 (12) / 1350, 0.06, 0.13 (4)
ACC_SEED = {13: 4, 12: 39}               # two accumulates (n = 16, then 5), the worse of the two: 13.7, 0.46, 0.08 (45) / 15.6, 0.68, 0.10 (45)
EVAL_SEED = {13: 6, 12: 11}               # eval at n = 5: of seeds 0..19 the largest smaller margin of the live and the EMA forward (141 / 54)


def labels(seed: int, n: int) -> np.ndarray:
    return (np.random.RandomState(seed).rand(n) < 0.5).astype(np.float32)


def blocks_of(depth: int):
    """the skip blocks of a trainer of this depth, top down"""
    return tuple(range(14, depth - 1, -1))


def rates_of(depth: int, rates: str):
    """-> (block 14's rate, {block: rate} of the blocks below) as the oracle and `_open` take them"""
    if rates == "zero":
        return 0.0, {b: 0.0 for b in blocks_of(depth) if b != 14}
    return RATES[14], {b: RATES[b] for b in blocks_of(depth) if b != 14}


def masks(trainer_seed: int, counter: int, n: int, depth: int = 12):
    """{block: bool (n,)} at the reference's rates: the specification of what the device draws"""
    return {b: T.drop_connect_keep(trainer_seed, counter, n, RATES[b], block=b) for b in blocks_of(depth)}


def bits(m) -> str:
    return "".join("1" if k else "0" for k in m)


def pick_mask_seeds(limit: int = 4000):
    """the enumeration the trainer seeds above come from -> (MASK_SEED, DROP13_SEED, ACC_MASK_SEED)"""
    def mixed(m):
        return 0 < m.sum() < m.size

    def everywhere_and_once(s, n):
        m = masks(s, 0, n)
        d14, d13, d12 = ~m[14], ~m[13], ~m[12]
        return (d14 & d13 & d12).any() and ((d14 ^ d13) & ~d12).any() and all(m[b].any() for b in m)

    def pairwise(s):
        m = masks(s, 0, 2)
        return all(m[b].any() for b in m) and len({bits(m[b]) for b in m}) == 3

    def only13(s):
        m = masks(s, 0, 2)
        return not m[13].any() and m[14].all() and m[12].all()

    def acc(s):
        ms = [masks(s, 0, 16), masks(s, 1, 5)]
        return all(mixed(m[b]) for m in ms for b in m) and all(len({bits(m[b]) for b in m}) == 3 for m in ms)

    first = lambda ok: next(s for s in range(limit) if ok(s))
    return ({2: first(pairwise), 11: first(lambda s: everywhere_and_once(s, 11)), 37: first(lambda s: everywhere_and_once(s, 37))},
            first(only13), first(acc))


@functools.lru_cache(maxsize=None)
def stress_sd():
    return B.stress_state_dict(0)


@functools.lru_cache(maxsize=None)
def start(depth: int):
    """(blocks below 14 by index, block 14, block 15, conv) of the stress weights"""
    sd = stress_sd()
    return ({b: B2.skip_block_params(sd, b) for b in blocks_of(depth) if b != 14}, B2.skip_block_params(sd, 14), BO.block_params(sd),
            CO.conv_params(sd))


@functools.lru_cache(maxsize=None)
def cpu_rows(depth: int) -> np.ndarray:
    """the real rows of the CPU checks: the input of block `depth` from a float32 CPU forward of the stress weights"""
    x = torch.from_numpy(B.random_crops(ROW_CROPS, ROW_SEED))
    sdt = B.to_torch(stress_sd(), torch.float32)
    out = [B.forward_taps(sdt, x[i:i + 8])[f"b{depth - 1}.out"] for i in range(0, ROW_CROPS, 8)]
    return torch.cat(out).permute(0, 2, 3, 1).contiguous().numpy()


def single_cases():
    """every single-accumulate case: (depth, kind, n, variant, rates)"""
    out = []
    for depth in DEPTHS:
        out += [(depth, "real", n, v, r) for r in ("zero", "ref") for n in SIZES for v in VARIANTS]
        out.append((depth, "synthetic", MAX_N, "plain", "zero"))
    return out


def case_seeds(depth: int, kind: str, n: int, rates: str):
    """-> (parameter seed, trainer seed): drop_connect = 0 cases use the parameter seed for both"""
    seed = SYN64_SEED[depth] if kind == "synthetic" else SEEDS[(depth, n, rates)]
    return seed, (seed if rates == "zero" else MASK_SEED[n])


def case_inputs(seed: int, n: int, variant: str):
    """-> (head, labels_a, labels_b, lam, loss_scale)"""
    two, scale = VARIANTS[variant]
    yb, lam = (labels(seed + 201, n), 0.7) if two else (None, 1.0)
    return O.default_params(seed), labels(seed + 200, n), yb, lam, scale


def run_oracles(depth: int, x, seed: int, trainer_seed: int, variant: str, rates: str, cfg=None, max_n: int = MAX_N):
    """one accumulate on the three oracles -> (o64, o32, ost, losses, (ya, yb, lam, scale))"""
    head, ya, yb, lam, scale = case_inputs(seed, x.shape[0], variant)
    cfg = cfg if cfg is not None else default_cfg(max_n=max_n, seed=trainer_seed)
    below, b14, b15, conv = start(depth)
    p14, drops = rates_of(depth, rates)
    os_ = B2.triple(below, b14, b15, conv, head, cfg, drop_connect=p14, drops=drops)
    losses = tuple(o.accumulate(x, ya, yb, lam, scale)[0] for o in os_)
    return os_ + (losses, (ya, yb, lam, scale))


def preconditions(o64, o32, ost, losses, ya, yb=None, lam=1.0):
    """-> (gate margin, rounding share, storage share, the name of the worst storage share)"""
    share = B2.storage_share(o64, o32, ost, losses)
    worst = max((k for k in share if k != "max"), key=lambda k: share[k])
    return B2.gate_margin(o64, o32), B2.rounding_share(o64, ya, yb, lam), share["max"], worst


def default_cfg(**kw):
    """`dfd_head_config_default`'s values (train.py's argparse defaults) as `O.config_values` returns them, for the oracles
    of the CPU checks; the GPU tests take the library's own"""
    base = dict(max_n=MAX_N, seed=0, dropout=0.5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, focal_gamma=2.0, focal_alpha=0.25,
                label_smoothing=0.1, clip_norm=1.0, ema_decay=0.999, bn_momentum=0.1)
    base.update(kw)
    return {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in base.items()}

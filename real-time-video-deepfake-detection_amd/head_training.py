"""Training of the classifier head on the device, on the engine's own pooled features.

The reference's recipe (train.py: FocalLoss, AdamW, gradient clipping, gradient accumulation, EMA, OneCycleLR)
applied to the 1280 -> 512 -> 256 -> 1 head (model.py:50-61) with the backbone frozen.  The arithmetic of a step runs
in libdfd_hip.so (csrc/head_train.hip, `dfd_head_train_*` in include/dfd_hip.h); this module holds what lives on the
host: the learning-rate schedule, the specification of the dropout masks, the epoch loop and the state-dict names.

Deviations from train.py: fp32 instead of AMP / GradScaler; of the backbone only `_conv_head` + `_bn1` can be
fine-tuned (`HeadTrainer(train_conv_head=True)`: csrc/head_train_conv.hip, the rows are then block 15's output, "trunk
rows", and the conv is a second AdamW group at `backbone_lr_scale` x lr as train.py:891-924); Mixup works on feature
rows (trunk rows with the conv stage) unless `augment=` is given (then the crops are augmented on the device every epoch and Mixup / CutMix act on the
images, train_augment.py); a last batch of one row is dropped (BatchNorm1d needs two).  `HeadTrainer(train_block15=True)`
adds the backbone's last block, ``net._blocks.15`` (csrc/head_train_block.hip): the rows are then block 14's output,
(n, 7, 7, 192), and the block's tensors join the conv's group.  `HeadTrainer(train_block14=True)` adds ``net._blocks.14``
below it (the identity skip with per-crop drop-connect): the rows are then block 13's output, the same shape.
`train_block13=True` and `train_block12=True` add ``net._blocks.13`` and ``net._blocks.12`` (block 14's geometry, each with
its own drop-connect rate and mask): the rows are the input rows of the deepest unfrozen block.  After them every 7 x 7
block of train.py's unfrozen group trains.  `train_block11=True` adds ``net._blocks.11``, the stride-2 block that takes the
14 x 14 maps to 7 x 7 (112 -> 672 -> 192, no skip, no drop-connect): the rows are then block 10's output, (n, 14, 14, 112).
The 14 x 14 skip blocks 10 and 9 stay frozen.
"""
from __future__ import annotations

import math
import time
from typing import Dict, List, Mapping, Optional

import numpy as np

from . import _lib

# reference state-dict key -> `dfd_head_params` field
KEYS = {
    "net._fc.1.weight": "w1", "net._fc.1.bias": "b1",
    "net._fc.2.weight": "g1", "net._fc.2.bias": "be1", "net._fc.2.running_mean": "rm1", "net._fc.2.running_var": "rv1",
    "net._fc.5.weight": "w2", "net._fc.5.bias": "b2",
    "net._fc.6.weight": "g2", "net._fc.6.bias": "be2", "net._fc.6.running_mean": "rm2", "net._fc.6.running_var": "rv2",
    "net._fc.9.weight": "w3", "net._fc.9.bias": "b3",
}
TRACKED = ("net._fc.2.num_batches_tracked", "net._fc.6.num_batches_tracked")
# reference state-dict key -> `dfd_headconv_params` field (the conv stage, train_conv_head=True)
CONV_KEYS = {"net._conv_head.weight": "w", "net._bn1.weight": "g", "net._bn1.bias": "be", "net._bn1.running_mean": "rm",
             "net._bn1.running_var": "rv"}
CONV_TRACKED = "net._bn1.num_batches_tracked"
# reference state-dict key -> `dfd_mbconv_params` field (block 15, train_block15=True); "nbt<l>" are not fields of the
# struct: BatchNorm's num_batches_tracked counters live on the host, as TRACKED and CONV_TRACKED do
BLOCK_PREFIX = "net._blocks.15."
BLOCK_KEYS = {BLOCK_PREFIX + "_expand_conv.weight": "exp_w", BLOCK_PREFIX + "_depthwise_conv.weight": "dw_w",
              BLOCK_PREFIX + "_se_reduce.weight": "se_w1", BLOCK_PREFIX + "_se_reduce.bias": "se_b1",
              BLOCK_PREFIX + "_se_expand.weight": "se_w2", BLOCK_PREFIX + "_se_expand.bias": "se_b2",
              BLOCK_PREFIX + "_project_conv.weight": "proj_w"}
for _l in range(3):
    BLOCK_KEYS.update({f"{BLOCK_PREFIX}_bn{_l}.weight": f"g{_l}", f"{BLOCK_PREFIX}_bn{_l}.bias": f"be{_l}",
                       f"{BLOCK_PREFIX}_bn{_l}.running_mean": f"rm{_l}", f"{BLOCK_PREFIX}_bn{_l}.running_var": f"rv{_l}",
                       f"{BLOCK_PREFIX}_bn{_l}.num_batches_tracked": f"nbt{_l}"})
BLOCK_TRACKED = tuple(k for k, f in BLOCK_KEYS.items() if f.startswith("nbt"))
# the state dict's shapes of the conv kernels (the struct holds them without the 1 x 1 axes)
BLOCK_SD_SHAPES = {"exp_w": (1152, 192, 1, 1), "dw_w": (1152, 1, 3, 3), "se_w1": (48, 1152, 1, 1), "se_w2": (1152, 48, 1, 1),
                   "proj_w": (320, 1152, 1, 1)}
# block 14 (train_block14=True): the same fields in block 14's shapes (`_lib.BLOCK14_SHAPES`)
BLOCK14_PREFIX = "net._blocks.14."
BLOCK14_KEYS = {BLOCK14_PREFIX + k[len(BLOCK_PREFIX):]: f for k, f in BLOCK_KEYS.items()}
BLOCK14_TRACKED = tuple(k for k, f in BLOCK14_KEYS.items() if f.startswith("nbt"))
BLOCK14_SD_SHAPES = {"exp_w": (1152, 192, 1, 1), "dw_w": (1152, 1, 5, 5), "se_w1": (48, 1152, 1, 1), "se_w2": (1152, 48, 1, 1),
                     "proj_w": (192, 1152, 1, 1)}
DROP_CONNECT_BLOCK14 = 0.2 * 14 / 16     # efficientnet-b0's drop_connect_rate times idx / len(blocks)
# blocks 13 and 12 (train_block13=True, train_block12=True): block 14's shapes under their own names
BLOCK13_PREFIX, BLOCK12_PREFIX = "net._blocks.13.", "net._blocks.12."
BLOCK13_KEYS = {BLOCK13_PREFIX + k[len(BLOCK_PREFIX):]: f for k, f in BLOCK_KEYS.items()}
BLOCK12_KEYS = {BLOCK12_PREFIX + k[len(BLOCK_PREFIX):]: f for k, f in BLOCK_KEYS.items()}
BLOCK13_TRACKED = tuple(k for k, f in BLOCK13_KEYS.items() if f.startswith("nbt"))
BLOCK12_TRACKED = tuple(k for k, f in BLOCK12_KEYS.items() if f.startswith("nbt"))
BLOCK13_SD_SHAPES = dict(BLOCK14_SD_SHAPES)
BLOCK12_SD_SHAPES = dict(BLOCK14_SD_SHAPES)
DROP_CONNECT_BLOCK13 = 0.2 * 13 / 16
DROP_CONNECT_BLOCK12 = 0.2 * 12 / 16
# block 11 (train_block11=True): the same fields in block 11's shapes (`_lib.BLOCK11_SHAPES`); no skip, no drop-connect
BLOCK11_PREFIX = "net._blocks.11."
BLOCK11_KEYS = {BLOCK11_PREFIX + k[len(BLOCK_PREFIX):]: f for k, f in BLOCK_KEYS.items()}
BLOCK11_TRACKED = tuple(k for k, f in BLOCK11_KEYS.items() if f.startswith("nbt"))
BLOCK11_SD_SHAPES = {"exp_w": (672, 112, 1, 1), "dw_w": (672, 1, 5, 5), "se_w1": (28, 672, 1, 1), "se_w2": (672, 28, 1, 1),
                     "proj_w": (192, 672, 1, 1)}
# the skip blocks a trainer can hold, top down: (block, keys, tracked keys, state-dict shapes)
_SKIP_BLOCKS = ((14, BLOCK14_KEYS, BLOCK14_TRACKED, BLOCK14_SD_SHAPES), (13, BLOCK13_KEYS, BLOCK13_TRACKED, BLOCK13_SD_SHAPES),
                (12, BLOCK12_KEYS, BLOCK12_TRACKED, BLOCK12_SD_SHAPES))
BN_MOMENTUM_BACKBONE = 0.01              # efficientnet_pytorch: 1 - batch_norm_momentum (0.99)
BN_EPS_BACKBONE = 1e-3                   # efficientnet_pytorch's batch_norm_epsilon, the eps weights.pack_b0 folds with
LAYER_WIDTHS = (1280, 512, 256)          # what dropout layer 0 / 1 / 2 acts on
LAYER_RATES = (1.0, 0.7, 0.5)            # model.py:51,55,59: dropout, dropout * 0.7, dropout * 0.5


# --------------------------------------------------------------------------- schedule
def one_cycle_lr(step: int, total_steps: int, max_lr: float, pct_start: float = 0.1, div_factor: float = 25.0,
                 final_div_factor: float = 1000.0) -> float:
    """torch.optim.lr_scheduler.OneCycleLR(anneal_strategy='cos', three_phase=False) in closed form: the value
    `get_last_lr()` returns after `step` calls of `scheduler.step()` (train.py:916-924; step 0 = the initial rate)."""
    if total_steps <= 0:
        raise ValueError("total_steps must be positive")
    initial, min_lr = max_lr / div_factor, max_lr / div_factor / final_div_factor
    up_end = float(pct_start * total_steps) - 1.0
    if step <= up_end:
        start, end, pct = initial, max_lr, step / up_end
    else:
        start, end, pct = max_lr, min_lr, (step - up_end) / ((total_steps - 1) - up_end)
    return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1.0)


# --------------------------------------------------------------------------- dropout masks
def _fmix32(x: np.ndarray) -> np.ndarray:
    """MurmurHash3's 32-bit finaliser on uint32 arrays (arithmetic mod 2^32)"""
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def _u32(v: int) -> np.ndarray:
    return np.array([v & 0xFFFFFFFF], dtype=np.uint32)


def dropout_rates(dropout: float):
    """the three layer rates as the library computes them: doubles of the float32 setting"""
    d = float(np.float32(dropout))
    return tuple(r * d for r in LAYER_RATES)


def dropout_keep_mask(seed: int, counter: int, layer: int, n: int, width: int, p: float) -> np.ndarray:
    """The specification of the trainer's dropout: bool (n, width), True = kept (and scaled by 1 / (1 - p)).

    key  = fmix(fmix(fmix(fmix(fmix(seed_lo + 0x9E3779B9) ^ seed_hi) ^ counter_lo) ^ counter_hi) ^ (layer + 1))
    u(i) = fmix(fmix(i ^ key) + key),   i = row * width + col
    keep = u(i) >= floor(p * 2^32)
    all in uint32 arithmetic; `counter` = accumulate calls since the trainer was opened, `layer` = 0, 1, 2."""
    if not 0.0 <= p < 1.0:
        raise ValueError("p outside [0, 1)")
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        k = _fmix32(_u32(seed) + np.uint32(0x9E3779B9))
        k = _fmix32(k ^ _u32(seed >> 32))
        k = _fmix32(k ^ _u32(counter))
        k = _fmix32(k ^ _u32(counter >> 32))
        k = _fmix32(k ^ _u32(layer + 1))
        idx = np.arange(n * width, dtype=np.uint32)
        u = _fmix32(_fmix32(idx ^ k) + k)
    return (u >= np.uint32(int(p * 4294967296.0))).reshape(n, width)


def drop_connect_keep(seed: int, counter: int, n: int, p: float, block: int = 14) -> np.ndarray:
    """The specification of block `block`'s drop-connect (14, 13 or 12): bool (n,), True = the crop's branch is kept (and
    scaled by 1 / (1 - p)).  The trainer's hash with layer index 17 - block (3 for block 14, 4 for 13, 5 for 12: the blocks
    drop independently) and one draw per crop; `p` is the double of the float32 setting, the rule `dropout_rates` uses;
    `counter` = accumulate calls since the trainer was opened."""
    if block not in (12, 13, 14):
        raise ValueError("block outside 12..14")
    return dropout_keep_mask(seed, counter, 17 - int(block), n, 1, float(np.float32(p))).reshape(n)


# --------------------------------------------------------------------------- loss and metrics on the host
def focal_loss(logits, targets, gamma: float = 2.0, alpha: float = 0.25, label_smoothing: float = 0.0) -> float:
    """train.py:380-392 in float64 numpy (validation loss; the training loss comes from the device)"""
    z = np.asarray(logits, np.float64).reshape(-1)
    t = np.asarray(targets, np.float64).reshape(-1)
    if label_smoothing > 0:
        t = t * (1.0 - label_smoothing) + 0.5 * label_smoothing
    e = np.exp(-np.abs(z))
    bce = np.maximum(z, 0.0) - z * t + np.log1p(e)
    p = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    p_t = p * t + (1.0 - p) * (1.0 - t)
    a_t = alpha * t + (1.0 - alpha) * (1.0 - t)
    return float(np.mean(a_t * (1.0 - p_t) ** gamma * bce))


def _metrics(logits: np.ndarray, labels: np.ndarray) -> Dict[str, float]:
    """accuracy / F1 / AUC as train.py:649-672 computes them (AUC by ranks, ties averaged)"""
    pred = (logits > 0).astype(np.float64)                 # sigmoid(z) > 0.5
    acc = float((pred == labels).mean()) if labels.size else 0.0
    tp, fp = float(((pred == 1) & (labels == 1)).sum()), float(((pred == 1) & (labels == 0)).sum())
    fn = float(((pred == 0) & (labels == 1)).sum())
    prec, rec = tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10)
    f1 = 2 * prec * rec / (prec + rec + 1e-10)
    pos, neg = int((labels == 1).sum()), int((labels == 0).sum())
    auc = 0.0
    if pos and neg:
        order = np.argsort(logits, kind="mergesort")
        ranks = np.empty(labels.size, np.float64)
        sl = logits[order]
        i = 0
        while i < sl.size:
            j = i
            while j + 1 < sl.size and sl[j + 1] == sl[i]:
                j += 1
            ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
            i = j + 1
        auc = float((ranks[labels == 1].sum() - pos * (pos + 1) / 2.0) / (pos * neg))
    return {"acc": acc, "f1": float(f1), "auc": auc}


# --------------------------------------------------------------------------- the epoch loop
_VAL_CHUNK = 256          # validation crops per `train_augment_features` call of fit_loop(augment=...)


def fit_loop(trainer, features, labels, epochs: int, batch_size: int = 32, grad_accum: int = 2, lr: float = 3e-4,
             mix_alpha: float = 0.0, val=None, patience: int = 5, rng=None, augment=None,
             cutmix_alpha: float = 0.0) -> List[Dict[str, float]]:
    """train.py's `train_one_epoch` / `validate` loop over any object with `accumulate`, `apply`, `evaluate`,
    `max_n` and `loss_settings` (HeadTrainer; the tests' float64 oracle).  A trainer may carry `row_width` (floats of one
    row; default 1280) and `extract_method` (the extractor call `augment=` uses; default "train_augment_features"): a
    trainer with the conv stage takes trunk rows of 15680 floats from "train_augment_trunk", one with block 15 rows of 9408
    floats from "train_augment_block14" (with block 14: "train_augment_block13"; with block 13 or 12: "train_augment_input13" /
    "train_augment_input12", `Handle.train_augment_block_input` at the deepest block; with block 11 rows of 21952 floats from
    "train_augment_rows11", `Handle.train_augment_block_rows(block=11)`), and feature-space Mixup then acts on those rows.  Returns a log shaped like
    weights/training_log.json: one dict per epoch (epoch, train_loss, train_acc, val_loss, val_acc, val_f1, val_auc,
    lr, time_seconds).

    Draws, all from `rng` (a numpy RandomState; default RandomState(0)), in this order: per epoch one
    `permutation(len(features))` (the shuffle); then per batch, only when mix_alpha > 0: `random_sample()` (mix this
    batch when < 0.5, train.py:566-567), and for a mixed batch `beta(mix_alpha, mix_alpha)` then `permutation(rows)`.
    A mixed batch is lam x + (1 - lam) x[perm] on the feature rows with lam = max(lam, 1 - lam), labels (y, y[perm]).

    One optimizer step per `grad_accum` batches and at the last batch of an epoch (train.py:596); the rate of step k
    is one_cycle_lr(k, total optimizer steps, lr).  Validation (on `val` = (features, labels)) runs on the EMA
    parameters as train.py:992-999 does; training stops after `patience` epochs without a lower validation loss.

    `augment=(extractor, policy)`: `features` (and `val[0]`) are (N, H, W, 3) uint8 crops (or `ResidentCrops`); every batch is augmented and
    pushed through the backbone anew by `extractor.train_augment_features` (a `_lib.Handle`), `policy` a
    `train_augment.AugmentPolicy`.  Draws then: first, when `val` is given, `draw_batch(AugmentPolicy.validation(), ...)`
    for the validation crops (extracted once, before the first epoch); per epoch the permutation; per batch the mix
    decision - `random_sample()` (mix when < 0.5) when mix_alpha > 0 or cutmix_alpha > 0, then, whenever
    cutmix_alpha > 0 (mix_alpha = 0 included, as train.py:569 draws it), a second `random_sample()` (Mixup when < 0.5 and
    mix_alpha > 0, else CutMix, train.py:566-576); with cutmix_alpha = 0 a mixed batch is always Mixup, as without augment;
    Mixup draws `beta(mix_alpha, mix_alpha)` and `permutation(rows)`, CutMix `beta(cutmix_alpha, cutmix_alpha)`,
    `permutation(rows)`, `randint(0, 225)` for cy and for cx (lam recomputed from the clipped box) - and then
    `train_augment.draw_batch`'s draws for the batch.  Mixing happens in image space on the device; the trainer gets
    (y, y[perm], lam).  Training accuracy is counted against the original labels.  Without `augment` nothing of this
    runs: no draw is added (cutmix_alpha needs `augment`).  The crops are a host array or a
    `train_augment.ResidentCrops` (the set uploaded once; each shuffled batch is gathered device to device); both give the
    same bits.  Validation crops are extracted in chunks of 256 images."""
    width = int(getattr(trainer, "row_width", 1280))
    if augment is not None:
        from . import train_augment as _ta
        extractor, policy = augment
        extract_rows = getattr(extractor, getattr(trainer, "extract_method", "train_augment_features"))
        def crops_of(src, what):
            src = src if isinstance(src, _ta.ResidentCrops) else np.ascontiguousarray(np.asarray(src))
            if src.dtype != np.uint8 or src.ndim != 4 or src.shape[3] != 3:
                raise ValueError(f"with augment= the {what} are (N, H, W, 3) uint8 crops")
            return src

        def extract(src, idx, rows, batch):
            if isinstance(src, _ta.ResidentCrops):                 # device gather, no upload
                buf, shape = src.gather(idx)
                return extract_rows(buf, rows, batch, shape=shape)
            return extract_rows(src[idx], rows, batch)

        x = crops_of(features, "features")
    else:
        if cutmix_alpha > 0:
            raise ValueError("cutmix_alpha needs augment= (CutMix acts on images)")
        x = np.ascontiguousarray(np.asarray(features, np.float32))
        if width != 1280 and x.ndim > 2:
            x = x.reshape(x.shape[0], -1)                          # (N, 7, 7, 320) trunk rows
        if x.ndim != 2 or (width != 1280 and x.shape[1] != width):   # (N, 14, 14, 112) rows of block 10 were flattened above
            raise ValueError(f"features (N, {width}) and one label per row")
    y = np.asarray(labels, np.float32).reshape(-1)
    if x.shape[0] != y.size:
        raise ValueError(f"features (N, {width}) and one label per row")
    if batch_size < 2 or batch_size > trainer.max_n:
        raise ValueError(f"batch_size outside 2..{trainer.max_n}")
    rng = rng if rng is not None else np.random.RandomState(0)
    starts = [s for s in range(0, y.size, batch_size) if min(batch_size, y.size - s) >= 2]
    if not starts:
        raise ValueError("not enough rows for one batch")
    steps_per_epoch = -(-len(starts) // grad_accum)
    total_steps = steps_per_epoch * epochs
    gamma, alpha, ls = trainer.loss_settings
    log: List[Dict[str, float]] = []
    step, best, stale = 0, math.inf, 0
    if augment is not None and val is not None:
        vimg = crops_of(val[0], "validation features")
        vrows, vbatch = _ta.draw_batch(_ta.AugmentPolicy.validation(), rng, vimg.shape[0], vimg.shape[1], vimg.shape[2])
        # no stage of the validation policy looks at another image: chunks bound the work memory of a call
        val = (np.concatenate([extract(vimg, np.arange(i, min(i + _VAL_CHUNK, vimg.shape[0])), vrows[i:i + _VAL_CHUNK], vbatch)
                               for i in range(0, vimg.shape[0], _VAL_CHUNK)]), val[1])
    for epoch in range(1, epochs + 1):
        t0 = time.time()
        perm = rng.permutation(y.size)
        loss_sum, correct, seen, cur_lr = 0.0, 0, 0, one_cycle_lr(step, total_steps, lr)
        for bi, s in enumerate(starts):
            idx = perm[s:s + batch_size]
            ya, yb, lam = y[idx], None, 1.0
            xb = x[idx] if augment is None else None
            if augment is not None:
                mix = None
                if (mix_alpha > 0 or cutmix_alpha > 0) and rng.random_sample() < 0.5:
                    which = rng.random_sample() if cutmix_alpha > 0 else 0.0
                    if mix_alpha > 0 and which < 0.5:
                        lam = float(rng.beta(mix_alpha, mix_alpha))
                        lam = max(lam, 1.0 - lam)
                        p2 = rng.permutation(idx.size)
                        mix = (_ta.MIX_MIXUP, lam, p2)
                    else:
                        lam = float(rng.beta(cutmix_alpha, cutmix_alpha))
                        p2 = rng.permutation(idx.size)
                        cy, cx = int(rng.randint(0, 225)), int(rng.randint(0, 225))
                        box, lam = _ta.cutmix_box(lam, cy, cx, 224)
                        mix = (_ta.MIX_CUTMIX, lam, p2, box)
                    yb = ya[p2]
                rows, batch = _ta.draw_batch(policy, rng, idx.size, x.shape[1], x.shape[2], mix=mix)
                xb = extract(x, idx, rows, batch)
            elif mix_alpha > 0 and rng.random_sample() < 0.5:
                lam = float(rng.beta(mix_alpha, mix_alpha))
                lam = max(lam, 1.0 - lam)
                p2 = rng.permutation(idx.size)
                xb = (lam * xb + (1.0 - lam) * xb[p2]).astype(np.float32)
                yb = ya[p2]
            loss, logits = trainer.accumulate(xb, ya, yb, lam, 1.0 / grad_accum)
            loss_sum += loss * idx.size
            correct += int(((logits > 0) == (y[idx] > 0.5)).sum())
            seen += idx.size
            if (bi + 1) % grad_accum == 0 or bi + 1 == len(starts):
                cur_lr = one_cycle_lr(step, total_steps, lr)
                trainer.apply(cur_lr)
                step += 1
        entry = {"epoch": epoch, "train_loss": round(loss_sum / max(seen, 1), 5), "train_acc": round(correct / max(seen, 1), 4),
                 "val_loss": None, "val_acc": None, "val_f1": None, "val_auc": None, "lr": cur_lr}
        if val is not None:
            vx, vy = np.asarray(val[0], np.float32), np.asarray(val[1], np.float32).reshape(-1)
            if width != 1280:
                vx = vx.reshape(vx.shape[0], -1)
            vz = trainer.evaluate(vx, use_ema=True)
            m = _metrics(vz.astype(np.float64), vy.astype(np.float64))
            vloss = focal_loss(vz, vy, gamma, alpha, ls)
            entry.update(val_loss=round(vloss, 5), val_acc=round(m["acc"], 4), val_f1=round(m["f1"], 4), val_auc=round(m["auc"], 4))
        entry["time_seconds"] = round(time.time() - t0, 1)
        log.append(entry)
        if val is not None:
            if vloss < best:
                best, stale = vloss, 0
            else:
                stale += 1
                if stale >= patience:
                    break
    return log


# --------------------------------------------------------------------------- the trainer
class HeadTrainer:
    """A trainer opened on a handle (`dfd_head_train_begin` .. `_end`); use as a context manager or `close()` it.

    `train_block15=True` (implies `train_conv_head`) also trains ``net._blocks.15`` (`dfd_head_train_unfreeze_block`):
    `accumulate` / `evaluate` then take rows of block 14's output - `Handle.extract_trunk(x, block=14)`'s (n, 7, 7, 192) or
    (n, 9408) - the block's tensors step at `backbone_lr_scale` x lr with the conv's, and `commit` / `export_state_dict`
    cover all three groups.

    `train_block14=True` (implies `train_block15`) also trains ``net._blocks.14`` (`dfd_head_train_unfreeze_block_at`) with
    per-crop drop-connect at rate `drop_connect`: the rows are then block 13's output - `Handle.extract_block(x, 13)`'s
    (n, 7, 7, 192) or (n, 9408) - and `commit` / `export_state_dict` cover all four groups.

    `train_block13=True` (implies `train_block14`) and `train_block12=True` (implies `train_block13`) also train
    ``net._blocks.13`` / ``net._blocks.12`` with their own drop-connect rates `drop_connect13` / `drop_connect12` (`drop_connect`
    keeps meaning block 14) and their own masks (`drop_connect_keep(block=...)`): the rows are then the input rows of the
    deepest unfrozen block - `Handle.extract_block_input(x, 13 or 12)`'s (n, 7, 7, 192) or (n, 9408) - and `commit` /
    `export_state_dict` cover all five or six groups.

    `train_block11=True` (implies `train_block12`) also trains ``net._blocks.11`` (MBConv k5 at stride 2, 112 -> 672 -> 192,
    no skip and so no drop-connect): the rows are then block 10's output - `Handle.extract_block_rows(x, 11)`'s
    (n, 14, 14, 112) or (n, 21952) - and `commit` / `export_state_dict` cover all seven groups.

    `model_or_handle`: a `DeepfakeEfficientNet` (its handle and state dict are used) or a `_lib.Handle` with
    `state_dict` (reference key names, at least the ten ``net._fc.*`` tensors and the four running statistics).
    `config`: fields of `dfd_head_config` - max_n, seed, dropout, beta1, beta2, eps, weight_decay, focal_gamma,
    focal_alpha, label_smoothing, clip_norm, ema_decay, bn_momentum (defaults: train.py's).

    `train_conv_head=True` also trains ``net._conv_head`` and ``net._bn1`` (`dfd_head_train_unfreeze_conv`; the state
    dict must hold them): `accumulate` / `evaluate` then take trunk rows - `Handle.extract_trunk`'s (n, 7, 7, 320) or
    (n, 15680) - the conv tensors step at `backbone_lr_scale` x lr, and `commit` / `export_state_dict` cover both."""

    def __init__(self, model_or_handle, state_dict: Optional[Mapping[str, np.ndarray]] = None, train_conv_head: bool = False,
                 backbone_lr_scale: float = 0.1, train_block15: bool = False, train_block14: bool = False,
                 drop_connect: float = DROP_CONNECT_BLOCK14, train_block13: bool = False, train_block12: bool = False,
                 drop_connect13: float = DROP_CONNECT_BLOCK13, drop_connect12: float = DROP_CONNECT_BLOCK12,
                 train_block11: bool = False, **config):
        if isinstance(model_or_handle, _lib.Handle):
            handle = model_or_handle
            if state_dict is None:
                raise ValueError("a bare handle needs the head's state_dict")
        else:
            handle = model_or_handle.handle
            if state_dict is None:
                state_dict = model_or_handle.state_dict()
        sd = {(k if k.startswith("net.") else "net." + k): v for k, v in state_dict.items()}
        params = {f: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], np.float32)
                  for k, f in KEYS.items()}
        self._tracked = [int(np.asarray(sd[k])) if k in sd else 0 for k in TRACKED]
        self.train_block11 = bool(train_block11)
        self.train_block12 = bool(train_block12) or self.train_block11
        self.train_block13 = bool(train_block13) or self.train_block12
        self.train_block14 = bool(train_block14) or self.train_block13
        self.train_block15 = bool(train_block15) or self.train_block14
        self.train_conv_head = bool(train_conv_head) or self.train_block15
        self.row_width = (_lib.BLOCK11_INPUT_ROW if self.train_block11 else _lib.BLOCK14_ROW if self.train_block15 else
                          _lib.TRUNK_ROW if self.train_conv_head else 1280)
        self.extract_method = ("train_augment_rows11" if self.train_block11 else "train_augment_input12" if self.train_block12 else "train_augment_input13" if self.train_block13 else
                               "train_augment_block13" if self.train_block14 else "train_augment_block14" if self.train_block15 else
                               "train_augment_trunk" if self.train_conv_head else "train_augment_features")
        if self.train_block15:
            block = {f: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], np.float32)
                     for k, f in BLOCK_KEYS.items() if not f.startswith("nbt")}
            self._block_tracked = [int(np.asarray(sd[k])) if k in sd else 0 for k in BLOCK_TRACKED]
        # the unfrozen skip blocks, top down: (block, keys, tracked keys, state-dict shapes, drop-connect rate)
        rates = {14: drop_connect, 13: drop_connect13, 12: drop_connect12}
        on = {14: self.train_block14, 13: self.train_block13, 12: self.train_block12}
        self._skip_blocks = [sb + (rates[sb[0]],) for sb in _SKIP_BLOCKS if on[sb[0]]]
        skip_params, self._skip_tracked = {}, {}
        for b, keys, tracked, _shapes, _rate in self._skip_blocks:
            skip_params[b] = {f: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], np.float32)
                              for k, f in keys.items() if not f.startswith("nbt")}
            self._skip_tracked[b] = [int(np.asarray(sd[k])) if k in sd else 0 for k in tracked]
        if self.train_block14:
            self._block14_tracked = self._skip_tracked[14]
        if self.train_block11:
            block11 = {f: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], np.float32)
                       for k, f in BLOCK11_KEYS.items() if not f.startswith("nbt")}
            self._block11_tracked = [int(np.asarray(sd[k])) if k in sd else 0 for k in BLOCK11_TRACKED]
        if self.train_conv_head:
            conv = {f: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], np.float32)
                    for k, f in CONV_KEYS.items()}
            self._conv_tracked = int(np.asarray(sd[CONV_TRACKED])) if CONV_TRACKED in sd else 0
        self.config = _lib.head_config(**config)
        self.max_n = int(self.config.max_n)
        self.loss_settings = (float(self.config.focal_gamma), float(self.config.focal_alpha), float(self.config.label_smoothing))
        self._h = handle
        self._open = False
        handle.head_train_begin(params, self.config)
        self._open = True
        if self.train_conv_head:
            try:
                handle.head_train_unfreeze_conv(conv, backbone_lr_scale, BN_MOMENTUM_BACKBONE, BN_EPS_BACKBONE)
            except Exception:
                self.close()
                raise
        if self.train_block15:
            try:
                handle.head_train_unfreeze_block(block, 15, BN_MOMENTUM_BACKBONE, BN_EPS_BACKBONE)
            except Exception:
                self.close()
                raise
        for b, _keys, _tracked, _shapes, rate in self._skip_blocks:
            try:
                handle.head_train_unfreeze_block_at(skip_params[b], b, BN_MOMENTUM_BACKBONE, BN_EPS_BACKBONE, rate)
            except Exception:
                self.close()
                raise
        if self.train_block11:
            try:
                handle.head_train_unfreeze_block_at(block11, 11, BN_MOMENTUM_BACKBONE, BN_EPS_BACKBONE, 0.0)
            except Exception:
                self.close()
                raise
        self.accumulates = 0
        self.steps = 0

    def __enter__(self):
        return self

    def __exit__(self, *_exc):
        self.close()

    def close(self):
        if self._open:
            self._open = False
            if getattr(self._h, "_p", None):
                self._h.head_train_end()

    def accumulate(self, features, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        """one train-mode forward / backward added to the gradients -> (unscaled loss, logits (n,))"""
        fn = (self._h.head_train_accumulate_block if self.train_block15 else
              self._h.head_train_accumulate_trunk if self.train_conv_head else self._h.head_train_accumulate)
        out = fn(features, labels_a, labels_b, lam, loss_scale)
        self.accumulates += 1
        return out

    def apply(self, lr: float) -> float:
        """clip, AdamW step, EMA update, gradients zeroed -> gradient norm before clipping"""
        norm = self._h.head_train_apply(lr)
        self.steps += 1
        return norm

    def evaluate(self, features, use_ema: bool = False) -> np.ndarray:
        """eval-mode logits (n,) on the live or the EMA parameters; any n (chunks of max_n)"""
        a = np.ascontiguousarray(np.asarray(features, np.float32))
        if a.shape[0] == 0:
            return np.empty(0, np.float32)
        fn = (self._h.head_train_eval_block if self.train_block15 else
              self._h.head_train_eval_trunk if self.train_conv_head else self._h.head_train_eval)
        return np.concatenate([fn(a[i:i + self.max_n], use_ema) for i in range(0, a.shape[0], self.max_n)])

    def export_state_dict(self, use_ema: bool = False) -> Dict[str, np.ndarray]:
        """the head under the reference's names: ten ``net._fc.*`` parameters, four running statistics (always the live
        ones) and the two ``num_batches_tracked`` counters; with the conv stage also ``net._conv_head.weight``
        ((1280, 320, 1, 1)), ``net._bn1.*`` and its counter; with block 15 also the 22 ``net._blocks.15.*`` entries of
        `BLOCK_KEYS` (conv kernels in the state dict's 4-d shapes); with block 14 also the 22 of `BLOCK14_KEYS`, with block 13
        those of `BLOCK13_KEYS`, with block 12 those of `BLOCK12_KEYS`, with block 11 those of `BLOCK11_KEYS`"""
        out = self._h.head_train_export(use_ema)
        sd = {k: out[f] for k, f in KEYS.items()}
        for k, t in zip(TRACKED, self._tracked):
            sd[k] = np.array(t + self.accumulates, dtype=np.int64)
        if self.train_conv_head:
            conv = self._h.head_train_export_conv(use_ema)
            sd.update({k: (conv[f].reshape(1280, 320, 1, 1) if f == "w" else conv[f]) for k, f in CONV_KEYS.items()})
            sd[CONV_TRACKED] = np.array(self._conv_tracked + self.accumulates, dtype=np.int64)
        if self.train_block15:
            blk = self._h.head_train_export_block(use_ema)
            sd.update({k: blk[f].reshape(BLOCK_SD_SHAPES.get(f, blk[f].shape)) for k, f in BLOCK_KEYS.items() if f in blk})
            for k, t in zip(BLOCK_TRACKED, self._block_tracked):
                sd[k] = np.array(t + self.accumulates, dtype=np.int64)
        for b, keys, tracked, shapes, _rate in self._skip_blocks:
            blk = self._h.head_train_export_block_at(b, use_ema)
            sd.update({k: blk[f].reshape(shapes.get(f, blk[f].shape)) for k, f in keys.items() if f in blk})
            for k, t in zip(tracked, self._skip_tracked[b]):
                sd[k] = np.array(t + self.accumulates, dtype=np.int64)
        if self.train_block11:
            blk = self._h.head_train_export_block_at(11, use_ema)
            sd.update({k: blk[f].reshape(BLOCK11_SD_SHAPES.get(f, blk[f].shape)) for k, f in BLOCK11_KEYS.items() if f in blk})
            for k, t in zip(BLOCK11_TRACKED, self._block11_tracked):
                sd[k] = np.array(t + self.accumulates, dtype=np.int64)
        return sd

    def commit(self, use_ema: bool = True):
        """fold BatchNorm and swap the head (and, with the conv stage, the head conv; with blocks 15 down to 11, their ten tensors each) the
        handle classifies with (`dfd_head_train_commit`)"""
        self._h.head_train_commit(use_ema)

    def fit(self, features, labels, epochs: int, batch_size: int = 32, grad_accum: int = 2, lr: float = 3e-4,
            mix_alpha: float = 0.0, val=None, patience: int = 5, rng=None, augment=None, cutmix_alpha: float = 0.0):
        """`fit_loop` on this trainer"""
        return fit_loop(self, features, labels, epochs, batch_size, grad_accum, lr, mix_alpha, val, patience, rng, augment,
                        cutmix_alpha)


__all__ = ["HeadTrainer", "fit_loop", "one_cycle_lr", "dropout_keep_mask", "dropout_rates", "focal_loss", "KEYS", "CONV_KEYS", "BLOCK_KEYS", "BLOCK14_KEYS",
           "BLOCK13_KEYS", "BLOCK12_KEYS", "BLOCK11_KEYS", "drop_connect_keep"]

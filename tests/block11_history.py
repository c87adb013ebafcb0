"""A trainer with block 11 unfrozen below block 12 and the extraction of block rows as a case of the call-history table
(tests/history_cases.py): does a depth-11 session, or an extraction of block 11's input rows, depend on what the handle did
before?

Importing this module REGISTERS the case (`H.CASES`, `H.BY_NAME`, family "trainer"), so that the table's coverage check
(tests/test_history_cases.py) knows the two new exports.  Its histories are the family's at the deepest older level
(`arg` = "block": a whole block-15 session at max_n = 64, finite and non-finite), which leave block 15's buffers and freed
device memory behind for the five stages' allocations.  The test files of the feature import this module, so any run that
collects the suite has the case in the table."""
import functools

import b0_layer_oracle as B
import block12_history as BH12
import history_cases as H

L = H.L
REACHES = ("dfd_extract_block_rows", "dfd_train_augment_block_rows")
SEED, MASK_SEED = 31, 3
DROPS = BH12.DROPS
BLOCKS = (15, 14, 13, 12, 11)
TAPS = BH12.TAPS + tuple(f"b11.{k}" for k in ("out", "gate", "ad", "dout", "dae"))


@functools.lru_cache(maxsize=None)
def params():
    """(head, conv, block 15, {14, 13, 12: block}, block 11) the trainer begins with: the table's stress weights"""
    import block11_train_oracle as B1
    import head_train_oracle as HO

    _, conv, b15, skips = BH12.params()
    return HO.default_params(SEED), conv, b15, skips, B1.block11_params(B.stress_state_dict(0))


def rows(n: int, seed: int):
    import block11_train_oracle as B1

    return B1.synthetic_rows(seed, n)


@functools.lru_cache(maxsize=None)
def batches():
    return [(rows(n, SEED + 500 + k), H.train_labels(SEED + 600 + k, n)) for k, n in enumerate(H.TRAIN_N)]


crops = BH12.crops


def _state(h, ema=False):
    out = {"conv.grads": h.head_train_conv_grads(), "grads": h.head_train_grads()}
    for b in BLOCKS:
        out[f"b{b}.grads"] = h.head_train_block_grads_at(b)
        out[f"b{b}.export"] = h.head_train_export_block_at(b, ema)
    return out


def run(h, dirty=H._noop):
    dirty()                                       # one session is one case: the history ends before its begin
    out = {}
    head, conv, b15, skips, b11 = params()
    h.head_train_begin(head, L.head_config(max_n=8, seed=MASK_SEED))
    try:
        h.head_train_unfreeze_conv(conv)
        h.head_train_unfreeze_block(b15)
        for b in (14, 13, 12):
            h.head_train_unfreeze_block_at(skips[b], b, drop_connect=DROPS[b])
        h.head_train_unfreeze_block_at(b11, 11, drop_connect=0.0)
        for k, (x, y) in enumerate(batches()):
            loss, logits = h.head_train_accumulate_block(x, y)
            step = {"loss": loss, "logits": logits.copy()}
            for t in TAPS:
                step["tap." + t] = h.head_train_tap(t, x.shape[0])
            step.update(_state(h))
            out[f"accumulate{k}"] = step
        out["grad_norm"] = h.head_train_apply(1e-3)
        held = rows(5, SEED + 700)
        out["eval_live"], out["eval_ema"] = h.head_train_eval_block(held, False).copy(), h.head_train_eval_block(held, True).copy()
        out["after_apply"] = _state(h)
        out["after_apply_ema"] = _state(h, True)
    finally:
        h.head_train_end()
    for block in (11, 12, 13, 14, 15):
        dirty()
        out[f"rows{block}"] = h.extract_block_rows(crops(), block)
    rgb, rows_, batch = H.aug_inputs(**H.AUG_CASE)
    dirty()
    out["augment11"] = h.train_augment_block_rows(rgb, rows_, batch, block=11)
    return out


CASE = H.Case("trainer_block11", "trainer", run, REACHES, ("repeat", "large", "nonfinite"), arg="block")
if CASE.name not in H.BY_NAME:
    H.CASES.append(CASE)
    H.BY_NAME[CASE.name] = CASE

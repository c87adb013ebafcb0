"""Block 14's stage of the head trainer and the extraction at blocks 13-15 as a case of the call-history table
(tests/history_cases.py): does a trainer with block 14 unfrozen, or an extraction at block 13, depend on what the handle
did before?

Importing this module REGISTERS the case (`H.CASES`, `H.BY_NAME`, family "trainer"), so that the table's coverage check
(tests/test_history_cases.py) knows the five new exports.  Its histories are the family's at the deepest older level
(`arg` = "block": a whole block-15 session at max_n = 64, finite and non-finite), which leave block 15's buffers and
freed device memory behind for the new stage's allocation.  The test files of the feature import this module, so any run that
collects the suite has the case in the table."""
import functools

import numpy as np

import b0_layer_oracle as B
import history_cases as H

L = H.L
REACHES = ("dfd_head_train_unfreeze_block_at", "dfd_head_train_export_block_at", "dfd_head_train_block_grads_at",
           "dfd_extract_block_out", "dfd_train_augment_block_out")
SEED, MASK_SEED, DROP_CONNECT = 25, 3, 0.2 * 14 / 16          # trainer seed 3: a mixed mask at n = 5 (11100)
TAPS = ("b14.out", "b14.gate", "b14.ad", "b14.keep", "b14.dout", "b14.dae")


@functools.lru_cache(maxsize=None)
def params():
    """(head, conv, block 15, block 14) the trainer begins with: the table's stress weights"""
    import block14_train_oracle as B4
    import block15_train_oracle as BO
    import head_train_oracle as HO
    import headconv_train_oracle as CO

    sd = B.stress_state_dict(0)
    return HO.default_params(SEED), CO.conv_params(sd), BO.block_params(sd), B4.block14_params(sd)


@functools.lru_cache(maxsize=None)
def batches():
    return [(H.train_rows("block", n, SEED + 500 + k), H.train_labels(SEED + 600 + k, n)) for k, n in enumerate(H.TRAIN_N)]


@functools.lru_cache(maxsize=None)
def crops():
    return B.random_crops(2, 31)


def _state(h, ema=False):
    return {"b14.grads": h.head_train_block_grads_at(14), "b14.export": h.head_train_export_block_at(14, ema),
            "b15.grads": h.head_train_block_grads_at(15), "b15.export": h.head_train_export_block_at(15, ema),
            "conv.grads": h.head_train_conv_grads(), "grads": h.head_train_grads()}


def run(h, dirty=H._noop):
    dirty()                                       # one session is one case: the history ends before its begin
    out = {}
    head, conv, b15, b14 = params()
    h.head_train_begin(head, L.head_config(max_n=8, seed=MASK_SEED))
    try:
        h.head_train_unfreeze_conv(conv)
        h.head_train_unfreeze_block(b15)
        h.head_train_unfreeze_block_at(b14, 14, drop_connect=DROP_CONNECT)
        for k, (x, y) in enumerate(batches()):
            loss, logits = h.head_train_accumulate_block(x, y)
            step = {"loss": loss, "logits": logits.copy()}
            for t in TAPS:
                step["tap." + t] = h.head_train_tap(t, x.shape[0])
            step.update(_state(h))
            out[f"accumulate{k}"] = step
        out["grad_norm"] = h.head_train_apply(1e-3)
        held = H.train_rows("block", 5, SEED + 700)
        out["eval_live"], out["eval_ema"] = h.head_train_eval_block(held, False).copy(), h.head_train_eval_block(held, True).copy()
        out["after_apply"] = _state(h)
        out["after_apply_ema"] = _state(h, True)
    finally:
        h.head_train_end()
    for block in (13, 14, 15):
        dirty()
        out[f"extract{block}"] = h.extract_block(crops(), block)
    rgb, rows, batch = H.aug_inputs(**H.AUG_CASE)
    dirty()
    out["augment13"] = h.train_augment_block(rgb, rows, batch, block=13)
    return out


CASE = H.Case("trainer_block14", "trainer", run, REACHES, ("repeat", "large", "nonfinite"), arg="block")
if CASE.name not in H.BY_NAME:
    H.CASES.append(CASE)
    H.BY_NAME[CASE.name] = CASE

"""GPU: block 11 of the head trainer (csrc/head_train_block.hip: dfd_head_train_unfreeze_block_at at 11, the _block entries
on block 10's output rows, _export_block_at / _block_grads_at, the "b11.*" taps, the stride-2 depthwise kernels, the guarded
statistic and weight-gradient launches at 672 / 112 channels, the seven-arena dfd_head_train_apply and _commit) and the
extraction of block rows (dfd_extract_block_rows, dfd_train_augment_block_rows) against the float64 oracle of
tests/block11_train_oracle.py, at depth 11 (blocks 11..15).

Bars: as tests/test_block12_train_gpu.py - every compared tensor's rms(d) / rms(ref) and max|d| / max|ref| against the
float64 oracle at most 4 x / 8 x the same metrics of the float32 CPU oracle, floored at 2^-23 / 2^-21 (`O.bar_ratio` <= 1).
Every figure is printed before it is asserted.

Inputs: "real" rows are `extract_block_rows(x, 11)` of b0_layer_oracle.stress_state_dict weights on random_crops (all
blocks, conv stage and head start from the same state dict); "synthetic" rows are standard normals.  max_n = 64, max_batch 16.

Preconditions, all on the oracles alone and asserted before the device is looked at: `gate_margin` >= 1, `rounding_share`
<= 1 and `storage_share` <= 0.5.  Sizes, variants, rates, trainer seeds (the masks) and parameter seeds are the table of
tests/block11_train_cases.py, picked on the CPU; tests/test_block11_train_oracle.py runs the same preconditions without a
device and RECORDS the masks.

Rows in front of block 11's depthwise conv / after it: 392 / 98 (n = 2), 2156 / 539 (11), 7252 / 1813 (37), 12544 / 3136 (64).
"""
import numpy as np
import pytest

import b0_layer_oracle as B
import block11_history  # noqa: F401  (registers the new exports and their case with the call-history table)
import block11_train_cases as C
import block11_train_oracle as B1
import block12_train_oracle as B2
import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
from rtdfd_amd import head_training as T
from rtdfd_amd import train_augment as TA

pytestmark = pytest.mark.gpu

MAX_N = C.MAX_N
BLOCKS = (15, 14, 13, 12, 11)
COUNTS = {"head": 788993, "conv": 412160, 15: 717232, 14: 587952, 13: 587952, 12: 587952, 11: 262492}     # floats of the seven arenas


@pytest.fixture(scope="module")
def stress_sd():
    return C.stress_sd()


@pytest.fixture(scope="module")
def sh(pkg, stress_sd):
    """the handle of this module's trainers and extractions: stress weights, classifier only"""
    h = pkg._lib.Handle(pkg.weights.pack_b0(stress_sd), device=0, max_batch=16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def real_rows(sh):
    """block 11's input rows, computed once"""
    x = B.random_crops(C.ROW_CROPS, C.ROW_SEED)
    return np.concatenate([sh.extract_block_rows(x[i:i + 16], 11) for i in range(0, C.ROW_CROPS, 16)])


def _open(pkg, h, head, rates="zero", **kw):
    b11, below, b14, b15, conv = C.start()
    p14, drops = C.rates_of(rates)
    cfg = pkg._lib.head_config(**kw)
    h.head_train_begin(head, cfg)
    try:
        h.head_train_unfreeze_conv(conv)
        h.head_train_unfreeze_block(b15)
        h.head_train_unfreeze_block_at(b14, 14, drop_connect=p14)
        for b in (13, 12):
            h.head_train_unfreeze_block_at(below[b], b, drop_connect=drops[b])
        h.head_train_unfreeze_block_at(b11, 11, drop_connect=0.0)
    except Exception:
        h.head_train_end()
        raise
    return O.config_values(cfg)


def _check(name, got, ref64, yard32, record):
    r = O.bar_ratio(got, ref64, yard32)
    print(f"{name}: rms {r['rms']:.3e} (yard {r['yard_rms']:.3e}) max {r['max']:.3e} (yard {r['yard_max']:.3e}) ratio {r['ratio']:.3f}")
    record.append((name, r["ratio"]))


def _assert_all(record):
    groups = {}
    for k, v in record:
        g = k.split(".")[0].replace("grad ", "").replace("param ", "").replace("ema ", "")
        groups[g] = max(groups.get(g, 0.0), v)
    print("worst ratio per group: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(groups.items())))
    bad = [(k, round(v, 3)) for k, v in record if not v <= 1.0]
    assert not bad, bad


def _all_grads(h):
    g = dict(h.head_train_grads())
    g.update({"conv." + k: v for k, v in h.head_train_conv_grads().items()})
    for b in BLOCKS:
        g.update({f"b{b}." + k: v for k, v in h.head_train_block_grads_at(b).items()})
    return g


def _all_export(h, ema=False):
    e = dict(h.head_train_export(ema))
    e.update({"conv." + k: v for k, v in h.head_train_export_conv(ema).items()})
    for b in BLOCKS:
        e.update({f"b{b}." + k: v for k, v in h.head_train_export_block_at(b, ema).items()})
    return e


GRAD_KEYS = tuple(f"b{b}." + k for b in BLOCKS for k in BO.BLOCK_GRAD_FIELDS) + tuple("conv." + k for k in CO.CONV_GRAD_FIELDS) + O.GRAD_FIELDS
STAT_KEYS = tuple(f"b{b}." + k for b in BLOCKS for k in BO.BLOCK_STAT_FIELDS) + tuple("conv." + k for k in CO.CONV_STAT_FIELDS) + O.STAT_FIELDS


def _compare_state(h, o64, o32, rec, skip_grads=()):
    g, g64, g32 = _all_grads(h), o64.grads(), o32.grads()
    for k in GRAD_KEYS:
        if not k.startswith(skip_grads or ("\0",)):
            _check("grad " + k, g[k], g64[k], g32[k], rec)
    e, e64, e32 = _all_export(h), o64.export(), o32.export()
    for k in STAT_KEYS:
        _check(k, e[k], e64[k], e32[k], rec)


def _preconditions(o64, o32, ost, losses, ya, yb=None, lam=1.0, what=""):
    margin, rshare, sshare, worst = C.preconditions(o64, o32, ost, losses, ya, yb, lam)
    print(f"gate margin{what} {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f} ({worst})")
    assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5    # conditions on the inputs, checked on the oracles alone


def _one_accumulate(pkg, sh, x, seed, trainer_seed, variant, rates):
    """one accumulate on the device and the three oracles -> (o64, o32, the record so far)"""
    head, ya, yb, lam, scale = C.case_inputs(seed, x.shape[0], variant)
    cfg = _open(pkg, sh, head, rates, max_n=MAX_N, seed=trainer_seed)
    o64, o32, ost = C.oracles(head, cfg, rates)
    (l64, z64), (l32, z32), (lst, _) = (o.accumulate(x, ya, yb, lam, scale) for o in (o64, o32, ost))
    _preconditions(o64, o32, ost, (l64, l32, lst), ya, yb, lam)
    loss, logits = sh.head_train_accumulate_block(x, ya, yb, lam, scale)
    rec = []
    _check("loss", [loss], [l64], [l32], rec)
    _check("logits", logits, z64, z32, rec)
    return o64, o32, rec


def _check_keeps(sh, n, spec):
    """`b*.keep` of the skip blocks equal to the specification, exactly; a dropped crop's output is its input row bit for bit"""
    for b in (14, 13, 12):
        keep = sh.head_train_tap(f"b{b}.keep", n)
        if spec is None:
            assert np.array_equal(keep, np.ones(n, np.float32)), b
            continue
        scale = np.float32(1.0 / (1.0 - float(np.float32(C.RATES[b]))))
        assert np.array_equal(keep, np.where(spec[b], scale, np.float32(0))), b
        out, below = sh.head_train_tap(f"b{b}.out", n), sh.head_train_tap(f"b{b - 1}.out", n)     # b11.out is block 12's input
        for i in range(n):
            assert np.array_equal(out[i].view(np.uint32), below[i].view(np.uint32)) == (not spec[b][i]), (b, i)


# --------------------------------------------------------------------------- 1. single accumulates
@pytest.mark.parametrize("kind,n,variant,rates", C.single_cases())
def test_one_accumulate_matches_float64(pkg, sh, real_rows, kind, n, variant, rates):
    seed, tseed = C.case_seeds(kind, n, rates)
    x = real_rows[:n] if kind == "real" else B1.synthetic_rows(seed + 100, n)
    spec = C.masks(tseed, 0, n) if rates == "ref" else None
    try:
        o64, o32, rec = _one_accumulate(pkg, sh, x, seed, tseed, variant, rates)
        _check_keeps(sh, n, spec)
        for k in B1.float_taps():                               # the five b11.* taps, then every tap of the blocks above
            got = sh.head_train_tap(k, n)
            assert got.shape == tuple(o64.taps[k].shape), k
            _check(k, got, o64.taps[k].numpy(), o32.taps[k].numpy(), rec)
        _compare_state(sh, o64, o32, rec)
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 2. what block 12 hands down
def test_block_12_all_dropped_hands_its_dout_down_unchanged(pkg, sh, real_rows):
    """every crop of block 12 dropped at n = 2 (blocks 13 and 14 keep both): dX12 = dOut12 + 0, so b11.dout == b12.dout
    element for element, block 12's gradients are exactly zero and block 11 still trains"""
    n, x = 2, real_rows[:2]
    spec = C.masks(C.DROP12_SEED, 0, n)
    assert not spec[12].any() and spec[13].all() and spec[14].all()
    try:
        o64, o32, rec = _one_accumulate(pkg, sh, x, C.DROP_SEED, C.DROP12_SEED, "plain", "ref")
        _check_keeps(sh, n, spec)
        d11, d12 = sh.head_train_tap("b11.dout", n), sh.head_train_tap("b12.dout", n)
        assert (d11 == d12).all() and np.abs(d12).max() > 0                       # element for element (-0.0 + 0.0 allowed)
        assert np.array_equal(sh.head_train_tap("b12.out", n), sh.head_train_tap("b11.out", n))
        g, g64 = _all_grads(sh), o64.grads()
        for k in BO.BLOCK_GRAD_FIELDS:
            assert not g["b12." + k].any() and not g64["b12." + k].any(), k       # exactly zero, on the device and in the oracle
            for b in (15, 14, 13, 11):
                assert g[f"b{b}." + k].any(), (b, k)
        for k in B1.float_taps():
            if not k.startswith("b12.") or k in ("b12.out", "b12.dout"):
                _check(k, sh.head_train_tap(k, n), o64.taps[k].numpy(), o32.taps[k].numpy(), rec)
        _compare_state(sh, o64, o32, rec, skip_grads=("b12.",))
        _assert_all(rec)
    finally:
        sh.head_train_end()


def test_with_masks_b11_dout_is_block_12s_sum(pkg, sh, real_rows):
    """b11.dout against dOut12 + dZe12 . We12 restated in closed form from the DEVICE's own taps and parameters"""
    n = 11
    seed, tseed = C.case_seeds("real", n, "ref")
    below = C.start()[1]
    try:
        o64, o32, rec = _one_accumulate(pkg, sh, real_rows[:n], seed, tseed, "plain", "ref")
        rows12 = sh.head_train_tap("b11.out", n)
        dout, dae = sh.head_train_tap("b12.dout", n), sh.head_train_tap("b12.dae", n)
        want = B2.skip_input_gradient(rows12, below[12], dout, dae).reshape(n, 49, 192)
        got = sh.head_train_tap("b11.dout", n)
        err = np.abs(got - want).max() / np.abs(want).max()
        branch = np.abs(want - dout).max() / np.abs(want).max()
        print(f"b11.dout against b12.dout + dZe12 . We12 from the device's taps: max rel {err:.3e}; the branch is {branch:.3f} of it")
        # as tests/test_block12_train_gpu.py: dae is stored in fp32 and passes a BatchNorm backward and a 1152-term sum
        assert err <= 1e-5 and branch > 1e-3 and not np.array_equal(got, dout)
        _check("b11.dout", got, o64.taps["b11.dout"].numpy(), o32.taps["b11.dout"].numpy(), rec)
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 3. accumulation and apply
def test_two_accumulates_add_up(pkg, sh, stress_sd, real_rows):
    seed = C.ACC_SEED
    head = O.default_params(seed)
    sd = dict(stress_sd)
    sd.update({k: head[f] for k, f in T.KEYS.items()})
    with T.HeadTrainer(sh, sd, max_n=16, seed=C.ACC_MASK_SEED, train_block11=True) as tr:
        assert tr.train_block11 and tr.train_block12 and tr.train_block13 and tr.train_block14 and tr.train_block15 and tr.train_conv_head
        assert tr.row_width == 21952 and tr.extract_method == "train_augment_rows11"
        o64, o32, ost = C.oracles(head, O.config_values(tr.config), "ref")
        for k, x in enumerate((real_rows[:16], real_rows[16:21])):
            y = C.labels(seed + 400 + k, x.shape[0])
            losses = tuple(o.accumulate(x, y, None, 1.0, 0.5)[0] for o in (o64, o32, ost))
            _preconditions(o64, o32, ost, losses, y, what=f", accumulate {k}:")
            tr.accumulate(x.reshape(x.shape[0], -1), y, None, 1.0, 0.5)        # both row layouts are taken
            spec = C.masks(C.ACC_MASK_SEED, k, x.shape[0])                      # the second call's masks use counter 1
            for b in spec:
                assert np.array_equal(sh.head_train_tap(f"b{b}.keep", x.shape[0]) != 0, spec[b]), (k, b)
        rec = []
        _compare_state(sh, o64, o32, rec)                       # gradients of every group, running statistics of all BatchNorms
        _assert_all(rec)
        exported = tr.export_state_dict()
        for k in T.BLOCK11_TRACKED + T.BLOCK12_TRACKED + T.BLOCK13_TRACKED + T.BLOCK14_TRACKED + T.BLOCK_TRACKED + (T.CONV_TRACKED,) + T.TRACKED:
            assert int(exported[k]) == int(np.asarray(stress_sd[k])) + 2, k
        assert set(T.BLOCK11_KEYS) | set(T.BLOCK12_KEYS) | set(T.BLOCK_KEYS) <= set(exported)
        assert exported["net._blocks.11._depthwise_conv.weight"].shape == (672, 1, 5, 5)
        assert exported["net._blocks.11._expand_conv.weight"].shape == (672, 112, 1, 1)


def _force(h, g):
    h.head_train_grads(set_to={k: g[k] for k in O.GRAD_FIELDS})
    h.head_train_conv_grads(set_to={k: g["conv." + k] for k in CO.CONV_GRAD_FIELDS})
    for b in BLOCKS:
        h.head_train_block_grads_at(b, set_to={k: g[f"b{b}." + k] for k in BO.BLOCK_GRAD_FIELDS})


@pytest.mark.parametrize("clip_norm", [1.0e4, 1.0])            # the forced norm is ~5e2: coefficient 1, and far above the clip
def test_apply_steps_every_group_at_its_rate_under_one_norm(pkg, sh, clip_norm):
    """Three forced applies.  One norm over seven arenas: the forced gradients give each arena a share of the squared norm in
    proportion to its size, so a norm without block 11's arena is sqrt(3682241 / 3944733) = 0.966 of the true one.  The norms
    must agree to 1e-5, so the norm without the arena must lie below 0.98 of it: 2 % is two thousand times the agreement
    asked for, and the forced gradients' squares average the same over every tensor to well under 1 %.  Under clip_norm = 1
    every parameter of every group is scaled by 1 / norm.  Block 11 steps at 0.1 x the head's rate, as the oracle's groups do."""
    assert sum(COUNTS.values()) == 3944733
    head = O.default_params(3)
    cfg = _open(pkg, sh, head, max_n=16, seed=0, clip_norm=clip_norm)
    try:
        o64, o32 = C.oracles(head, cfg, n=2)
        rec = []
        for step, lr in enumerate((3e-4, 1.2e-5, 1e-3)):
            lr = float(np.float32(lr))
            g = C.forced_grads(50 + step)
            assert sum(v.size for k, v in g.items() if k.startswith("b11.")) == COUNTS[11] and sum(v.size for v in g.values()) == 3944733
            _force(sh, g)
            o64.set_grads(g)
            o32.set_grads(g)
            n64, n32 = o64.apply(lr), o32.apply(lr)
            norm = sh.head_train_apply(lr)
            assert (n64 < clip_norm) == (clip_norm > 1.0)
            _check(f"grad norm, step {step}", [norm], [n64], [n32], rec)
            sq_new = sum(float((v.astype(np.float64) ** 2).sum()) for k, v in g.items() if k.startswith("b11."))
            total = sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values())
            print(f"step {step}: norm {norm:.4f}, all seven arenas {np.sqrt(total):.4f}, without block 11's arena {np.sqrt(total - sq_new):.4f}")
            assert abs(norm - np.sqrt(total)) <= 1e-5 * np.sqrt(total)
            assert np.sqrt(total - sq_new) < 0.98 * norm
            assert all(not v.any() for v in _all_grads(sh).values())          # zeroed exactly, every group
        for ema in (False, True):
            e, e64, e32 = _all_export(sh, ema), o64.export(ema), o32.export(ema)
            for k in GRAD_KEYS:
                _check(("ema " if ema else "param ") + k, e[k], e64[k], e32[k], rec)
        _assert_all(rec)
        if clip_norm > 1.0:                                     # block 11's rate made explicit: 0.1 x the head's
            w0 = C.start()[0]["exp_w"].astype(np.float64)
            moved, at_scale = (np.abs(w - w0).mean() for w in (_all_export(sh)["b11.exp_w"], o64.export()["b11.exp_w"]))
            head_moved = np.abs(_all_export(sh)["w1"] - head["w1"].astype(np.float64)).mean()
            print(f"mean |step| of b11.exp_w: device {moved:.4e}, oracle {at_scale:.4e}; of the head's w1 {head_moved:.4e}")
            assert abs(moved - at_scale) <= 1e-3 * at_scale and head_moved > 5.0 * moved
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 4. eval
def test_eval_block_matches_float64_and_ignores_the_chunking(pkg, sh, real_rows):
    seed = C.EVAL_SEED
    head, x = O.default_params(seed), real_rows[:5]
    cfg = _open(pkg, sh, head, "ref", max_n=16, seed=C.DROP12_SEED, clip_norm=1.0e4, ema_decay=0.5)
    try:
        o64, o32 = C.oracles(head, cfg, "ref", n=2)
        g = C.forced_grads(70)
        _force(sh, g)
        o64.set_grads(g)
        o32.set_grads(g)
        lr = float(np.float32(1e-3))
        o64.apply(lr), o32.apply(lr), sh.head_train_apply(lr)  # live and EMA parameters differ from here on
        stats = {k: v for k, v in _all_export(sh).items() if k in STAT_KEYS}
        rec, seen = [], []
        for ema in (False, True):
            z64, z32 = o64.evaluate(x, ema), o32.evaluate(x, ema)
            margin = B1.gate_margin(o64, o32)
            print(f"gate margin, use_ema={ema}: {margin:.2f}")
            assert margin >= 1.0
            whole = sh.head_train_eval_block(x, ema)
            _check(f"eval logits, use_ema={ema}", whole, z64, z32, rec)      # eval applies no drop-connect (the trainer seed drops block 12 at n = 2)
            parts = np.concatenate([sh.head_train_eval_block(x[i:i + 2], ema) for i in range(0, 5, 2)])
            assert np.array_equal(whole, parts)                 # n = 5 equals 2 + 2 + 1: running statistics, no batch in them
            seen.append(whole)
        assert not np.array_equal(seen[0], seen[1])
        after = _all_export(sh)
        for k in stats:
            assert np.array_equal(after[k], stats[k]), k       # eval leaves the running statistics alone
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 5. commit
def test_commit_swaps_all_five_blocks_conv_and_head_in_place(pkg, stress_sd, real_rows):
    imgs = B.random_crops(2, 7)
    L = pkg._lib
    blob = pkg.weights.pack_b0(stress_sd)
    h, never = L.Handle(blob, device=0, max_batch=2), L.Handle(blob, device=0, max_batch=2)
    modes = [(bf, k5) for bf in (0, 1) for k5 in (1, 0)]       # bf16 activations; block 11's per-image launch on and off

    def outputs(handle, mode):
        bf, k5 = mode
        handle.set_option("bf16_activations", bf)
        handle.set_option("fuse_k5", k5)
        handle.set_option("fuse_k5_min", 1)                    # the per-image launch at any batch size, so 2 crops reach it
        try:
            return handle.classify(imgs).copy()
        finally:
            handle.set_option("bf16_activations", 0)
            handle.set_option("fuse_k5", 1)
            handle.set_option("fuse_k5_min", 0)

    try:
        before = {mode: outputs(h, mode) for mode in modes}    # also builds the cached weight splits
        rows11 = h.extract_block_rows(imgs, 11)
        with T.HeadTrainer(h, stress_sd, train_block11=True, max_n=16, seed=4, ema_decay=0.5) as tr:
            for k in range(2):
                tr.accumulate(real_rows[k:k + 16], C.labels(20 + k, 16))
                tr.apply(1e-3)
            for mode in modes:                                 # an open, trained, uncommitted trainer changes nothing
                assert np.array_equal(outputs(h, mode), before[mode]) and np.array_equal(outputs(never, mode), before[mode])
            for ema in (False, True):
                tr.commit(use_ema=ema)
                sd = dict(stress_sd)
                exported = tr.export_state_dict(use_ema=ema)
                for b in BLOCKS:
                    k = f"net._blocks.{b}._bn2.num_batches_tracked"
                    assert int(exported[k]) == int(np.asarray(stress_sd[k])) + 2, k
                sd.update(exported)
                fresh = L.Handle(pkg.weights.pack_b0(sd), device=0, max_batch=2)
                try:
                    for mode in modes:
                        got, want = outputs(h, mode), outputs(fresh, mode)
                        print(f"use_ema={ema} (bf16, fuse_k5)={mode}: before {before[mode].ravel()} committed {got.ravel()} fresh {want.ravel()}")
                        assert np.array_equal(got, want) and not np.array_equal(got, before[mode])
                    for b in (12, 13, 14, 15):                  # the output of every committed block below, block 11's first
                        got_b, want_b = h.extract_block_rows(imgs, b), fresh.extract_block_rows(imgs, b)
                        assert np.array_equal(got_b, want_b), b
                    assert np.array_equal(fresh.extract_block_rows(imgs, 11), rows11)
                finally:
                    fresh.close()
                assert np.array_equal(h.extract_block_rows(imgs, 11), rows11)    # block 10 and everything below are untouched
            for k in ("_expand_conv.weight", "_depthwise_conv.weight", "_se_expand.bias", "_bn1.weight", "_project_conv.weight"):
                k = f"net._blocks.11.{k}"
                assert not np.array_equal(exported[k], np.asarray(stress_sd[k])), k
        assert np.array_equal(outputs(never, modes[0]), before[modes[0]])
    finally:
        h.close()
        never.close()


# --------------------------------------------------------------------------- 6. extraction
def test_extract_block_rows_is_the_tap_of_the_block_below(pkg, sh):
    x = B.random_crops(5, 3)
    xd = sh.alloc(x.nbytes).upload(x)
    try:
        for mode in (0, 1):
            sh.set_option("bf16_activations", mode)
            for b in (11, 12, 13, 14, 15):
                got = sh.extract_block_rows(x, b)
                shape = (5, 14, 14, 112) if b == 11 else (5, 7, 7, 192)
                want = sh.tap(xd.ptr, 5, f"b{b - 1}.out", int(np.prod(shape)))
                assert got.shape == shape and want.size == np.prod(shape)
                assert np.array_equal(got.ravel(), want) and np.abs(got).max() > 0, (mode, b)
                if b >= 12:                                 # the older entry's bits
                    assert np.array_equal(got, sh.extract_block_input(x, b)), (mode, b)
    finally:
        sh.set_option("bf16_activations", 0)
        xd.free()
    for block in (10, 16, 0, -1):
        with pytest.raises(pkg._lib.DfdError) as e:
            sh.extract_block_rows(x, block)
        assert e.value.code == -1 and len(str(e.value)) > 30
    with pytest.raises(pkg._lib.DfdError) as e:
        sh.extract_block_input(x, 11)                          # the older entry keeps refusing block 11
    assert e.value.code == -1
    with pytest.raises(pkg._lib.DfdError):
        sh.extract_block_rows(B.random_crops(17, 3), 11)       # n > max_batch is the caller's chunking
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, seed=0)
    try:
        got = m.extract_block_rows(x, 11)                      # chunks of 2, 2, 1
        want = np.concatenate([m.handle.extract_block_rows(x[i:i + 2], 11) for i in range(0, 5, 2)])
        assert got.shape == (5, 14, 14, 112) and np.array_equal(got, want)
        assert np.array_equal(m.extract_block_rows(x, 12), m.extract_block_input(x, 12))
    finally:
        m.handle.close()


def test_train_augment_block_rows_equals_augment_then_extract(pkg, seeded_sd):
    h = pkg._lib.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=2)
    try:
        rgb = np.random.RandomState(8).randint(0, 256, (5, 64, 96, 3)).astype(np.uint8)
        rows, batch = TA.draw_batch(TA.AugmentPolicy(), np.random.RandomState(6), 5, 64, 96, 224,
                                    mix=(TA.MIX_MIXUP, 0.8, np.array([4, 3, 0, 1, 2])))
        x = h.train_augment(rgb, rows, batch, 224)
        buf = h.alloc(rgb.nbytes).upload(rgb)
        try:
            for b in (11, 12, 13, 14, 15):
                want = np.concatenate([h.extract_block_rows(x[i:i + 2], b) for i in range(0, 5, 2)])
                got = h.train_augment_block_rows(rgb, rows, batch, block=b)                    # uploaded; chunks of 2, 2, 1
                assert got.shape == ((5, 14, 14, 112) if b == 11 else (5, 7, 7, 192)) and np.array_equal(got, want), b
                assert np.array_equal(h.train_augment_block_rows(buf, rows, batch, block=b, shape=rgb.shape[:3]), want), b    # resident
                if b >= 12:
                    assert np.array_equal(got, h.train_augment_block_input(rgb, rows, batch, block=b)), b
            assert np.array_equal(h.train_augment_rows11(rgb, rows, batch), h.train_augment_block_rows(rgb, rows, batch, block=11))
        finally:
            buf.free()
        for block in (10, 16):
            with pytest.raises(pkg._lib.DfdError) as e:
                h.train_augment_block_rows(rgb, rows, batch, block=block)
            assert e.value.code == -1 and len(str(e.value)) > 30
        with pytest.raises(pkg._lib.DfdError) as e:
            h.train_augment_block_input(rgb, rows, batch, block=11)
        assert e.value.code == -1
    finally:
        h.close()


# --------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_handle_usable(pkg, sh):
    L = pkg._lib
    b11, below, b14, b15, conv = C.start()
    b13, b12 = below[13], below[12]
    head, x, y = O.default_params(0), B1.synthetic_rows(0, 4), C.labels(0, 4)
    x12 = B2.synthetic_rows(0, 4)

    def refused(fn, *a, code=-1, **k):
        with pytest.raises(L.DfdError) as e:
            fn(*a, **k)
        assert e.value.code == code and len(str(e.value)) > 30, str(e.value)    # the documented code with a message

    refused(sh.head_train_unfreeze_block_at, b11, 11, drop_connect=0.0)         # no trainer is open
    sh.head_train_begin(head, L.head_config(max_n=4))
    try:
        sh.head_train_unfreeze_conv(conv)
        sh.head_train_unfreeze_block(b15)
        refused(sh.head_train_unfreeze_block_at, b11, 11, drop_connect=0.0, code=-7)     # 12 is frozen: DFD_ERR_UNSUPPORTED
        sh.head_train_unfreeze_block_at(b14, 14)
        sh.head_train_unfreeze_block_at(b13, 13)
        refused(sh.head_train_unfreeze_block_at, b11, 11, drop_connect=0.0, code=-7)     # 12 comes before 11
        refused(sh.head_train_export_block_at, 11, code=-7)                     # frozen 11: DFD_ERR_UNSUPPORTED, as 13 and 12
        refused(sh.head_train_block_grads_at, 11, code=-7)
        for other in (10, 16, 0):
            refused(sh.head_train_unfreeze_block_at, b11, other, drop_connect=0.0, code=-7)      # blocks outside 11..14
            refused(sh.head_train_export_block_at, other, code=-7)
        sh.head_train_unfreeze_block_at(b12, 12)
        sh.head_train_accumulate_block(x12, y)                                  # the depth-12 trainer still works
        for name in B1.TAPS + ("b11.keep",):
            refused(sh.head_train_tap, name, 4)                                 # the b11 taps without the stage
        refused(sh.head_train_unfreeze_block_at, b11, 11, drop_connect=0.0)     # after an accumulate
    finally:
        sh.head_train_end()
    sh.head_train_begin(head, L.head_config(max_n=4))
    try:
        sh.head_train_unfreeze_conv(conv)
        sh.head_train_unfreeze_block(b15)
        for b, p in ((14, b14), (13, b13), (12, b12)):
            sh.head_train_unfreeze_block_at(p, b, drop_connect=C.RATES[b])
        for bad in (0.15, 1.0, -0.1, float("nan")):
            refused(sh.head_train_unfreeze_block_at, b11, 11, drop_connect=bad) # block 11 has no skip: only 0
        refused(sh.head_train_unfreeze_block_at, b11, 11, drop_connect=0.0, bn_eps=0.0)
        refused(sh.head_train_export_block_at, 11, code=-7)
        sh.head_train_unfreeze_block_at(b11, 11, drop_connect=0.0)
        refused(sh.head_train_unfreeze_block_at, b11, 11, drop_connect=0.0)     # a second time
        assert sh.head_train_export_block_at(11)["dw_w"].shape == (672, 5, 5)
        refused(sh.head_train_accumulate_block, x[:1], y[:1])                   # n < 2
        refused(sh.head_train_accumulate_block, B1.synthetic_rows(0, 5), C.labels(0, 5))     # n > max_n
        refused(sh.head_train_tap, "b11.ad", 4)                                 # nothing accumulated yet
        loss, logits = sh.head_train_accumulate_block(x, y)
        assert np.isfinite(loss) and np.isfinite(logits).all()
        assert sh.head_train_tap("b11.ad", 4).shape == (4, 49, 672) and sh.head_train_tap("b11.dae", 4).shape == (4, 196, 672)
        assert sh.head_train_tap("b11.out", 4).shape == (4, 49, 192) and sh.head_train_tap("b11.gate", 4).shape == (4, 672)
        refused(sh.head_train_tap, "b11.keep", 4)                               # no skip, no mask
        refused(sh.head_train_tap, "b11.nothing", 4)
        refused(sh.head_train_tap, "b10.out", 4)
        assert np.isfinite(sh.head_train_apply(1e-3)) and np.isfinite(sh.head_train_eval_block(x[:1])).all()
        assert np.array_equal(sh.head_train_export_block_at(11)["rm2"].shape, (192,))
    finally:
        sh.head_train_end()
    refused(sh.head_train_export_block_at, 11)                                  # after end: no trainer
    assert np.isfinite(sh.classify(B.random_crops(1, 0))).all()
    # dfd_destroy with an open trainer and all six stages frees everything
    h = L.Handle(pkg.weights.pack_b0(pkg.weights.seeded_state_dict(0)), device=0, max_batch=1)
    h.head_train_begin(head, L.head_config(max_n=4))
    h.head_train_unfreeze_conv(conv)
    h.head_train_unfreeze_block(b15)
    for b, p in ((14, b14), (13, b13), (12, b12)):
        h.head_train_unfreeze_block_at(p, b)
    h.head_train_unfreeze_block_at(b11, 11, drop_connect=0.0)
    h.head_train_accumulate_block(x, y)
    h.close()


# --------------------------------------------------------------------------- 8. after the trainer
def test_classify_after_a_depth_11_trainer_gives_a_fresh_handles_bits(pkg, stress_sd, real_rows):
    """tests/test_call_history_gpu.py's rule: a trainer that ran and ended without commit leaves no trace"""
    L = pkg._lib
    blob = pkg.weights.pack_b0(stress_sd)
    imgs = B.random_crops(3, 11)
    fresh = L.Handle(blob, device=0, max_batch=4)
    try:
        want = fresh.classify(imgs).copy()
    finally:
        fresh.close()
    h = L.Handle(blob, device=0, max_batch=4)
    try:
        _open(pkg, h, O.default_params(1), "ref", max_n=8, seed=3)
        try:
            h.head_train_accumulate_block(real_rows[:8], C.labels(1, 8))
            h.head_train_apply(1e-3)
            h.head_train_eval_block(real_rows[:3])
        finally:
            h.head_train_end()
        assert np.array_equal(h.classify(imgs), want)
    finally:
        h.close()


# --------------------------------------------------------------------------- 9. fit_head
def test_fit_head_with_block11_and_augmentation(pkg):
    """DeepfakeEfficientNet.fit_head(train_block11=True, augment=policy): uint8 crops, every batch through
    `train_augment_block_rows(block=11)`; all seven groups committed on the SAME handle"""
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=4, seed=0)
    try:
        crops = np.random.RandomState(5).randint(0, 256, (12, 48, 48, 3)).astype(np.uint8)
        y = (np.arange(12) % 2).astype(np.float32)
        key = "net._blocks.11._expand_conv.weight"
        x = B.random_crops(2, 1)
        handle, w0, out0, in0 = m.handle, np.array(m.state_dict()[key]), m.extract_block_rows(x, 12).copy(), m.extract_block_rows(x, 11).copy()
        log = m.fit_head(crops, y, epochs=2, batch_size=6, grad_accum=1, lr=1e-3, train_block11=True, augment=TA.AugmentPolicy(),
                         rng=np.random.RandomState(2), trainer_config={"ema_decay": 0.5})
        assert len(log) == 2 and m.handle is handle
        assert all(np.isfinite(e["train_loss"]) and np.isfinite(e["lr"]) and np.isfinite(e["train_acc"]) for e in log)
        w1 = np.array(m.state_dict()[key])
        assert w1.shape == w0.shape == (672, 112, 1, 1) and not np.array_equal(w1, w0)
        # the commit changed b11.exp.w on the handle: block 11's output moved, its input did not
        assert not np.array_equal(m.extract_block_rows(x, 12), out0) and np.array_equal(m.extract_block_rows(x, 11), in0)
        assert int(m.state_dict()["net._blocks.11._bn0.num_batches_tracked"]) == 4
        fresh = pkg._lib.Handle(pkg.weights.pack_b0(m.state_dict()), device=0, max_batch=4)
        try:
            assert np.array_equal(fresh.classify(x), m.handle.classify(x))
        finally:
            fresh.close()
    finally:
        m.handle.close()

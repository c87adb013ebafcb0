"""GPU: blocks 13 and 12 of the head trainer (csrc/head_train_block.hip: dfd_head_train_unfreeze_block_at at 13 and 12, the
_block entries on the input rows of the deepest block, _export_block_at / _block_grads_at, the "b13.*" / "b12.*" taps, the
gradient a skip block hands down, the six-arena dfd_head_train_apply and _commit) and the extraction of block inputs
(dfd_extract_block_input, dfd_train_augment_block_input) against the float64 oracle of tests/block12_train_oracle.py, at
depth 13 (blocks 13..15) and depth 12 (blocks 12..15).

Bars: as tests/test_block14_train_gpu.py - every compared tensor's rms(d) / rms(ref) and max|d| / max|ref| against the
float64 oracle at most 4 x / 8 x the same metrics of the float32 CPU oracle, floored at 2^-23 / 2^-21 (`O.bar_ratio` <= 1).
Every figure is printed before it is asserted.

Inputs: "real" rows are `extract_block_input(x, depth)` of b0_layer_oracle.stress_state_dict weights on random_crops (all
blocks, conv stage and head start from the same state dict); "synthetic" rows are standard normals.  max_n = 64.

Preconditions, all on the oracles alone and asserted before the device is looked at: `gate_margin` >= 1, `rounding_share`
<= 1 and `storage_share` <= 0.5.  Sizes, variants, rates, trainer seeds (the masks) and parameter seeds are the table of
tests/block12_train_cases.py, picked on the CPU; tests/test_block12_train_oracle.py runs the same preconditions without a
device and RECORDS the masks.

m = 49 n rows: 98 (under one chunk, no multiple of 16), 539 (one 512-row chunk and a remainder, two 256-row chunks and a
remainder), 1813 (ragged, five 8-crop depthwise partials with a short last one), 3136 (synthetic; 64 crops are max_n).

With every crop kept the gradient of a skip block's _bn2 bias is the column sum of the gradient arriving at the block, zero
in exact arithmetic for blocks 14, 13 and 12 alike: dOut14 = dZe15 . We15 and every branch term dZe_b . We_b have zero
column sums (a train-mode BN0 removes a per-channel constant), and so has their sum.  Reference, yardstick and device hold
rounding noise there, and the bar compares the device's noise with the yardstick's as it compares everything else.
"""
import numpy as np
import pytest

import b0_layer_oracle as B
import block12_history  # noqa: F401  (registers the new exports and their case with the call-history table)
import block12_train_cases as C
import block12_train_oracle as B2
import block15_train_oracle as BO
import head_train_oracle as O
import headconv_train_oracle as CO
from rtdfd_amd import head_training as T
from rtdfd_amd import train_augment as TA

pytestmark = pytest.mark.gpu

MAX_N = C.MAX_N


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
    """{depth: the input rows of block `depth`}, computed once"""
    x = B.random_crops(C.ROW_CROPS, C.ROW_SEED)
    return {d: np.concatenate([sh.extract_block_input(x[i:i + 16], d) for i in range(0, C.ROW_CROPS, 16)]) for d in C.DEPTHS}


def _open(pkg, h, depth, head, rates="zero", **kw):
    below, b14, b15, conv = C.start(depth)
    p14, drops = C.rates_of(depth, rates)
    cfg = pkg._lib.head_config(**kw)
    h.head_train_begin(head, cfg)
    try:
        h.head_train_unfreeze_conv(conv)
        h.head_train_unfreeze_block(b15)
        h.head_train_unfreeze_block_at(b14, 14, drop_connect=p14)
        for b in sorted(below, reverse=True):
            h.head_train_unfreeze_block_at(below[b], b, drop_connect=drops[b])
    except Exception:
        h.head_train_end()
        raise
    return O.config_values(cfg)


def _oracles(depth, head, cfg, rates="zero", n=3):
    below, b14, b15, conv = C.start(depth)
    p14, drops = C.rates_of(depth, rates)
    make = B2.triple if n == 3 else B2.pair
    return make(below, b14, b15, conv, head, cfg, drop_connect=p14, drops=drops)


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


def _blocks(depth):
    return (15,) + C.blocks_of(depth)


def _all_grads(h, depth):
    g = dict(h.head_train_grads())
    g.update({"conv." + k: v for k, v in h.head_train_conv_grads().items()})
    for b in _blocks(depth):
        g.update({f"b{b}." + k: v for k, v in h.head_train_block_grads_at(b).items()})
    return g


def _all_export(h, depth, ema=False):
    e = dict(h.head_train_export(ema))
    e.update({"conv." + k: v for k, v in h.head_train_export_conv(ema).items()})
    for b in _blocks(depth):
        e.update({f"b{b}." + k: v for k, v in h.head_train_export_block_at(b, ema).items()})
    return e


def _grad_keys(depth):
    return tuple(f"b{b}." + k for b in _blocks(depth) for k in BO.BLOCK_GRAD_FIELDS) + tuple("conv." + k for k in CO.CONV_GRAD_FIELDS) + O.GRAD_FIELDS


def _stat_keys(depth):
    return tuple(f"b{b}." + k for b in _blocks(depth) for k in BO.BLOCK_STAT_FIELDS) + tuple("conv." + k for k in CO.CONV_STAT_FIELDS) + O.STAT_FIELDS


def _compare_state(h, depth, o64, o32, rec, skip_grads=()):
    g, g64, g32 = _all_grads(h, depth), o64.grads(), o32.grads()
    for k in _grad_keys(depth):
        if not k.startswith(skip_grads or ("\0",)):
            _check("grad " + k, g[k], g64[k], g32[k], rec)
    e, e64, e32 = _all_export(h, depth), o64.export(), o32.export()
    for k in _stat_keys(depth):
        _check(k, e[k], e64[k], e32[k], rec)


def _preconditions(o64, o32, ost, losses, ya, yb=None, lam=1.0, what=""):
    margin, rshare, sshare, worst = C.preconditions(o64, o32, ost, losses, ya, yb, lam)
    print(f"gate margin{what} {margin:.2f}, rounding share {rshare:.3f}, storage share {sshare:.3f} ({worst})")
    assert margin >= 1.0 and rshare <= 1.0 and sshare <= 0.5    # conditions on the inputs, checked on the oracles alone


def _one_accumulate(pkg, sh, depth, x, seed, trainer_seed, variant, rates):
    """one accumulate on the device and the three oracles -> (o64, o32, the record so far)"""
    head, ya, yb, lam, scale = C.case_inputs(seed, x.shape[0], variant)
    cfg = _open(pkg, sh, depth, head, rates, max_n=MAX_N, seed=trainer_seed)
    o64, o32, ost = _oracles(depth, head, cfg, rates)
    (l64, z64), (l32, z32), (lst, _) = (o.accumulate(x, ya, yb, lam, scale) for o in (o64, o32, ost))
    _preconditions(o64, o32, ost, (l64, l32, lst), ya, yb, lam)
    loss, logits = sh.head_train_accumulate_block(x, ya, yb, lam, scale)
    rec = []
    _check("loss", [loss], [l64], [l32], rec)
    _check("logits", logits, z64, z32, rec)
    return o64, o32, rec


def _check_keeps(sh, depth, n, x, spec):
    """`b*.keep` equal to the specification, exactly; a dropped crop's output is its input row bit for bit"""
    for b in C.blocks_of(depth):
        keep = sh.head_train_tap(f"b{b}.keep", n)
        if spec is None:
            assert np.array_equal(keep, np.ones(n, np.float32)), b
            continue
        scale = np.float32(1.0 / (1.0 - float(np.float32(C.RATES[b]))))
        assert np.array_equal(keep, np.where(spec[b], scale, np.float32(0))), b
        out = sh.head_train_tap(f"b{b}.out", n)
        below = x.reshape(n, 49, 192) if b == depth else sh.head_train_tap(f"b{b - 1}.out", n)
        for i in range(n):
            assert np.array_equal(out[i].view(np.uint32), below[i].view(np.uint32)) == (not spec[b][i]), (b, i)


# --------------------------------------------------------------------------- 1. single accumulates
@pytest.mark.parametrize("depth,kind,n,variant,rates", C.single_cases())
def test_one_accumulate_matches_float64(pkg, sh, real_rows, depth, kind, n, variant, rates):
    seed, tseed = C.case_seeds(depth, kind, n, rates)
    x = real_rows[depth][:n] if kind == "real" else B2.synthetic_rows(seed + 100, n)
    spec = C.masks(tseed, 0, n, depth) if rates == "ref" else None
    try:
        o64, o32, rec = _one_accumulate(pkg, sh, depth, x, seed, tseed, variant, rates)
        _check_keeps(sh, depth, n, x, spec)
        for k in B2.float_taps(depth):                          # every b12.* / b13.* tap, b14.dout among block 14's, block 15's taps
            _check(k, sh.head_train_tap(k, n), o64.taps[k].numpy(), o32.taps[k].numpy(), rec)
        _compare_state(sh, depth, o64, o32, rec)
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 2. the skip gradient alone
@pytest.mark.parametrize("depth", C.DEPTHS)
def test_the_gradient_handed_down_is_dout_plus_the_branch(pkg, sh, real_rows, depth):
    """b13.dout against dOut14 + dZe14 . We14 restated in closed form from the DEVICE's own taps and parameters (so only the
    new epilogue is under test), then every crop of block 13 dropped."""
    n = 11
    seed, tseed = C.case_seeds(depth, "real", n, "ref")
    x = real_rows[depth][:n]
    below, b14, _, _ = C.start(depth)
    try:
        o64, o32, rec = _one_accumulate(pkg, sh, depth, x, seed, tseed, "plain", "ref")
        for b in range(14, depth, -1):                          # block b hands down into b{b-1}.dout
            p = b14 if b == 14 else below[b]
            rows_b = sh.head_train_tap(f"b{b - 1}.out", n)
            dout, dae = sh.head_train_tap(f"b{b}.dout", n), sh.head_train_tap(f"b{b}.dae", n)
            want = B2.skip_input_gradient(rows_b, p, dout, dae).reshape(n, 49, 192)
            got = sh.head_train_tap(f"b{b - 1}.dout", n)
            err = np.abs(got - want).max() / np.abs(want).max()
            branch = np.abs(want - dout).max() / np.abs(want).max()
            print(f"b{b - 1}.dout against b{b}.dout + dZe{b} . We{b} from the device's taps: max rel {err:.3e}; the branch is {branch:.3f} of it")
            # dae is stored in fp32 (2^-24 relative) and passes a BatchNorm backward and a 1152-term sum: 1e-5 leaves room for
            # that and is far below either term of the sum
            assert err <= 1e-5 and branch > 1e-3 and np.abs(dout).max() > 1e-3 * np.abs(want).max()
            assert not np.array_equal(got, dout)
            _check(f"b{b - 1}.dout", got, o64.taps[f"b{b - 1}.dout"].numpy(), o32.taps[f"b{b - 1}.dout"].numpy(), rec)
        _assert_all(rec)
    finally:
        sh.head_train_end()
    n, x = 2, real_rows[depth][:2]
    spec = C.masks(C.DROP13_SEED, 0, n, depth)
    assert not spec[13].any() and spec[14].all()
    try:
        o64, o32, rec = _one_accumulate(pkg, sh, depth, x, C.DROP_SEED[depth], C.DROP13_SEED, "plain", "ref")
        _check_keeps(sh, depth, n, x, spec)
        g, g64 = _all_grads(sh, depth), o64.grads()
        for k in BO.BLOCK_GRAD_FIELDS:
            assert not g["b13." + k].any() and not g64["b13." + k].any(), k      # exactly zero, on the device and in the oracle
            for b in _blocks(depth):
                assert b == 13 or g[f"b{b}." + k].any(), (b, k)                   # the other blocks still get gradients
        e = _all_export(sh, depth)
        for k in BO.BLOCK_STAT_FIELDS:
            assert not np.array_equal(e["b13." + k], (below[13])[k]), k           # the statistics come before the mask
        if depth == 12:                                         # dX_13 == dOut_13 element for element (-0.0 + 0.0 allowed)
            d12, d13 = sh.head_train_tap("b12.dout", n), sh.head_train_tap("b13.dout", n)
            assert (d12 == d13).all() and np.abs(d13).max() > 0
        for k in B2.float_taps(depth):
            if not k.startswith("b13.") or k in ("b13.out", "b13.dout"):
                _check(k, sh.head_train_tap(k, n), o64.taps[k].numpy(), o32.taps[k].numpy(), rec)
        _compare_state(sh, depth, o64, o32, rec, skip_grads=("b13.",))
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 3. accumulation and apply
@pytest.mark.parametrize("depth", C.DEPTHS)
def test_two_accumulates_add_up(pkg, sh, stress_sd, real_rows, depth):
    seed = C.ACC_SEED[depth]
    head = O.default_params(seed)
    sd = dict(stress_sd)
    sd.update({k: head[f] for k, f in T.KEYS.items()})
    flags = {"train_block13": True} if depth == 13 else {"train_block12": True}
    with T.HeadTrainer(sh, sd, max_n=16, seed=C.ACC_MASK_SEED, **flags) as tr:
        assert tr.train_block13 and tr.train_block14 and tr.train_block15 and tr.train_conv_head and tr.row_width == 9408
        assert tr.train_block12 == (depth == 12) and tr.extract_method == f"train_augment_input{depth}"
        o64, o32, ost = _oracles(depth, head, O.config_values(tr.config), "ref")
        rows = real_rows[depth]
        for k, x in enumerate((rows[:16], rows[16:21])):
            y = C.labels(seed + 400 + k, x.shape[0])
            losses = tuple(o.accumulate(x, y, None, 1.0, 0.5)[0] for o in (o64, o32, ost))
            _preconditions(o64, o32, ost, losses, y, what=f", accumulate {k}:")
            tr.accumulate(x.reshape(x.shape[0], -1), y, None, 1.0, 0.5)        # both row layouts are taken
            spec = C.masks(C.ACC_MASK_SEED, k, x.shape[0], depth)              # the second call's masks use counter 1
            for b in spec:
                assert 0 < spec[b].sum() < x.shape[0]
                assert np.array_equal(sh.head_train_tap(f"b{b}.keep", x.shape[0]) != 0, spec[b]), (k, b)
        rec = []
        _compare_state(sh, depth, o64, o32, rec)                # gradients of every group, running statistics of all BatchNorms
        _assert_all(rec)
        exported = tr.export_state_dict()
        tracked = T.BLOCK13_TRACKED + T.BLOCK14_TRACKED + T.BLOCK_TRACKED + (T.CONV_TRACKED,) + T.TRACKED + (T.BLOCK12_TRACKED if depth == 12 else ())
        for k in tracked:
            assert int(exported[k]) == int(np.asarray(stress_sd[k])) + 2, k
        assert set(T.BLOCK13_KEYS) | set(T.BLOCK14_KEYS) | set(T.BLOCK_KEYS) <= set(exported)
        assert (set(T.BLOCK12_KEYS) <= set(exported)) == (depth == 12)
        assert exported["net._blocks.13._depthwise_conv.weight"].shape == (1152, 1, 5, 5)


def _forced_grads(pkg, depth, seed):
    """magnitudes log-uniform in [1e-4, 1], random signs: Adam's g / (sqrt(v) + eps) is well conditioned everywhere"""
    rs = np.random.RandomState(seed)
    shapes = {k: pkg._lib.HEAD_SHAPES[k] for k in O.GRAD_FIELDS}
    shapes.update({"conv." + k: pkg._lib.CONV_SHAPES[k] for k in CO.CONV_GRAD_FIELDS})
    shapes.update({"b15." + k: pkg._lib.BLOCK_SHAPES[k] for k in BO.BLOCK_GRAD_FIELDS})
    for b in C.blocks_of(depth):
        shapes.update({f"b{b}." + k: pkg._lib.BLOCK14_SHAPES[k] for k in BO.BLOCK_GRAD_FIELDS})
    return {k: (10.0 ** rs.uniform(-4.0, 0.0, s) * np.where(rs.rand(*s) < 0.5, -1.0, 1.0)).astype(np.float32) for k, s in shapes.items()}


def _force(h, depth, g):
    h.head_train_grads(set_to={k: g[k] for k in O.GRAD_FIELDS})
    h.head_train_conv_grads(set_to={k: g["conv." + k] for k in CO.CONV_GRAD_FIELDS})
    for b in _blocks(depth):
        h.head_train_block_grads_at(b, set_to={k: g[f"b{b}." + k] for k in BO.BLOCK_GRAD_FIELDS})


@pytest.mark.parametrize("clip_norm", [1.0e4, 1.0])            # the forced norm is ~5e2: coefficient 1, and far above the clip
@pytest.mark.parametrize("depth", C.DEPTHS)
def test_apply_steps_every_group_at_its_rate_under_one_norm(pkg, sh, depth, clip_norm):
    """Three forced applies.  One norm over five or six arenas: the forced gradients give each arena a share of the squared
    norm in proportion to its size, so a norm without the new arenas is sqrt(2506337 / 3094289) = 0.900 of the true one at
    depth 13 and sqrt(2506337 / 3682241) = 0.825 at depth 12 - below 0.95 where the norms must agree to 1e-5 - and under
    clip_norm = 1 every parameter of every group is scaled by 1 / norm.  The new blocks step at 0.1 x the head's rate, as the oracle's groups do."""
    head = O.default_params(3)
    cfg = _open(pkg, sh, depth, head, max_n=16, seed=0, clip_norm=clip_norm)
    new = tuple(f"b{b}." for b in range(depth, 14))
    try:
        o64, o32 = _oracles(depth, head, cfg, n=2)
        rec = []
        for step, lr in enumerate((3e-4, 1.2e-5, 1e-3)):
            lr = float(np.float32(lr))
            g = _forced_grads(pkg, depth, 50 + step)
            _force(sh, depth, g)
            o64.set_grads(g)
            o32.set_grads(g)
            n64, n32 = o64.apply(lr), o32.apply(lr)
            norm = sh.head_train_apply(lr)
            assert (n64 < clip_norm) == (clip_norm > 1.0)
            _check(f"grad norm, step {step}", [norm], [n64], [n32], rec)
            sq_new = sum(float((v.astype(np.float64) ** 2).sum()) for k, v in g.items() if k.startswith(new))
            total = sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values())
            print(f"step {step}: norm {norm:.4f}, all arenas {np.sqrt(total):.4f}, without the new arenas {np.sqrt(total - sq_new):.4f}")
            assert abs(norm - np.sqrt(total)) <= 1e-5 * np.sqrt(total)
            assert np.sqrt(total - sq_new) < 0.95 * norm
            assert all(not v.any() for v in _all_grads(sh, depth).values())          # zeroed exactly, every group
        for ema in (False, True):
            e, e64, e32 = _all_export(sh, depth, ema), o64.export(ema), o32.export(ema)
            for k in _grad_keys(depth):
                _check(("ema " if ema else "param ") + k, e[k], e64[k], e32[k], rec)
        _assert_all(rec)
        if clip_norm > 1.0:                                     # the deepest block's rate made explicit: 0.1 x the head's
            w0 = C.start(depth)[0][depth]["exp_w"].astype(np.float64)
            key = f"b{depth}.exp_w"
            moved, at_scale = (np.abs(w - w0).mean() for w in (_all_export(sh, depth)[key], o64.export()[key]))
            head_moved = np.abs(_all_export(sh, depth)["w1"] - head["w1"].astype(np.float64)).mean()
            print(f"mean |step| of {key}: device {moved:.4e}, oracle {at_scale:.4e}; of the head's w1 {head_moved:.4e}")
            assert abs(moved - at_scale) <= 1e-3 * at_scale and head_moved > 5.0 * moved
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 4. eval
@pytest.mark.parametrize("depth", C.DEPTHS)
def test_eval_block_matches_float64_and_ignores_the_chunking(pkg, sh, real_rows, depth):
    seed = C.EVAL_SEED[depth]
    head, x = O.default_params(seed), real_rows[depth][:5]
    cfg = _open(pkg, sh, depth, head, "ref", max_n=16, seed=C.DROP13_SEED, clip_norm=1.0e4, ema_decay=0.5)
    try:
        o64, o32 = _oracles(depth, head, cfg, "ref", n=2)
        g = _forced_grads(pkg, depth, 70)
        _force(sh, depth, g)
        o64.set_grads(g)
        o32.set_grads(g)
        lr = float(np.float32(1e-3))
        o64.apply(lr), o32.apply(lr), sh.head_train_apply(lr)  # live and EMA parameters differ from here on
        stats = {k: v for k, v in _all_export(sh, depth).items() if k in _stat_keys(depth)}
        rec, seen = [], []
        for ema in (False, True):
            z64, z32 = o64.evaluate(x, ema), o32.evaluate(x, ema)
            margin = B2.gate_margin(o64, o32)
            print(f"gate margin, use_ema={ema}: {margin:.2f}")
            assert margin >= 1.0
            whole = sh.head_train_eval_block(x, ema)
            _check(f"eval logits, use_ema={ema}", whole, z64, z32, rec)      # eval applies no drop-connect (the trainer seed drops block 13 at n = 2)
            parts = np.concatenate([sh.head_train_eval_block(x[i:i + 2], ema) for i in range(0, 5, 2)])
            assert np.array_equal(whole, parts)                 # n = 5 equals 2 + 2 + 1
            seen.append(whole)
        assert not np.array_equal(seen[0], seen[1])
        after = _all_export(sh, depth)
        for k in stats:
            assert np.array_equal(after[k], stats[k]), k       # eval leaves the running statistics alone
        _assert_all(rec)
    finally:
        sh.head_train_end()


# --------------------------------------------------------------------------- 5. commit
def test_commit_swaps_all_four_blocks_conv_and_head_in_place(pkg, stress_sd, real_rows):
    imgs = B.random_crops(2, 7)
    L = pkg._lib
    blob = pkg.weights.pack_b0(stress_sd)
    h, never = L.Handle(blob, device=0, max_batch=2), L.Handle(blob, device=0, max_batch=2)

    def outputs(handle, mode):
        handle.set_option("bf16_activations", mode)
        try:
            return handle.classify(imgs).copy()
        finally:
            handle.set_option("bf16_activations", 0)

    try:
        before = [outputs(h, mode) for mode in (0, 1)]         # also builds the cached weight splits
        rows12 = h.extract_block_input(imgs, 12)
        with T.HeadTrainer(h, stress_sd, train_block12=True, max_n=16, seed=4, ema_decay=0.5) as tr:
            for k in range(2):
                tr.accumulate(real_rows[12][k:k + 16], C.labels(20 + k, 16))
                tr.apply(1e-3)
            for mode in (0, 1):                                # an open, trained, uncommitted trainer changes nothing
                assert np.array_equal(outputs(h, mode), before[mode]) and np.array_equal(outputs(never, mode), before[mode])
            for ema in (False, True):
                tr.commit(use_ema=ema)
                sd = dict(stress_sd)
                exported = tr.export_state_dict(use_ema=ema)
                for b in (12, 13, 14, 15):
                    k = f"net._blocks.{b}._bn2.num_batches_tracked"
                    assert int(exported[k]) == int(np.asarray(stress_sd[k])) + 2, k
                sd.update(exported)
                fresh = L.Handle(pkg.weights.pack_b0(sd), device=0, max_batch=2)
                try:
                    for mode in (0, 1):
                        got, want = outputs(h, mode), outputs(fresh, mode)
                        print(f"use_ema={ema} bf16={mode}: before {before[mode].ravel()} committed {got.ravel()} fresh {want.ravel()}")
                        assert np.array_equal(got, want) and not np.array_equal(got, before[mode])
                    for b in (13, 14, 15):                      # the output of every committed block below
                        got_b, want_b = h.extract_block_input(imgs, b), fresh.extract_block_input(imgs, b)
                        assert np.array_equal(got_b, want_b) and not np.array_equal(got_b, rows12), b
                finally:
                    fresh.close()
                assert np.array_equal(h.extract_block_input(imgs, 12), rows12)   # block 11 and everything below are untouched
            for b in (12, 13):
                for k in ("_expand_conv.weight", "_depthwise_conv.weight", "_se_expand.bias", "_bn1.weight", "_project_conv.weight"):
                    k = f"net._blocks.{b}.{k}"
                    assert not np.array_equal(exported[k], np.asarray(stress_sd[k])), k
        assert np.array_equal(outputs(never, 0), before[0])
    finally:
        h.close()
        never.close()


# --------------------------------------------------------------------------- 6. extraction
def test_extract_block_input_is_the_tap_of_the_block_below(pkg, sh):
    x = B.random_crops(5, 3)
    xd = sh.alloc(x.nbytes).upload(x)
    try:
        for mode in (0, 1):
            sh.set_option("bf16_activations", mode)
            seen = []
            for b in (12, 13, 14, 15):
                got = sh.extract_block_input(x, b)
                want = sh.tap(xd.ptr, 5, f"b{b - 1}.out", 5 * 9408)
                assert got.shape == (5, 7, 7, 192) and want.size == 5 * 9408
                assert np.array_equal(got.ravel(), want) and np.abs(got).max() > 0, (mode, b)
                if b >= 14:                                 # the older entry serves the outputs of blocks 13..15
                    assert np.array_equal(got, sh.extract_block(x, b - 1)), (mode, b)
                seen.append(got)
            assert all(not np.array_equal(seen[i], seen[i + 1]) for i in range(3))
    finally:
        sh.set_option("bf16_activations", 0)
        xd.free()
    for block in (11, 16, 0, -1):
        with pytest.raises(pkg._lib.DfdError) as e:
            sh.extract_block_input(x, block)
        assert e.value.code == -1 and len(str(e.value)) > 30
    with pytest.raises(pkg._lib.DfdError):
        sh.extract_block_input(B.random_crops(17, 3), 12)      # n > max_batch is the caller's chunking
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, seed=0)
    try:
        got = m.extract_block_input(x, 12)                     # chunks of 2, 2, 1
        want = np.concatenate([m.handle.extract_block_input(x[i:i + 2], 12) for i in range(0, 5, 2)])
        assert got.shape == (5, 7, 7, 192) and np.array_equal(got, want)
        assert np.array_equal(m.extract_block_input(x, 14), m.extract_block(x, 13))
    finally:
        m.handle.close()


def test_train_augment_block_input_equals_augment_then_extract(pkg, seeded_sd):
    h = pkg._lib.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=2)
    try:
        rgb = np.random.RandomState(8).randint(0, 256, (5, 64, 96, 3)).astype(np.uint8)
        rows, batch = TA.draw_batch(TA.AugmentPolicy(), np.random.RandomState(6), 5, 64, 96, 224,
                                    mix=(TA.MIX_MIXUP, 0.8, np.array([4, 3, 0, 1, 2])))
        x = h.train_augment(rgb, rows, batch, 224)
        buf = h.alloc(rgb.nbytes).upload(rgb)
        try:
            for b in (12, 13, 14, 15):
                want = np.concatenate([h.extract_block_input(x[i:i + 2], b) for i in range(0, 5, 2)])
                got = h.train_augment_block_input(rgb, rows, batch, block=b)                  # uploaded
                assert got.shape == (5, 7, 7, 192) and np.array_equal(got, want), b
                assert np.array_equal(h.train_augment_block_input(buf, rows, batch, block=b, shape=rgb.shape[:3]), want), b    # resident
                if b >= 14:
                    assert np.array_equal(got, h.train_augment_block(rgb, rows, batch, block=b - 1)), b
            assert np.array_equal(h.train_augment_input12(rgb, rows, batch), h.train_augment_block_input(rgb, rows, batch, block=12))
            assert np.array_equal(h.train_augment_input13(rgb, rows, batch), h.train_augment_block_input(rgb, rows, batch, block=13))
        finally:
            buf.free()
        for block in (11, 16):
            with pytest.raises(pkg._lib.DfdError) as e:
                h.train_augment_block_input(rgb, rows, batch, block=block)
            assert e.value.code == -1 and len(str(e.value)) > 30
    finally:
        h.close()


# --------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_handle_usable(pkg, sh):
    L = pkg._lib
    below, b14, b15, conv = C.start(12)
    b13, b12 = below[13], below[12]
    head, x, y = O.default_params(0), B2.synthetic_rows(0, 4), C.labels(0, 4)

    def refused(fn, *a, code=-1, **k):
        with pytest.raises(L.DfdError) as e:
            fn(*a, **k)
        assert e.value.code == code and len(str(e.value)) > 30, str(e.value)    # the documented code with a message

    refused(sh.head_train_unfreeze_block_at, b13, 13)                           # no trainer is open
    sh.head_train_begin(head, L.head_config(max_n=4))
    try:
        sh.head_train_unfreeze_conv(conv)
        sh.head_train_unfreeze_block(b15)
        for b, p in ((13, b13), (12, b12)):
            refused(sh.head_train_unfreeze_block_at, p, b, code=-7)             # the block above is frozen: DFD_ERR_UNSUPPORTED
        sh.head_train_unfreeze_block_at(b14, 14)
        refused(sh.head_train_unfreeze_block_at, b12, 12, code=-7)              # 13 comes before 12
        for b in (13, 12):
            refused(sh.head_train_export_block_at, b, code=-7)                  # frozen 13 / 12 keep DFD_ERR_UNSUPPORTED
            refused(sh.head_train_block_grads_at, b, code=-7)
        for other in (11, 16, 0):
            refused(sh.head_train_unfreeze_block_at, b13, other, code=-7)       # blocks outside 12..14
            refused(sh.head_train_export_block_at, other, code=-7)
        sh.head_train_accumulate_block(x, y)                                    # the depth-14 trainer still works
        for name in B2.taps_of(13) + B2.taps_of(12):
            refused(sh.head_train_tap, name, 4)                                 # the new taps without their stages
        refused(sh.head_train_unfreeze_block_at, b13, 13)                       # after an accumulate
    finally:
        sh.head_train_end()
    sh.head_train_begin(head, L.head_config(max_n=4))
    try:
        sh.head_train_unfreeze_conv(conv)
        sh.head_train_unfreeze_block(b15)
        sh.head_train_unfreeze_block_at(b14, 14)
        refused(sh.head_train_unfreeze_block_at, b14, 14)                       # already unfrozen
        for bad in (1.0, -0.1, float("nan")):
            refused(sh.head_train_unfreeze_block_at, b13, 13, drop_connect=bad)
        refused(sh.head_train_unfreeze_block_at, b13, 13, bn_eps=0.0)
        sh.head_train_unfreeze_block_at(b13, 13, drop_connect=C.RATES[13])
        refused(sh.head_train_unfreeze_block_at, b13, 13)                       # a second time
        for name in B2.taps_of(12):
            refused(sh.head_train_tap, name, 4)
        assert sh.head_train_export_block_at(13)["dw_w"].shape == (1152, 5, 5)
        refused(sh.head_train_export_block_at, 12, code=-7)
        sh.head_train_unfreeze_block_at(b12, 12, drop_connect=C.RATES[12])
        refused(sh.head_train_unfreeze_block_at, b12, 12)
        refused(sh.head_train_accumulate_block, x[:1], y[:1])                   # n < 2
        refused(sh.head_train_accumulate_block, B2.synthetic_rows(0, 5), C.labels(0, 5))     # n > max_n
        refused(sh.head_train_tap, "b12.ad", 4)                                 # nothing accumulated yet
        loss, logits = sh.head_train_accumulate_block(x, y)
        assert np.isfinite(loss) and np.isfinite(logits).all()
        assert sh.head_train_tap("b12.ad", 4).shape == (4, 49, 1152) and sh.head_train_tap("b13.keep", 4).shape == (4,)
        refused(sh.head_train_tap, "b12.nothing", 4)
        refused(sh.head_train_tap, "b15.keep", 4)
        assert np.isfinite(sh.head_train_apply(1e-3)) and np.isfinite(sh.head_train_eval_block(x[:1])).all()
        assert np.array_equal(sh.head_train_export_block_at(12)["rm2"].shape, (192,))
    finally:
        sh.head_train_end()
    refused(sh.head_train_export_block_at, 13)                                  # after end: no trainer
    assert np.isfinite(sh.classify(B.random_crops(1, 0))).all()
    # dfd_destroy with an open trainer and all five stages frees everything
    h = L.Handle(pkg.weights.pack_b0(pkg.weights.seeded_state_dict(0)), device=0, max_batch=1)
    h.head_train_begin(head, L.head_config(max_n=4))
    h.head_train_unfreeze_conv(conv)
    h.head_train_unfreeze_block(b15)
    for b, p in ((14, b14), (13, b13), (12, b12)):
        h.head_train_unfreeze_block_at(p, b)
    h.head_train_accumulate_block(x, y)
    h.close()


# --------------------------------------------------------------------------- 8. after the trainer
def test_classify_after_a_depth_12_trainer_gives_a_fresh_handles_bits(pkg, stress_sd, real_rows):
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
        _open(pkg, h, 12, O.default_params(1), "ref", max_n=8, seed=3)
        try:
            h.head_train_accumulate_block(real_rows[12][:8], C.labels(1, 8))
            h.head_train_apply(1e-3)
            h.head_train_eval_block(real_rows[12][:3])
        finally:
            h.head_train_end()
        assert np.array_equal(h.classify(imgs), want)
    finally:
        h.close()


# --------------------------------------------------------------------------- 9. fit_head
def test_fit_head_with_block12_and_augmentation(pkg):
    """DeepfakeEfficientNet.fit_head(train_block12=True, augment=policy): uint8 crops, every batch through
    `train_augment_block_input(block=12)`; all six groups committed on the SAME handle"""
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=4, seed=0)
    try:
        crops = np.random.RandomState(5).randint(0, 256, (12, 48, 48, 3)).astype(np.uint8)
        y = (np.arange(12) % 2).astype(np.float32)
        key = "net._blocks.12._expand_conv.weight"
        x = B.random_crops(2, 1)
        handle, w0, out0, in0 = m.handle, np.array(m.state_dict()[key]), m.extract_block_input(x, 13).copy(), m.extract_block_input(x, 12).copy()
        log = m.fit_head(crops, y, epochs=2, batch_size=6, grad_accum=1, lr=1e-3, train_block12=True, augment=TA.AugmentPolicy(),
                         rng=np.random.RandomState(2), trainer_config={"ema_decay": 0.5})
        assert len(log) == 2 and m.handle is handle
        assert all(np.isfinite(e["train_loss"]) and np.isfinite(e["lr"]) and np.isfinite(e["train_acc"]) for e in log)
        w1 = np.array(m.state_dict()[key])
        assert w1.shape == w0.shape and not np.array_equal(w1, w0)
        # the commit changed b12.exp.w on the handle: block 12's output moved, its input did not
        assert not np.array_equal(m.extract_block_input(x, 13), out0) and np.array_equal(m.extract_block_input(x, 12), in0)
        assert int(m.state_dict()["net._blocks.12._bn0.num_batches_tracked"]) == 4
        fresh = pkg._lib.Handle(pkg.weights.pack_b0(m.state_dict()), device=0, max_batch=4)
        try:
            assert np.array_equal(fresh.classify(x), m.handle.classify(x))
        finally:
            fresh.close()
    finally:
        m.handle.close()

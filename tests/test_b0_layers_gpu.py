"""GPU: every classifier layer against float64 at the precision it claims (teacher forcing, tests/b0_layer_oracle.py).

For every tap a launch plan materialises, the layer's float64 reference is evaluated from the HIP path's own input to
that layer (its taps), so the difference left is that kernel's own arithmetic.

  * fp32 bars, per tap: rms(d) / rms(ref) <= 4x the fp32 yardstick's + 2^-23, and max |d| / u <= 8x the
    yardstick's + 2^-21, u = every element's fp32 conditioning scale (b0_layer_oracle.scale: the op evaluated on
    magnitudes), which measures each element - so each (image, channel) slice - on its own scale.  The yardstick is
    torch's plain fp32 evaluation of the same op from the same inputs (CPU).  Every op here, the composite ones
    included - expand + depthwise of a fused launch, the stem inside stem_dw_kernel, the gate recomputed through the
    depthwise with bf16 storage - is a chain of torch ops and has such a counterpart, so no op needs a bar of its own.
    The logit - one value per crop - holds the max bar per batch and the rms bar on its errors pooled over the four
    batches of a config (a rms ratio of 5 against 5 draws is noise).
  * bf16 bars ("bf16_activations"): every rounding point of that path is mirrored (b0_layer_oracle's docstring lists
    them), so every tap it stores as bf16 is within 1 ulp of the mirror and <= 1 % of its elements are not
    bit-identical.  gate, feat and logit are fp32 in that path and hold the fp32 bars.

Matrix: the fp32 configs fuse0 / fuse1 / default (= fuse 2) / late_all (fuse_late_skip = 0) / split_gemm0 and the bf16
configs with planes 3 and 1, expand fused and not; each on seeded_state_dict(0) (the shared handle) and on
stress_state_dict(0) (a handle of its own), each on 5 random crops and on the 7 edge crops (both batches ragged against
the 4-image groups of the whole-image 7 x 7 launches and against every GEMM tile).  The default config also runs at
n = 1 and n = 16 (the handle's capacity).

Measured on an MI355X, worst over taps, weights and batches (fp32: HIP error / yardstick error, the worse of the two
metrics; bf16: largest error in ulps, largest fraction of elements not bit-identical):
    fuse0 3.72 (logit rms pooled)        fuse1 2.49 (b8.out)             default 2.47 (b8.out)
    late_all 2.48 (b8.out)                split_gemm0 2.98 (b8.out)       default at n = 1 / 16: 2.04 (b13.out)
    bf16_p3_fused   fp32 3.13, bf16 1.00 ulp, 0.375 %      bf16_p3_unfused fp32 1.57, bf16 1.00 ulp, 0.410 %
    bf16_p1_fused   fp32 1.22, bf16 1.00 ulp, 0.374 %      bf16_p1_unfused fp32 3.73, bf16 1.00 ulp, 0.406 %
  The whole file runs in ~86 s.  Kernel bugs found: none.
"""
import pytest
import torch

import b0_layer_oracle as O

pytestmark = pytest.mark.gpu

BATCHES = {"random5": O.random_crops(5), "edge7": O.edge_crops()}


@pytest.fixture(scope="module")
def stress_sd():
    return O.stress_state_dict(0)


@pytest.fixture(scope="module")
def stress_handle(pkg, stress_sd):
    h = pkg._lib.Handle(pkg.weights.pack_b0(stress_sd), device=0, max_batch=16)
    yield h
    h.close()


def run_config(pkg, h, sd, cfg, x):
    """every tap of `cfg` on crops `x` against its bar -> {tap: O.check result}.  Also: the expanded tensor of every
    block whose expand Config.expand_fused calls fused is reported as not materialised."""
    n = x.shape[0]
    sd64, sd32 = O.to_torch(sd), O.to_torch(sd, torch.float32)
    ksd = O.kernel_state_dict(sd, cfg) if cfg.bf16 else None
    xd = h.alloc(x.nbytes).upload(x)
    cache = {"x": torch.from_numpy(x).double()}

    def get64(name):
        if name not in cache:
            cache[name] = O.from_tap(h.tap(xd.ptr, n, name, O.tap_size(name, n)), name, n)
        return cache[name]

    try:
        for k, v in cfg.options().items():
            h.set_option(k, v)
        for i in range(1, 16):
            if cfg.expand_fused(i):
                with pytest.raises(pkg._lib.DfdError, match="not materialised"):
                    h.tap(xd.ptr, n, f"b{i}.exp", O.tap_size(f"b{i}.exp", n))
        return {name: O.check(cfg, name, get64, lambda k: get64(k).float(), sd64, sd32, ksd) for name in cfg.taps()}
    finally:
        for k, v in O.DEFAULT.options().items():                  # the handle's defaults
            h.set_option(k, v)
        xd.free()


def _fmt(r):
    if r["kind"] == "bf16":
        return f"{r['ulp']:.2f} ulp, {r['diff']:.2%} not bit-identical"
    return f"rms {r['rms']:.2e}, max|d|/u {r['max']:.2e}: {r['vs_yard']:.2f}x the yardstick, {r['ratio']:.2f}x the bar"


def _judge(cfg, runs):
    """runs: {label: {tap: result}} -> (failures, summary line).  O.POOLED taps: rms bar over all runs pooled."""
    bad = []
    worst_fp32, worst_ulp, worst_diff = (0.0, ""), (0.0, ""), (0.0, "")
    for label, res in runs.items():
        for tap, r in res.items():
            where = f"{label}/{tap}"
            if not r["ratio"] <= 1.0:
                bad.append(f"{cfg.name} {where}: {_fmt(r)}")
            if r["kind"] == "fp32" and tap not in O.POOLED:
                worst_fp32 = max(worst_fp32, (r["vs_yard"], where))
            elif r["kind"] == "bf16":
                worst_ulp = max(worst_ulp, (r["ulp"], where))
                worst_diff = max(worst_diff, (r["diff"], where))
    for tap in O.POOLED:
        p = O.pooled_rms_ratio([res[tap]["sq"] for res in runs.values()])
        if not p["ratio"] <= 1.0:
            bad.append(f"{cfg.name} {tap}, rms pooled over {len(runs)} batches: {p['vs_yard']:.2f}x the yardstick")
        worst_fp32 = max(worst_fp32, (p["vs_yard"], f"{tap} rms pooled"))
    line = f"LAYERS {cfg.name}: fp32 worst {worst_fp32[0]:.2f}x the yardstick ({worst_fp32[1]})"
    if cfg.bf16:
        line += f"; bf16 worst {worst_ulp[0]:.2f} ulp ({worst_ulp[1]}), {worst_diff[0]:.3%} not bit-identical ({worst_diff[1]})"
    return bad, line


@pytest.mark.parametrize("cfg", O.FP32_CONFIGS + O.BF16_CONFIGS, ids=lambda c: c.name)
def test_every_layer_holds_its_precision(pkg, b0_handle, seeded_sd, stress_handle, stress_sd, cfg):
    runs = {}
    for wname, h, sd in (("seeded", b0_handle, seeded_sd), ("stress", stress_handle, stress_sd)):
        for bname, x in BATCHES.items():
            runs[f"{wname}/{bname}"] = run_config(pkg, h, sd, cfg, x)
    bad, line = _judge(cfg, runs)
    print(line)
    assert not bad, "\n".join(bad)


def test_default_config_at_one_and_sixteen_crops(pkg, b0_handle, seeded_sd):
    runs = {f"n{n}": run_config(pkg, b0_handle, seeded_sd, O.DEFAULT, O.random_crops(n, seed=3)) for n in (1, 16)}
    bad, line = _judge(O.DEFAULT, runs)
    print(line)
    assert not bad, "\n".join(bad)

"""CPU: the launch-by-launch Grad-CAM oracle (tests/gradcam_oracle.py) and the teeth of the checks
tests/test_gradcam_stages_gpu.py asserts with it.

`model` restates the three launches of csrc/gradcam.hip in float32 numpy (row blocks of 8, four wave partials summed in
wave order, the map kernel's operation order, the resize tables, the overlay) and returns what Handle.gradcam_tap
returns, guard rows included.  Unmutated, it must pass every check the GPU test makes (gradcam_oracle.check_outputs /
check_crafted) at every case the GPU test runs.  Each defect - a mistake a kernel could make - must FAIL at least one of
those checks at a named case of the GPU test (WITNESSES).

The CPU parts of the oracle's own evidence are here too: the float64 chain against torch autograd on the edge crops, the
host resize against float64 torch interpolation, and the conditions of the crafted cases (asserted inside
gradcam_oracle.crafted_cases on the float64 oracle).
"""
import numpy as np
import pytest
import torch

import b0_layer_oracle as B
import gradcam_oracle as GO
from oracle import b0_ref

F = np.float32
DEFECTS = ("ragged_rows", "drop_wave_d1", "drop_wave_g", "mu_no_z", "one_div49", "no_b", "no_relu", "mask_ge", "no_half_pixel",
           "border_lo", "skip_second_minmax", "jet_round", "byte_round", "batch_max", "bgr_swap", "no_clamp", "bf16_wrong_half")


# --------------------------------------------------------------------------- the float32 model of the three launches
def _mlp(a, w, waves, drop=None):
    """rows of a (m, K) times w (K, N): the reduction split over `waves` waves, partials summed in wave order"""
    step = a.shape[1] // waves
    parts = [a[:, i * step:(i + 1) * step] @ w[i * step:(i + 1) * step] for i in range(waves)]
    if drop is not None:
        wave, block = drop
        parts[wave][:, block * 64:(block + 1) * 64] = 0
    v = parts[0]
    for p in parts[1:]:
        v = v + p
    return v.astype(F)


def _guarded(n, cols):
    return np.full((n + GO.GUARD, cols), GO.SENTINEL, np.uint32)


def model_heat(cam, defect=None):
    n = cam.shape[0]
    lo, hi = cam.min(axis=1, keepdims=True), cam.max(axis=1, keepdims=True)
    m7 = ((cam - lo) / (F(1e-7) + (hi - lo))).reshape(n, 7, 7)
    t = np.arange(224, dtype=F)
    f = t * F(7 / 224) if defect == "no_half_pixel" else (t + F(0.5)) * F(7 / 224) - F(0.5)
    s = np.floor(f).astype(np.int64)
    fr = (f - s.astype(F)).astype(F)
    if defect != "border_lo":
        fr[s < 0] = 0
    s[s < 0] = 0
    fr[s >= 6] = 0
    s[s >= 6] = 6
    s1 = np.minimum(s + 1, 6)
    one = F(1)
    h = m7[:, :, s] * (one - fr) + m7[:, :, s1] * fr
    r = h[:, s, :] * (one - fr)[:, None] + h[:, s1, :] * fr[:, None]
    if defect == "skip_second_minmax":
        return r.astype(F)
    lo, hi = r.min(axis=(1, 2), keepdims=True), r.max(axis=(1, 2), keepdims=True)
    return ((r - lo) / (F(1e-7) + (hi - lo))).astype(F)


def model_overlay(x, heat, jet, defect=None):
    mean, std = np.array([0.485, 0.456, 0.406], F), np.array([0.229, 0.224, 0.225], F)
    v = F(255) * heat
    idx = np.minimum((np.rint(v) if defect == "jet_round" else v).astype(np.int32), 255)
    jetf = jet.astype(F) / F(255)
    img = x.astype(F) * std[None, :, None, None] + mean[None, :, None, None]
    if defect != "no_clamp":
        img = np.minimum(np.maximum(img, F(0)), F(1))
    img = img.transpose(0, 2, 3, 1)                          # RGB last
    if defect != "bgr_swap":
        img = img[..., ::-1]
    pre = jetf[idx] + img
    vmax = pre.max() if defect == "batch_max" else pre.max(axis=(1, 2, 3), keepdims=True)
    v = F(255) * (pre / vmax)
    return (np.rint(v) if defect == "byte_round" else v).astype(np.int32).astype(np.uint8)


def model(t, z, fc1, fc2, x=None, overlay=False, defect=None):
    """float32 restatement of gradcam_launch on host arrays -> the dict of Handle.gradcam_tap"""
    n = z.shape[0]
    w1, w2, w3, b = (np.asarray(t[k], F) for k in ("fc1.w", "fc2.w", "fc3.w", "head.b"))
    fc1, fc2 = np.asarray(fc1, F)[:n], np.asarray(fc2, F)[:n]
    D1, G, cam = _guarded(n, 512), _guarded(n, 1280), _guarded(n, 49)
    live = (lambda a: a >= 0) if defect == "mask_ge" else (lambda a: a > 0)
    d1 = _mlp(np.where(live(fc2), w3[0][None, :], F(0)).astype(F), w2, 4, (2, 1) if defect == "drop_wave_d1" else None)
    d1 = np.where(live(fc1), d1, F(0)).astype(F)
    g = _mlp(d1, w1, 4, (1, 3) if defect == "drop_wave_g" else None)
    D1[:n], G[:n] = d1.view(np.uint32), g.view(np.uint32)
    if defect == "ragged_rows":                             # the whole last row block stored: rows n .. of zero inputs
        top = -(-n // 8) * 8
        D1[n:top], G[n:top] = 0, 0
    if z.dtype == np.uint16 and defect == "bf16_wrong_half":
        zf = z.astype(np.uint32).view(F)
    else:
        zf = GO.widen(z)
    with np.errstate(over="ignore"):
        s = (F(1) / (F(1) + np.exp(-zf))).astype(F)
    term = s if defect == "mu_no_z" else s * (F(1) + zf * (F(1) - s))
    mu = term[:, 0]
    for p in range(1, 49):
        mu = mu + term[:, p]
    w = g * (mu / F(49))
    if defect != "one_div49":
        w = w / F(49)
    sums = (w[:, None, :] * (zf if defect == "no_b" else zf - b)).sum(axis=2, dtype=F)
    c = sums if defect == "no_relu" else np.maximum(sums, F(0))
    cam[:n] = c.astype(F).view(np.uint32)
    heat = model_heat(c.astype(F), defect)
    out = {"z": z, "z_bf16": z.dtype == np.uint16, "fc1": fc1, "fc2": fc2, "heat": heat, "overlay": None}
    for k, a in (("D1", D1), ("G", G), ("cam7", cam)):
        out[k], out["guard_" + k] = a[:n].view(F), a[n:]
    if overlay:
        from rtdfd_amd import luts

        out["overlay"] = model_overlay(x, heat, luts.JET_BGR, defect)
    return out


# --------------------------------------------------------------------------- the cases of the GPU test, on CPU tensors
@pytest.fixture(scope="module")
def gc(pkg):
    from rtdfd_amd import gradcam

    return gradcam


@pytest.fixture(scope="module")
def world(pkg, seeded_sd):
    """per weights set: the folded tensors and a float32 CPU forward's (x, z, fc1, fc2) on the random and the edge crops"""
    out = {}
    for wname, sd in (("seeded", seeded_sd), ("stress", B.stress_state_dict(0))):
        t = pkg.weights.pack_b0_tensors(sd)
        x = np.concatenate([B.random_crops(5), B.edge_crops()])
        taps = {}
        with torch.no_grad():
            b0_ref.extract_features(GO._net(pkg.weights.to_torch(sd)), torch.from_numpy(x), taps)
        z, f1, f2 = GO.forward_tensors(t, taps["b15.out"])
        out[wname] = dict(t=t, sd=sd, x=x, z=z, fc1=f1, fc2=f2, x15=taps["b15.out"])
    return out


def _cases(world):
    """name -> (weights set, kwargs of `model`, crafted case or None): every tap call of the GPU test"""
    cases = {}
    for wname, w in world.items():
        for cname, sl in (("random", slice(0, 5)), ("edge", slice(5, 12))):
            cases[f"{wname}/{cname}"] = (wname, dict(z=w["z"][sl], fc1=w["fc1"][sl], fc2=w["fc2"][sl], x=w["x"][sl], overlay=True), None)
    w = world["seeded"]
    for c in GO.crafted_cases(w["t"], (w["z"][:5], w["fc1"][:5], w["fc2"][:5]), w["x"][:5]):
        cases["crafted/" + c["name"]] = ("seeded", dict(z=c["z"], fc1=c["fc1"], fc2=c["fc2"], x=c["x"], overlay=c["overlay"]), c)
    z, f1, f2 = GO.ragged_base((w["z"], w["fc1"], w["fc2"]))
    for n in GO.RAGGED_N:
        cases[f"ragged/{n}/fp32"] = ("seeded", dict(z=z[:n], fc1=f1[:n], fc2=f2[:n]), None)
        cases[f"ragged/{n}/bf16"] = ("seeded", dict(z=GO.rne_bits(z[:n]), fc1=f1[:n], fc2=f2[:n]), None)
    return cases


@pytest.fixture(scope="module")
def cases(world):
    return _cases(world)


def _failures(world, cases, name, gc, defect=None):
    wname, kw, crafted = cases[name]
    t = world[wname]["t"]
    out = model(t, defect=defect, **kw)
    fails, fig = GO.check_outputs(t, out, kw["z"].shape[0], gc, kw.get("x"))
    if crafted is not None:
        fails += GO.check_crafted(crafted, out, gc)
    return fails, fig


def test_unmutated_model_passes_every_check_at_every_case(world, cases, gc):
    worst = {}
    for name in cases:
        fails, fig = _failures(world, cases, name, gc)
        assert not fails, (name, fails)
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("float32 model / yardstick, worst per stage (heat: abs distance to the interpolate chain):",
          {k: float(f"{v:.3g}") for k, v in worst.items()})


# defect -> the cases at which a check must fail
WITNESSES = {
    "ragged_rows": ("ragged/9/fp32", "ragged/9/bf16", "ragged/1/fp32", "ragged/7/fp32"),
    "drop_wave_d1": ("seeded/random", "stress/edge"),
    "drop_wave_g": ("seeded/random", "stress/edge"),
    "mu_no_z": ("seeded/random", "stress/random"),
    "one_div49": ("seeded/random",),
    "no_b": ("stress/random", "stress/edge"),
    "no_relu": ("seeded/edge", "crafted/all_negative"),
    "mask_ge": ("seeded/random", "crafted/signed_zeros"),
    "no_half_pixel": ("seeded/random", "ragged/1/fp32"),
    "border_lo": ("seeded/random", "ragged/1/fp32"),
    "skip_second_minmax": ("crafted/single_peak",),
    "jet_round": ("seeded/random",),
    "byte_round": ("seeded/random",),
    "batch_max": ("crafted/overlay_clamp_and_maxima",),
    "bgr_swap": ("seeded/random",),
    "no_clamp": ("crafted/overlay_clamp_and_maxima", "seeded/edge"),
    "bf16_wrong_half": ("ragged/8/bf16", "ragged/1/bf16"),
}


def test_every_defect_has_a_witness(cases):
    assert set(WITNESSES) == set(DEFECTS)
    for names in WITNESSES.values():
        assert names and all(n in cases for n in names)


@pytest.mark.parametrize("defect", DEFECTS)
def test_defect_fails_an_asserted_check_at_a_case_the_gpu_test_runs(world, cases, gc, defect):
    for name in WITNESSES[defect]:
        fails, _ = _failures(world, cases, name, gc, defect)
        assert fails, f"{defect} survives {name}"


def test_ragged_rows_is_invisible_at_a_full_block(world, cases, gc):
    """why n = 9 is in the list: at n = 8 and 16 the defect stores nothing past the batch"""
    for n in (8, 16):
        assert not _failures(world, cases, f"ragged/{n}/fp32", gc, "ragged_rows")[0]


def test_second_minmax_matters_only_for_an_interior_peak(world, cases, gc):
    """without it the interior peak's maximum stays at (63 / 64)^2 = 0.969; a corner peak already reaches 1 - 1e-7"""
    _, kw, _ = cases["crafted/single_peak"]
    out = model(world["seeded"]["t"], defect="skip_second_minmax", **kw)
    hi = out["heat"].reshape(5, -1).max(axis=1)
    assert np.allclose(hi[:3], (63 / 64) ** 2, atol=1e-6) and np.all(hi[3:] >= 1 - 1e-6)


# --------------------------------------------------------------------------- the oracle's own evidence
def test_float64_chain_matches_autograd_on_edge_crops(pkg, world):
    """the closed form the stage references restate, against autograd, where the ReLU cuts (16 - 37 % positive cells)
    and z leaves the range of exp"""
    w = world["seeded"]
    cam_ag, _, _ = GO.autograd_cam(pkg.weights.to_torch(w["sd"]), torch.from_numpy(w["x"][5:]))
    _, sums = GO.oracle64(w["t"], w["z"][5:], w["fc1"][5:], w["fc2"][5:])
    cam = np.maximum(sums, 0).reshape(-1, 7, 7)
    peak = np.abs(cam_ag).reshape(7, -1).max(axis=1)
    live = peak > 0
    assert live.sum() >= 5
    err = np.abs(cam - cam_ag).reshape(7, -1).max(axis=1)
    assert np.all(err[live] <= 1e-4 * peak[live]) and np.all(err[~live] == 0), (err, peak)
    pos = (cam_ag > 0).reshape(7, -1).mean(axis=1)
    assert pos[live].min() < 0.5, pos                        # the ReLU does cut on these crops
    assert np.abs(w["z"][5:]).max() > 100                    # and exp(-z) overflows float32


def test_host_resize_matches_float64_interpolate(gc):
    rs = np.random.RandomState(9)
    cam = np.maximum(rs.randn(50, 49), 0).astype(np.float32)
    d = np.abs(GO.heat_host(cam, gc) - GO.heat_independent(cam)).max()
    print(f"host chain against the float64 interpolate chain over 50 random maps: {d:.2e}")
    assert d <= GO.HEAT_INDEPENDENT_ABS


def test_model_heat_and_overlay_are_the_library_restatements(pkg, gc):
    rs = np.random.RandomState(4)
    cam = np.maximum(rs.randn(6, 49), 0).astype(np.float32)
    heat = model_heat(cam)
    assert np.array_equal(heat, GO.heat_host(cam, gc))
    x = (rs.randn(6, 3, 224, 224) * 2).astype(np.float32)
    assert np.array_equal(model_overlay(x, heat, pkg.luts.JET_BGR), GO.overlay_host(x, heat, gc))


def test_bf16_bits_round_trip():
    z = np.random.RandomState(1).randn(3, 49, 1280).astype(np.float32) * 30
    bits = GO.rne_bits(z)
    assert bits.dtype == np.uint16 and np.array_equal(GO.rne_bits(GO.widen(bits)), bits)
    assert np.abs(GO.widen(bits) - z).max() <= np.abs(z).max() * 2.0 ** -8


def test_tap_constants_agree_with_the_header(pkg):
    import ctypes
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dfd_hip.h")).read()
    guard = int(re.search(r"#define DFD_GRADCAM_TAP_GUARD (\d+)", hdr).group(1))
    sentinel = int(re.search(r"#define DFD_GRADCAM_TAP_SENTINEL (0x[0-9A-Fa-f]+)u", hdr).group(1), 16)
    assert guard == pkg._lib.GRADCAM_TAP_GUARD == GO.GUARD == 8          # one row block of the MLP-backward kernels
    assert sentinel == pkg._lib.GRADCAM_TAP_SENTINEL == GO.SENTINEL
    assert np.isnan(np.array([sentinel], np.uint32).view(np.float32)[0])
    assert ctypes.sizeof(pkg._lib.GradcamTapParams) == 4 * 4 + 9 * ctypes.sizeof(ctypes.c_void_p)

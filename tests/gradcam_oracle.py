"""Test-side Grad-CAM oracle (pytorch_grad_cam 1.3.x semantics, target layer net._conv_head, target = the logit):
torch autograd on CPU with the head conv's output A as a leaf, built from oracle.b0_ref's pieces; and the closed form
the device computes, on the folded tensors of weights.pack_b0_tensors."""
import numpy as np
import torch

import b0_layer_oracle as B
import gemm_oracle as G
from oracle import b0_ref

GC_C = 1280


def _net(sd):
    return {(k if k.startswith("net.") else "net." + k): v for k, v in sd.items()}


def autograd_cam(sd_torch, x: torch.Tensor):
    """-> (cam7 (n,7,7) float32 before normalisation, logits (n,1), x15 (n,320,7,7))"""
    sd = _net(sd_torch)
    taps = {}
    with torch.no_grad():
        b0_ref.extract_features(sd, x.float(), taps)
    x15 = taps["b15.out"]
    with torch.no_grad():
        a0 = b0_ref._same_conv(x15, sd["net._conv_head.weight"], 1)
    A = a0.clone().requires_grad_(True)
    y = b0_ref._swish(b0_ref._bn(A, sd, "net._bn1", b0_ref._BN_EPS))
    logits = b0_ref.head(sd, torch.nn.functional.adaptive_avg_pool2d(y, 1).flatten(1))
    logits[:, 0].sum().backward()                        # ClassifierOutputTarget(0) per row, summed: rows independent
    alpha = A.grad.mean(dim=(2, 3), keepdim=True)
    cam = torch.relu((alpha * A).sum(dim=1))
    return cam.detach().numpy().astype(np.float32), logits.detach().numpy(), x15


def closed_form_cam(t, x15: torch.Tensor):
    """The device's algebra on the folded tensors t (pack_b0_tensors): z = BN(conv_head(x15)) NHWC, g = dL/dfeat,
    mu = mean_p swish'(z), cam = relu(sum_k g mu / 49 (z - b))."""
    T = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in t.items()}
    n = x15.shape[0]
    xs = x15.permute(0, 2, 3, 1).reshape(n, 49, 320)
    z = xs @ T["head.w"].T + T["head.b"]                 # (n,49,1280)
    s = torch.sigmoid(z)
    feat = (z * s).mean(dim=1)
    f1 = torch.relu(feat @ T["fc1.w"].T + T["fc1.b"])
    f2 = torch.relu(f1 @ T["fc2.w"].T + T["fc2.b"])
    d2 = T["fc3.w"][0] * (f2 > 0)
    d1 = (d2 @ T["fc2.w"]) * (f1 > 0)
    g = d1 @ T["fc1.w"]                                  # (n,1280)
    mu = (s * (1 + z * (1 - s))).mean(dim=1)
    w = g * mu / 49
    cam = torch.relu(((z - T["head.b"]) * w[:, None, :]).sum(dim=2))
    return cam.reshape(n, 7, 7).numpy().astype(np.float32)


def heat_of(cam7, gradcam_mod):
    """pytorch_grad_cam's returned map from raw 7x7 maps: scale_cam_image to 224, ReLU, mean over one layer,
    scale_cam_image again"""
    m = gradcam_mod.scale_cam_image(cam7, (224, 224))
    m = np.maximum(m[:, None], 0).mean(axis=1)
    return gradcam_mod.scale_cam_image(m)


def denormalise(x: np.ndarray) -> np.ndarray:
    """(n,3,224,224) normalised RGB -> (n,224,224,3) BGR float32 in [0,1]"""
    mean = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 3, 1, 1)
    std = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 3, 1, 1)
    img = np.clip(x.astype(np.float32) * std + mean, 0, 1).astype(np.float32)
    return np.ascontiguousarray(img[:, ::-1].transpose(0, 2, 3, 1))


# =========================================================================== the launches, one by one (dfd_gradcam_tap)
# Each launch's reference is evaluated from the device's own input to it (teacher forcing, as b0_layer_oracle): D1 from
# (fc1, fc2), G from the device's D1, the position sums and cam7 from the device's G and z, heat from the device's cam7,
# the overlay from the device's heat.  Per float launch: the float64 reference, the float32 torch evaluation of the same
# formula (the yardstick) and the conditioning scale u (the op on magnitudes); the bars are b0_layer_oracle's.
GUARD = 8                        # _lib.GRADCAM_TAP_GUARD: one row block of the MLP-backward kernels
SENTINEL = 0x7FC5A5A5            # _lib.GRADCAM_TAP_SENTINEL
HEAT_INDEPENDENT_ABS = 1e-6      # heat against the float64 interpolate chain: about twelve roundings of <= 2^-24 on [0, 1]


def weights_of(t, dtype):
    """the folded tensors the three launches read (pack_b0_tensors), as torch tensors of `dtype`"""
    return {k: torch.from_numpy(np.asarray(t[k], np.float32)).to(dtype) for k in ("fc1.w", "fc2.w", "fc3.w", "head.b")}


def widen(z: np.ndarray) -> np.ndarray:
    """z as the map kernel reads it: float32, or uint16 bf16 bit patterns widened"""
    return G.from_bits(z) if z.dtype == np.uint16 else np.asarray(z, np.float32)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)


def ref_d1(W, fc1, fc2):
    """-> (D1 (n,512), u)"""
    d2 = W["fc3.w"][0] * (fc2 > 0)
    m1 = (fc1 > 0).to(d2.dtype)
    return (d2 @ W["fc2.w"]) * m1, (d2.abs() @ W["fc2.w"].abs()) * m1


def ref_g(W, d1):
    """-> (G (n,1280), u)"""
    return d1 @ W["fc1.w"], d1.abs() @ W["fc1.w"].abs()


def ref_sums(W, g, z):
    """the 49 pre-ReLU position sums of every crop, sum_k g mu / 49 (z - b) with mu = mean_p swish'(z) -> (sums (n,49), u)"""
    s = torch.sigmoid(z)
    nchw = lambda v: v.permute(0, 2, 1).reshape(v.shape[0], GC_C, 7, 7)
    mu = B.mean_hw(nchw(s * (1 + z * (1 - s))))
    mu_mag = B.mean_hw(nchw(s * (1 + z.abs() * (1 - s))))
    b = W["head.b"]
    sums = torch.einsum("nk,npk->np", g * mu / 49, z - b)
    return sums, torch.einsum("nk,npk->np", g.abs() * mu_mag / 49, z.abs() + b.abs())


def float_stage(name, W64, W32, inputs, got):
    """one float launch against its bar -> dict(ratio (<= 1 passes), vs_yard, rms, max).  inputs: numpy arrays, the
    device's own inputs to the launch; got: the device's output.  cam7 (ReLU is 1-Lipschitz) holds the bar of its
    pre-ReLU sum: its distance to relu(reference) is measured as an error of that sum."""
    fn = {"D1": ref_d1, "G": ref_g, "cam7": ref_sums}[name]
    with torch.no_grad():
        ref, u = fn(W64, *(_t(a, torch.float64) for a in inputs))
        yard = fn(W32, *(_t(a, torch.float32) for a in inputs))[0].double()
    got = _t(got, torch.float64)
    if name == "cam7":
        got = ref + (got - torch.relu(ref))
    m, y = B.fp32_metrics(got, ref, u), B.fp32_metrics(yard, ref, u)
    return {"ratio": B.fp32_ratio(m, y), "vs_yard": B.yard_ratio(m, y), **m}


def heat_host(cam7, gradcam_mod):
    """reference (a): the host restatement of the library's chain on (n,49) raw maps"""
    return heat_of(np.asarray(cam7, np.float32).reshape(-1, 7, 7), gradcam_mod)


def _minmax64(m):
    m = m - m.amin(dim=(1, 2), keepdim=True)
    return m / (1e-7 + m.amax(dim=(1, 2), keepdim=True))


def heat_independent(cam7) -> np.ndarray:
    """reference (b): float64 torch bilinear interpolation (align_corners=False) between float64 min-max steps"""
    m = _minmax64(torch.from_numpy(np.asarray(cam7, np.float64).reshape(-1, 7, 7)))
    r = torch.nn.functional.interpolate(m[:, None], size=(224, 224), mode="bilinear", align_corners=False)[:, 0]
    return _minmax64(torch.clamp_min(r, 0)).numpy()


def overlay_host(x, heat, gradcam_mod) -> np.ndarray:
    imgs = denormalise(x)
    return np.stack([gradcam_mod.show_cam_on_image(imgs[i], heat[i], use_rgb=False) for i in range(len(imgs))])


def check_outputs(t, out, n, gradcam_mod, x=None):
    """Every check the GPU test makes on one tap result `out` (Handle.gradcam_tap's dict; tests' float32 model returns
    the same) -> (failures: list of strings, figures: stage -> ratio to the yardstick).  t: pack_b0_tensors."""
    W64, W32 = weights_of(t, torch.float64), weights_of(t, torch.float32)
    fails, fig = [], {}
    z = widen(out["z"])
    stages = (("D1", (out["fc1"], out["fc2"])), ("G", (out["D1"],)), ("cam7", (out["G"], z)))
    for name, inputs in stages:
        g = out["guard_" + name]
        if g.shape[0] != GUARD or not np.all(g == SENTINEL):
            fails.append(f"{name}: {int((g != SENTINEL).sum())} guard values changed behind row {n - 1}")
        left = int((out[name].view(np.uint32) == SENTINEL).sum())
        if left:
            fails.append(f"{name}: {left} values never stored")
            continue
        m = float_stage(name, W64, W32, inputs, out[name])
        fig[name] = m["vs_yard"]
        if not m["ratio"] <= 1.0:
            fails.append(f"{name}: past the fp32 bar: {m}")
    if out.get("heat") is not None:
        want = heat_host(out["cam7"], gradcam_mod)
        if not np.array_equal(out["heat"], want):
            d = np.abs(out["heat"] - want)
            fails.append(f"heat: not bit-equal to the host chain on the device's cam7: {int((d > 0).sum())} pixels, max {d.max():.3e}")
        e = float(np.abs(out["heat"] - heat_independent(out["cam7"])).max())
        fig["heat"] = e
        if not e <= HEAT_INDEPENDENT_ABS:
            fails.append(f"heat: {e:.3e} from the float64 interpolate chain")
    if out.get("overlay") is not None:
        want = overlay_host(x, out["heat"], gradcam_mod)
        if not np.array_equal(out["overlay"], want):
            d = np.abs(out["overlay"].astype(np.int16) - want)
            fails.append(f"overlay: not bit-equal to show_cam_on_image: {int((d > 0).sum())} bytes, max {int(d.max())}")
    return fails, fig


# --------------------------------------------------------------------------- cases
def forward_tensors(t, x15: torch.Tensor):
    """the tensors a forward leaves for Grad-CAM, in float32 on the CPU: z (n,49,1280), fc1, fc2 (the CPU test's base;
    the GPU test takes the device's own from start "x")"""
    T = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in t.items()}
    n = x15.shape[0]
    z = x15.float().permute(0, 2, 3, 1).reshape(n, 49, 320) @ T["head.w"].T + T["head.b"]
    feat = (z * torch.sigmoid(z)).mean(dim=1)
    f1 = torch.relu(feat @ T["fc1.w"].T + T["fc1.b"])
    f2 = torch.relu(f1 @ T["fc2.w"].T + T["fc2.b"])
    return z.numpy(), f1.numpy(), f2.numpy()


def oracle64(t, z, fc1, fc2):
    """the whole chain in float64, no teacher forcing -> (g (n,1280), sums (n,49)) as numpy"""
    W = weights_of(t, torch.float64)
    with torch.no_grad():
        g = ref_g(W, ref_d1(W, _t(fc1, torch.float64), _t(fc2, torch.float64))[0])[0]
        return g.numpy(), ref_sums(W, g, _t(widen(z), torch.float64))[0].numpy()


def rne_bits(z: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even"""
    return G.to_bits(B.rne_bf16(torch.from_numpy(np.ascontiguousarray(z, np.float32))).numpy())


def _pattern_z(t, g, pattern):
    """z = b + a_p sign(g_k) / 2 for one crop: every position sum is a_p S with one S = sum_k |g_k| mu_k / 98 > 0 (z stays
    within b +- 0.5, where swish' > 0), so the sign pattern of the map is `pattern`'s"""
    b = np.asarray(t["head.b"], np.float32)
    sg = np.where(g >= 0, 1.0, -1.0).astype(np.float32)
    return (b[None, :] + np.asarray(pattern, np.float32)[:, None] * (0.5 * sg)[None, :]).astype(np.float32)


def crafted_cases(t, base, x5):
    """The degenerate start-"z" cases, built on a real forward's tensors base = (z, fc1, fc2) of 5 crops with their inputs
    x5.  -> list of dict(name, z, fc1, fc2, x, overlay, expect): `expect` names what `check_crafted` asserts besides
    the stage checks.  The conditions that keep each construction honest are asserted here on the float64 oracle."""
    z0, f10, f20 = (np.array(a, np.float32) for a in base)
    g0, s0 = oracle64(t, z0, f10, f20)
    assert np.all(np.abs(g0).max(axis=1) > 0), "every base crop needs a live head"
    rs = np.random.RandomState(3)
    cases = []

    def add(name, z=z0, fc1=f10, fc2=f20, x=None, overlay=False, **expect):
        cases.append(dict(name=name, z=z, fc1=fc1, fc2=fc2, x=x, overlay=overlay, expect=expect))

    # a dead head on crops 0 and 2: all of fc2 at zero -> g = 0, every output of the crop zero, overlay = JET[0] + image
    f2 = f20.copy()
    f2[[0, 2]] = 0
    g, _ = oracle64(t, z0, f10, f2)
    assert not g[[0, 2]].any() and np.all(np.abs(g[[1, 3, 4]]).max(axis=1) > 0)
    add("dead_head", fc2=f2, x=x5, overlay=True, zero_rows=[0, 2])
    # -0.0 and exact +0.0 where the forward left positive activations: their masks are 0
    f1, f2 = f10.copy(), f20.copy()
    zero_cols = {}
    for a, key in ((f1, "D1"), (f2, None)):
        for i in range(5):
            pos = np.flatnonzero(a[i] > 0)
            assert pos.size >= 8
            pick = rs.choice(pos, 8, replace=False)
            a[i, pick[:4]] = -0.0
            a[i, pick[4:]] = 0.0
            if key:
                zero_cols[i] = pick
    assert np.signbit(f1).any() and np.signbit(f2).any()
    add("signed_zeros", fc1=f1, fc2=f2, d1_zero=zero_cols)
    # z equal at all 49 positions: a constant map, heat all zero (hi == lo in the first min-max)
    z = np.repeat(z0[np.arange(5), s0.argmax(axis=1)][:, None, :], 49, axis=1)
    _, s = oracle64(t, z, f10, f20)
    assert np.all(np.ptp(s, axis=1) <= 1e-12 * np.abs(s).max(axis=1)) and (s[:, 0] > 0).any(), "constant maps, one positive at least"
    add("const_map", z=z, heat_zero=True, const_cam=True)
    # exactly one positive cell: interior (3, 3) on crops 0-2, the corner (0, 0) on crop 3, the corner (6, 6) on crop 4;
    # and every sum negative
    peaks = [24, 24, 24, 0, 48]
    pats = -np.ones((5, 49), np.float32)
    pats[np.arange(5), peaks] = 1.0
    z = np.stack([_pattern_z(t, g0[i], pats[i]) for i in range(5)])
    _, s = oracle64(t, z, f10, f20)
    assert np.array_equal(s > 0, pats > 0) and np.abs(s).min() > 1e-3 * np.abs(s).max(), "exactly the one cell positive"
    add("single_peak", z=z, peak_max=True, positive=peaks)
    z = np.stack([_pattern_z(t, g0[i], -np.linspace(0.5, 1.0, 49)) for i in range(5)])
    _, s = oracle64(t, z, f10, f20)
    assert np.all(s < 0)
    add("all_negative", z=z, heat_zero=True, cam_zero=True)
    # z at +-100 on a tenth of the entries (__expf at inf and 0)
    z = z0.copy()
    hit = rs.rand(*z.shape) < 0.1
    z[hit] = np.where(rs.rand(int(hit.sum())) < 0.5, -100.0, 100.0)
    add("z_pm100", z=z)
    # an input at +-30 (the overlay's clamp acts) and crops whose image maxima differ (a per-batch overlay maximum shows)
    x = np.array(x5, np.float32)
    x[0] = np.where(rs.rand(3, 224, 224) < 0.5, -30.0, 30.0)
    x[1] = B.IMG_LO
    x[2] = B.IMG_HI
    d = denormalise(x)
    assert d[0].min() == 0 and d[0].max() == 1 and d[1].max() < 1e-6 and d[2].min() > 1 - 1e-6
    add("overlay_clamp_and_maxima", x=x, overlay=True)
    return cases


def check_crafted(case, out, gradcam_mod):
    """the outputs the crafted cases state, beyond the stage checks -> list of failures"""
    e, fails = case["expect"], []
    heat, cam = out["heat"], out["cam7"]
    for i in e.get("zero_rows", ()):
        if any(out[k][i].any() for k in ("D1", "G", "cam7", "heat")):
            fails.append(f"crop {i}: a dead head must give all-zero outputs")
        want = gradcam_mod.show_cam_on_image(denormalise(case["x"][i:i + 1])[0], np.zeros((224, 224), np.float32))
        if not np.array_equal(out["overlay"][i], want):
            fails.append(f"crop {i}: the overlay of a zero map must be JET[0] + image")
    for i, cols in e.get("d1_zero", {}).items():
        if out["D1"][i, cols].any():
            fails.append(f"crop {i}: D1 behind a +-0.0 activation must be 0")
    if e.get("heat_zero") and heat.any():
        fails.append("heat must be all zero")
    if e.get("cam_zero") and cam.any():
        fails.append("cam7 must be all zero")
    if e.get("const_cam") and np.ptp(cam, axis=1).any():
        fails.append("cam7 must be constant per crop")
    if e.get("positive") is not None:
        for i, p in enumerate(e["positive"]):
            if list(np.flatnonzero(cam[i] > 0)) != [p]:
                fails.append(f"crop {i}: exactly cell {p} must be positive")
    if e.get("peak_max"):
        hi = heat.reshape(len(heat), -1).max(axis=1)
        if not np.all(hi >= 1 - 1e-6):                     # 0.969 without the second min-max (interior peaks)
            fails.append(f"the map's maximum must reach 1 - O(1e-7): {hi}")
    return fails


RAGGED_N = (1, 7, 8, 9, 16)


def ragged_base(base):
    """16 rows of (z, fc1, fc2) from a forward's 12: the first four once more with their positions reversed"""
    z, f1, f2 = (np.asarray(a, np.float32) for a in base)
    assert z.shape[0] >= 12
    return np.concatenate([z[:12], z[:4, ::-1]]), np.concatenate([f1[:12], f1[:4]]), np.concatenate([f2[:12], f2[:4]])


# --------------------------------------------------------------------------- start "x": the link to the forward's taps
def _bar(got, ref, yard, u):
    m, y = B.fp32_metrics(got, ref, u), B.fp32_metrics(yard.double(), ref, u)
    return {"ratio": B.fp32_ratio(m, y), "vs_yard": B.yard_ratio(m, y), **m}


def link_check(t, out, taps):
    """Ties the z, fc1 and fc2 that start "x" returns to the forward of the same crops (fp32 storage): z against the
    float64 head conv of the device's own "b15.out" tap and swish(z) against the "head" tap, both at the head tap's bar;
    fc1 / fc2 against float64 from the "feat" tap (fc2 from the device's fc1).  taps: name -> flat device tap.
    -> (failures, figures)"""
    n = out["fc1"].shape[0]
    T = {k: torch.from_numpy(np.asarray(t[k], np.float32)) for k in ("head.w", "head.b", "fc1.w", "fc1.b", "fc2.w", "fc2.b")}
    T64 = {k: v.double() for k, v in T.items()}
    res = {}
    with torch.no_grad():
        x15 = _t(np.asarray(taps["b15.out"]).reshape(n * 49, 320), torch.float64)
        z = _t(out["z"], torch.float64).reshape(n * 49, GC_C)
        ref = x15 @ T64["head.w"].T + T64["head.b"]
        uz = x15.abs() @ T64["head.w"].abs().T + T64["head.b"].abs()
        res["z"] = _bar(z, ref, x15.float() @ T["head.w"].T + T["head.b"], uz)
        head = _t(np.asarray(taps["head"]).reshape(n * 49, GC_C), torch.float64)
        res["head"] = _bar(head, z * torch.sigmoid(z), z.float() * torch.sigmoid(z.float()), B._swish_mag(z, uz))
        src = _t(np.asarray(taps["feat"]).reshape(n, GC_C), torch.float64)
        for k in ("fc1", "fc2"):
            w, b = T64[k + ".w"], T64[k + ".b"]
            pre = src @ w.T + b
            yard = src.float() @ T[k + ".w"].T + T[k + ".b"]
            got = _t(out[k], torch.float64)
            res[k] = _bar(pre + (got - torch.relu(pre)), pre, yard, src.abs() @ w.abs().T + b.abs())      # ReLU: 1-Lipschitz
            src = got
    fails = [f"link {k}: past the fp32 bar: {m}" for k, m in res.items() if not m["ratio"] <= 1.0]
    return fails, {k: m["vs_yard"] for k, m in res.items()}

"""GPU: the three Grad-CAM launches of csrc/gradcam.hip one by one (dfd_gradcam_tap / Handle.gradcam_tap), each against a
float64 or exact reference of that launch evaluated from the device's own input to it (tests/gradcam_oracle.py):

  D1, G, cam7   the fp32 bars of b0_layer_oracle (rms <= 4x the float32 torch yardstick's + 2^-23, max |d| / u <= 8x its
                + 2^-21; cam7 at the bar of its pre-ReLU sum), guard rows behind row n - 1 intact, no sentinel left
  heat          bit-equal to the host restatement of the library's chain on the device's cam7, and within 1e-6 of an
                independent float64 torch-interpolate chain
  overlay       bit-equal to show_cam_on_image on the device's heat
  start "x"     z, fc1 and fc2 tied to the "b15.out", "head" and "feat" taps of the same crops (link_check)

on seeded and stress weights, random and edge crops, crafted degenerate inputs injected at start "z" (dead head, signed
zeros, constant map, single interior / corner peak, all-negative sums, z at +-100, a clamped overlay, unequal image
maxima), ragged batches n = 1, 7, 8, 9, 16 with fp32 and bf16 z, and the real bf16-storage path.
tests/test_gradcam_stage_oracle.py shows on the CPU that each of these checks fails for a named kernel defect.

Measured on the first MI355X run - worst HIP error / float32 yardstick error per stage (rms or max / u, whichever is
worse; the bar is 4x / 8x plus 1 / 4 ulps), heat as the absolute distance to the interpolate chain (bar 1e-6):
  seeded / random crops   D1 0.70  G 0.79  cam7 0.27  heat 1.6e-7   link: z 1.17  head 0.38  fc1 1.44  fc2 1.29
  seeded / edge crops     D1 0.64  G 0.68  cam7 0.24  heat 1.5e-7   link: z 1.14  head 0.32  fc1 1.31  fc2 1.58
  stress / random crops   D1 0.70  G 0.80  cam7 0.49  heat 1.5e-7   link: z 1.12  head 0.35  fc1 1.51  fc2 1.32
  stress / edge crops     D1 0.65  G 0.69  cam7 0.56  heat 1.8e-7   link: z 1.13  head 0.38  fc1 1.40  fc2 1.41
  crafted (start "z")     D1 0.74  G 0.79  cam7 2.08  heat 1.6e-7
  ragged, fp32 z          D1 0.77  G 0.91  cam7 0.29  heat 1.7e-7
  ragged, bf16 z          D1 0.77  G 0.91  cam7 0.29  heat 1.8e-7
  bf16 storage (real)     D1 0.71  G 0.80  cam7 0.46  heat 1.5e-7
  bf16 storage, cam7 against the float64 chain on the fp32 handle's tensors, of the peak: total 8.168e-2 = storage
  rounding 8.168e-2 (the float64 chain on the device's own bf16 tensors) + kernels 8.7e-7
heat and overlay were bit-equal to the library's arithmetic in every row; every guard row intact.  Bugs found: none.
"""
import numpy as np
import pytest

import b0_layer_oracle as B
import gradcam_oracle as GO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gc(pkg):
    from rtdfd_amd import gradcam

    return gradcam


@pytest.fixture(scope="module")
def crops():
    return {"random": B.random_crops(5), "edge": B.edge_crops()}


@pytest.fixture(scope="module")
def seeded_t(pkg, seeded_sd):
    return pkg.weights.pack_b0_tensors(seeded_sd)


@pytest.fixture(scope="module")
def seeded_runs(b0_handle, crops):
    """start "x" on the shared fp32 handle, once per crop set: the base of the crafted and the ragged cases too"""
    return {k: b0_handle.gradcam_tap(x=x, overlay=True) for k, x in crops.items()}


def _fmt(fig):
    return ", ".join(f"{k} {v:.3g}" for k, v in fig.items())


def _taps(h, x):
    n = x.shape[0]
    xd = h.alloc(x.nbytes).upload(x)
    try:
        return {name: h.tap(xd.ptr, n, name, n * 49 * 1280) for name in ("b15.out", "head", "feat")}
    finally:
        xd.free()


def _check_start_x(h, t, x, out, gc, label):
    n = x.shape[0]
    assert not out["z_bf16"] and out["z"].dtype == np.float32
    fails, fig = GO.check_outputs(t, out, n, gc, x)
    lf, lfig = GO.link_check(t, out, _taps(h, x))
    print(f"gradcam stages [{label}] / yardstick: {_fmt(fig)} (heat: abs to the interpolate chain); link: {_fmt(lfig)}")
    assert not fails and not lf, (label, fails, lf)
    # the tap launches what the product launches
    logits, heat, overlay, cam7 = h.gradcam(x, overlay=True, raw=True)
    assert np.array_equal(heat, out["heat"]) and np.array_equal(overlay, out["overlay"])
    assert np.array_equal(cam7.reshape(n, 49), out["cam7"])
    assert np.array_equal(logits, h.classify(x))


@pytest.mark.parametrize("which", ["random", "edge"])
def test_start_x_seeded(b0_handle, seeded_t, crops, seeded_runs, gc, which):
    _check_start_x(b0_handle, seeded_t, crops[which], seeded_runs[which], gc, f"seeded/{which}")
    if which == "edge":
        # the ReLU cuts on these crops and z leaves exp's float32 range
        pos = (seeded_runs[which]["cam7"] > 0).mean(axis=1)
        live = seeded_runs[which]["cam7"].max(axis=1) > 0
        assert pos[live].min() < 0.5 and np.abs(seeded_runs[which]["z"]).max() > 100, pos


def test_start_x_stress(pkg, ssd_sd, crops, gc):
    sd = B.stress_state_dict(0)
    t = pkg.weights.pack_b0_tensors(sd)
    assert np.abs(t["head.b"]).max() > 3                                 # the - b term carries weight
    h = pkg._lib.Handle(pkg.weights.pack_all(sd, ssd_sd), device=0, max_batch=16)
    try:
        for which, x in crops.items():
            _check_start_x(h, t, x, h.gradcam_tap(x=x, overlay=True), gc, f"stress/{which}")
    finally:
        h.close()


def test_crafted_cases(b0_handle, seeded_t, crops, seeded_runs, gc):
    base = seeded_runs["random"]
    worst = {}
    for c in GO.crafted_cases(seeded_t, (base["z"], base["fc1"], base["fc2"]), crops["random"]):
        out = b0_handle.gradcam_tap(x=c["x"], z=c["z"], fc1=c["fc1"], fc2=c["fc2"], overlay=c["overlay"])
        fails, fig = GO.check_outputs(seeded_t, out, 5, gc, c["x"])
        fails += GO.check_crafted(c, out, gc)
        assert not fails, (c["name"], fails)
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"gradcam stages [crafted] / yardstick: {_fmt(worst)}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_ragged_batches_keep_their_guards(b0_handle, seeded_t, seeded_runs, gc, bf16):
    """both template instances on the fp32 handle; z as bf16 bits is read exactly, so the fp32 bars hold"""
    a, b = seeded_runs["random"], seeded_runs["edge"]
    z, f1, f2 = GO.ragged_base(tuple(np.concatenate([a[k], b[k]]) for k in ("z", "fc1", "fc2")))
    if bf16:
        z = GO.rne_bits(z)
    worst = {}
    for n in GO.RAGGED_N:
        out = b0_handle.gradcam_tap(z=z[:n], fc1=f1[:n], fc2=f2[:n])
        assert out["z_bf16"] == bf16 and out["D1"].shape == (n, 512) and out["guard_cam7"].shape == (GO.GUARD, 49)
        fails, fig = GO.check_outputs(seeded_t, out, n, gc)
        assert not fails, (n, fails)
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"gradcam stages [ragged, {'bf16' if bf16 else 'fp32'} z] / yardstick: {_fmt(worst)}")


def test_bf16_storage_path(b0_handle, seeded_t, crops, seeded_runs, gc):
    """the real bf16 path: the kernels hold the fp32 bars on the device's own bf16 z; the end-to-end distance to the
    fp32-storage float64 oracle is split into what the storage rounding moved and what the kernels added"""
    x, base = crops["random"], seeded_runs["random"]
    b0_handle.set_option("bf16_activations", 1)
    try:
        out = b0_handle.gradcam_tap(x=x, overlay=True)
    finally:
        b0_handle.set_option("bf16_activations", 0)
    assert out["z_bf16"] and out["z"].dtype == np.uint16
    fails, fig = GO.check_outputs(seeded_t, out, 5, gc, x)
    want = np.maximum(GO.oracle64(seeded_t, base["z"], base["fc1"], base["fc2"])[1], 0)      # fp32 storage, float64 chain
    own = np.maximum(GO.oracle64(seeded_t, out["z"], out["fc1"], out["fc2"])[1], 0)          # the device's bf16 tensors, float64 chain
    peak = np.abs(want).max(axis=1)
    total, storage, kernels = (float((np.abs(a - b).max(axis=1) / peak).max())
                               for a, b in ((out["cam7"], want), (own, want), (out["cam7"], own)))
    print(f"gradcam stages [bf16 storage] / yardstick: {_fmt(fig)}; cam7 against the fp32-storage float64 oracle, of the peak: "
          f"total {total:.3e} = storage {storage:.3e} + kernels {kernels:.3e}")
    assert not fails, fails


def test_argument_checks(pkg, b0_handle, seeded_runs, crops):
    base = seeded_runs["random"]
    z, f1, f2 = base["z"], base["fc1"], base["fc2"]
    big = np.zeros((17, 49, 1280), np.float32)
    for kw, code in ((dict(z=big, fc1=np.zeros((17, 512)), fc2=np.zeros((17, 256))), -6),        # DFD_ERR_CAPACITY
                     (dict(x=np.zeros((17, 3, 224, 224), np.float32)), -6),
                     (dict(z=z, fc1=f1, fc2=f2, n=0), -1),                                       # DFD_ERR_ARG
                     (dict(x=crops["random"], n=0), -1),
                     (dict(z=z, fc1=None, fc2=f2), -1),
                     (dict(z=z, fc1=f1, fc2=None), -1),
                     (dict(z=None, x=None, fc1=f1, fc2=f2), -1),
                     (dict(z=z, fc1=f1, fc2=f2, overlay=True), -1)):                             # an overlay needs x
        with pytest.raises(pkg._lib.DfdError) as e:
            b0_handle.gradcam_tap(**kw)
        assert e.value.code == code, (kw.keys(), e.value.code)
    # the handle stays usable, and the refused calls launched nothing that leaked into it
    again = b0_handle.gradcam_tap(x=crops["random"], overlay=True)
    for k in ("z", "fc1", "fc2", "D1", "G", "cam7", "heat", "overlay"):
        assert np.array_equal(again[k], base[k]), k

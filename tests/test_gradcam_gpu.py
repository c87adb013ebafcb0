"""GPU: Grad-CAM of the head conv (dfd_gradcam_*, Handle.gradcam*, gradcam.GradCAM, DeepfakeDetector.explain_face)
against the CPU autograd oracle (tests/gradcam_oracle.py), with bit-equality of the logits to `classify`."""
import numpy as np
import pytest
import torch

import gradcam_oracle as GO

pytestmark = pytest.mark.gpu

CAM7_REL = 1e-3          # max |cam7 - oracle| / max |oracle|, fp32 handle
HEAT_ABS = 2e-3


@pytest.fixture(scope="module")
def gc(pkg):
    from rtdfd_amd import gradcam

    return gradcam


@pytest.fixture(scope="module")
def crops16():
    rs = np.random.RandomState(5)
    return rs.randn(16, 3, 224, 224).astype(np.float32)


@pytest.fixture(scope="module")
def oracle16(pkg, seeded_sd, crops16, gc):
    cam, logits, _ = GO.autograd_cam(pkg.weights.to_torch(seeded_sd), torch.from_numpy(crops16))
    return cam, logits, GO.heat_of(cam, gc)


def _check_maps(cam7, heat, want_cam, want_heat, cam_rel=CAM7_REL, heat_abs=HEAT_ABS):
    peak = np.abs(want_cam).reshape(len(want_cam), -1).max(axis=1)
    e7 = float((np.abs(cam7 - want_cam).reshape(len(want_cam), -1).max(axis=1) / peak).max())
    eh = float(np.abs(heat - want_heat).max())
    assert e7 <= cam_rel and eh <= heat_abs, (e7, eh)
    return e7, eh


@pytest.mark.parametrize("n", [1, 7, 16])
def test_logits_bitwise_equal_classify(b0_handle, crops16, n):
    x = crops16[:n]
    want = b0_handle.classify(x)
    logits, heat = b0_handle.gradcam(x)
    assert logits.shape == (n, 1) and heat.shape == (n, 224, 224) and heat.dtype == np.float32
    assert np.array_equal(logits, want)
    assert np.array_equal(b0_handle.classify(x), want)          # nothing leaks through the reused workspace


def test_maps_match_oracle_fp32(b0_handle, crops16, oracle16):
    want_cam, want_logits, want_heat = oracle16
    # the seeded weights give non-degenerate maps (the comparison cannot pass on all-zero maps)
    peaks = want_cam.reshape(16, -1).max(axis=1)
    pos = (want_cam > 0).reshape(16, -1).mean(axis=1)
    assert peaks.min() > 0.02 and pos.min() > 0.6, (peaks, pos)
    logits, heat, overlay, cam7 = b0_handle.gradcam(crops16, overlay=True, raw=True)
    assert cam7.shape == (16, 7, 7) and overlay.shape == (16, 224, 224, 3) and overlay.dtype == np.uint8
    assert np.abs(logits - want_logits).max() <= 1e-3
    e7, eh = _check_maps(cam7, heat, want_cam, want_heat)
    print(f"fp32 handle: cam7 rel err {e7:.2e}, heat abs err {eh:.2e}, peaks {peaks.min():.3f}..{peaks.max():.3f}, "
          f"positive cells {pos.min():.2f}..{pos.max():.2f}")
    assert heat.min() >= 0 and heat.max() <= 1 and np.all(heat.reshape(16, -1).max(axis=1) > 0.99)


def test_batch256_rows_against_oracle(pkg, seeded_sd, ssd_sd, gc):
    torch.manual_seed(1)
    x = torch.randn(256, 3, 224, 224)
    h = pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, ssd_sd), device=0, max_batch=256)
    try:
        h.warmup(256, 0)
        logits, heat, cam7 = h.gradcam(x.numpy(), raw=True)
        assert np.array_equal(logits, h.classify(x.numpy()))
        sd = pkg.weights.to_torch(seeded_sd)
        for lo in (0, 248):
            want_cam, _, _ = GO.autograd_cam(sd, x[lo:lo + 8])
            _check_maps(cam7[lo:lo + 8], heat[lo:lo + 8], want_cam, GO.heat_of(want_cam, gc))
    finally:
        h.close()


def test_bf16_handle(b0_handle, crops16, oracle16):
    want_cam, _, want_heat = oracle16
    b0_handle.set_option("bf16_activations", 1)
    try:
        want_logits = b0_handle.classify(crops16)
        logits, heat, cam7 = b0_handle.gradcam(crops16, raw=True)
        assert np.array_equal(logits, want_logits)
        peak = np.abs(want_cam).reshape(16, -1).max(axis=1)
        e7 = float((np.abs(cam7 - want_cam).reshape(16, -1).max(axis=1) / peak).max())
        eh = float(np.abs(heat - want_heat).max())
        print(f"bf16 handle: cam7 rel err {e7:.3e}, heat abs err {eh:.3e}")
        # measured on the first MI355X run: cam7 8.97e-2 of the peak, heat 8.67e-2 (bf16 z, then z - b cancels)
        assert e7 <= 0.15 and eh <= 0.15, (e7, eh)
    finally:
        b0_handle.set_option("bf16_activations", 0)


def test_reproducible(b0_handle, crops16):
    a = b0_handle.gradcam(crops16[:9], overlay=True, raw=True)
    b = b0_handle.gradcam(crops16[:9], overlay=True, raw=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_overlay_matches_host_show_cam(b0_handle, crops16, gc):
    x = crops16[:6]
    _, heat, overlay = b0_handle.gradcam(x, overlay=True)
    imgs = GO.denormalise(x)
    for i in range(6):
        want = gc.show_cam_on_image(imgs[i], heat[i], use_rgb=False)      # BGR image + BGR map = BGR overlay
        d = np.abs(overlay[i].astype(np.int16) - want.astype(np.int16))
        assert np.array_equal(overlay[i], want), (i, int(d.max()), int((d > 0).sum()))     # every cast truncates, as the library's
    # the heat map itself equals the host restatement applied to the device's raw map, bit for bit
    # (tests/test_gradcam_stages_gpu.py holds both equalities on every case it runs)
    _, heat2, cam7 = b0_handle.gradcam(x, raw=True)
    assert np.array_equal(GO.heat_of(cam7, gc), heat2)


def test_device_entry_point(b0_handle, crops16):
    x = crops16[:5]
    want = b0_handle.gradcam(x, overlay=True, raw=True)
    xd = b0_handle.alloc(x.nbytes).upload(x)
    ld, hd = b0_handle.alloc(5 * 4), b0_handle.alloc(5 * 224 * 224 * 4)
    od, cd = b0_handle.alloc(5 * 224 * 224 * 3), b0_handle.alloc(5 * 49 * 4)
    try:
        b0_handle.gradcam_device(xd.ptr, 5, ld.ptr, cd.ptr, hd.ptr, od.ptr)
        got = (ld.download((5, 1)), hd.download((5, 224, 224)), od.download((5, 224, 224, 3), np.uint8),
               cd.download((5, 7, 7)))
        for u, v in zip(got, want):
            assert np.array_equal(u, v)
        b0_handle.gradcam_device(xd.ptr, 5, ld.ptr)                # every map output optional
        assert np.array_equal(ld.download((5, 1)), want[0])
    finally:
        for b in (xd, ld, hd, od, cd):
            b.free()


def test_capacity(pkg, b0_handle, crops16):
    x = np.concatenate([crops16, crops16[:1]])
    with pytest.raises(pkg._lib.DfdError) as e:
        b0_handle.gradcam(x)
    assert e.value.code == -6                                        # DFD_ERR_CAPACITY
    assert np.array_equal(b0_handle.classify(crops16[:3]), b0_handle.gradcam(crops16[:3])[0])


def _mt_frame():
    rs = np.random.RandomState(11)
    frame = rs.randint(40, 215, (480, 640, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:480, 0:640]
    frame = np.clip(frame * 0.4 + (110 + 60 * np.sin(xx / 19.0) * np.cos(yy / 27.0))[..., None] * 0.6, 0, 255)
    # the last box is 12 px tall: the cascade never finds a face in it (tests/test_mtcnn_gpu.py)
    boxes = np.array([[20, 30, 300, 280], [330, 40, 200, 180], [100, 330, 90, 75], [400, 300, 230, 170],
                      [10, 440, 40, 12]], np.int32)
    return frame.astype(np.uint8), boxes


def test_gradcam_crops_mtcnn(mt_handle):
    frame, boxes = _mt_frame()
    want = mt_handle.classify_crops(frame, boxes, apply_clahe=True).reshape(-1)
    logits, heat, overlay, cam7 = mt_handle.gradcam_crops(frame, boxes, apply_clahe=True, overlay=True, raw=True)
    logits = logits.reshape(-1)
    assert np.array_equal(logits, want, equal_nan=True)
    kept = ~np.isnan(logits)
    assert kept.any() and not kept[-1]
    assert not heat[~kept].any() and not overlay[~kept].any() and not cam7[~kept].any()
    x = mt_handle.preprocess_crops(frame, boxes, apply_clahe=True)[kept]
    l2, h2, o2, c2 = mt_handle.gradcam(x, overlay=True, raw=True)
    assert np.array_equal(l2.reshape(-1), logits[kept])
    assert np.array_equal(h2, heat[kept]) and np.array_equal(o2, overlay[kept]) and np.array_equal(c2, cam7[kept])


def test_detector_explain_face(pkg, mt_handle):
    DeepfakeDetector = pkg.deepfake_detection.DeepfakeDetector
    frame, boxes = _mt_frame()
    det = DeepfakeDetector(enable_gradcam=True, use_tta=False, num_tta_augmentations=1, handle=mt_handle)
    seen = 0
    for x, y, w, h in boxes:
        face = np.ascontiguousarray(frame[y:y + h, x:x + w])
        res = det.explain_face(face)
        ref = det.analyze_face(face)
        assert ref[2] is None                                          # the reference's third slot, whatever enable_gradcam
        if ref[0] is None:
            assert res is None
            continue
        seen += 1
        assert res["fake_probability"] == ref[0]
        assert res["heatmap"].shape == (224, 224) and res["heatmap"].dtype == np.float32
        assert res["overlay"].shape == (224, 224, 3) and res["overlay"].dtype == np.uint8
    assert seen > 0


def test_gradcam_class_chunks(pkg, seeded_sd, crops16, gc):
    m = pkg.model.DeepfakeEfficientNet(max_batch=16, state_dict=seeded_sd)
    x = np.concatenate([crops16, crops16[::-1], crops16[:8]])      # B = 40
    try:
        cam = gc.GradCAM(model=m, target_layers=[m.get_feature_extractor()])
        got = cam(torch.from_numpy(x), targets=[gc.ClassifierOutputTarget(0)] * 40)
        assert got.shape == (40, 224, 224) and got.dtype == np.float32
        want = np.concatenate([m.handle.gradcam(x[i:i + 16])[1] for i in (0, 16, 32)])
        assert np.array_equal(got, want)
        assert np.array_equal(cam(x), got)
    finally:
        m.handle.close()

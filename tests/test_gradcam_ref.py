"""CPU: the Grad-CAM algebra the device runs (closed form on folded tensors) against torch autograd, the host
restatements of scale_cam_image / show_cam_on_image, and the public surface (gradcam.py, deepfake_detection
re-exports, C ABI declarations).  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import gradcam_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gc(pkg):
    from rtdfd_amd import gradcam

    return gradcam


@pytest.fixture(scope="module")
def crops():
    rs = np.random.RandomState(7)
    return (rs.randn(4, 3, 224, 224)).astype(np.float32)


def test_closed_form_matches_autograd(pkg, seeded_sd, crops):
    cam_ag, _, x15 = GO.autograd_cam(pkg.weights.to_torch(seeded_sd), torch.from_numpy(crops))
    cam_cf = GO.closed_form_cam(pkg.weights.pack_b0_tensors(seeded_sd), x15)
    assert cam_ag.shape == cam_cf.shape == (4, 7, 7)
    err = float(np.abs(cam_ag - cam_cf).max())
    assert err <= 1e-6, err
    # non-degenerate maps: the comparison cannot pass on all-zero maps
    for c in cam_ag:
        assert c.max() > 0.01 and (c > 0).mean() > 0.5, (c.max(), (c > 0).mean())


def test_scale_constant_map_is_zero(gc):
    out = gc.scale_cam_image(np.full((2, 7, 7), 0.3, np.float32), (224, 224))
    assert out.shape == (2, 224, 224) and out.dtype == np.float32
    assert not out.any()


def test_scale_corners_and_range(gc):
    rs = np.random.RandomState(1)
    m = rs.rand(3, 7, 7).astype(np.float32)
    out = gc.scale_cam_image(m, (224, 224))
    norm = gc.scale_cam_image(m)
    for o, n7 in zip(out, norm):
        assert o[0, 0] == n7[0, 0] and o[0, -1] == n7[0, -1] and o[-1, 0] == n7[-1, 0] and o[-1, -1] == n7[-1, -1]
        assert o.min() >= 0 and o.max() <= 1
    # the 7x7 normalisation itself: min 0, max just below 1
    assert np.all(norm.min(axis=(1, 2)) == 0) and np.all(norm.max(axis=(1, 2)) < 1)


def test_scale_symmetric_map_stays_symmetric(gc):
    rs = np.random.RandomState(2)
    m = rs.rand(7, 7).astype(np.float32)
    m = np.maximum(m, m[::-1])                      # exactly symmetric under both flips
    m = np.maximum(m, m[:, ::-1])
    out = gc.scale_cam_image(m[None], (224, 224))[0]
    np.testing.assert_array_equal(out, out[::-1])
    np.testing.assert_array_equal(out, out[:, ::-1])


def test_resize_inter_linear_weights(gc):
    """cv2 INTER_LINEAR 7 -> 224: dst 16 sits at source x = 16.5 / 32 - 0.5 = 0.015625 of the way from cell 0 to 1"""
    m = np.zeros((7, 7), np.float32)
    m[:, 1] = 1.0
    r = gc._resize_linear(m, (224, 224))
    assert r[0, 15] == 0.0 and r[0, 16] == np.float32(0.015625) and r[0, 47] == np.float32(0.984375)
    assert r[0, 48] == np.float32(0.984375) and r[0, 223] == 0.0     # cell 1's centre lies between dst 47 and 48


def test_show_cam_on_image_literal(gc, pkg):
    rs = np.random.RandomState(3)
    img = rs.rand(5, 6, 3).astype(np.float32)
    mask = rs.rand(5, 6).astype(np.float32)
    jet = pkg.luts.JET_BGR
    for use_rgb in (False, True):
        want = np.zeros((5, 6, 3), np.float32)
        for y in range(5):
            for x in range(6):
                bgr = jet[int(np.float32(255) * mask[y, x])]
                col = bgr[::-1] if use_rgb else bgr
                for c in range(3):
                    want[y, x, c] = np.float32(col[c]) / np.float32(255) + img[y, x, c]
        want = want / want.max()
        want = (np.float32(255) * want).astype(np.uint8)
        got = gc.show_cam_on_image(img, mask, use_rgb=use_rgb)
        np.testing.assert_array_equal(got, want)
    with pytest.raises(Exception):
        gc.show_cam_on_image(img * 2 + 1, mask)


def test_jet_table(pkg):
    jet = pkg.luts.JET_BGR
    assert jet.shape == (256, 3) and jet.dtype == np.uint8
    x = np.arange(256) / 255.0
    for c, k in enumerate((1, 2, 3)):
        want = np.floor(255 * np.clip(1.5 - np.abs(4 * x - k), 0, 1) + 0.5)
        np.testing.assert_array_equal(jet[:, c], want)
    # the device carries the same table (csrc/gradcam.hip)
    src = open(os.path.join(ROOT, "real-time-video-deepfake-detection_amd", "csrc", "gradcam.hip")).read()
    body = re.search(r"kJetBgr\[256\]\[3\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1)
    dev = np.array([int(v) for v in re.findall(r"\d+", body)], np.uint8).reshape(256, 3)
    np.testing.assert_array_equal(dev, jet)


def test_gradcam_argument_checks(pkg, gc):
    m = pkg.model.DeepfakeEfficientNet(max_batch=2)
    x = np.zeros((1, 3, 224, 224), np.float32)
    cam = gc.GradCAM(model=m, target_layers=[m.get_feature_extractor()], use_cuda=True)
    with pytest.raises(ValueError):
        gc.GradCAM(m, [m.net._fc[1]])
    with pytest.raises(ValueError):
        gc.GradCAM(m, [m.get_feature_extractor(), m.get_feature_extractor()])
    with pytest.raises(ValueError):
        gc.GradCAM(object(), [m.get_feature_extractor()])
    with pytest.raises(NotImplementedError):
        cam(x, aug_smooth=True)
    with pytest.raises(NotImplementedError):
        cam(x, eigen_smooth=True)
    with pytest.raises(ValueError):
        cam(x, targets=[gc.ClassifierOutputTarget(1)])
    with pytest.raises(ValueError):
        cam(np.zeros((1, 3, 112, 112), np.float32))
    assert m._handle is None                   # nothing above reached the device
    t = gc.ClassifierOutputTarget(0)
    assert t(np.array([[1.5], [2.5]]))[1] == 2.5 and t(np.array([4.0])) == 4.0


def test_reexports_and_abi_declarations(pkg, gc):
    from rtdfd_amd import deepfake_detection as dd

    assert dd.GradCAM is gc.GradCAM
    assert dd.ClassifierOutputTarget is gc.ClassifierOutputTarget
    assert dd.show_cam_on_image is gc.show_cam_on_image
    assert callable(dd.DeepfakeDetector.explain_face)
    hdr = open(os.path.join(ROOT, "include", "dfd_hip.h")).read()
    for name in ("dfd_gradcam_nchw_device", "dfd_gradcam_nchw", "dfd_gradcam_crops", "dfd_gradcam_tap"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pkg._lib.SIGNATURES, name
    for meth in ("gradcam", "gradcam_device", "gradcam_crops", "gradcam_tap"):
        assert callable(getattr(pkg._lib.Handle, meth)), meth

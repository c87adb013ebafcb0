"""Grad-CAM surface the reference imports from ``pytorch_grad_cam`` (reference deepfake_detection.py:5-7:
``GradCAM``, ``ClassifierOutputTarget``, ``show_cam_on_image``; requirements.txt ``grad-cam>=1.3.0``).

The classifier is a HIP forward without autograd, so `GradCAM` supports exactly the one layer the reference names as
its hook target, ``model.get_feature_extractor()`` (= ``net._conv_head``, reference model.py:100-102), and the logit
as target (``targets=None`` or ``ClassifierOutputTarget(0)``: the (B,1) output has one category).  The map is computed
on the GPU by `Handle.gradcam` (include/dfd_hip.h, csrc/gradcam.hip) from the closed form of the gradient; what it
returns is pytorch_grad_cam 1.3.x's ``grayscale_cam``: (B,224,224) float32 in [0,1].

`scale_cam_image` and `show_cam_on_image` are host numpy restatements of the library's utilities (cv2's
INTER_LINEAR resize and COLORMAP_JET restated, see `luts.JET_BGR`) for maps and images the caller brings; the device
computes the same formulas.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import luts
from .model import DeepfakeEfficientNet

COLORMAP_JET = 2          # cv2.COLORMAP_JET: the only colour map built


class ClassifierOutputTarget:
    """pytorch_grad_cam.utils.model_targets.ClassifierOutputTarget: the score of one output category."""

    def __init__(self, category: int):
        self.category = category

    def __call__(self, model_output):
        if len(model_output.shape) == 1:
            return model_output[self.category]
        return model_output[:, self.category]


def _resize_linear(m: np.ndarray, size) -> np.ndarray:
    """cv2.resize(m, (w, h)) with INTER_LINEAR on a float32 map: source x = (dx + 0.5) * sw / w - 0.5, clamped to the
    border (weight 0 on the missing neighbour); a horizontal pass a (1 - fx) + b fx, then the vertical one."""
    m = np.asarray(m, np.float32)
    w, h = size

    def axis(dst, src):
        f = ((np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        fr = (f - s.astype(np.float32)).astype(np.float32)
        lo = s < 0
        s[lo], fr[lo] = 0, 0
        hi = s >= src - 1
        s[hi], fr[hi] = src - 1, 0
        return s, np.minimum(s + 1, src - 1), fr

    x0, x1, fx = axis(w, m.shape[1])
    y0, y1, fy = axis(h, m.shape[0])
    one = np.float32(1)
    rows = m[:, x0] * (one - fx) + m[:, x1] * fx                      # (src h, w)
    return (rows[y0] * (one - fy)[:, None] + rows[y1] * fy[:, None]).astype(np.float32)


def scale_cam_image(cam, target_size=None) -> np.ndarray:
    """pytorch_grad_cam.utils.image.scale_cam_image (1.3.x): per map m - min, / (1e-7 + max), then cv2.resize."""
    result = []
    for img in np.asarray(cam, np.float32):
        img = img - np.min(img)
        img = img / (np.float32(1e-7) + np.max(img))
        if target_size is not None:
            img = _resize_linear(img, target_size)
        result.append(img)
    return np.float32(result)


def show_cam_on_image(img: np.ndarray, mask: np.ndarray, use_rgb: bool = False,
                      colormap: int = COLORMAP_JET) -> np.ndarray:
    """pytorch_grad_cam.utils.image.show_cam_on_image (1.3.x): JET(uint8(255 * mask)) / 255 + img, divided by the
    image's max, uint8(255 * .) (every uint8 cast truncates).  img: (H,W,3) float in [0,1], in BGR order unless
    use_rgb; the result has img's channel order."""
    if colormap != COLORMAP_JET:
        raise NotImplementedError("only COLORMAP_JET is built")
    heatmap = luts.JET_BGR[np.uint8(255 * np.asarray(mask, np.float32))]
    if use_rgb:
        heatmap = heatmap[..., ::-1]
    heatmap = np.float32(heatmap) / 255
    if np.max(img) > 1:
        raise Exception("The input image should np.float32 in the range [0, 1]")
    cam = heatmap + np.asarray(img, np.float32)
    cam = cam / np.max(cam)
    return np.uint8(255 * cam)


class GradCAM:
    """pytorch_grad_cam.GradCAM over the port's classifier.  ``model``: a `DeepfakeEfficientNet`;
    ``target_layers``: ``[model.get_feature_extractor()]`` (anything else raises ValueError).  ``use_cuda`` is
    accepted for signature parity (the map is always computed on the GPU)."""

    def __init__(self, model, target_layers: Sequence, use_cuda: bool = False):
        # by duck type: the package can be imported under two names (rtdfd_amd alias), each with its own class object
        if not (isinstance(model, DeepfakeEfficientNet) or
                (type(model).__name__ == "DeepfakeEfficientNet" and callable(getattr(model, "get_feature_extractor", None)))):
            raise ValueError(f"GradCAM: the model must be a DeepfakeEfficientNet, got {type(model).__name__}")
        layers = list(target_layers)
        if len(layers) != 1 or layers[0] is not model.get_feature_extractor():
            raise ValueError("GradCAM: only target_layers=[model.get_feature_extractor()] (net._conv_head) is supported")
        self.model = model
        self.target_layers = layers
        self.use_cuda = use_cuda

    def __call__(self, input_tensor, targets: Optional[Sequence] = None, aug_smooth: bool = False,
                 eigen_smooth: bool = False) -> np.ndarray:
        """(B,3,224,224) normalised input -> (B,224,224) float32 maps, in chunks of the handle's max_batch."""
        if aug_smooth or eigen_smooth:
            raise NotImplementedError("GradCAM: aug_smooth / eigen_smooth are not built")
        for t in targets or ():
            if not isinstance(t, ClassifierOutputTarget) or t.category != 0:
                raise ValueError("GradCAM: the classifier has one output; only ClassifierOutputTarget(0) is valid")
        x = input_tensor.detach().cpu().numpy() if hasattr(input_tensor, "detach") else input_tensor
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 4 or x.shape[1:] != (3, 224, 224):
            raise ValueError(f"GradCAM: expected (B,3,224,224) input, got {x.shape}")
        h = self.model.handle
        maps = [h.gradcam(x[i:i + h.max_batch])[1] for i in range(0, x.shape[0], h.max_batch)]
        return np.concatenate(maps, axis=0)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, exc_tb):
        return False


__all__ = ["GradCAM", "ClassifierOutputTarget", "show_cam_on_image", "scale_cam_image", "COLORMAP_JET"]

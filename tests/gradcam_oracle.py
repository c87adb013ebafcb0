"""Test-side Grad-CAM oracle (pytorch_grad_cam 1.3.x semantics, target layer net._conv_head, target = the logit):
torch autograd on CPU with the head conv's output A as a leaf, built from oracle.b0_ref's pieces; and the closed form
the device computes, on the folded tensors of weights.pack_b0_tensors."""
import numpy as np
import torch

from oracle import b0_ref


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

"""Test-side numpy oracle of the train-time augmentation chain (csrc/train_augment.hip): every stage restated from the
library the reference runs it through (Pillow for the uint8 stages, torch for the tensor stages), plus `chain`, which
applies the stages of a `rows` / `batch` table (train_augment.draw_batch) in the kernels' order and returns every tap.

test_train_augment_oracle.py holds each function to Pillow / torch on the CPU; test_train_augment_gpu.py holds the
kernels to these functions.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from oracle import jpeg_ref, mtcnn_ref
from rtdfd_amd import train_augment as TA

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


# ------------------------------------------------------------------------------------------------ uint8 stages
def jpeg_roundtrip(img: np.ndarray, quality: int, reference_channels: bool = True) -> np.ndarray:
    """libjpeg's 4:2:0 round trip of an RGB image at `quality` (oracle/jpeg_ref.py, which takes and returns BGR).  The
    reference's cv2 calls round-trip the channel-reversed image: its result has red and blue swapped."""
    if reference_channels:
        return np.ascontiguousarray(jpeg_ref.roundtrip_np(np.ascontiguousarray(img), int(quality))[..., ::-1])
    return np.ascontiguousarray(jpeg_ref.roundtrip_np(np.ascontiguousarray(img[..., ::-1]), int(quality))[..., ::-1])


def resize(img: np.ndarray, size: int) -> np.ndarray:
    """Image.resize((size, size), BILINEAR): the two 8-bit fixed-point passes"""
    return mtcnn_ref.pil_resize_bilinear(img, size, size)


def crop_flip(img: np.ndarray, x: int, y: int, t: int, flip: bool) -> np.ndarray:
    out = img[y:y + t, x:x + t]
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def luma(img: np.ndarray) -> np.ndarray:
    a = img.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.int64)


def blend(deg: np.ndarray, img: np.ndarray, f) -> np.ndarray:
    """Image.blend(degenerate, image, f): float32 d + f (v - d), clamped, truncated"""
    d = np.broadcast_to(deg, img.shape).astype(np.int64)
    o = d.astype(np.float32) + np.float32(f) * (img.astype(np.int64) - d).astype(np.float32)
    return np.clip(o, 0, 255).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros((), np.int64), img, f)


def contrast(img, f):
    l = luma(img)
    return blend(np.int64(int(int(l.sum()) / l.size + 0.5)), img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def rgb2hsv(img: np.ndarray) -> np.ndarray:
    """Pillow Convert.c rgb2hsv with its float / double promotions"""
    f32, f64 = np.float32, np.float64
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(f32)
    mx = np.where(maxc == 0, 1, maxc).astype(f32)
    s = cr / mx
    rc, gc, bc = ((maxc - r).astype(f32) / cr, (maxc - g).astype(f32) / cr, (maxc - b).astype(f32) / cr)
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32), (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)))
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(flat, 0, uh), np.where(flat, 0, us), maxc], -1).astype(np.uint8)


def _c_round(v: np.ndarray) -> np.ndarray:
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def hsv2rgb(hsv: np.ndarray) -> np.ndarray:
    f32, f64 = np.float32, np.float64
    uh, us, uv = (hsv[..., k].astype(np.int64) for k in range(3))
    hh = uh.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(hh).astype(np.int64)
    f = (hh - i.astype(f32).astype(f64)).astype(f32)
    fs = (us.astype(f32).astype(f64) / 255.0).astype(f32)
    v = uv.astype(f64)
    p = np.clip(_c_round(v * (1.0 - fs.astype(f64))), 0, 255)
    q = np.clip(_c_round(v * (1.0 - (fs * f).astype(f64))), 0, 255)
    t = np.clip(_c_round(v * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64)))), 0, 255)
    table = [(uv, t, p), (q, uv, p), (p, uv, t), (p, q, uv), (t, p, uv), (uv, p, q)]
    out = np.zeros(hsv.shape, np.int64)
    for k, (rr, gg, bb) in enumerate(table):
        m = (i % 6 == k)[..., None]
        out = np.where(m, np.stack([rr, gg, bb], -1), out)
    out = np.where((us == 0)[..., None], uv[..., None], out)
    return out.astype(np.uint8)


def hue(img, f):
    """torchvision adjust_hue on a PIL image: HSV, h += uint8(int32(f * 255)), back"""
    hsv = rgb2hsv(img)
    shift = int(float(np.float32(f)) * 255.0) & 255
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + shift) & 255).astype(np.uint8)
    return hsv2rgb(hsv)


def gray(img):
    return np.repeat(luma(img)[..., None], 3, -1).astype(np.uint8)


def _fix(v) -> int:
    return int(np.floor(v * 65536.0 + 0.5))


def affine_nearest(img: np.ndarray, m) -> np.ndarray:
    """Image.transform(size, AFFINE, m, NEAREST), fill 0: ImagingScaleAffine without rotation terms, affine_fixed otherwise"""
    h, w = img.shape[:2]
    m = [float(v) for v in m]
    out = np.zeros_like(img)
    if m[1] == 0.0 and m[3] == 0.0:
        def axis(start, step, n_out, n_in):
            tab, o = np.full(n_out, -1, np.int64), start
            for k in range(n_out):
                c = -1 if o < 0.0 else int(o)
                tab[k] = c if 0 <= c < n_in else -1
                o += step
            return tab
        xt, yt = axis(m[2] + m[0] * 0.5, m[0], w, w), axis(m[5] + m[4] * 0.5, m[4], h, h)
        xi, yi = np.broadcast_to(xt[None, :], (h, w)), np.broadcast_to(yt[:, None], (h, w))
    else:
        a0, a1, a3, a4 = _fix(m[0]), _fix(m[1]), _fix(m[3]), _fix(m[4])
        a2, a5 = _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
        x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
        xi, yi = (a2 + x * a0 + y * a1) >> 16, (a5 + x * a3 + y * a4) >> 16
    ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    out[ok] = img[yi[ok], xi[ok]]
    return out


def perspective(img: np.ndarray, c) -> np.ndarray:
    """Image.transform(size, PERSPECTIVE, c, BILINEAR), fill 0: double arithmetic, truncated"""
    h, w = img.shape[:2]
    c = [float(v) for v in c]
    xs, ys = np.arange(w, dtype=np.float64)[None, :] + 0.5, np.arange(h, dtype=np.float64)[:, None] + 0.5
    den = c[6] * xs + c[7] * ys + 1.0
    xin, yin = (c[0] * xs + c[1] * ys + c[2]) / den, (c[3] * xs + c[4] * ys + c[5]) / den
    ok = ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
    xin, yin = np.where(ok, xin, 0.5) - 0.5, np.where(ok, yin, 0.5) - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    x0, x1, y0 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1), np.clip(y, 0, h - 1)
    two = (y + 1 >= 0) & (y + 1 < h)
    yb = np.where(two, y + 1, y0)
    a, b = img[y0, x0].astype(np.float64), img[y0, x1].astype(np.float64)
    v1 = a + (b - a) * dx
    e, g = img[yb, x0].astype(np.float64), img[yb, x1].astype(np.float64)
    v2 = np.where(two[..., None], e + (g - e) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    return np.where(ok[..., None], out, 0).astype(np.uint8)


def blur_float64(img: np.ndarray, k_outer, k_centre) -> np.ndarray:
    """the 3 x 3 blur before rounding: reflect padding, float32 products of the weights, double accumulation"""
    k1 = np.array([k_outer, k_centre, k_outer], np.float32)
    p = np.pad(img.astype(np.float64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    h, w = img.shape[:2]
    acc = np.zeros(img.shape, np.float64)
    for i in range(3):
        for j in range(3):
            acc += float(np.float32(k1[i] * k1[j])) * p[i:i + h, j:j + w]
    return acc


def blur(img, k_outer, k_centre):
    return np.clip(np.rint(blur_float64(img, k_outer, k_centre)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ tensor stages
def normalize(img: np.ndarray) -> np.ndarray:
    v = img.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(((v - MEAN) / STD).transpose(2, 0, 1))


def erase(x: np.ndarray, box) -> np.ndarray:
    ex, ey, ew, eh = (int(v) for v in box)
    out = x.copy()
    out[:, ey:ey + eh, ex:ex + ew] = 0.0
    return out


def noise(x: np.ndarray, std, seed: int, counter: int, row: int, dtype=np.float64) -> np.ndarray:
    """clamp(x + std z, 0, 1); float64: the reference, float32: the same formula's yardstick"""
    z = TA.noise_normal(seed, counter, row, x.size, dtype=dtype).reshape(x.shape)
    return np.clip(x.astype(dtype) + dtype(np.float32(std)) * z, dtype(0), dtype(1))


def mix(x: np.ndarray, batch, dtype=np.float64) -> np.ndarray:
    kind = int(batch["mix_kind"])
    if kind == TA.MIX_NONE:
        return x.astype(dtype)
    perm = np.asarray(TA.batch_perm(batch))
    if kind == TA.MIX_MIXUP:
        lam = dtype(np.float32(batch["lam"]))
        return lam * x.astype(dtype) + (dtype(1) - lam) * x[perm].astype(dtype)
    x1, y1, x2, y2 = (int(v) for v in batch["box"])
    out = x.astype(dtype).copy()
    out[:, :, y1:y2, x1:x2] = x[perm][:, :, y1:y2, x1:x2]
    return out


# ------------------------------------------------------------------------------------------------ the chain
JITTER = {TA.JITTER_BRIGHTNESS: brightness, TA.JITTER_CONTRAST: contrast, TA.JITTER_SATURATION: saturation, TA.JITTER_HUE: hue}


def chain(rgb: np.ndarray, rows, batch, out_size: int, noise_dtype=np.float64) -> Dict[str, object]:
    """every tap of the kernels' chain: uint8 stages as lists of (T, T, 3) arrays ("jpeg": (H, W, 3); "resize": (S, S, 3) with S = T + 20 or
    T), float stages as (n, 3, T, T) arrays"""
    n, t = rgb.shape[0], out_size
    taps: Dict[str, object] = {k: [] for k in ("jpeg", "resize", "crop", "jitter0", "jitter1", "jitter2", "jitter3", "gray", "rotate",
                                                "affine", "perspective", "blur")}
    norm, er, no = [], [], []
    for i in range(n):
        r = rows[i]
        fl = int(r["flags"])
        img = jpeg_roundtrip(rgb[i], int(r["jpeg_quality"]), not fl & TA.F_JPEG_RGB) if fl & TA.F_JPEG else rgb[i]
        taps["jpeg"].append(img)
        img = resize(img, t + 20 if fl & TA.F_CROP else t)
        taps["resize"].append(img)
        img = crop_flip(img, int(r["crop_x"]), int(r["crop_y"]), t, bool(fl & TA.F_FLIP)) if fl & TA.F_CROP else crop_flip(img, 0, 0, t, bool(fl & TA.F_FLIP))
        taps["crop"].append(img)
        for k in range(4):
            op = int(r["jitter_op"][k])
            if op != TA.JITTER_NONE:
                img = JITTER[op](img, r["jitter_factor"][k])
            taps[f"jitter{k}"].append(img)
        if fl & TA.F_GRAY:
            img = gray(img)
        taps["gray"].append(img)
        if fl & TA.F_ROTATE:
            img = affine_nearest(img, r["rotate"])
        taps["rotate"].append(img)
        if fl & TA.F_AFFINE:
            img = affine_nearest(img, r["affine"])
        taps["affine"].append(img)
        if fl & TA.F_PERSPECTIVE:
            img = perspective(img, r["perspective"])
        taps["perspective"].append(img)
        if fl & TA.F_BLUR:
            img = blur(img, r["blur_k"][0], r["blur_k"][1])
        taps["blur"].append(img)
        x = normalize(img)
        norm.append(x)
        if fl & TA.F_ERASE:
            x = erase(x, r["erase"])
        er.append(x)
        x = x.astype(noise_dtype)
        if fl & TA.F_NOISE:
            x = noise(er[-1], r["noise_std"], int(batch["seed"]), int(batch["counter"]), i, dtype=noise_dtype)
        no.append(x)
    taps["norm"], taps["erase"], taps["noise"] = np.stack(norm), np.stack(er), np.stack(no)
    taps["mix"] = mix(taps["noise"], batch, dtype=noise_dtype)
    return taps

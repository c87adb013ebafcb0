"""Train-time image augmentation: the host half (policy, parameter draws, noise specification).

The arithmetic of the chain runs in libdfd_hip.so (csrc/train_augment.hip, `dfd_train_augment*` in include/dfd_hip.h,
DESIGN 4h); this module draws the per-image parameter rows the kernels read.  The chain is the reference's training
transform (train.py:462-489, 282-349): the JPEG round trip, Resize(T + 20), RandomCrop(T), flip, ColorJitter, RandomGrayscale,
RandomRotation, RandomAffine, RandomPerspective, GaussianBlur, ToTensor / Normalize, RandomErasing, GaussianNoise and
Mixup / CutMix over the batch.

Three reference quirks are reproduced: JPEGAugmentation hands its RGB array to cv2.imencode, which reads BGR, and
converts BGR2RGB after decoding - the result is the round trip of the channel-reversed image, red and blue swapped
(`jpeg_reference_channels=False` round-trips the image itself); GaussianNoise clamps the NORMALISED tensor to [0, 1] (train.py:309 after
Normalize, :510), which zeroes every below-mean pixel of a noised image; Mixup uses lam = max(lam, 1 - lam).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np

from .head_training import _fmix32, _u32

# dfd_train_aug_image.flags
F_JPEG, F_CROP, F_FLIP, F_GRAY, F_ROTATE, F_AFFINE, F_PERSPECTIVE, F_BLUR, F_ERASE, F_NOISE, F_JPEG_RGB = (1 << k for k in range(11))
JITTER_NONE, JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = range(5)
MIX_NONE, MIX_MIXUP, MIX_CUTMIX = range(3)
MARGIN = 20                       # Resize(T + 20) before RandomCrop(T)

# `dfd_train_aug_image` / `dfd_train_aug_batch` (include/dfd_hip.h); the library asserts the same sizes
ROW_DTYPE = np.dtype([("rotate", "<f8", 6), ("affine", "<f8", 6), ("perspective", "<f8", 8), ("flags", "<u4"),
                      ("jpeg_quality", "<i4"), ("crop_x", "<i4"), ("crop_y", "<i4"), ("jitter_op", "<i4", 4),
                      ("jitter_factor", "<f4", 4), ("blur_k", "<f4", 2), ("erase", "<i4", 4), ("noise_std", "<f4"),
                      ("reserved", "<i4")])
BATCH_DTYPE = np.dtype([("seed", "<u8"), ("counter", "<u8"), ("perm", "<u8"), ("mix_kind", "<i4"), ("lam", "<f4"),
                        ("box", "<i4", 4)])
assert ROW_DTYPE.itemsize == 240 and BATCH_DTYPE.itemsize == 48


class Batch(np.ndarray):
    """a 0-d BATCH_DTYPE record; `partners` holds the int32 permutation its `perm` pointer is set to at call time"""
    partners: Optional[np.ndarray] = None

    def __array_finalize__(self, obj):
        self.partners = getattr(obj, "partners", None)


def new_batch(seed: int = 0, counter: int = 0) -> Batch:
    b = np.zeros((), BATCH_DTYPE).view(Batch)
    b["seed"], b["counter"] = np.uint64(seed), np.uint64(counter)
    return b


def batch_perm(batch) -> Optional[np.ndarray]:
    return getattr(batch, "partners", None)


@dataclasses.dataclass
class AugmentPolicy:
    """train.py's probabilities and ranges (:462-489).  Stages without a coin in the reference are booleans."""
    jpeg_p: float = 0.5
    jpeg_quality: Tuple[int, int] = (20, 75)
    jpeg_reference_channels: bool = True      # the reference round-trips the channel-reversed image (cv2 reads RGB as BGR)
    crop: bool = True                         # Resize(T + 20) + RandomCrop(T); False: Resize(T), the validation transform
    flip_p: float = 0.5
    jitter: bool = True
    brightness: float = 0.3
    contrast: float = 0.3
    saturation: float = 0.25
    hue: float = 0.08
    gray_p: float = 0.08
    rotate: bool = True
    degrees: float = 15.0
    affine: bool = True
    translate: Tuple[float, float] = (0.08, 0.08)
    scale: Tuple[float, float] = (0.9, 1.1)
    perspective_p: float = 0.3
    distortion: float = 0.15
    blur_p: float = 0.2
    blur_sigma: Tuple[float, float] = (0.1, 1.5)
    erase_p: float = 0.25
    erase_scale: Tuple[float, float] = (0.02, 0.2)
    erase_ratio: Tuple[float, float] = (0.3, 3.3)
    noise_p: float = 0.3
    noise_std: Tuple[float, float] = (0.01, 0.04)

    @classmethod
    def validation(cls) -> "AugmentPolicy":
        """every stage off: Resize(T) alone (train.py:491-496)"""
        return cls(jpeg_p=0.0, crop=False, flip_p=0.0, jitter=False, gray_p=0.0, rotate=False, affine=False, perspective_p=0.0,
                   blur_p=0.0, erase_p=0.0, noise_p=0.0)


class ResidentCrops:
    """A training set of (N, H, W, 3) uint8 crops kept in HBM across epochs: uploaded once, `gather(idx)` makes the
    contiguous batch `Handle.train_augment_features` reads, device to device.  `fit_loop(..., augment=...)` takes it in
    place of the host array (on the handle that extracts).  `free()` it, or use it as a context manager."""

    def __init__(self, handle, crops):
        a = np.ascontiguousarray(np.asarray(crops))
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[0] < 1:
            raise ValueError(f"expected (N,H,W,3) uint8 crops, got {a.dtype} {a.shape}")
        self.handle, self.shape, self.dtype, self.ndim = handle, a.shape, a.dtype, 4
        self._set = handle.alloc(a.nbytes).upload(a)
        self._batch = None

    def gather(self, idx):
        """-> (DeviceBuffer holding crops `idx` contiguously, (n, H, W)); the buffer is reused by the next call"""
        idx = np.asarray(idx).reshape(-1)
        need = idx.size * self.shape[1] * self.shape[2] * 3
        if self._batch is None or self._batch.nbytes < need:
            if self._batch is not None:
                self._batch.free()
            self._batch = self.handle.alloc(need)
        self.handle.train_augment_gather(self._set, self.shape[:3], idx, self._batch)
        return self._batch, (idx.size, self.shape[1], self.shape[2])

    def free(self):
        for b in (self._set, self._batch):
            if b is not None:
                b.free()
        self._set = self._batch = None

    def __enter__(self):
        return self

    def __exit__(self, *_exc):
        self.free()


# ------------------------------------------------------------------------------------------------ matrices
def rotate_matrix(angle_deg: float, w: int, h: int):
    """the six coefficients Image.rotate(angle) hands to transform(AFFINE): cos / sin rounded to 15 places, centre (w/2, h/2)"""
    a = -math.radians(angle_deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def inverse_affine_matrix(center, angle: float, translate, scale: float, shear=(0.0, 0.0)):
    """torchvision.transforms.functional._get_inverse_affine_matrix"""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def perspective_coeffs(startpoints, endpoints):
    """torchvision's _get_perspective_coeffs: the eight coefficients mapping output (end) points to input (start) points,
    a float64 least-squares solve.  The float64 solution is kept; torchvision rounds it to float32 before it hands the
    coefficients to Pillow."""
    a = np.zeros((8, 8), np.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i] = [p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]]
        a[2 * i + 1] = [0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]]
    b = np.asarray(startpoints, np.float64).reshape(8)
    return np.linalg.lstsq(a, b, rcond=None)[0].tolist()


def blur_weights(sigma: float):
    """torchvision _get_gaussian_kernel1d(3, sigma) in float32 -> (outer tap, centre tap)"""
    import torch       # torch's float32 exp, so that the weights are torchvision's to the bit

    x = torch.linspace(-1.0, 1.0, 3)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    k = (pdf / pdf.sum()).numpy()
    return float(k[0]), float(k[1])


def cutmix_box(lam: float, cy: int, cx: int, size: int):
    """train.py:335-348: the clipped box (x1, y1, x2, y2) and lam recomputed from it"""
    ratio = np.sqrt(1.0 - lam)
    cut_h, cut_w = int(size * ratio), int(size * ratio)
    y1, y2 = max(0, cy - cut_h // 2), min(size, cy + cut_h // 2)
    x1, x2 = max(0, cx - cut_w // 2), min(size, cx + cut_w // 2)
    return (x1, y1, x2, y2), 1.0 - (y2 - y1) * (x2 - x1) / (size * size)


# ------------------------------------------------------------------------------------------------ the draws
def draw_batch(policy: AugmentPolicy, rng: np.random.RandomState, n: int, H: int, W: int, out_size: int = 224, mix=None):
    """Parameter rows of `n` images and the batch record -> (rows: ROW_DTYPE (n,), batch: Batch).

    Every parameter follows torchvision's `get_params` of the transform it belongs to.  torchvision draws from torch's
    and Python's global generators, whose order cannot be reproduced here (and torchvision is not a dependency): the
    distributions are the reference's, the stream is this module's.  All draws come from `rng`, in this order:

      once per call   randint(2^32) twice: the low and high word of the noise seed (counter = 0)
      per image, in image order:
        jpeg            random_sample() <= jpeg_p; when taken randint over the quality range, both ends included
        crop            randint(21) for y, then for x                                 (policy.crop)
        flip            random_sample() < flip_p
        jitter          permutation(4) (the order of brightness, contrast, saturation, hue), then uniform() for the
                        brightness, contrast, saturation and hue factor - all four always  (policy.jitter)
        gray            random_sample() < gray_p
        rotate          uniform(-degrees, degrees)                                     (policy.rotate)
        affine          uniform(-max_dx, max_dx), uniform(-max_dy, max_dy), each rounded to an int; uniform(scale)
        perspective     random_sample() < perspective_p; when taken eight randint: top-left x, y, top-right x, y,
                        bottom-right x, y, bottom-left x, y
        blur            random_sample() < blur_p; when taken uniform(sigma)
        erase           random_sample() < erase_p; when taken up to ten attempts of uniform(scale), uniform(log ratio) and,
                        for a box that fits, randint for y and for x (no fitting box: nothing is erased)
        noise           random_sample() <= noise_p; when taken uniform(std)
    A coin whose probability is 0 is still drawn; a stage switched off by a boolean draws nothing.

    `mix`: None or (kind, lam, partners[, box]) as `head_training.fit_loop` draws them (MIX_MIXUP / MIX_CUTMIX)."""
    t = int(out_size)
    rows = np.zeros(n, ROW_DTYPE)
    seed = int(rng.randint(0, 2 ** 32, dtype=np.uint64)) | (int(rng.randint(0, 2 ** 32, dtype=np.uint64)) << 32)
    batch = new_batch(seed, 0)
    for r in rows:
        flags = 0
        if rng.random_sample() <= policy.jpeg_p and policy.jpeg_p > 0:
            flags |= F_JPEG if policy.jpeg_reference_channels else F_JPEG | F_JPEG_RGB
            r["jpeg_quality"] = rng.randint(policy.jpeg_quality[0], policy.jpeg_quality[1] + 1)
        if policy.crop:
            flags |= F_CROP
            r["crop_y"] = rng.randint(0, MARGIN + 1)
            r["crop_x"] = rng.randint(0, MARGIN + 1)
        if rng.random_sample() < policy.flip_p:
            flags |= F_FLIP
        if policy.jitter:
            order = rng.permutation(4)
            f = [rng.uniform(max(0.0, 1 - policy.brightness), 1 + policy.brightness),
                 rng.uniform(max(0.0, 1 - policy.contrast), 1 + policy.contrast),
                 rng.uniform(max(0.0, 1 - policy.saturation), 1 + policy.saturation), rng.uniform(-policy.hue, policy.hue)]
            for k, fn in enumerate(order):
                r["jitter_op"][k] = JITTER_BRIGHTNESS + int(fn)
                r["jitter_factor"][k] = f[int(fn)]
        if rng.random_sample() < policy.gray_p:
            flags |= F_GRAY
        if policy.rotate:
            angle = float(rng.uniform(-policy.degrees, policy.degrees))
            if angle % 360.0 != 0.0:                       # Image.rotate returns a copy for a zero angle
                flags |= F_ROTATE
                r["rotate"] = rotate_matrix(angle, t, t)
        if policy.affine:
            max_dx, max_dy = float(policy.translate[0] * t), float(policy.translate[1] * t)
            tx, ty = int(round(rng.uniform(-max_dx, max_dx))), int(round(rng.uniform(-max_dy, max_dy)))
            sc = float(rng.uniform(policy.scale[0], policy.scale[1]))
            flags |= F_AFFINE
            r["affine"] = inverse_affine_matrix((t * 0.5, t * 0.5), 0.0, (tx, ty), sc)
        if rng.random_sample() < policy.perspective_p:
            hw, d = t // 2, policy.distortion
            lo = int(d * hw)
            tl = [rng.randint(0, lo + 1), rng.randint(0, lo + 1)]
            tr = [rng.randint(t - lo - 1, t), rng.randint(0, lo + 1)]
            br = [rng.randint(t - lo - 1, t), rng.randint(t - lo - 1, t)]
            bl = [rng.randint(0, lo + 1), rng.randint(t - lo - 1, t)]
            start = [[0, 0], [t - 1, 0], [t - 1, t - 1], [0, t - 1]]
            flags |= F_PERSPECTIVE
            r["perspective"] = perspective_coeffs(start, [[int(v) for v in p] for p in (tl, tr, br, bl)])
        if rng.random_sample() < policy.blur_p:
            flags |= F_BLUR
            r["blur_k"] = blur_weights(float(rng.uniform(policy.blur_sigma[0], policy.blur_sigma[1])))
        if rng.random_sample() < policy.erase_p:
            area = t * t
            lr = (math.log(policy.erase_ratio[0]), math.log(policy.erase_ratio[1]))
            for _ in range(10):
                ea = area * float(rng.uniform(policy.erase_scale[0], policy.erase_scale[1]))
                aspect = math.exp(float(rng.uniform(lr[0], lr[1])))
                eh, ew = int(round(math.sqrt(ea * aspect))), int(round(math.sqrt(ea / aspect)))
                if not (eh < t and ew < t):
                    continue
                ey = int(rng.randint(0, t - eh + 1))
                ex = int(rng.randint(0, t - ew + 1))
                flags |= F_ERASE
                r["erase"] = (ex, ey, ew, eh)
                break
        if rng.random_sample() <= policy.noise_p and policy.noise_p > 0:
            flags |= F_NOISE
            r["noise_std"] = rng.uniform(policy.noise_std[0], policy.noise_std[1])
        r["flags"] = flags
    if mix is not None:
        kind, lam, partners = int(mix[0]), float(mix[1]), np.ascontiguousarray(np.asarray(mix[2], np.int32))
        if partners.shape != (n,):
            raise ValueError("one partner per image")
        batch["mix_kind"], batch["lam"] = kind, lam
        if kind == MIX_CUTMIX:
            batch["box"] = tuple(int(v) for v in mix[3])
        batch.partners = partners
    return rows, batch


# ------------------------------------------------------------------------------------------------ noise
def noise_words(seed: int, counter: int, row: int, count: int):
    """the two uint32 words behind element i = 0 .. count-1 of image `row`:

    key   = fmix(fmix(fmix(fmix(fmix(seed_lo + 0x9E3779B9) ^ seed_hi) ^ counter_lo) ^ counter_hi) ^ (row + 1))
    u1(i) = fmix(fmix(2 i ^ key) + key),   u2(i) = fmix(fmix((2 i + 1) ^ key) + key)
    in uint32 arithmetic (fmix = MurmurHash3's finaliser, as in head_training.dropout_keep_mask); i = (c T + y) T + x."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        k = _fmix32(_u32(seed) + np.uint32(0x9E3779B9))
        k = _fmix32(k ^ _u32(seed >> 32))
        k = _fmix32(k ^ _u32(counter))
        k = _fmix32(k ^ _u32(counter >> 32))
        k = _fmix32(k ^ _u32(row + 1))
        idx = np.arange(count, dtype=np.uint32) * np.uint32(2)
        u1 = _fmix32(_fmix32(idx ^ k) + k)
        u2 = _fmix32(_fmix32((idx + np.uint32(1)) ^ k) + k)
    return u1, u2


def noise_normal(seed: int, counter: int, row: int, count: int, dtype=np.float64) -> np.ndarray:
    """The specification of stage 12's z: Box-Muller on the two words of `noise_words`,

    a = ((u1 >> 8) + 1) 2^-24  in (0, 1],   b = (u2 >> 8) 2^-24  in [0, 1),   z = sqrt(-2 ln a) cos(c b),  c = float32(2 pi)
    a, b and c are exact float32 values; the kernels evaluate z in float32 (`dtype=np.float32` here does the same with
    numpy's functions), `dtype=np.float64` is the reference the float32 results are held to."""
    u1, u2 = noise_words(seed, counter, row, count)
    a = (((u1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24).astype(dtype)
    b = ((u2 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(dtype)
    c = dtype(np.float32(6.2831855))
    return (np.sqrt(dtype(-2.0) * np.log(a)) * np.cos(c * b)).astype(dtype)


__all__ = ["AugmentPolicy", "ResidentCrops", "draw_batch", "noise_normal", "noise_words", "new_batch", "batch_perm", "rotate_matrix",
           "inverse_affine_matrix", "perspective_coeffs", "blur_weights", "cutmix_box", "ROW_DTYPE", "BATCH_DTYPE"]

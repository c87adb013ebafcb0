"""Test helper (CPU): references, yardsticks, bars and cases for the any-size frequency-domain kernels
(csrc/freq_domain.hip): the reference's `analyze_frequency_domain` (deepfake_detection.py:457-487) restated in numpy
float64, the fp32 yardsticks (scipy's complex64 FFT and float32 DCT of the float32 plane), and a float64 reference of
`compute_frequency_features` (oracle.imgproc_ref's own feeds scipy a float32 plane for its DCT channel, so its channel 1
is itself fp32; here both transforms run in float64 on the oracle's gray and resize).

Device layouts: "rows" and "spectrum" of a window are [w][h] = [kx][ky] (see dfd_frequency_domain_tap in
include/dfd_hip.h); the helpers return the references in the same layouts."""
import numpy as np

import frames as F
from oracle import imgproc_ref as I

EPS64 = 2.0 ** -53
FFT_RMS_X, FFT_MAX_X = 4.0, 8.0         # tests/forensic_oracle.py: times the fp32 yardstick's error against float64
FEATURE_MAX, FEATURE_MEAN = 2e-3, 1e-4  # tests/test_freq_gpu.py's bars for size 224
THRESHOLD, BOOST = 0.15, 0.15
MAX_SIDE = 4096


# ------------------------------------------------------------------------------------------------ the check
def mask_size(h, w):
    return min(h, w) // 4


def signed(n):
    """signed frequency of bin k of an n-point transform: k for k < ceil(n / 2), else k - n"""
    k = np.arange(n)
    return np.where(k < (n + 1) // 2, k, k - n)


def mask_unshifted(h, w):
    """[h][w] bool, True on the bins the reference zeroes, in bin order: both signed frequencies in [-m, m)"""
    m = mask_size(h, w)
    sy, sx = signed(h), signed(w)
    return ((sy >= -m) & (sy < m))[:, None] & ((sx >= -m) & (sx < m))[None, :]


def mask_reference(h, w):
    """the same mask as the reference builds it: a slice of the shifted spectrum, moved back to bin order"""
    m = mask_size(h, w)
    z = np.zeros((h, w), bool)
    ch, cw = h // 2, w // 2
    z[ch - m:ch + m, cw - m:cw + m] = True
    return np.fft.ifftshift(z)


def reference(gray):
    """the reference's arithmetic on a uint8 gray window -> dict(high, total, ratio, verdict), float64"""
    f_shift = np.fft.fftshift(np.fft.fft2(gray))
    magnitude = np.abs(f_shift)
    h, w = magnitude.shape
    ch, cw = h // 2, w // 2
    high_region = magnitude.copy()
    m = min(h, w) // 4
    high_region[ch - m:ch + m, cw - m:cw + m] = 0
    high, total = float(np.sum(high_region)), float(np.sum(magnitude))
    ratio = high / (total + 1e-10)
    return {"high": high, "total": total, "ratio": ratio, "verdict": BOOST if ratio < THRESHOLD else 0.0}


def verdict(high, total):
    return BOOST if float(high) / (float(total) + 1e-10) < THRESHOLD else 0.0


def bgr_of(gray):
    """a BGR crop whose cv2 gray is `gray`: (g * 16384 + 8192) >> 14 == g"""
    return np.ascontiguousarray(np.repeat(gray[..., None], 3, -1))


# ------------------------------------------------------------------------------------------------ transforms
def fft_float64(g):
    """(rows, spectrum) in float64, in the device's transposed layouts [w][h]"""
    g64 = g.astype(np.float64)
    return np.fft.fft(g64, axis=1).T, np.fft.fft2(g64).T


def fft_yardstick(g):
    """the fp32 yardstick: scipy's complex64 transforms of the float32 plane, same layouts"""
    import scipy.fft

    g32 = g.astype(np.float32)
    a, b = scipy.fft.fft(g32, axis=1).T, scipy.fft.fft2(g32).T
    assert a.dtype == np.complex64 and b.dtype == np.complex64
    return a, b


def fft_error(got, ref64):
    """(rms, max) of |got - ref64| over a rectangle of any shape"""
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    d = np.abs(np.asarray(got).astype(np.complex128) - ref64)
    return float(np.sqrt(np.mean(d * d))), float(d.max())


def fft_ratios(got, ref64, yard):
    """(rms ratio, max ratio) of got's error to the yardstick's; a zero yardstick error demands a zero error"""
    (r, m), (yr, ym) = fft_error(got, ref64), fft_error(yard, ref64)
    q = lambda a, b: 0.0 if a == 0 else (np.inf if b == 0 else a / b)
    return q(r, yr), q(m, ym)


def meets_bar(ratios):
    return ratios[0] <= FFT_RMS_X and ratios[1] <= FFT_MAX_X


def sums_of_mag(mag_wh, h, w):
    """float64 (high, total) of a float32 magnitude array in the device layout [w][h]"""
    m64 = np.asarray(mag_wh, np.float64).T
    return float(m64[~mask_unshifted(h, w)].sum()), float(m64.sum())


# ------------------------------------------------------------------------------------------------ features
def feature_gray(img, size):
    g = I.bgr2gray_u8(img) if img.ndim == 3 else img
    return I.resize_linear_u8(g, size, size)


def _norm(a):
    lo, hi = a.min(), a.max()
    return (a - lo) / (hi - lo) if hi - lo > 1e-6 else np.zeros_like(a)


def features_float64(img, size):
    """-> (features [2][S][S] float64, spectrum [kx][ky] complex128 unshifted, dct [ky][kx] float64)"""
    from scipy.fft import dctn

    g = feature_gray(img, size).astype(np.float64)
    spec = np.fft.fft2(g)
    d = dctn(g / 255.0, type=2, norm="ortho")
    assert d.dtype == np.float64
    f = np.stack([_norm(np.log1p(np.abs(np.fft.fftshift(spec)))), _norm(np.log1p(np.abs(d)))])
    return f, spec.T, d


def features_yardstick(img, size):
    """fp32: (features, spectrum [kx][ky] complex64, dct float32) from scipy on the float32 plane"""
    import scipy.fft

    g = feature_gray(img, size).astype(np.float32)
    spec = scipy.fft.fft2(g)
    d = scipy.fft.dctn(g / np.float32(255.0), type=2, norm="ortho")
    assert spec.dtype == np.complex64 and d.dtype == np.float32
    f = np.stack([_norm(np.log1p(np.abs(np.fft.fftshift(spec)))), _norm(np.log1p(np.abs(d)))]).astype(np.float32)
    return f, spec.T, d


FEATURE_SIZES = (2, 16, 30, 64, 126, 250, 258, 512)
FEATURE_SIZE_MAX = 1024


def feature_images():
    """four of the images tests/test_freq_gpu.py runs at 224"""
    return {"rand300": np.random.RandomState(5).randint(0, 255, (300, 300, 3)).astype(np.uint8),
            "face": F.face_frame(), "gradient": F.gradient_image(), "natural224": F.natural_like(224, 224, 9)}


# ------------------------------------------------------------------------------------------------ cases
SHAPES = ((1, 1), (1, 7), (2, 2), (3, 5),                   # m = 0; sides below one tile
          (15, 17), (16, 16), (17, 16),                     # either side of a tile
          (31, 33), (48, 64), (65, 63),                     # the 64-column group border
          (97, 113),                                        # primes
          (160, 120), (257, 255),                           # table longer than the block
          (300, 20), (2, 4096), (4095, 3))                  # the length limit


def random_window(h, w):
    return np.random.RandomState(1000 * h + w).randint(0, 256, (h, w)).astype(np.uint8)


def constant_window(h=48, w=64, v=137):
    return np.full((h, w), v, np.uint8)


def lit_pixel(h=31, w=33, y=5, x=7):
    g = np.zeros((h, w), np.uint8)
    g[y, x] = 255
    return g


def gaussian_blob(h=120, w=100):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = (yy - h / 2.0) ** 2 + (xx - w / 2.0) ** 2
    return np.clip(128 + 100 * np.exp(-r2 / (2 * 25.0 ** 2)), 0, 255).astype(np.uint8)


def gradient_window():
    return I.bgr2gray_u8(F.gradient_image())


def natural_window(h=160, w=120):
    return I.bgr2gray_u8(F.natural_like(h, w, 3))


_CASES = None


def cases():
    """name -> uint8 gray window [h][w]: a random window at every shape, and one window of each special kind"""
    global _CASES
    if _CASES is None:
        c = {f"random_{h}x{w}": random_window(h, w) for h, w in SHAPES}
        c["constant_48x64"] = constant_window()
        c["lit_pixel_31x33"] = lit_pixel()
        c["gaussian_120x100"] = gaussian_blob()
        c["gradient_256x256"] = gradient_window()
        c["natural_160x120"] = natural_window()
        _CASES = c
    return _CASES


_REFS = {}


def case_reference(name):
    """computed once per case and shared: dict(ref, rows64, spec64, rows_yard, spec_yard)"""
    if name not in _REFS:
        g = cases()[name]
        r64, s64 = fft_float64(g)
        ry, sy = fft_yardstick(g)
        _REFS[name] = {"ref": reference(g), "rows64": r64, "spec64": s64, "rows_yard": ry, "spec_yard": sy}
    return _REFS[name]

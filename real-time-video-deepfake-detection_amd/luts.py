"""Integer lookup tables of the 8-bit colour conversions, generated on the host and shipped
to the GPU inside the weights blob (as exactly-representable float32 values; the C side
converts them to int32 device tables at `dfd_create`).

The per-pixel arithmetic of BGR->Lab, Lab->BGR and BGR->HSV on the GPU is integer/LUT only
(OpenCV's 8-bit fixed-point formulation, which is what reference
deepfake_detection.py:363-368 and frame_analysis.py:318 execute through cv2), so the kernels
are bit-exact against the oracle by construction.  `tests/test_imgproc.py` checks these tables
against the oracle's independent construction.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

GAMMA_SHIFT = 3
LAB_SHIFT = 12
LAB_SHIFT2 = LAB_SHIFT + GAMMA_SHIFT
CBRT_TAB_SIZE = 256 * 3 // 2 * (1 << GAMMA_SHIFT)        # 3072
BASE_SHIFT = 14                                          # Lab2RGBinteger::base_shift
BASE = 1 << BASE_SHIFT
INV_GAMMA_SHIFT = 12
INV_GAMMA_TAB_SIZE = 1 << INV_GAMMA_SHIFT                # 4096
INV_SHIFT = LAB_SHIFT + BASE_SHIFT - INV_GAMMA_SHIFT     # 14: descale of the 12-bit matrix product
AB_MIN = -8145                                           # minABvalue
AB_TAB_SIZE = BASE * 9 // 4                              # 36864
HSV_SHIFT = 12

_WHITE = np.array([0.950456, 1.0, 1.088754])
_M_FWD = np.array([[0.412453, 0.357580, 0.180423],
                   [0.212671, 0.715160, 0.072169],
                   [0.019334, 0.119193, 0.950227]])
_M_INV = np.array([[3.240479, -1.53715, -0.498535],
                   [-0.969256, 1.875991, 0.041556],
                   [0.055648, -0.204043, 1.057311]])


def _srgb_to_linear(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.04045, v / 12.92, np.power((v + 0.055) / 1.055, 2.4))


def _linear_to_srgb(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1 / 2.4) - 0.055)


def _trunc_div(a: int, b: int) -> int:
    """C's integer division."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _f(v) -> np.float32:
    return np.float32(v)


def build() -> Dict[str, np.ndarray]:
    """name -> int64 array; every value is < 2^24 in magnitude (exact in float32).

    The tables are the ones OpenCV's 8-bit Lab conversions use (imgproc/src/color_lab.cpp `initLabTabs`,
    `RGB2Lab_b`, `Lab2RGBinteger`): binary32 arithmetic where OpenCV uses softfloat, the gamma curves in double."""
    t: Dict[str, np.ndarray] = {}
    # forward: sRGBGammaTab_b, LabCbrtTab_b, 12-bit RGB->XYZ/white matrix
    g = _srgb_to_linear((np.arange(256, dtype=np.float32) / _f(255)).astype(np.float64)).astype(np.float32)
    t["lut.gamma"] = np.rint(_f(255 * 8) * g).astype(np.int64)
    x = (_f(1) / _f(255 * 8)) * np.arange(CBRT_TAB_SIZE, dtype=np.float32)
    lin = (x.astype(np.float64) * np.float64(_f(841) / _f(108)) + np.float64(_f(16) / _f(116))).astype(np.float32)   # fused multiply-add
    fx = np.where(x < _f(216) / _f(24389), lin, np.cbrt(x.astype(np.float64)).astype(np.float32))
    t["lut.cbrt"] = np.rint(_f(32768) * fx.astype(np.float32)).astype(np.int64)
    t["lut.fwd_coef"] = np.rint(4096.0 * _M_FWD / _WHITE[:, None]).astype(np.int64).ravel()
    # inverse: LabToYF_b (y and f(y) per L), adiv / bdiv per a / b, abToXZ_b, 12-bit XYZ*white->RGB matrix, sRGBInvGammaTab_b
    L_y, L_fy = [], []
    for i in range(256):
        if i <= 20:                                          # L <= 8
            y = _f(i * BASE * 20 * 9) / _f(17 * 29 * 29 * 29)
            fy = _f(BASE) * (_f(16) / _f(116) + _f(i * 5) / _f(3 * 17 * 29))
        else:
            fy = _f(i * 100 * BASE) / _f(255 * 116) + _f(16 * BASE) / _f(116)
            y = fy * fy * fy / _f(BASE * BASE)
        L_y.append(int(np.rint(y)))
        L_fy.append(int(np.rint(fy)))
    t["lut.L_y"] = np.array(L_y, np.int64)
    t["lut.L_fy"] = np.array(L_fy, np.int64)
    t["lut.a_div"] = np.array([((5 * a * 53687 + 128) >> 13) - 128 * BASE // 500 for a in range(256)], np.int64)
    t["lut.b_div"] = np.array([((b * 41943 + 16) >> 9) - 128 * BASE // 200 + 1 for b in range(256)], np.int64)
    k_lin = BASE * 16 // 116 * 108 // 841
    t["lut.ab_xz"] = np.array([_trunc_div(v * 108, 841) - k_lin if v <= 3390 else v * v // BASE * v // BASE
                               for v in range(AB_MIN, AB_MIN + AB_TAB_SIZE)], np.int64)
    t["lut.inv_coef"] = np.rint(4096.0 * _M_INV * _WHITE[None, :]).astype(np.int64).ravel()
    xs = ((_f(1) / _f(INV_GAMMA_TAB_SIZE)) * np.arange(INV_GAMMA_TAB_SIZE, dtype=np.float32)).astype(np.float64)
    t["lut.inv_gamma"] = np.rint(_f(255) * _linear_to_srgb(xs).astype(np.float32)).astype(np.int64)
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256)
    hdiv = np.zeros(256)
    sdiv[1:] = np.rint((255 << HSV_SHIFT) / i)
    hdiv[1:] = np.rint((180 << HSV_SHIFT) / (6.0 * i))
    t["lut.hsv_sdiv"] = sdiv.astype(np.int64)
    t["lut.hsv_hdiv"] = hdiv.astype(np.int64)
    for k, v in t.items():
        assert np.abs(v).max() < (1 << 24), k
    return t


def as_float_tensors() -> Dict[str, np.ndarray]:
    return {k: v.astype(np.float32) for k, v in build().items()}


# OpenCV's COLORMAP_JET (cv2.applyColorMap(u8, cv2.COLORMAP_JET)) as used by show_cam_on_image (gradcam.py and the
# overlay of csrc/gradcam.hip, which carries the same table): row i = B, G, R of gray level i.  Restated as the
# piecewise-linear jet - x = i / 255, B / G / R = clip(1.5 - |4x - k|, 0, 1) for k = 1 / 2 / 3, rounded to 8 bits.
# PARITY WITH OPENCV UNPINNED: cv2 is not available to compare against.
JET_BGR = np.array([
    (128, 0, 0), (132, 0, 0), (136, 0, 0), (140, 0, 0), (144, 0, 0), (147, 0, 0), (152, 0, 0), (156, 0, 0),
    (160, 0, 0), (163, 0, 0), (168, 0, 0), (172, 0, 0), (176, 0, 0), (179, 0, 0), (184, 0, 0), (188, 0, 0),
    (192, 0, 0), (195, 0, 0), (200, 0, 0), (204, 0, 0), (208, 0, 0), (211, 0, 0), (216, 0, 0), (220, 0, 0),
    (224, 0, 0), (227, 0, 0), (232, 0, 0), (236, 0, 0), (240, 0, 0), (243, 0, 0), (248, 0, 0), (252, 0, 0),
    (255, 0, 0), (255, 4, 0), (255, 8, 0), (255, 13, 0), (255, 16, 0), (255, 21, 0), (255, 25, 0), (255, 29, 0),
    (255, 33, 0), (255, 36, 0), (255, 40, 0), (255, 45, 0), (255, 49, 0), (255, 53, 0), (255, 57, 0), (255, 61, 0),
    (255, 65, 0), (255, 68, 0), (255, 72, 0), (255, 77, 0), (255, 81, 0), (255, 85, 0), (255, 89, 0), (255, 93, 0),
    (255, 97, 0), (255, 100, 0), (255, 104, 0), (255, 109, 0), (255, 113, 0), (255, 117, 0), (255, 121, 0), (255, 125, 0),
    (255, 129, 0), (255, 132, 0), (255, 137, 0), (255, 141, 0), (255, 145, 0), (255, 148, 0), (255, 153, 0), (255, 157, 0),
    (255, 161, 0), (255, 164, 0), (255, 169, 0), (255, 173, 0), (255, 177, 0), (255, 180, 0), (255, 185, 0), (255, 189, 0),
    (255, 193, 0), (255, 196, 0), (255, 201, 0), (255, 205, 0), (255, 209, 0), (255, 212, 0), (255, 217, 0), (255, 221, 0),
    (255, 225, 0), (255, 228, 0), (255, 233, 0), (255, 237, 0), (255, 241, 0), (255, 244, 0), (255, 249, 0), (255, 253, 0),
    (254, 255, 1), (250, 255, 5), (245, 255, 10), (242, 255, 14), (238, 255, 17), (234, 255, 21), (229, 255, 26), (226, 255, 30),
    (222, 255, 33), (218, 255, 37), (213, 255, 42), (210, 255, 46), (206, 255, 49), (202, 255, 53), (197, 255, 58), (194, 255, 62),
    (190, 255, 66), (186, 255, 69), (181, 255, 74), (178, 255, 78), (174, 255, 82), (170, 255, 85), (165, 255, 90), (162, 255, 94),
    (158, 255, 98), (154, 255, 101), (149, 255, 106), (146, 255, 110), (142, 255, 114), (138, 255, 117), (133, 255, 122), (130, 255, 126),
    (126, 255, 130), (122, 255, 133), (118, 255, 137), (114, 255, 141), (109, 255, 146), (105, 255, 150), (101, 255, 154), (98, 255, 158),
    (94, 255, 162), (90, 255, 165), (86, 255, 169), (82, 255, 173), (77, 255, 178), (73, 255, 182), (69, 255, 186), (66, 255, 190),
    (62, 255, 194), (58, 255, 197), (54, 255, 201), (50, 255, 205), (45, 255, 210), (41, 255, 214), (37, 255, 218), (33, 255, 222),
    (30, 255, 226), (26, 255, 229), (22, 255, 233), (18, 255, 237), (13, 255, 242), (9, 255, 246), (5, 255, 250), (1, 255, 254),
    (0, 253, 255), (0, 249, 255), (0, 245, 255), (0, 241, 255), (0, 236, 255), (0, 232, 255), (0, 228, 255), (0, 225, 255),
    (0, 221, 255), (0, 217, 255), (0, 213, 255), (0, 209, 255), (0, 204, 255), (0, 200, 255), (0, 196, 255), (0, 193, 255),
    (0, 189, 255), (0, 185, 255), (0, 181, 255), (0, 177, 255), (0, 172, 255), (0, 168, 255), (0, 164, 255), (0, 161, 255),
    (0, 157, 255), (0, 153, 255), (0, 149, 255), (0, 145, 255), (0, 140, 255), (0, 136, 255), (0, 132, 255), (0, 129, 255),
    (0, 125, 255), (0, 121, 255), (0, 117, 255), (0, 113, 255), (0, 108, 255), (0, 104, 255), (0, 100, 255), (0, 97, 255),
    (0, 93, 255), (0, 89, 255), (0, 85, 255), (0, 81, 255), (0, 76, 255), (0, 72, 255), (0, 68, 255), (0, 65, 255),
    (0, 61, 255), (0, 57, 255), (0, 53, 255), (0, 49, 255), (0, 44, 255), (0, 40, 255), (0, 36, 255), (0, 33, 255),
    (0, 29, 255), (0, 25, 255), (0, 21, 255), (0, 17, 255), (0, 12, 255), (0, 8, 255), (0, 4, 255), (0, 0, 255),
    (0, 0, 252), (0, 0, 248), (0, 0, 244), (0, 0, 240), (0, 0, 235), (0, 0, 231), (0, 0, 227), (0, 0, 224),
    (0, 0, 220), (0, 0, 216), (0, 0, 212), (0, 0, 208), (0, 0, 203), (0, 0, 199), (0, 0, 195), (0, 0, 192),
    (0, 0, 188), (0, 0, 184), (0, 0, 180), (0, 0, 176), (0, 0, 171), (0, 0, 167), (0, 0, 163), (0, 0, 160),
    (0, 0, 156), (0, 0, 152), (0, 0, 148), (0, 0, 144), (0, 0, 139), (0, 0, 135), (0, 0, 132), (0, 0, 128),
], dtype=np.uint8)

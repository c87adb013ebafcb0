"""Progressive JPEG decoding as a case of the call-history table (tests/history_cases.py): does a progressive batch decode
depend on what the handle decoded before?  The work buffers (pinned coefficients, planes) are shared with the baseline
decoder and a progressive file's planes are only written where a scan sends a coefficient, so the zeroing has to earn this.

Importing this module REGISTERS the case (`H.CASES`, `H.BY_NAME`, family "jpeg_decode") and exempts the handle-less export
`dfd_jpeg_coefficients_ex` with `dfd_jpeg_coefficients`'s reason, so that the table's coverage check
(tests/test_history_cases.py) knows the new export.  The case's own history - a larger baseline batch, then a larger
progressive batch - is not the family's, so the table lists the case with "repeat" alone and
tests/test_jpeg_progressive_gpu.py runs it after `HISTORIES` below.  The test files of the feature import this module, so
any run that collects the suite has the case in the table."""
import functools

import numpy as np

import history_cases as H

if "dfd_jpeg_coefficients_ex" not in H.EXEMPT:
    H.EXEMPT["dfd_jpeg_coefficients_ex"] = H.EXEMPT["dfd_jpeg_coefficients"]

REACHES = ("dfd_decode_jpeg", "dfd_decode_jpeg_batch")


@functools.lru_cache(maxsize=None)
def case_files():
    """three progressive 4:2:0 files of 40 x 56 (one with restart intervals, one with optimised tables) and a gray one"""
    a = [H.noise_frame(40, 56, 90 + i) for i in range(3)]
    return ([H.pillow_jpeg(a[0], 85, 2, progressive=True), H.pillow_jpeg(a[1], 85, 2, progressive=True, restart_marker_blocks=3),
             H.pillow_jpeg(a[2], 85, 2, progressive=True, optimize=True)],
            [H.pillow_jpeg(a[0][:, :, 0].copy(), 90, progressive=True)])


@functools.lru_cache(maxsize=None)
def history_files():
    """(a larger baseline batch, a larger progressive batch): 8 files of 256 x 320 each, other content (Pillow cannot write
    much larger progressive files of noise into memory)"""
    src = [H.unlike(H.noise_frame(256, 320, 94 + i), *[H.noise_frame(40, 56, 90 + k) for k in range(3)]) for i in range(8)]
    return [H.pillow_jpeg(s, 85, 2) for s in src], [H.pillow_jpeg(s, 85, 2, progressive=True) for s in src[::-1]]


def large(h, device=0):
    base, prog = history_files()
    h.set_option("jpeg_progressive", 1)
    h.set_option("jpeg_device_progressive", device)
    h.decode_jpeg_batch(base)
    h.decode_jpeg_batch(prog)
    h.decode_jpeg(prog[0])
    h.set_option("jpeg_device_progressive", 0)


HISTORIES = {"large": large}


def run(h, dirty=H._noop, device=0):
    """device: option "jpeg_device_progressive" for the batch calls (0, the default: the host pool)"""
    colour, gray = case_files()
    out = {}
    h.set_option("jpeg_progressive", 1)
    h.set_option("jpeg_device_progressive", device)
    try:
        for name, call in (("batch", lambda: h.decode_jpeg_batch(colour)), ("batch_gray", lambda: h.decode_jpeg_batch(gray)),
                           ("single", lambda: h.decode_jpeg(colour[1]))):
            dirty()
            out[name] = np.asarray(call())
    finally:
        h.set_option("jpeg_progressive", 0)
        h.set_option("jpeg_device_progressive", 0)
    return out


CASE = H.Case("jpeg_progressive", "jpeg_decode", run, REACHES, ("repeat",))
if CASE.name not in H.BY_NAME:
    H.CASES.append(CASE)
    H.BY_NAME[CASE.name] = CASE

"""The any-size frequency-domain entries as a case of the call-history table (tests/history_cases.py): the case, its
histories and its inputs, in that table's terms - does any of these paths' output depend on what the handle did before?
Their work buffers are padded planes that a larger earlier call leaves full of other windows' values, so this is the
property the padded form has to earn.

Importing this module REGISTERS the case with the table (`H.CASES`, `H.BY_NAME`), family "frequency", so that the table's
coverage check (tests/test_history_cases.py: every export of `_lib.SIGNATURES` is reached by a case or exempt) knows the
five new entry points.  The case's own histories - the new entries at their largest shapes - are not the family's
(`H.HISTORIES["frequency"]` runs the 224 kernels), so the table lists the case with "repeat" alone and
tests/test_freq_domain_history_gpu.py runs it after `HISTORIES` below; tests/test_freq_domain_history.py holds the
inputs to the table's rule (every history array differs from every case array in every position they share).  Both
test files import this module, so any run that collects the suite has the case in the table."""
import functools

import numpy as np

import history_cases as H
from rtdfd_amd import _lib as L

BOXES = [(0, 0, 1, 1), (3, 5, 17, 15), (20, 10, 63, 65), (47, 25, 63, 65), (0, 88, 110, 2), (109, 0, 1, 90)]     # corners, edges, overlap
FEATURE_SIZES = (30, 250)
TAPS = ("rows", "spectrum", "mag", "sums")
FEATURE_TAPS = ("gray", "spectrum", "dct")
REACHES = ("dfd_frequency_domain", "dfd_frequency_domain_device", "dfd_frequency_domain_tap", "dfd_frequency_features_sized",
           "dfd_frequency_features_tap")


@functools.lru_cache(maxsize=None)
def case_inputs():
    """(BGR frame 90 x 110 for the boxes, gray window 33 x 31 for the taps, BGR image 120 x 100 for the features)"""
    return H.noise_frame(90, 110, 61), H.noise_frame(33, 31, 62)[:, :, 0].copy(), H.noise_frame(120, 100, 63)


@functools.lru_cache(maxsize=None)
def history_frame():
    return H.unlike(H.noise_frame(1080, 1920, 64), *case_inputs())


@functools.lru_cache(maxsize=None)
def history_boxes():
    rs = np.random.RandomState(65)
    big = [(0, 0, 1900, 1000), (20, 80, 1000, 1000), (0, 0, 1920, 3), (1917, 0, 3, 1080)]
    return big + [(int(rs.randint(0, 1920 - w)), int(rs.randint(0, 1080 - h)), w, h) for w, h in ((96, 96), (300, 260), (257, 255), (33, 500))]


@functools.lru_cache(maxsize=None)
def history_gray():
    """700 x 900 gray window for the tap of the history: unlike every case input, a colour one in each of its channels"""
    g = H.noise_frame(700, 900, 67)[:, :, 0].copy()
    planes = [p for c in case_inputs() for p in ([c] if c.ndim == 2 else [c[..., k] for k in range(3)])]
    for _ in range(8):
        again = False
        for p in planes:
            v = g[:p.shape[0], :p.shape[1]]
            eq = v == p
            if eq.any():
                v[eq] += np.uint8(1)
                again = True
        if not again:
            return g
    raise AssertionError("history_gray: did not settle")


def large(h):
    """the new entries at their largest shapes with other content: every work buffer is left full of it"""
    for f in (history_frame(), H.white_frame(1080, 1920), H.checker_frame(1080, 1920)):
        h.frequency_domain(f, history_boxes())
        h.frequency_features(f, 1024, sized=True)
    h.frequency_domain_tap(history_gray(), "spectrum")
    h.frequency_features_tap(history_frame(), 1024, "spectrum")
    h.frequency_features_tap(history_frame(), 1024, "dct")


@functools.lru_cache(maxsize=None)
def grow_frames():
    return [H.unlike(H.noise_frame(8, 8, 66), *case_inputs()), history_frame()]


def grow(h):
    """a small call, then one that makes ensure() re-allocate"""
    small, big = grow_frames()
    h.frequency_domain(small)
    h.frequency_features(small, 2, sized=True)
    h.frequency_domain(big, history_boxes()[:2])
    h.frequency_features(big, 512, sized=True)


def cross(h):
    """one call of every family of the table at its largest shape, then this one's"""
    H.cross(h, "")
    large(h)


HISTORIES = {"large": large, "grow": grow, "cross": cross}


THIN = ("boxes", "tap.spectrum", "features250", "features30.dct")     # what `run` records under "cross"


def run(h, dirty=H._noop, thin=False):
    """`dirty` runs in front of every recorded call; thin: only the calls of THIN (the cross history is fifteen
    families' largest calls)"""
    frame, gray, img = case_inputs()
    out = {}

    def record(name, call):
        if thin and name not in THIN:
            return
        dirty()
        out[name] = call()

    record("boxes", lambda: h.frequency_domain(frame, BOXES))
    record("whole_gray", lambda: h.frequency_domain(gray))
    buf = L.DeviceBuffer(h, frame.nbytes).upload(frame)
    try:
        record("device", lambda: h.frequency_domain_device(buf.ptr, frame.shape[0], frame.shape[1], frame.strides[0], 3, BOXES))
    finally:
        buf.free()
    for name in TAPS:
        record(f"tap.{name}", lambda: h.frequency_domain_tap(gray, name))
    for size in FEATURE_SIZES:
        record(f"features{size}", lambda: h.frequency_features(img, size, sized=True))
        for name in FEATURE_TAPS:
            record(f"features{size}.{name}", lambda: h.frequency_features_tap(img, size, name))
    return out


CASE = H.Case("frequency_domain", "frequency", run, REACHES, ("repeat",), thinnable=True)
if CASE.name not in H.BY_NAME:
    H.CASES.append(CASE)
    H.BY_NAME[CASE.name] = CASE

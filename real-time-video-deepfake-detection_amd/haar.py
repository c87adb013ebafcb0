"""Haar cascade fallback of the reference's face detection (reference face_detection.py:12,108-123).

The reference builds ``cv2.CascadeClassifier(cv2.data.haarcascades + 'haarcascade_frontalface_default.xml')`` at
import and uses it whenever the SSD model files are missing - which is how the reference runs as shipped.
This module reads that XML format (OpenCV's "new" cascade layout: BOOST stages of stumps over upright HAAR features)
into the arrays `weights.pack_all(..., haar=...)` puts into the blob; csrc/haar_api.hip evaluates them.

The XML itself ships with OpenCV, not with the reference tree or this one: point ``$DFD_HAAR_CASCADE`` at it.
Not supported (rejected with a clear error): tilted features, trees deeper than stumps, LBP / HOG cascades, the old
(OpenCV 1.x) cascade layout.  A cascade whose numbers would take the device outside its tables or its window - a feature
index past the feature table, a rectangle past the window, non-finite values - is a ``ValueError`` here
(`validate_cascade`) and ``DFD_ERR_BLOB`` at `dfd_create` (csrc/haar_validate.h, the same list).
"""
from __future__ import annotations

import xml.etree.ElementTree as ET
from typing import Dict

import numpy as np


def load_cascade_xml(path_or_text: str) -> Dict[str, np.ndarray]:
    text = path_or_text if path_or_text.lstrip().startswith("<") else open(path_or_text).read()
    root = ET.fromstring(text)
    cas = root.find("cascade")
    if cas is None:
        raise ValueError("Haar XML: no <cascade> element (old-format cascades are not supported)")
    if (cas.findtext("stageType") or "").strip() != "BOOST" or (cas.findtext("featureType") or "").strip() != "HAAR":
        raise ValueError("Haar XML: only BOOST cascades of HAAR features are supported")
    win = (int(cas.findtext("width")), int(cas.findtext("height")))
    stages, stumps = [], []
    for st in cas.find("stages"):
        first = len(stumps)
        for wk in st.find("weakClassifiers"):
            nodes = [float(v) for v in wk.findtext("internalNodes").split()]
            leaves = [float(v) for v in wk.findtext("leafValues").split()]
            if len(nodes) != 4 or len(leaves) != 2 or nodes[0] > 0 or nodes[1] > 0:
                raise ValueError("Haar XML: only stump weak classifiers (one internal node) are supported")
            # internalNodes: left right featureIdx threshold; left / right <= 0 are leaf indices (negated)
            stumps.append((nodes[2], nodes[3], leaves[int(-nodes[0])], leaves[int(-nodes[1])]))
        stages.append((first, len(stumps) - first, float(st.findtext("stageThreshold"))))
    rects = []
    for f in cas.find("features"):
        if int((f.findtext("tilted") or "0").strip()) != 0:
            raise ValueError("Haar XML: tilted features are not supported")
        rs = [[float(v) for v in r.text.split()] for r in f.find("rects")]
        if not 2 <= len(rs) <= 3:
            raise ValueError("Haar XML: a feature has 2 or 3 rectangles")
        while len(rs) < 3:
            rs.append([0, 0, 0, 0, 0.0])
        rects.append(rs)
    cas = {"haar.win": np.asarray(win, np.float32), "haar.stages": np.asarray(stages, np.float32).reshape(-1, 3),
           "haar.stumps": np.asarray(stumps, np.float32).reshape(-1, 4),
           "haar.rects": np.asarray(rects, np.float32).reshape(len(rects), 15)}
    validate_cascade(cas)
    return cas


def validate_cascade(cas: Dict[str, np.ndarray]) -> None:
    """ValueError unless the arrays are a cascade the device can evaluate inside its buffers: the list of
    csrc/haar_validate.h, which `dfd_create` applies to the blob (DFD_ERR_BLOB).  Slots 0 and 1 of a feature are always
    read, so their geometry must fit whatever their weight; slot 2 is read only with a non-zero weight."""
    def bad(what):
        raise ValueError("Haar cascade: " + what)

    def ints(v, lo, hi):
        return bool(np.all((v >= lo) & (v <= hi) & (v == np.floor(v))))       # NaN and infinities fail every comparison

    win = np.asarray(cas["haar.win"], np.float32).ravel()
    stages = np.asarray(cas["haar.stages"], np.float32).reshape(-1, 3)
    stumps = np.asarray(cas["haar.stumps"], np.float32).reshape(-1, 4)
    rects = np.asarray(cas["haar.rects"], np.float32).reshape(-1, 3, 5)
    if win.size != 2 or not ints(win, 4, 4096):
        bad("window is not an integer size of 4 .. 4096")
    if not (len(stages) and len(stumps) and len(rects)):
        bad("no stages, stumps or features")
    first, count = stages[:, 0].astype(np.float64), stages[:, 1].astype(np.float64)
    if not (ints(first, 0, len(stumps)) and ints(count, 1, len(stumps)) and np.all(first + count <= len(stumps))):
        bad("a stage's stumps run outside the stump table")
    if np.any(first[1:] != (first + count)[:-1]):
        bad("stages are not contiguous in order")
    if not np.all(np.isfinite(stages[:, 2])):
        bad("a stage threshold is not finite")
    if not ints(stumps[:, 0], 0, len(rects) - 1):
        bad("a stump's feature index is outside the feature table")
    if not np.all(np.isfinite(stumps[:, 1:])):
        bad("a stump's threshold or leaf is not finite")
    if not np.all(np.isfinite(rects)):
        bad("a rectangle holds a value that is not finite")
    unused = rects[:, 2, 4] == 0
    if np.any(rects[unused, 2, :4] != 0):
        bad("an unused third rectangle has geometry")
    r = np.concatenate([rects[:, :2].reshape(-1, 5), rects[~unused, 2]]).astype(np.float64)
    if not (ints(r[:, 0], 0, win[0]) and ints(r[:, 1], 0, win[1]) and ints(r[:, 2], 1, win[0]) and ints(r[:, 3], 1, win[1])
            and np.all(r[:, 0] + r[:, 2] <= win[0]) and np.all(r[:, 1] + r[:, 3] <= win[1])):
        bad("a rectangle is not an integer box inside the window")


def detect_faces_haar(frame, handle):
    """reference face_detection.py:108-123: [(x, y, w, h), ...] with scaleFactor 1.1, minNeighbors 5, minSize 30"""
    return handle.detect_faces_haar(frame, 1.1, 5, 30)

"""CPU restatement of facenet-pytorch's ``MTCNN.detect`` (with landmarks), ``select_boxes`` and ``extract`` for any
constructor arguments.  TEST INFRASTRUCTURE ONLY.

Built from the pieces of oracle/mtcnn_ref.py (networks, NMS, bbreg, rerec, pad, the Pillow-exact resize), which stay as
they are; what is added is what that file fixes to the reference's construction: the pyramid from ``min_face_size`` and
``factor``, the three thresholds, the landmark mapping, the orderings, the margin and the output size of extract_face.
facenet-pytorch is not installed here: like oracle/mtcnn_ref.py this rests on a reading of the package's source.

Ties in every ordering: ``np.argsort(key, kind="stable")[::-1]`` - of equal keys the later row first.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import mtcnn_ref as M


@dataclass
class Params:
    image_size: int = 160
    margin: int = 0
    min_face_size: int = 20
    thresholds: tuple = (0.6, 0.7, 0.7)
    factor: float = 0.709
    selection: str = "largest"        # none | probability | largest | center_weighted_size | largest_over_threshold
    keep_all: bool = False
    post_process: bool = True


@dataclass
class Trace:
    """Every score a threshold acts on (for the 'no score near a threshold' guard of the GPU test)."""
    margins: list = field(default_factory=list)
    levels: int = 0

    def note(self, scores, thr):
        s = np.asarray(scores, np.float32).reshape(-1)
        if s.size:
            self.margins.append(float(np.abs(s - np.float32(thr)).min()))

    def closest(self) -> float:
        return min(self.margins) if self.margins else 1.0


def scale_pyramid(h: int, w: int, P: Params):
    m = 12.0 / P.min_face_size
    minl = min(h, w) * m
    scale_i = m
    scales = []
    while minl >= 12:
        scales.append(scale_i)
        scale_i = scale_i * P.factor
        minl = minl * P.factor
    return scales


def detect_face(sd, rgb: np.ndarray, P: Params, trace: Trace | None = None):
    """rows (k, 5) float32 (x1, y1, x2, y2, prob) after the three stages, points (k, 5, 2) float32."""
    t0, t1, t2 = P.thresholds
    with torch.no_grad():
        img = torch.from_numpy(np.ascontiguousarray(rgb)).permute(2, 0, 1)[None].float()
        h, w = img.shape[2:]
        rows = []
        scales = scale_pyramid(h, w, P)
        if trace is not None:
            trace.levels = len(scales)
        for scale in scales:
            data = (M.imresample(img, (int(h * scale + 1), int(w * scale + 1))) - 127.5) * 0.0078125
            reg, probs = M.pnet(sd, data)
            if trace is not None:
                trace.note(probs[0, 1].numpy(), t0)
            bs = M.generate_bounding_box(reg, probs[:, 1], scale, t0)
            rows.append(bs[M.nms_iou(bs[:, :4], bs[:, 4], 0.5)])
        boxes = np.concatenate(rows, 0) if rows else np.zeros((0, 9), np.float32)
        boxes = boxes[M.nms_iou(boxes[:, :4], boxes[:, 4], 0.7)]
        regw = boxes[:, 2] - boxes[:, 0]
        regh = boxes[:, 3] - boxes[:, 1]
        boxes = np.stack([boxes[:, 0] + boxes[:, 5] * regw, boxes[:, 1] + boxes[:, 6] * regh,
                          boxes[:, 2] + boxes[:, 7] * regw, boxes[:, 3] + boxes[:, 8] * regh, boxes[:, 4]], 1)
        boxes = M.rerec(boxes.astype(np.float32))
        points = np.zeros((0, 5, 2), np.float32)
        if len(boxes):
            data, valid = M._crops(img, boxes, 24)
            boxes = boxes[valid]
            reg, prob = M.rnet(sd, data)
            score = prob[:, 1].numpy()
            if trace is not None:
                trace.note(score, t1)
            ipass = score > np.float32(t1)
            boxes = np.concatenate([boxes[ipass, :4], score[ipass, None]], 1)
            mv = reg.numpy()[ipass]
            pick = M.nms_iou(boxes[:, :4], boxes[:, 4], 0.7)
            boxes = M.rerec(M.bbreg(boxes[pick], mv[pick]))
        if len(boxes):
            data, valid = M._crops(img, boxes, 48)
            boxes = boxes[valid]
            reg, pts, prob = M.onet(sd, data)
            score = prob[:, 1].numpy()
            if trace is not None:
                trace.note(score, t2)
            ipass = score > np.float32(t2)
            pts = pts.numpy()[ipass]
            boxes = np.concatenate([boxes[ipass, :4], score[ipass, None]], 1)
            # landmarks on the O-Net input boxes, before bbreg
            w_i = boxes[:, 2] - boxes[:, 0] + 1
            h_i = boxes[:, 3] - boxes[:, 1] + 1
            px = w_i[:, None] * pts[:, 0:5] + boxes[:, 0:1] - 1
            py = h_i[:, None] * pts[:, 5:10] + boxes[:, 1:2] - 1
            points = np.stack([px, py], 2).astype(np.float32)
            boxes = M.bbreg(boxes, reg.numpy()[ipass])
            pick = M.nms_min(boxes[:, :4], boxes[:, 4], 0.7)
            boxes, points = boxes[pick], points[pick]
        return boxes.astype(np.float32), points.astype(np.float32).reshape(-1, 5, 2)


def order_rows(boxes: np.ndarray, selection: str, h: int, w: int, threshold: float = 0.9, center_weight: float = 2.0):
    """indices of the rows in the order `selection` asks for (a subset for largest_over_threshold)."""
    idx = np.arange(len(boxes))
    if selection in (None, "none") or len(boxes) == 0:
        return idx
    b = boxes.astype(np.float32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    if selection == "probability":
        key = b[:, 4]
    elif selection == "largest":
        key = area
    elif selection == "center_weighted_size":
        centers = np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2], 1)
        offsets = centers - np.array((w / 2, h / 2))                # float32 array - Python floats -> float64
        key = area - np.sum(np.power(offsets, 2.0), 1) * center_weight
    elif selection == "largest_over_threshold":
        mask = b[:, 4] > np.float32(threshold)
        idx, key = idx[mask], area[mask]
    else:
        raise ValueError(selection)
    return idx[np.argsort(key, kind="stable")[::-1]]


def detect(sd, rgb: np.ndarray, P: Params, trace: Trace | None = None):
    """(rows (k, 5), points (k, 5, 2)) in P.selection's order; row 0 only without keep_all."""
    boxes, points = detect_face(sd, rgb, P, trace)
    order = order_rows(boxes, P.selection, rgb.shape[0], rgb.shape[1])
    if trace is not None and P.selection == "largest_over_threshold":
        trace.note(boxes[:, 4], 0.9)
    if not P.keep_all:
        order = order[:1]
    return boxes[order], points[order]


def crop_box(box, h: int, w: int, P: Params):
    """extract_face's integer box: the margin scaled to the box, in float32 (what numpy 2 computes on the float32 row
    MTCNN.detect returns; numpy 1 promoted the scalars to float64, which differs only within an ulp of an integer)."""
    box = np.asarray(box, np.float32)
    mf, den, two = np.float32(P.margin), np.float32(P.image_size - P.margin), np.float32(2)    # every step in float32
    m = [mf * (box[2] - box[0]) / den, mf * (box[3] - box[1]) / den]
    return (int(max(box[0] - m[0] / two, 0)), int(max(box[1] - m[1] / two, 0)),
            int(min(box[2] + m[0] / two, w)), int(min(box[3] + m[1] / two, h)))


def resize_crop(rgb: np.ndarray, ibox, size: int) -> np.ndarray:
    """img.crop(box).resize((size, size), BILINEAR) for a box inside the image."""
    x1, y1, x2, y2 = ibox
    return M.pil_resize_bilinear(rgb[y1:y2, x1:x2], size, size)


def extract_face(rgb: np.ndarray, box, P: Params) -> np.ndarray:
    """(3, S, S) float32 RGB planes, 0..255 or standardised; zeros for an empty clipped box."""
    h, w = rgb.shape[:2]
    x1, y1, x2, y2 = crop_box(box, h, w, P)
    if x2 <= x1 or y2 <= y1:
        return np.zeros((3, P.image_size, P.image_size), np.float32)
    face = np.ascontiguousarray(resize_crop(rgb, (x1, y1, x2, y2), P.image_size).transpose(2, 0, 1)).astype(np.float32)
    if P.post_process:
        face = (face - np.float32(127.5)) / np.float32(128.0)
    return face


def forward(sd, rgb: np.ndarray, P: Params, trace: Trace | None = None):
    """(rows, points, faces (k, 3, S, S)) of MTCNN.forward; k = 0 when no face passes."""
    rows, points = detect(sd, rgb, P, trace)
    faces = np.stack([extract_face(rgb, r[:4], P) for r in rows]) if len(rows) else np.zeros((0, 3, P.image_size, P.image_size), np.float32)
    return rows, points, faces

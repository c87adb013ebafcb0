"""Host mirror of ``facenet_pytorch.MTCNN``: every constructor argument of the package, one image or a list, all faces
(``keep_all``), landmarks, any ``image_size`` / ``margin``.  The cascade, the ordering of the faces and the crops run in
libdfd_hip.so (`dfd_mtcnn_detect` / `dfd_mtcnn_extract`, include/dfd_hip.h).  The construction the reference uses
(reference deepfake_detection.py:24-28: ``MTCNN(select_largest=False, post_process=False, device=DEVICE)``, called as
``mtcnn(PIL_image)`` at :377) keeps its own entry point (`dfd_mtcnn_align`) and its bits.

facenet-pytorch is not installed where this is built: the semantics rest on a reading of its published source, not on
running it.  One stated difference: ``selection_method="largest_over_threshold"`` returns the probability and landmarks
of the box it selects (the package indexes the unfiltered arrays with the filtered order there).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import MT_SELECT, Handle, mtcnn_params


class MTCNN:
    def __init__(self, image_size: int = 160, margin: int = 0, min_face_size: int = 20, thresholds=(0.6, 0.7, 0.7),
                 factor: float = 0.709, post_process: bool = True, select_largest: bool = True,
                 selection_method=None, keep_all: bool = False, device=None, *, handle: Optional[Handle] = None):
        if not selection_method:
            selection_method = "largest" if select_largest else "probability"
        if selection_method not in ("probability", "largest", "largest_over_threshold", "center_weighted_size"):
            raise ValueError(f"unknown selection_method {selection_method!r}")
        if len(tuple(thresholds)) != 3:
            raise ValueError("thresholds: three values (P-Net, R-Net, O-Net)")
        self.image_size, self.margin, self.min_face_size = image_size, margin, min_face_size
        self.thresholds, self.factor = list(thresholds), factor
        self.post_process, self.select_largest, self.keep_all = post_process, select_largest, keep_all
        self.selection_method = selection_method
        self.device = device
        self._handle = handle

    def to(self, *_a, **_k):
        return self

    def eval(self):
        return self

    @property
    def handle(self) -> Handle:
        if self._handle is None:
            from . import runtime

            self._handle = runtime.default_handle()
        return self._handle

    @staticmethod
    def _as_bgr(img) -> np.ndarray:
        a = np.asarray(img)                      # PIL RGB image or (H, W, 3) uint8 RGB array, as the package accepts
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError("MTCNN expects an RGB uint8 image (PIL or HxWx3 array)")
        return np.ascontiguousarray(a[..., ::-1])

    @staticmethod
    def _is_batch(img) -> bool:
        return isinstance(img, (list, tuple)) or (isinstance(img, np.ndarray) and img.ndim == 4)

    def _params(self, selection, keep_all):
        return mtcnn_params(self.image_size, self.margin, self.min_face_size, self.thresholds, self.factor, selection,
                            keep_all, self.post_process)

    def _is_reference_call(self) -> bool:
        return ((self.image_size, self.margin, self.min_face_size, tuple(self.thresholds), self.factor)
                == (160, 0, 20, (0.6, 0.7, 0.7), 0.709) and not self.keep_all and not self.post_process
                and self.selection_method == "probability")

    @staticmethod
    def _tensor(face):
        try:
            import torch

            return torch.from_numpy(face)
        except ImportError:
            return face

    def forward(self, img, save_path=None, return_prob: bool = False):
        """Per image a (3, S, S) float RGB tensor (``keep_all``: (n, 3, S, S)), 0..255 or standardised with
        ``post_process`` (torch when importable, else numpy), or None; a list of those for a list of images.  With
        ``return_prob`` also the probability (``keep_all``: an array of them; [None] / None where no face passes)."""
        batch = self._is_batch(img)
        paths = self._save_paths(save_path, img, batch)
        if paths is None and not batch and self._is_reference_call():   # the reference's construction: its own entry point
            face, box = self.handle.mtcnn_align(self._as_bgr(img))
            face = None if face is None else self._tensor(face)
            return (face, None if box is None else float(box[4])) if return_prob else face
        imgs = [self._as_bgr(a) for a in (img if batch else [img])]
        # keep_all: MTCNN.detect's order (select_largest); else row 0 of select_boxes(method=selection_method)
        sel = ("largest" if self.select_largest else "none") if self.keep_all else self.selection_method
        res = self.handle.mtcnn_extract(imgs, self._params(sel, self.keep_all))
        faces, probs = [], []
        for rows, _lm, crops in res:
            if len(rows) == 0:
                faces.append(None)
                probs.append([None] if self.keep_all else None)
            elif self.keep_all:
                faces.append(self._tensor(crops))
                probs.append(rows[:, 4].copy())
            else:
                faces.append(self._tensor(crops[0]))
                probs.append(float(rows[0, 4]))
        if paths is not None:
            self._save(res, paths)
        if not batch:
            faces, probs = faces[0], probs[0]
        return (faces, probs) if return_prob else faces

    __call__ = forward

    @staticmethod
    def _save_paths(save_path, img, batch):
        """None, or one path per image (the package takes a string for one image, a list of strings for a list)"""
        if save_path is None:
            return None
        paths = list(save_path) if isinstance(save_path, (list, tuple)) else [save_path]
        if len(paths) != (len(img) if batch else 1):
            raise ValueError("save_path: one path per image")
        for p in paths:
            if not isinstance(p, str) or not p.lower().endswith((".jpg", ".jpeg")):
                raise ValueError(f"save_path {p!r}: only .jpg / .jpeg files are written")
        return paths

    def _save(self, res, paths):
        """The package's `save_img` of every crop: the uint8 RGB crop before `post_process`, as Pillow's default JPEG
        (quality 75, 4:2:0), face 0 at `path`, face k at `name_<k + 1>.ext`.  The crops of the whole call are encoded
        in one device pass; the files' bytes equal `PIL.Image.fromarray(crop).save(path)`."""
        import os

        crops, names = [], []
        for (rows, _lm, faces), path in zip(res, paths):
            stem, ext = os.path.splitext(path)
            for k in range(len(rows) if self.keep_all else min(1, len(rows))):
                f = faces[k]
                if self.post_process:
                    f = f * 128.0 + 127.5                   # fixed_image_standardization, undone exactly (float32)
                crops.append(np.ascontiguousarray(f.transpose(1, 2, 0)).astype(np.uint8))
                names.append(path if k == 0 else f"{stem}_{k + 1}{ext}")
        for name, data in zip(names, self.handle.encode_jpegs(crops, quality=75, subsampling=2, rgb=True)):
            os.makedirs(os.path.dirname(name) or ".", exist_ok=True)
            with open(name, "wb") as fh:
                fh.write(data)

    def detect(self, img, landmarks: bool = False):
        """(boxes (n, 4) float32, probs (n,)[, points (n, 5, 2)]) of every face that passes the cascade, by descending
        probability (``select_largest``: area); (None, [None][, None]) without one; lists of those for a list of images."""
        batch = self._is_batch(img)
        imgs = [self._as_bgr(a) for a in (img if batch else [img])]
        res = self.handle.mtcnn_detect(imgs, self._params("largest" if self.select_largest else "none", True), landmarks=landmarks)
        boxes, probs, points = [], [], []
        for rows, lm, _ in res:
            if len(rows) == 0:
                boxes.append(None); probs.append([None]); points.append(None)
            else:
                boxes.append(rows[:, :4].copy()); probs.append(rows[:, 4].copy()); points.append(lm)
        if not batch:
            boxes, probs, points = boxes[0], probs[0], points[0]
        return (boxes, probs, points) if landmarks else (boxes, probs)

    def select_boxes(self, all_boxes, all_probs, all_points, imgs, method: str = "probability", threshold: float = 0.9,
                     center_weight: float = 2.0):
        """The package's ``select_boxes`` on arrays a caller already holds (``forward`` orders on the device): per image
        row 0 of the order, as (1, 4), (1,), (1, 5, 2) arrays, or None.  Equal keys: the later row first."""
        if method not in MT_SELECT or method in (None, "none"):
            raise ValueError(f"unknown method {method!r}")
        batch = self._is_batch(imgs)
        if not batch:
            imgs, all_boxes, all_probs, all_points = [imgs], [all_boxes], [all_probs], [all_points]
        out_b, out_p, out_l = [], [], []
        for boxes, points, probs, img in zip(all_boxes, all_points, all_probs, imgs):
            if boxes is None:
                out_b.append(None); out_p.append([None]); out_l.append(None)
                continue
            boxes, probs, points = np.array(boxes), np.array(probs), np.array(points)
            area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
            if method == "largest_over_threshold":
                mask = probs > threshold
                boxes, probs, points, area = boxes[mask], probs[mask], points[mask], area[mask]
                if len(boxes) == 0:
                    out_b.append(None); out_p.append([None]); out_l.append(None)
                    continue
            if method == "probability":
                key = probs
            elif method == "center_weighted_size":
                a = np.asarray(img)
                w, h = (img.size if hasattr(img, "size") and not isinstance(img, np.ndarray) else (a.shape[1], a.shape[0]))
                centers = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], 1)
                key = area - np.sum(np.power(centers - (w / 2, h / 2), 2.0), 1) * center_weight
            else:
                key = area
            order = np.argsort(key, kind="stable")[::-1]
            out_b.append(boxes[order][[0]]); out_p.append(probs[order][[0]]); out_l.append(points[order][[0]])
        if not batch:
            return out_b[0], out_p[0], out_l[0]
        return out_b, out_p, out_l

    def extract(self, img, batch_boxes, save_path=None):
        """The package's ``extract``: the crops of ``forward`` for this object's configuration (the boxes are found again
        on the device in the same pass that crops them; ``batch_boxes`` only says where there is none)."""
        faces = self.forward(img, save_path=save_path)
        if self._is_batch(img):
            return [None if b is None else f for f, b in zip(faces, batch_boxes)]
        return None if batch_boxes is None else faces

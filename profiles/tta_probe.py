"""What test-time augmentation costs per frame of `DeepfakeDetector.predict` (K = 3 images per face, the reference's
constructor default), at 480x640 and 1080p:

  (a) per_face_loop : the flow before the batched path - the fused call classifies every face, that result is dropped,
                      and each face goes through `analyze_face` (CLAHE, per copy an augment and a batch-1 classification:
                      six library calls per face)
  (b) batched       : `predict` as it is now - the copies ride in the fused call's own pass (dfd_tta_arm)
  (c) tta_off       : `predict` with use_tta=False

One JSON line per frame size: faces per frame, median ms per call and frames/s of the three, and the ratios (b)/(a) and
(b)/(c) of the medians.  Host clock around synchronised work (every call returns after its last stream wait); every
case is warmed up on the same frames first; the cases are interleaved round by round so that clock drift hits all three.

    python profiles/tta_probe.py [--rounds 7] [--frames 8]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frames as F  # noqa: E402
import rtdfd_amd  # noqa: E402

D = rtdfd_amd.deepfake_detection.DeepfakeDetector


class PerFaceLoop(D):
    """`predict` as it was before the batched path: an unarmed fused call, then `analyze_face` per detected face"""

    def _tta_copies(self, request=False):
        return 0

    def predict(self, frame):
        self.frame_count += 1
        frame = np.ascontiguousarray(frame)
        forensic, faces, _ = self._frame_on_gpu(frame, max_faces=200)
        voted = 0
        for (x, y, w, h) in faces:
            p = self.analyze_face(frame[y:y + h, x:x + w])[0]
            if p is not None:
                self.temporal_tracker.update(p)
                voted += 1
        if not voted and not len(faces):
            self.temporal_tracker.update(forensic['fake_probability'])
        return frame, False, None, {'faces_detected': len(faces)}


def _time(det, frames):
    out = []
    for fr in frames:
        t = time.perf_counter()
        det.predict(fr)
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8, help="distinct frames per size")
    args = ap.parse_args()
    W = rtdfd_amd.weights
    h = rtdfd_amd._lib.Handle(W.pack_all(W.seeded_state_dict(0), W.seeded_ssd_state_dict(0)), device=0, max_batch=64)
    random.seed(0)
    for hh, ww in ((480, 640), (1080, 1920)):
        frames = [F.natural_like(hh, ww, seed=100 + i) for i in range(args.frames)]
        cases = {"per_face_loop": PerFaceLoop(use_tta=True, num_tta_augmentations=3, handle=h),
                 "batched": D(use_tta=True, num_tta_augmentations=3, handle=h),
                 "tta_off": D(use_tta=False, num_tta_augmentations=1, handle=h)}
        faces = [d['faces_detected'] for d in (cases["tta_off"].predict(fr)[3] for fr in frames)]
        for det in cases.values():                                  # warm-up: every shape and batch size met below
            _time(det, frames)
        ms = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, det in cases.items():
                ms[k] += _time(det, frames)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps({"size": f"{ww}x{hh}", "frames": len(frames), "rounds": args.rounds,
                          "faces_per_frame": round(float(np.mean(faces)), 2),
                          **{k: {"median_ms": round(med[k], 3), "p10_ms": round(float(np.percentile(ms[k], 10)), 3),
                                 "p90_ms": round(float(np.percentile(ms[k], 90)), 3), "frames_per_s": round(1e3 / med[k], 1)}
                             for k in cases},
                          "batched_over_per_face_loop": round(med["batched"] / med["per_face_loop"], 3),
                          "batched_over_tta_off": round(med["batched"] / med["tta_off"], 3)}), flush=True)
        for det in cases.values():
            det.release()
    h.close()


if __name__ == "__main__":
    main()

"""Frames of the fused / batched sized-forensics tests (tests/test_forensic_sized_fused_gpu.py): small ragged sources
(120 x 160, 90 x 144) and one under the detector's 30 px floor (24 x 40), built on the wave fixture of
tests/forensic_sized_oracle.py.  tests/test_forensic_sized_fused_fixtures.py asserts on the CPU that the moving sequence
sits away from every threshold of the reference at the sizes the GPU test compares scores at."""
import io

import numpy as np
from PIL import Image

import forensic_sized_oracle as Z

SIZES = (32, 80, 272)                       # < 4 blocks | odd factor, blocks do not tile | above 256, no power of two
SOURCES = ((120, 160), (90, 144), (24, 40))
PATTERN = (True, False, False, True)        # full / fast of the 4-frame sequence


def jpeg(frame_bgr, **kw):
    """Pillow-encoded baseline 4:2:0 file unless told otherwise (quality 90: the decoded moving sequence then sits away
    from every threshold as well)"""
    buf = io.BytesIO()
    kw.setdefault("subsampling", "4:2:0")
    Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format="JPEG", quality=90, **kw)
    return buf.getvalue()


def moving(n=4, h=120, w=160, seed=7):
    """a bright textured square moving over a wave background: n frames of h x w for the temporal signal"""
    side = max(4, min(h, w) // 3)
    patch = np.random.RandomState(5).randint(120, 255, (side, side, 3)).astype(np.uint8)
    out = []
    for i in range(n):
        f = Z.wave_frame(h, w, seed=seed).copy()
        x0 = 2 + ((w - side - 4) * i) // max(1, n - 1)
        y0 = (h - side) // 2
        f[y0:y0 + side, x0:x0 + side] = patch
        out.append(f)
    return out


def stream_frames(k, count, start=0):
    """`count` consecutive frames of test stream k from its frame number `start`: the three source sizes in turn from a
    stream-dependent offset, the square at a position that moves with the frame number"""
    out = []
    for t in range(start, start + count):
        h, w = SOURCES[(k + t) % 3]
        out.append(moving(8, h, w, seed=11 + k)[t % 8])
    return out

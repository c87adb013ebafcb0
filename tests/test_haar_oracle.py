"""CPU: the Haar oracle (oracle/haar_ref.py) held to a second reading, and the conditions under which a GPU pass of
tests/test_haar_stages_gpu.py means something.  cv2 is absent, so nothing here pins OpenCV itself.

* `scale_stages` (integral images and per-position codes of one scale) against a reading written here on its own: one
  window at a time, sums in Python integers (the normalisation sums pixel by pixel, the features from a table built by
  plain loops), float32 arithmetic as correctly rounded Python floats (struct 'f'), `math.sqrt` in double.  The resize and the
  gray conversion are oracle.imgproc_ref's, which tests/test_imgproc*.py hold to cv2's published arithmetic.
* `candidates`, rebuilt on `scale_stages`, returns the lists recorded before the rebuild (tests/golden).
* The scale-factor finding: round(521 / factor) differs between the double 1.1 and float32(1.1) at scale 5 only, and the
  oracle's grouped boxes of the 120 x 521 frame are the double ones.
* The XML reader / `validate_cascade` refuse every malformed cascade and round-trip `wide` and `ties` bit for bit.
* Fixture conditions: codes, candidate counts, ties and inexact products really occur on the frames the GPU tests use."""
import json
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

import haar_cases as C
from oracle import haar_ref


def f32(x):
    """a Python float rounded to float32 (round to nearest even); through a double the basic operations on float32
    operands round once"""
    return struct.unpack("f", struct.pack("f", x))[0]


def second_reading(img, cas, step):
    """-> (sum, sqsum, codes, ties) of one scaled image, window by window.  ties = [stage sums equal to their threshold,
    stump values equal to theirs, feature products that are inexact in float32]"""
    h, w = img.shape
    px = [[int(v) for v in row] for row in img]
    win_w, win_h = int(cas["haar.win"][0]), int(cas["haar.win"][1])
    stages, stumps, rects = (cas[k].tolist() for k in ("haar.stages", "haar.stumps", "haar.rects"))

    def box(x0, y0, bw, bh, power=1):
        return sum(px[y][x] ** power for y in range(y0, y0 + bh) for x in range(x0, x0 + bw))

    ii = [[0] * (w + 1) for _ in range(h + 1)]
    qq = [[0] * (w + 1) for _ in range(h + 1)]
    for y in range(h):
        run = runq = 0
        for x in range(w):
            run += px[y][x]
            runq += px[y][x] ** 2
            ii[y + 1][x + 1] = ii[y][x + 1] + run
            qq[y + 1][x + 1] = qq[y][x + 1] + runq

    def area(x0, y0, bw, bh):
        """a feature's rectangle from the table above (itself compared with the oracle's, and with `box` per window below)"""
        return ii[y0 + bh][x0 + bw] - ii[y0][x0 + bw] - ii[y0 + bh][x0] + ii[y0][x0]

    codes, ties = [], [0, 0, 0]
    for y in range(0, h - win_h, step):
        row = []
        for x in range(0, w - win_w, step):
            nw, nh = win_w - 2, win_h - 2
            vs, vq = box(x + 1, y + 1, nw, nh), box(x + 1, y + 1, nw, nh, 2)       # pixel by pixel
            assert vs == area(x + 1, y + 1, nw, nh)
            nf = nw * nh * vq - vs * vs                            # exact: far below 2^53
            norm = f32(1.0 / math.sqrt(float(nf))) if nf > 0 else 1.0
            code = 1
            for si, (first, count, thr) in enumerate(stages):
                acc = 0.0
                for fi, sthr, left, right in stumps[int(first):int(first + count)]:
                    r = rects[int(fi)]
                    terms = []
                    for j in range(3 if r[14] != 0 else 2):
                        rx, ry, rw, rh, wt = r[5 * j:5 * j + 5]
                        s = area(x + int(rx), y + int(ry), int(rw), int(rh))
                        terms.append(f32(wt * float(s)))
                        ties[2] += Fraction(wt) * s != Fraction(terms[-1])
                    v = f32(terms[0] + terms[1])
                    if len(terms) == 3:
                        v = f32(v + terms[2])
                    p = f32(v * norm)
                    ties[1] += p == sthr
                    acc += left if p < sthr else right
                ties[0] += acc == thr
                if acc < thr:
                    code = -si
                    break
            row.append(code)
        codes.append(row)
    return ii, qq, codes, ties


SMALL = {name: [C.Case("noise", C.noise_frame(wh + 13, ww + 18, [(14, 16, 7)], 71), 1.25),
                C.Case("half-flat", C.half_flat_frame(wh + 22, ww + 30, 72), 1.5),
                C.Case("checker", C.checker_frame(wh + 9, ww + 9), 1.25),
                C.Case("flat", C.flat_frame(wh + 4, ww + 5), 1.1)]
         for name, (ww, wh) in C.WINDOWS.items()}


@pytest.mark.parametrize("name", ["toy", "wide", "ties", "accept_all"])
def test_scale_stages_equals_a_second_reading(name):
    cas = C.CASCADES[name]()
    windows = 0
    for case in SMALL[name]:
        gray = C.gray_of(case.frame)
        n_scales = 0
        for k, t in C.all_scales(gray, cas, case.scale_factor):
            ii, qq, codes, _ = second_reading(t["scaled"], cas, t["step"])
            assert t["sum"].dtype == np.uint32 and t["sqsum"].dtype == np.uint64 and t["result"].dtype == np.int32
            assert t["sum"].tolist() == ii and t["sqsum"].tolist() == qq, (case.name, k)
            assert t["result"].tolist() == codes, (case.name, k)
            assert t["step"] == (1 if t["factor"] > 2.0 else 2)
            windows += t["result"].size
            n_scales += 1
        assert n_scales >= 2, case.name
        assert haar_ref.scale_stages(gray, cas, case.scale_factor, n_scales) is None
        assert haar_ref.scale_stages(gray, cas, case.scale_factor, n_scales + 3) is None
    assert windows >= 150, windows


def test_candidates_on_scale_stages_equal_the_recorded_lists():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "haar_toy_candidates.json")
    with open(path) as f:
        rec = json.load(f)["frames"]
    assert [tuple(r["size"]) for r in rec] == [(240, 320), (480, 640), (1080, 1920), (200, 260), (20, 300)]
    for r in rec:
        gray = C.gray_of(C.noise_frame(r["size"][0], r["size"][1], [tuple(b) for b in r["blobs"]], r["seed"]))
        for key, (sf, ms) in (("candidates_1.1_30", (1.1, 30)), ("candidates_1.25_40", (1.25, 40))):
            got = haar_ref.candidates(gray, C.toy(), sf, ms)
            assert [[int(v) for v in c] for c in got] == r[key], (r["size"], key)
    assert sum(len(r["candidates_1.1_30"]) for r in rec) >= 1000


def test_float_scale_factor_parts_from_double_at_scale_5_of_521():
    as_float = float(np.float32(1.1))
    assert as_float == 1.100000023841858 and as_float != 1.1

    def sizes(sf):
        out, f = [], 1.0
        while round(521 / f) > 24:                                 # Python's round: half to even, as cvRound
            out.append(round(521 / f))
            f *= sf
        return out
    d, s = sizes(1.1), sizes(as_float)
    assert len(d) == len(s) and [i for i in range(len(d)) if d[i] != s[i]] == [5]
    assert (d[5], s[5]) == (324, 323)
    # the oracle's own scale geometry says the same
    assert haar_ref.scale_geometry((120, 521), C.toy(), 1.1, 5)[3] == 324
    assert haar_ref.scale_geometry((120, 521), C.toy(), as_float, 5)[3] == 323
    frame = C.factor_frame()
    boxes, ncand = haar_ref.detect(frame, C.toy())
    assert ncand == 176 and tuple(int(v) for v in boxes[2]) == (261, 21, 78, 78)
    boxes_f, ncand_f = haar_ref.detect(frame, C.toy(), scale_factor=as_float)
    assert ncand_f == 177 and tuple(int(v) for v in boxes_f[2]) == (261, 22, 77, 77)
    # the transposed frame parts the same way
    t, tf = haar_ref.detect(C.factor_frame(True), C.toy()), haar_ref.detect(C.factor_frame(True), C.toy(), scale_factor=as_float)
    assert t != tf and (t[1], tf[1]) == (176, 177)


def test_sides_up_to_4096_where_the_float_factor_changes_a_scaled_size():
    """DESIGN lists them: the sides in 25 .. 4096 at which some scale of a 24-pixel window rounds differently"""
    as_float = float(np.float32(1.1))
    hit = []
    for side in range(25, 4097):
        f = g = 1.0
        while True:
            a, b = round(side / f), round(side / g)
            if a <= 24 and b <= 24:
                break
            if a != b:
                hit.append(side)
                break
            f *= 1.1
            g *= as_float
    assert hit == [521, 1563, 1833, 2459, 2605, 2622, 2716, 2902, 2936, 2949, 3055, 3188, 3572, 3647, 3708, 3758, 3803,
                   3830, 3931, 4050], hit


def test_reader_refuses_malformed_cascades_and_round_trips_the_generated_ones(pkg):
    haar = pkg.haar
    for name in ("wide", "ties", "toy", "accept_all"):
        cas = C.CASCADES[name]()
        haar.validate_cascade(cas)
        back = haar.load_cascade_xml(C.cascade_xml(cas))
        assert sorted(back) == sorted(cas)
        for k in cas:
            assert back[k].dtype == np.float32 and back[k].shape == cas[k].shape and back[k].tobytes() == cas[k].tobytes(), (name, k)
    for base in (C.ties(), C.wide()):
        cases = C.malformed(base)
        assert len(cases) >= 18
        for what, cas, in_xml in cases:
            with pytest.raises(ValueError, match="Haar cascade"):
                haar.validate_cascade(cas)
            if in_xml:
                with pytest.raises(ValueError, match="Haar cascade"):
                    haar.load_cascade_xml(C.cascade_xml(cas))
    # a window the XML states as a fraction, and one below 4 pixels
    with pytest.raises(ValueError):
        haar.load_cascade_xml(C.TOY_XML.replace("<width>24</width>", "<width>24.5</width>"))
    tiny = {k: v.copy() for k, v in C.accept_all().items()}
    tiny["haar.win"][:] = (3, 24)
    with pytest.raises(ValueError, match="window"):
        haar.validate_cascade(tiny)


def test_wide_fixture_reaches_every_code_and_rounds_its_products():
    cas = C.wide()
    assert cas["haar.win"].tolist() == [20.0, 28.0] and len(cas["haar.stages"]) >= 8 and len(cas["haar.stumps"]) >= 40
    rects = cas["haar.rects"].reshape(-1, 3, 5)
    used = rects[..., 4] != 0
    assert (used.sum(1) == 2).any() and (used.sum(1) == 3).any()
    x, y, w, h = (rects[..., i][used] for i in range(4))
    assert (x == 0).any() and (y == 0).any() and (x + w == 20).any() and (y + h == 28).any()      # every border
    assert (w == 1).any() and (h == 1).any()                                                     # 1 pixel thin
    weights = set(rects[..., 4][used].tolist())
    assert {-1.0, 2.0, 3.0, 1.5, 2.25, float(np.float32(1 / 3))} <= weights
    n_stages = len(cas["haar.stages"])
    codes, total, step1, last_rejected, windows, gone = set(), 0, 0, 0, 0, [0] * n_stages
    for case in C.frames("wide"):
        gray = C.gray_of(case.frame)
        for _, t in C.all_scales(gray, cas, case.scale_factor):
            codes |= set(np.unique(t["result"]).tolist())
            for s in range(n_stages):
                gone[s] += int((t["result"] == -s).sum())
            windows += t["result"].size
            last_rejected += int((t["result"][:, -1] == 0).sum())
        cand = haar_ref.candidates(gray, cas, case.scale_factor, 0)
        total += len(cand)
        step1 += sum(1 for c in cand if c[2] > 2 * 20)             # from a scale with factor > 2, where the grid step is 1
    assert codes == set(range(-(n_stages - 1), 2)), codes
    assert total >= 50 and last_rejected >= 1 and step1 >= 1
    # every stage rejects a share of what reaches it, and lets a share through
    for s in range(n_stages):
        assert 0.1 <= gone[s] / windows <= 0.9, (s, gone, windows)
        windows -= gone[s]
    # products that float32 has to round (second reading on one small frame)
    small = SMALL["wide"][0]
    ties = [0, 0, 0]
    for _, t in C.all_scales(C.gray_of(small.frame), cas, small.scale_factor):
        ties = [a + b for a, b in zip(ties, second_reading(t["scaled"], cas, t["step"])[3])]
    assert ties[2] >= 1, ties


def test_ties_fixture_lands_on_its_thresholds():
    """stage sums equal to the stage threshold (not rejected) and stump values equal to the stump threshold (right leaf):
    counted by the second reading over the small frames, which include flat and half-flat ones"""
    cas = C.ties()
    assert all(int(c) % 2 == 1 for c in cas["haar.stages"][:, 1]) and set(cas["haar.stages"][:, 2].tolist()) == {1.0}
    assert set(cas["haar.stumps"][:, 2:].ravel().tolist()) == {-1.0, 1.0} and (cas["haar.stumps"][:, 1] == 0).any()
    ties = [0, 0, 0]
    for case in SMALL["ties"]:
        for _, t in C.all_scales(C.gray_of(case.frame), cas, case.scale_factor):
            ties = [a + b for a, b in zip(ties, second_reading(t["scaled"], cas, t["step"])[3])]
    assert ties[0] >= 20 and ties[1] >= 20, ties
    # and on the frames the GPU tests tap: flat windows pass stage 0 on the tie +1 -1 +1 == 1.0
    t = haar_ref.scale_stages(C.gray_of(C.frames("ties")[1].frame), cas, 1.1, 0)
    assert (t["result"] != 0).all() and t["result"].size >= 20


def test_accept_all_counts_for_the_capacity_tests():
    """300 x 300 at factor 4: 138^2 + 51^2 windows; 538 x 538 passes the 65,536 a call can hold"""
    cas = C.accept_all()

    def count(side):
        n, k = 0, 0
        while True:
            g = haar_ref.scale_geometry((side, side), cas, 4.0, k)
            if g is None:
                return n
            step = 1 if g[0] > 2.0 else 2
            n += len(range(0, g[4] - 24, step)) * len(range(0, g[3] - 24, step))
            k += 1
    assert count(300) == 138 ** 2 + 51 ** 2 == 21645
    assert count(538) == 257 ** 2 + 110 ** 2 + 10 ** 2 > 65536
    assert len(haar_ref.candidates(C.gray_of(C.flat_frame(300, 300)), cas, 4.0, 0)) == 21645

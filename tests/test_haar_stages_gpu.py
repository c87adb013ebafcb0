"""GPU: the Haar fallback (csrc/haar_api.hip) launch by launch and end to end against oracle/haar_ref.py, on the cascades
and frames of tests/haar_cases.py (tests/test_haar_oracle.py holds the oracle to a second reading and shows that these
fixtures reach every stage code, ties, inexact products and the scan kernels' block edges).

Everything is integer or bit-exact float32: every comparison is equality, there is no tolerance anywhere.

* per stage: the five buffers of dfd_haar_tap (gray, scaled, sum, sqsum, result) == haar_ref.scale_stages for every
  cascade, frame and scale index; one index past the last scale is DFD_ERR_ARG
* raw candidates: detect_faces_haar(min_neighbors 0) == haar_ref.candidates as an ordered list, over scale factors
  1.1 / 1.25 / 1.5 / 4.0 and min sizes 0 / 30 / larger than any window; grouped boxes for min_neighbors 1 / 2 / 5
* the 120 x 521 and 521 x 120 frames, on which the double factor 1.1 and the float 1.1f part ways at scale 5, through
  detect_faces_haar, face_detection.detect_bounding_box and a Haar-only analyze_request (frame and JPEG route)
* max_out truncation with guard values behind the array; the 65,536-candidate capacity and the call after it
* malformed cascades are refused by dfd_create before any launch; argument errors"""
import io

import numpy as np
import pytest

import haar_cases as C
from oracle import haar_ref

pytestmark = pytest.mark.gpu

LARGE = 1 << 16                                                    # max_out that holds every candidate a call can return
TAPS = ("gray", "scaled", "sum", "sqsum", "result")


@pytest.fixture(scope="module")
def handles(pkg, seeded_sd):
    """cascade name -> a Haar-only handle, made on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, None, None, haar=C.CASCADES[name]()), device=0, max_batch=2)
        return made[name]
    yield get
    for h in made.values():
        h.close()


def _boxes(rects):
    return [tuple(int(v) for v in r) for r in rects]


@pytest.fixture(scope="module")
def want_candidates():
    """(cascade, frame name, scale factor, min size) -> the oracle's candidate list, computed once"""
    memo = {}

    def get(name, case, sf, min_size):
        key = (name, case.name, sf, min_size)
        if key not in memo:
            memo[key] = _boxes(haar_ref.candidates(C.gray_of(case.frame), C.CASCADES[name](), sf, min_size))
        return memo[key]
    return get


CASES = [(name, i) for name in ("wide", "ties", "toy", "accept_all") for i in range(len(C.frames(name)))]
IDS = [f"{name}-{C.frames(name)[i].name}" for name, i in CASES]


@pytest.mark.parametrize("name,i", CASES, ids=IDS)
def test_every_buffer_of_every_scale_equals_the_oracle(handles, pkg, name, i):
    h, cas, case = handles(name), C.CASCADES[name](), C.frames(name)[i]
    gray = C.gray_of(case.frame)
    n = 0
    for k, want in C.all_scales(gray, cas, case.scale_factor):
        got = h.haar_tap(case.frame, case.scale_factor, k)
        assert got["factor"] == want["factor"] and got["step"] == want["step"] and got["window"] == want["window"], k
        for tap in TAPS:
            assert got[tap].dtype == want[tap].dtype and got[tap].shape == want[tap].shape, (k, tap)
            assert np.array_equal(got[tap], want[tap]), (k, tap, np.argwhere(got[tap] != want[tap])[:5])
        n += 1
    assert n >= 1 and got["n_scales"] == n
    with pytest.raises(pkg._lib.DfdError) as e:                    # one past the last scale
        h.haar_tap(case.frame, case.scale_factor, n, names=("result",))
    assert e.value.code == -1 and "scale index" in str(e.value)


@pytest.mark.parametrize("name,i", CASES, ids=IDS)
def test_raw_candidates_equal_the_oracle_in_order(handles, want_candidates, name, i):
    """min_neighbors 0: groupRectangles returns its input, so the boxes ARE the candidate list in scan order"""
    h, case = handles(name), C.frames(name)[i]
    want = want_candidates(name, case, case.scale_factor, 0)
    got, n = h.detect_faces_haar(case.frame, case.scale_factor, 0, 0, max_out=LARGE, with_candidates=True)
    assert n == len(want) and got == want


MATRIX_FRAMES = ("blobs", "step1-scale", "row-padded")


@pytest.mark.parametrize("name", ["wide", "ties", "toy"])
def test_raw_candidates_over_scale_factors_and_min_sizes(handles, want_candidates, name):
    h = handles(name)
    total = 0
    for case in (c for c in C.frames(name) if c.name in MATRIX_FRAMES):
        for sf in (1.1, 1.25, 1.5, 4.0):
            for min_size in (0, 30, 10000):                        # 10000: larger than any window, nothing is evaluated
                want = want_candidates(name, case, sf, min_size)
                got, n = h.detect_faces_haar(case.frame, sf, 0, min_size, max_out=LARGE, with_candidates=True)
                assert n == len(want) and got == want, (case.name, sf, min_size)
                assert min_size < 10000 or want == []
                total += n
    assert total >= 100, "the fixture produced next to no candidates"


@pytest.mark.parametrize("name", ["wide", "ties", "toy"])
@pytest.mark.parametrize("frame", MATRIX_FRAMES + ("half-flat",))
def test_grouped_boxes_equal_the_oracle(handles, want_candidates, name, frame):
    h = handles(name)
    case = next(c for c in C.frames(name) if c.name == frame)
    cand = want_candidates(name, case, case.scale_factor, 0)
    for min_neighbors in (1, 2, 5):
        want = _boxes(haar_ref.group_rectangles(cand, min_neighbors, 0.2))
        got, n = h.detect_faces_haar(case.frame, case.scale_factor, min_neighbors, 0, max_out=LARGE, with_candidates=True)
        assert n == len(cand) and got == want, min_neighbors


# ----------------------------------------------------------------------------------------------- the scale factor
@pytest.mark.parametrize("transposed", [False, True], ids=["120x521", "521x120"])
def test_factor_frames_take_the_double_factor_on_every_route(pkg, handles, seeded_sd, transposed):
    """At side 521, scale 5, the double 1.1 gives round(521 / 1.1^5) = 324 and the float 1.1f gives 323
    (test_haar_oracle.py).  Every route to the cascade must report the double's boxes: the direct entry, the host
    fallback of face_detection, and the fused per-frame call behind analyze_request, from a frame and from a JPEG."""
    from PIL import Image

    h, cas = handles("toy"), C.toy()
    as_float = float(np.float32(1.1))
    frame = C.factor_frame(transposed)
    want, ncand = haar_ref.detect(frame, cas)
    wrong, _ = haar_ref.detect(frame, cas, scale_factor=as_float)
    assert _boxes(want) != _boxes(wrong) and len(want) == 3        # the frame tells the two factors apart
    got, n = h.detect_faces_haar(frame, 1.1, 5, 30, with_candidates=True)
    assert n == ncand == 176 and got == _boxes(want)
    assert h.detect_faces_haar(frame, as_float, 5, 30) == _boxes(wrong)       # the entry takes the double it is given
    assert pkg.face_detection.detect_bounding_box(frame, handle=h) == _boxes(want)
    cand = _boxes(haar_ref.candidates(C.gray_of(frame), cas, 1.1, 30))
    assert h.detect_faces_haar(frame, 1.1, 0, 30, max_out=LARGE) == cand
    # analyze_request reports faces[0] alone: a frame whose only box is the one the factor moves
    single = C.noise_frame(120, 521, C.FACTOR_BLOBS[1:2], 1)
    if transposed:
        single = np.ascontiguousarray(single.transpose(1, 0, 2))
    buf = io.BytesIO()
    Image.fromarray(single[..., ::-1]).save(buf, "JPEG", quality=92)
    decoded = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[..., ::-1])
    det = pkg.deepfake_detection.DeepfakeDetector(use_tta=False, num_tta_augmentations=1, detection_threshold=0.55, handle=h)
    for pixels, request in ((single, dict(frame=single)), (decoded, dict(jpeg=buf.getvalue()))):
        want1, wrong1 = haar_ref.detect(pixels, cas)[0], haar_ref.detect(pixels, cas, scale_factor=as_float)[0]
        assert len(want1) == 1 and _boxes(want1) != _boxes(wrong1)
        res = det.analyze_request(**request)
        assert res["analysis_mode"] == "face+frame" and res["faces_detected"] == 1
        b = res["face_bbox"]
        assert (b["x"], b["y"], b["width"], b["height"]) == _boxes(want1)[0], sorted(request)


# ------------------------------------------------------------------------------------------- truncation, capacity
def test_max_out_truncates_and_writes_nothing_behind_it(pkg, handles):
    import ctypes

    h = handles("toy")
    frame = C.factor_frame()
    want = _boxes(haar_ref.detect(frame, C.toy())[0])
    assert len(want) == 3
    for max_out in (1, 2, 3, 4):
        assert h.detect_faces_haar(frame, 1.1, 5, 30, max_out=max_out) == want[:max_out]
        out = np.full((max_out + 4, 4), -777, np.int32)            # guard rows behind the array
        n, nc = ctypes.c_int(), ctypes.c_int()
        rc = h._lib.dfd_detect_faces_haar(h._p, frame.ctypes.data_as(ctypes.c_void_p),
                                          frame.shape[0], frame.shape[1], frame.strides[0], 1.1, 5, 30,
                                          out.ctypes.data_as(ctypes.c_void_p), max_out, ctypes.byref(n), ctypes.byref(nc))
        assert rc == 0 and n.value == min(max_out, 3) and nc.value == 176
        assert _boxes(out[: n.value]) == want[:max_out] and (out[n.value:] == -777).all()
    # raw candidates truncate the same way
    cand = _boxes(haar_ref.candidates(C.gray_of(frame), C.toy(), 1.1, 30))
    assert h.detect_faces_haar(frame, 1.1, 0, 30, max_out=50) == cand[:50]


def test_candidate_capacity_and_the_call_after_it(pkg, handles):
    """accept_all at scale factor 4: 300 x 300 gives 138^2 + 51^2 = 21,645 candidates, 538 x 538 passes the 65,536 one call
    can hold (DFD_ERR_CAPACITY), and the handle is sound afterwards"""
    h, cas = handles("accept_all"), C.accept_all()
    frame = C.noise_frame(300, 300, [], 81)
    want = _boxes(haar_ref.candidates(C.gray_of(frame), cas, 4.0, 0))
    assert len(want) == 21645
    got, n = h.detect_faces_haar(frame, 4.0, 0, 0, max_out=LARGE, with_candidates=True)
    assert n == 21645 and got == want
    with pytest.raises(pkg._lib.DfdError) as e:
        h.detect_faces_haar(C.noise_frame(538, 538, [], 82), 4.0, 0, 0, max_out=LARGE)
    assert e.value.code == -6 and "candidate windows exceed the buffer of 65536" in str(e.value)
    small = C.frames("accept_all")[2]
    want = _boxes(haar_ref.candidates(C.gray_of(small.frame), cas, small.scale_factor, 0))
    assert h.detect_faces_haar(small.frame, small.scale_factor, 0, 0, max_out=LARGE) == want and len(want) >= 10
    got, n = h.detect_faces_haar(frame, 4.0, 0, 0, max_out=LARGE, with_candidates=True)
    assert n == 21645


@pytest.mark.parametrize("name", ["wide", "ties", "toy", "accept_all"])
def test_frames_no_scale_fits_give_nothing(pkg, handles, name):
    h = handles(name)
    for frame in C.no_scale_frames(name):
        assert h.detect_faces_haar(frame, 1.1, 0, 0, with_candidates=True) == ([], 0)
        assert haar_ref.candidates(C.gray_of(frame), C.CASCADES[name](), 1.1, 0) == []
        with pytest.raises(pkg._lib.DfdError) as e:
            h.haar_tap(frame, 1.1, 0, names=())
        assert e.value.code == -1


# ----------------------------------------------------------------------------------------- refusals before any launch
def test_malformed_cascades_are_refused_at_creation(pkg, seeded_sd):
    """dfd_create validates the cascade on the host (csrc/haar_validate.h; the same code runs under the sanitizers in
    test_host_asan.py) and returns DFD_ERR_BLOB naming haar: none of these ever reaches haar_eval_kernel"""
    cases = C.malformed()
    assert len(cases) >= 18
    for what, cas, _ in cases:
        with pytest.raises(ValueError):
            pkg.haar.validate_cascade(cas)                         # the build under test has the check: the blob is refused
        with pytest.raises(pkg._lib.DfdError) as e:
            pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, None, None, haar=cas), device=0, max_batch=1)
        assert e.value.code == -2 and "haar" in str(e.value), what
    odd = dict(C.ties())
    odd["haar.stumps"] = odd["haar.stumps"].ravel()[:-1]
    with pytest.raises(pkg._lib.DfdError) as e:
        pkg._lib.Handle(pkg.weights.pack_all(seeded_sd, None, None, haar=odd), device=0, max_batch=1)
    assert e.value.code == -2 and "haar" in str(e.value)


def test_argument_errors(pkg, handles):
    import ctypes

    h = handles("toy")
    frame = C.frames("toy")[0].frame
    for sf in (1.0, 0.5, 0.0, -1.1, float("nan")):
        with pytest.raises(pkg._lib.DfdError) as e:
            h.detect_faces_haar(frame, sf, 5, 30)
        assert e.value.code == -1
        with pytest.raises(pkg._lib.DfdError) as e:
            h.haar_tap(frame, sf, 0)
        assert e.value.code == -1
    for max_out in (0, -3):
        with pytest.raises(pkg._lib.DfdError) as e:
            h.detect_faces_haar(frame, 1.1, 5, 30, max_out=max_out)
        assert e.value.code == -1
    with pytest.raises(pkg._lib.DfdError) as e:
        h.haar_tap(frame, 1.1, -1)
    assert e.value.code == -1
    out = np.zeros((4, 4), np.int32)
    n = ctypes.c_int()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)             # noqa: E731
    short = frame.shape[1] * 3 - 1                                 # a stride below 3 * width
    assert h._lib.dfd_detect_faces_haar(h._p, ptr(frame), frame.shape[0], frame.shape[1], short, 1.1, 5, 30, ptr(out), 4,
                                        ctypes.byref(n), None) == -1
    dims, factor = np.zeros(8, np.int32), ctypes.c_double()
    assert h._lib.dfd_haar_tap(h._p, ptr(frame), frame.shape[0], frame.shape[1], short, 1.1, 0, None, None, 0, None, ptr(dims),
                               ctypes.byref(factor)) == -1
    buf, nb = np.zeros(1 << 16, np.uint8), ctypes.c_size_t()
    assert h._lib.dfd_haar_tap(h._p, ptr(frame), frame.shape[0], frame.shape[1], frame.strides[0], 1.1, 0, b"norm", ptr(buf), buf.size,
                               ctypes.byref(nb), ptr(dims), ctypes.byref(factor)) == -1       # a buffer the tap does not know
    assert "no buffer named" in h._lib.dfd_last_error(h._p).decode()
    assert h._lib.dfd_haar_tap(h._p, ptr(frame), frame.shape[0], frame.shape[1], frame.strides[0], 1.1, 0, b"sum", ptr(buf), 16,
                               ctypes.byref(nb), ptr(dims), ctypes.byref(factor)) == -1       # a capacity below the buffer
    assert nb.value == (frame.shape[0] + 1) * (frame.shape[1] + 1) * 4 and (buf == 0).all()
    assert h._lib.dfd_detect_faces_haar(h._p, None, frame.shape[0], frame.shape[1], frame.strides[0], 1.1, 5, 30, ptr(out), 4,
                                        ctypes.byref(n), None) == -1
    # the handle still works
    assert h.detect_faces_haar(frame, 1.1, 0, 0, max_out=LARGE) == _boxes(haar_ref.candidates(C.gray_of(frame), C.toy(), 1.1, 0))

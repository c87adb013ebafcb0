"""GPU: dfd_mtcnn_detect / dfd_mtcnn_extract and the MTCNN class (every face, landmarks, margin, image_size, orderings,
pyramid parameters, lists of images) against tests/mtcnn_api_oracle.py, with the seeded cascade of the `mt_handle` fixture.

Comparison rule (that of tests/test_mtcnn_gpu.py).  Where device and oracle take the same keep / drop decisions the number
of faces, the integer crop geometry and the crops are exact.  The images are seeded so that, IN THE ORACLE ALONE, no score
lies within 1e-4 of the threshold that acts on it - every P-Net cell, R-Net and O-Net window against `thresholds`, every
returned probability against the 0.9 of "largest_over_threshold": the closest is 1.6e-4 (searched on the CPU over seeds
100-129; `_check_clear` asserts it for every image a test uses and tells the author to pick another seed, it does not skip).
Float outputs get the tolerances below: 4 x the largest |device - oracle| measured on the GPU over the images of this file
(probabilities 5.364e-7, box corners 1.144e-4 px, landmark coordinates 7.248e-4 px; every comparison prints what it
sees).
"""
import numpy as np
import pytest

from tests import mt_images
from tests import mtcnn_api_oracle as A

pytestmark = pytest.mark.gpu

TOL_PROB = 4 * 5.364e-7
TOL_BOX = 4 * 1.144e-4
TOL_PTS = 4 * 7.248e-4

# (h, w, seed): faces with the default cascade parameters / Q / R below (oracle, CPU)
DEFAULT_IMAGES = [(300, 280, 100), (300, 280, 119), (260, 340, 121), (260, 340, 127), (300, 280, 3), (12, 40, 8)]   # 5 3 4 2 3 0
Q = dict(min_face_size=24, factor=0.65, thresholds=(0.62, 0.68, 0.6))
Q_IMAGES = [(300, 280, 117), (300, 280, 124), (200, 230, 119)]                                                  # 3 5 2
R = dict(min_face_size=16, factor=0.78, thresholds=(0.55, 0.65, 0.6))
R_IMAGES = [(150, 170, 125), (150, 170, 128)]                                                                   # 18 16
SELECTIONS = ["probability", "largest", "center_weighted_size", "largest_over_threshold"]


@pytest.fixture(scope="module")
def sd(pkg, mtcnn_sd):
    return pkg.weights.to_torch(mtcnn_sd)


def _rgb(case):
    return mt_images.textured(*case)


def _bgr(rgb):
    return np.ascontiguousarray(rgb[..., ::-1])


def _params(pkg, P):
    return pkg._lib.mtcnn_params(P.image_size, P.margin, P.min_face_size, P.thresholds, P.factor, P.selection, P.keep_all,
                                 P.post_process)


def _check_clear(trace, case):
    assert trace.closest() >= 1e-4, (f"image {case}: an oracle score lies {trace.closest():.2e} from its threshold: "
                                     "threshold-ambiguous input, pick another seed")


def _compare(got_rows, got_pts, want_rows, want_pts, what):
    assert got_rows.shape == want_rows.shape, (what, got_rows.shape, want_rows.shape)      # the number of faces is exact
    if len(want_rows) == 0:
        return 0.0, 0.0, 0.0
    dp = float(np.abs(got_rows[:, 4] - want_rows[:, 4]).max())
    db = float(np.abs(got_rows[:, :4] - want_rows[:, :4]).max())
    dl = float(np.abs(got_pts - want_pts).max()) if got_pts is not None else 0.0
    print(f"{what}: faces {len(want_rows)} max|d| prob {dp:.3e} box {db:.3e} points {dl:.3e}")
    assert dp <= TOL_PROB and db <= TOL_BOX and dl <= TOL_PTS, (what, dp, db, dl)
    return dp, db, dl


@pytest.mark.parametrize("case", DEFAULT_IMAGES)
def test_detect_every_face_with_landmarks(pkg, mt_handle, sd, case):
    rgb = _rgb(case)
    P = A.Params(selection="none", keep_all=True)
    t = A.Trace()
    want_rows, want_pts = A.detect(sd, rgb, P, t)
    _check_clear(t, case)
    (rows, pts, _), = mt_handle.mtcnn_detect([_bgr(rgb)], _params(pkg, P), landmarks=True)
    assert pts.shape == (len(rows), 5, 2)
    _compare(rows, pts, want_rows, want_pts, f"detect {case}")
    # the class: detect(landmarks=True) -> (boxes, probs, points), None without a face
    m = pkg.mtcnn.MTCNN(select_largest=False, handle=mt_handle)
    boxes, probs, points = m.detect(rgb, landmarks=True)
    if len(want_rows) == 0:
        assert boxes is None and probs == [None] and points is None
    else:
        assert np.array_equal(boxes, rows[:, :4]) and np.array_equal(probs, rows[:, 4]) and np.array_equal(points, pts)


def test_multi_face_images_have_several_faces(sd):
    counts = [len(A.detect(sd, _rgb(c), A.Params(selection="none", keep_all=True))[0]) for c in DEFAULT_IMAGES]
    assert counts == [5, 3, 4, 2, 3, 0], counts


@pytest.mark.parametrize("size", [160, 224, 112])
@pytest.mark.parametrize("margin", [0, 14, 40])
def test_keep_all_crops_are_bit_exact(pkg, mt_handle, sd, size, margin):
    for case in DEFAULT_IMAGES[:3]:
        rgb = _rgb(case)
        P = A.Params(image_size=size, margin=margin, selection="none", keep_all=True, post_process=False)
        want_rows, want_pts, want_faces = A.forward(sd, rgb, P)
        # same integer geometry from the device's own boxes as from the oracle's (else the crops could not be compared)
        (rows, _, faces), = mt_handle.mtcnn_extract([_bgr(rgb)], _params(pkg, P))
        _compare(rows, None, want_rows, None, f"extract {case} {size}/{margin}")
        for k in range(len(rows)):
            assert A.crop_box(rows[k, :4], *rgb.shape[:2], P) == A.crop_box(want_rows[k, :4], *rgb.shape[:2], P), \
                f"{case} face {k}: a box corner within {TOL_BOX} px of an integer - pick another seed"
        assert faces.shape == want_faces.shape and np.array_equal(faces, want_faces)
        m = pkg.mtcnn.MTCNN(image_size=size, margin=margin, post_process=False, select_largest=False, keep_all=True, handle=mt_handle)
        out, probs = m(rgb, return_prob=True)
        assert tuple(out.shape) == (len(want_rows), 3, size, size) and np.array_equal(np.asarray(out), want_faces)
        assert np.array_equal(probs, rows[:, 4])
        std = pkg.mtcnn.MTCNN(image_size=size, margin=margin, post_process=True, select_largest=False, keep_all=True, handle=mt_handle)(rgb)
        assert np.array_equal(np.asarray(std), (want_faces - np.float32(127.5)) / np.float32(128.0))


@pytest.mark.parametrize("selection", SELECTIONS)
def test_orderings_follow_the_oracle(pkg, mt_handle, sd, selection):
    for case in DEFAULT_IMAGES[:5]:
        rgb = _rgb(case)
        t = A.Trace()
        Pall = A.Params(selection=selection, keep_all=True, post_process=False)
        want_rows, want_pts = A.detect(sd, rgb, Pall, t)
        _check_clear(t, case)
        (rows, pts, _), = mt_handle.mtcnn_detect([_bgr(rgb)], _params(pkg, Pall), landmarks=True)
        _compare(rows, pts, want_rows, want_pts, f"{selection} {case}")
        # the oracle's order of the DEVICE's rows is the order the device returned them in
        (plain, _, _), = mt_handle.mtcnn_detect([_bgr(rgb)], _params(pkg, A.Params(selection="none", keep_all=True)), landmarks=False)
        assert np.array_equal(plain[A.order_rows(plain, selection, *rgb.shape[:2])], rows)
        # keep_all=False: row 0 of that order, and its crop
        P1 = A.Params(selection=selection, keep_all=False, post_process=False)
        (r1, _, f1), = mt_handle.mtcnn_extract([_bgr(rgb)], _params(pkg, P1))
        assert np.array_equal(r1, rows[:1])
        w1 = A.forward(sd, rgb, P1)[2]
        assert np.array_equal(f1, w1)
        m = pkg.mtcnn.MTCNN(post_process=False, select_largest=selection == "largest", selection_method=selection, handle=mt_handle)
        face, prob = m(rgb, return_prob=True)
        if len(want_rows) == 0:
            assert face is None and prob is None
        else:
            assert np.array_equal(np.asarray(face), w1[0]) and prob == float(rows[0, 4])
    # select_largest orders MTCNN.detect
    rgb = _rgb(DEFAULT_IMAGES[0])
    boxes, probs = pkg.mtcnn.MTCNN(select_largest=True, handle=mt_handle).detect(rgb)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    assert len(boxes) == 5 and np.all(np.diff(area) <= 0)


@pytest.mark.parametrize("name,kw,cases", [("Q", Q, Q_IMAGES), ("R", R, R_IMAGES)])
def test_pyramid_parameters_and_thresholds(pkg, mt_handle, sd, name, kw, cases):
    for case in cases:
        rgb = _rgb(case)
        P = A.Params(selection="none", keep_all=True, post_process=False, image_size=112, margin=14, **kw)
        t = A.Trace()
        want_rows, want_pts, want_faces = A.forward(sd, rgb, P, t)
        _check_clear(t, case)
        assert len(want_rows) >= 2
        # level count: the default pyramid has another number of levels, and gives other rows
        assert t.levels == len(A.scale_pyramid(*rgb.shape[:2], P)) != len(A.scale_pyramid(*rgb.shape[:2], A.Params()))
        (rows, pts, faces), = mt_handle.mtcnn_extract([_bgr(rgb)], _params(pkg, P), landmarks=True)
        _compare(rows, pts, want_rows, want_pts, f"{name} {case}")
        assert np.array_equal(faces, want_faces)
        m = pkg.mtcnn.MTCNN(select_largest=False, handle=mt_handle, **kw)
        boxes, probs = m.detect(rgb)
        assert np.array_equal(boxes, rows[:, :4]) and np.array_equal(probs, rows[:, 4])


def test_a_list_of_images_equals_the_single_calls(pkg, mt_handle):
    cases = [DEFAULT_IMAGES[0], DEFAULT_IMAGES[5], DEFAULT_IMAGES[2], Q_IMAGES[2], DEFAULT_IMAGES[1]]
    imgs = [_bgr(_rgb(c)) for c in cases]
    p = pkg._lib.mtcnn_params(224, 14, selection="none", keep_all=True, post_process=True)
    together = mt_handle.mtcnn_extract(imgs, p, landmarks=True)
    assert [len(r[0]) for r in together] == [5, 0, 4, 0, 3]
    for img, (rows, pts, faces) in zip(imgs, together):
        (r1, p1, f1), = mt_handle.mtcnn_extract([img], p, landmarks=True)
        assert np.array_equal(rows, r1) and np.array_equal(pts, p1) and np.array_equal(faces, f1)
    # room for fewer faces than an image has: the binding asks again with more, same rows
    again = mt_handle.mtcnn_extract(imgs, p, landmarks=True, max_faces=2)
    for a, b in zip(again, together):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the class takes the list
    m = pkg.mtcnn.MTCNN(image_size=224, margin=14, select_largest=False, keep_all=True, handle=mt_handle)
    faces, probs = m([_rgb(c) for c in cases], return_prob=True)
    assert faces[1] is None and probs[1] == [None] and np.array_equal(np.asarray(faces[0]), together[0][2])
    boxes, probs, points = m.detect([_rgb(c) for c in cases], landmarks=True)
    assert boxes[3] is None and np.array_equal(points[4], together[4][1])


def test_host_box_path_gives_identical_arrays(pkg, mt_handle, monkeypatch):
    imgs = [_bgr(_rgb(c)) for c in (DEFAULT_IMAGES[0], R_IMAGES[0], DEFAULT_IMAGES[5], DEFAULT_IMAGES[3])]
    for kw in (dict(selection="none"), dict(selection="center_weighted_size", image_size=112, margin=40, **R)):
        p = pkg._lib.mtcnn_params(keep_all=True, **kw)
        got = {}
        for flag in ("1", "0"):
            monkeypatch.setenv("DFD_MT_DEVICE_BOXES", flag)
            got[flag] = mt_handle.mtcnn_extract(imgs, p, landmarks=True)
        assert sum(len(r[0]) for r in got["1"]) >= 7
        for a, b in zip(got["1"], got["0"]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # a crop beyond the device blocks' capacity (tests/test_mtcnn_gpu.py: 700 x 900) takes the host path by itself
    big = _bgr(mt_images.textured(700, 900, 3))
    p = pkg._lib.mtcnn_params(selection="none", keep_all=True)
    monkeypatch.setenv("DFD_MT_DEVICE_BOXES", "1")
    a = mt_handle.mtcnn_extract([big], p, landmarks=True)[0]
    monkeypatch.setenv("DFD_MT_DEVICE_BOXES", "0")
    b = mt_handle.mtcnn_extract([big], p, landmarks=True)[0]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_existing_entry_points_keep_their_bits(pkg, mt_handle, sd):
    from oracle import mtcnn_ref as M

    for case in DEFAULT_IMAGES[:3] + [tuple(c) for c in mt_images.CASES]:
        rgb = _rgb(case)
        bgr = _bgr(rgb)
        tap = mt_handle.mtcnn_tap(bgr, "stage3") if min(rgb.shape[:2]) >= 20 else np.zeros((0, 5), np.float32)
        # detect() without landmarks: exactly the rows of the "stage3" tap
        boxes, probs = pkg.mtcnn.MTCNN(select_largest=False, handle=mt_handle).detect(rgb)
        if len(tap) == 0:
            assert boxes is None
        else:
            assert np.array_equal(boxes, tap[:, :4]) and np.array_equal(probs, tap[:, 4])
        # dfd_mtcnn_align: the crop the oracle of the reference's construction gives (what it returned before), and the
        # same bits as the new call with that construction
        face, box = mt_handle.mtcnn_align(bgr)
        want = M.mtcnn_forward(sd, rgb)
        assert (face is None) == (want is None)
        p = pkg._lib.mtcnn_params(selection="probability", keep_all=False, post_process=False)
        (r1, _, f1), = mt_handle.mtcnn_extract([bgr], p)
        if face is not None:
            assert np.array_equal(face, want)
            assert np.array_equal(r1[0], box) and np.array_equal(f1[0], face)
        ref = pkg.mtcnn.MTCNN(select_largest=False, post_process=False, handle=mt_handle)(rgb)
        assert (ref is None) == (face is None) and (face is None or np.array_equal(np.asarray(ref), face))


def test_bad_parameters_are_argument_errors(pkg, mt_handle):
    bgr = _bgr(_rgb(DEFAULT_IMAGES[0]))
    good = pkg._lib.mtcnn_params(selection="none", keep_all=True)
    before = mt_handle.mtcnn_detect([bgr], good)[0]
    bad = [dict(image_size=40, margin=40), dict(image_size=0), dict(margin=-1), dict(factor=1.0), dict(factor=0.0),
           dict(min_face_size=11), dict(thresholds=(0.6, 1.5, 0.7)), dict(thresholds=(float("nan"), 0.7, 0.7))]
    for kw in bad:
        with pytest.raises(pkg._lib.DfdError) as e:
            mt_handle.mtcnn_detect([bgr], pkg._lib.mtcnn_params(**kw))
        assert e.value.code == -1, (kw, e.value)                                  # DFD_ERR_ARG
    p = pkg._lib.mtcnn_params()
    p.selection = 9
    with pytest.raises(pkg._lib.DfdError) as e:
        mt_handle.mtcnn_detect([bgr], p)
    assert e.value.code == -1
    with pytest.raises(pkg._lib.DfdError) as e:
        mt_handle.mtcnn_detect([bgr], good, max_faces=0)
    assert e.value.code == -1
    after = mt_handle.mtcnn_detect([bgr], good)[0]                                # the handle answers a good call afterwards
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and len(after[0]) == 5
    with pytest.raises(ValueError):
        pkg.mtcnn.MTCNN(selection_method="nearest", handle=mt_handle)


def test_a_blob_without_the_cascade_is_a_state_error(pkg, b0_handle):
    with pytest.raises(pkg._lib.DfdError) as e:
        b0_handle.mtcnn_detect([_bgr(_rgb(DEFAULT_IMAGES[0]))])
    assert e.value.code == -5                                                     # DFD_ERR_STATE

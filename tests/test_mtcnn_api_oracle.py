"""CPU: the parameterised MTCNN oracle (tests/mtcnn_api_oracle.py) against the pieces it generalises - with the
reference's construction it is oracle/mtcnn_ref.mtcnn_forward bit for bit, and its crop (any box, output size and margin,
margins that clip at the border included) is PIL's crop + BILINEAR resize bit for bit."""
import numpy as np
import pytest

from oracle import mtcnn_ref as M
from tests import mt_images
from tests import mtcnn_api_oracle as A


@pytest.fixture(scope="module")
def sd(pkg, mtcnn_sd):
    return pkg.weights.to_torch(mtcnn_sd)


@pytest.mark.parametrize("idx", range(len(mt_images.CASES)))
def test_reference_construction_is_mtcnn_ref(sd, idx):
    rgb = mt_images.images()[idx]
    P = A.Params(selection="probability", keep_all=False, post_process=False)
    taps = {}
    want = M.mtcnn_forward(sd, rgb, taps)
    rows, points, faces = A.forward(sd, rgb, P)
    all_rows, all_points = A.detect_face(sd, rgb, P)
    assert np.array_equal(all_rows, taps["stage3"].astype(np.float32))
    assert all_points.shape == (len(all_rows), 5, 2)
    assert A.scale_pyramid(*rgb.shape[:2], P) == M.scale_pyramid(*rgb.shape[:2])
    if want is None:
        # no row, or a selected box that is empty once clipped (mtcnn_ref returns None there, this oracle a zero face)
        assert len(rows) == 0 or not faces.any()
    else:
        assert len(rows) == 1 and np.array_equal(rows[0], taps["selected"])
        assert np.array_equal(faces[0], want)


BOXES = [((30.2, 41.7, 141.9, 160.3), 160, 0), ((30.2, 41.7, 141.9, 160.3), 224, 14), ((5.5, 3.1, 88.0, 120.9), 112, 40),
         ((-12.0, 150.4, 60.6, 239.9), 160, 40), ((200.3, 10.0, 299.5, 95.0), 224, 40), ((100.0, 100.0, 260.0, 260.0), 160, 0),
         ((40.0, 40.0, 200.0, 200.0), 112, 14), ((120.7, 60.2, 310.0, 250.0), 96, 20)]


@pytest.mark.parametrize("box,size,margin", BOXES)
def test_generalised_crop_is_pil(box, size, margin):
    Image = pytest.importorskip("PIL.Image")
    rgb = mt_images.textured(240, 300, 21)
    P = A.Params(image_size=size, margin=margin, post_process=False)
    ibox = A.crop_box(box, 240, 300, P)
    # extract_face as the package writes it, on the PIL image
    m = [margin * (box[2] - box[0]) / (size - margin), margin * (box[3] - box[1]) / (size - margin)]
    want_box = (int(max(box[0] - m[0] / 2, 0)), int(max(box[1] - m[1] / 2, 0)), int(min(box[2] + m[0] / 2, 300)),
                int(min(box[3] + m[1] / 2, 240)))
    assert ibox == want_box
    bil = getattr(Image, "Resampling", Image).BILINEAR
    want = np.asarray(Image.fromarray(rgb).crop(want_box).resize((size, size), bil))
    got = A.extract_face(rgb, box, P)
    assert np.array_equal(got, want.transpose(2, 0, 1).astype(np.float32))
    std = A.extract_face(rgb, box, A.Params(image_size=size, margin=margin, post_process=True))
    assert np.array_equal(std, (got - 127.5) / 128.0)


def test_orderings():
    rows = np.array([[10, 10, 50, 60, 0.95], [100, 80, 180, 170, 0.80], [60, 50, 90, 95, 0.99], [10, 10, 50, 60, 0.95],
                     [0, 0, 200, 200, 0.85]], np.float32)
    assert list(A.order_rows(rows, "none", 200, 240)) == [0, 1, 2, 3, 4]
    assert list(A.order_rows(rows, "probability", 200, 240)) == [2, 3, 0, 4, 1]        # equal keys: the later row first
    assert list(A.order_rows(rows, "largest", 200, 240)) == [4, 1, 3, 0, 2]
    assert list(A.order_rows(rows, "largest_over_threshold", 200, 240)) == [3, 0, 2]
    cw = A.order_rows(rows, "center_weighted_size", 200, 240)
    assert cw[0] == 4 and sorted(cw) == [0, 1, 2, 3, 4]

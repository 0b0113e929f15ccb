"""The drawing calls pipeline_v3_RTDETR/inference.py makes through the `cv2` shim (or OpenCV, when it is installed): rectangle pixels as
imgproc/drawing.cpp paints them for thickness 1, 2 and filled, and putText marking pixels near its baseline origin."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def cv2():
    import ffp_amd.compat as compat
    compat.install()
    import cv2
    return cv2


def test_rectangle_thickness_2(cv2):
    img = np.zeros((30, 40, 3), np.uint8)
    out = cv2.rectangle(img, (10, 10), (20, 16), (0, 255, 0), 2)
    exp = np.zeros((30, 40), bool)
    exp[9:12, 10:21] = exp[15:18, 10:21] = True          # horizontal edges: one pixel either side, the edge's own length
    exp[10:17, 9:12] = exp[10:17, 19:22] = True          # vertical edges
    for x, y in ((10, 10), (20, 10), (20, 16), (10, 16)):   # radius-1 circles (plus shapes) at the corners
        exp[y, x - 1:x + 2] = exp[y - 1:y + 2, x] = True
    got = (img == (0, 255, 0)).all(-1)
    np.testing.assert_array_equal(got, exp)
    assert not got[9, 9] and not got[17, 21]               # outer diagonal corner pixels stay unpainted
    assert ((img == 0).all(-1) | got).all()
    assert out is img or np.shares_memory(out, img)


def test_rectangle_thickness_1_and_filled(cv2):
    img = np.zeros((12, 12), np.uint8)
    cv2.rectangle(img, (8, 7), (2, 3), 200, 1)               # corners in any order
    exp = np.zeros((12, 12), np.uint8)
    exp[3, 2:9] = exp[7, 2:9] = 200
    exp[3:8, 2] = exp[3:8, 8] = 200
    np.testing.assert_array_equal(img, exp)
    img2 = np.zeros((12, 12, 3), np.uint8)
    cv2.rectangle(img2, (-3, 5), (4, 20), (1, 2, 3), -1)     # clipped to the image
    exp2 = np.zeros((12, 12, 3), np.uint8)
    exp2[5:12, 0:5] = (1, 2, 3)
    np.testing.assert_array_equal(img2, exp2)


def test_put_text(cv2):
    img = np.zeros((60, 200, 3), np.uint8)
    cv2.putText(img, "Face: 0.87", (10, 40), cv2.FONT_HERSHEY_SIMPLEX, 0.5, (0, 255, 0), 2)
    ys, xs = np.nonzero(img[..., 1])
    assert len(ys) > 20 and (img[..., 0] == 0).all() and (img[..., 2] == 0).all()
    assert xs.min() >= 8 and ys.max() <= 44 and ys.min() >= 20       # left end of the baseline at org

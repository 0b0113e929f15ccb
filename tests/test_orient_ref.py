"""tests/orient_ref.py, the numpy restatement the orient kernel is tested against, against the two host routes it stands in for: Pillow's
ImageOps.exif_transpose on an image that carries the tag, and the cv2 shim's _oriented on a decoded frame. No device."""
import numpy as np
import pytest
from PIL import Image, ImageOps

import orient_ref


def sample():
    return np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)        # every pixel differs from every other


@pytest.mark.parametrize("o", range(1, 9))
def test_equals_pillows_exif_transpose(o):
    a = sample()
    im = Image.fromarray(a)
    exif = im.getexif()
    exif[0x0112] = o
    im.info["exif"] = exif.tobytes()
    got = np.asarray(ImageOps.exif_transpose(im))
    want = orient_ref.orient(a, o)
    assert got.shape == want.shape == orient_ref.out_shape(5, 7, o) + (3,)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("o", range(1, 9))
def test_equals_the_cv2_shims_oriented(o):
    import ffp_amd.compat as compat
    compat.install()
    import cv2 as shim
    if not hasattr(shim, "_oriented"):
        pytest.fail("the cv2 shim stands aside for a real OpenCV here: its _oriented is not there to compare with")
    a = sample()
    assert np.array_equal(shim._oriented(a, o), orient_ref.orient(a, o))


def test_gray_images_and_refused_values():
    g = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(orient_ref.orient(g, 6), np.rot90(g, -1))          # 6: a quarter turn clockwise
    assert np.array_equal(orient_ref.orient(g, 8), np.rot90(g, 1))
    assert np.array_equal(orient_ref.orient(g, 3), np.rot90(g, 2))
    for o in (0, 9):
        with pytest.raises(ValueError):
            orient_ref.orient(g, o)

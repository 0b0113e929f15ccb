"""Host checks of tests/image_input_ref.py, the reference tests/test_gpu_image_input.py holds the image-input kernels to: its geometry against
numbers worked out by hand, its compositions against the end-to-end functions of the three oracles, and the one place where the oracle and the
kernels word the resize scale differently."""
import numpy as np
import pytest

from oracle import ultra_post

import image_input_ref as R
import rtdetr_ref
import scrfd_ref

rng = np.random.default_rng(20)
FRAME = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
yy, xx = np.mgrid[0:97, 0:131]
CHECKER = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, 2)

# LetterBox(auto=True, stride 32) by hand, r = min(imgsz / h, imgsz / w), new = round(side * r), pad = (imgsz - new) % 32 split as round(p / 2 -+ 0.1):
#   128 x 96 -> r 0.5: 64 x 48, 16 rows of pad, 8 + 8          131 x 97 -> r 64/131: 64 x round(47.39) = 47, 17 rows, 8 + 9
#   30 x 20 -> r 64/30: 64 x round(42.67) = 43, 21 rows, 10 + 11  64 x 64 at 96 -> r 1.5: 96 x 96
#   1 x 97 -> r 64/97: round(0.66) = 1 x 64, 63 % 32 = 31 columns, 15 + 16   127 x 1 -> r 64/127: 64 x round(0.504) = 1, 31 rows, 15 + 16
#   131 x 1 -> r 64/131: 64 x round(0.489) = 0 rows: cv2.resize raises
YOLO_GEOMETRY = {      # (box, imgsz): (net_h, net_w, new_h, new_w, top, bottom, left, right)
    ((0, 0, 64, 64), 64): (64, 64, 64, 64, 0, 0, 0, 0),
    ((67, 33, 131, 97), 64): (64, 64, 64, 64, 0, 0, 0, 0),
    ((0, 0, 128, 96), 64): (64, 64, 48, 64, 8, 8, 0, 0),
    ((0, 0, 131, 97), 64): (64, 64, 47, 64, 8, 9, 0, 0),
    ((10, 20, 40, 40), 64): (64, 64, 43, 64, 10, 11, 0, 0),
    ((3, 1, 67, 65), 96): (96, 96, 96, 96, 0, 0, 0, 0),
    ((5, 0, 6, 97), 64): (64, 32, 64, 1, 0, 0, 15, 16),
    ((4, 96, 131, 97), 64): (32, 64, 1, 64, 15, 16, 0, 0),
    ((0, 96, 131, 97), 64): (0, 64, 0, 64, 0, 0, 0, 0),
}
# RetinaFace.detect by hand: the picture ratio h / w against det_h / det_w picks the side that fills, int() truncates the other, scale = new_h / h
#   131 x 97 (0.7405) at 64 x 64: 64 x int(47.39) = 47, 47 / 97      at 96 x 64 (0.667): int(64 / 0.7405) = 86 x 64, 64 / 97
#   30 x 20 (0.667) at 64 x 64: 64 x int(42.67) = 42, 2.1            at 96 x 64: the ratios tie, 96 x int(64.0) = 64, 3.2
SCRFD_GEOMETRY = {      # (box, (det_w, det_h)): ((net_h, net_w, new_h, new_w, top, bottom, left, right), det_scale)
    ((0, 0, 64, 64), (64, 64)): ((64, 64, 64, 64, 0, 0, 0, 0), 1.0),
    ((0, 0, 131, 97), (64, 64)): ((64, 64, 47, 64, 0, 17, 0, 0), 47 / 97),
    ((10, 20, 40, 40), (64, 64)): ((64, 64, 42, 64, 0, 22, 0, 0), 2.1),
    ((67, 33, 131, 97), (96, 64)): ((64, 96, 64, 64, 0, 0, 0, 32), 1.0),
    ((0, 0, 131, 97), (96, 64)): ((64, 96, 64, 86, 0, 0, 0, 10), 64 / 97),
    ((10, 20, 40, 40), (96, 64)): ((64, 96, 64, 96, 0, 0, 0, 0), 3.2),
}


def test_geometry_matches_hand_checked_numbers():
    for (box, imgsz), want in YOLO_GEOMETRY.items():
        assert R.geometry(R.YOLO, box, imgsz) == want, (box, imgsz)
    for (box, size), (want, scale) in SCRFD_GEOMETRY.items():
        assert R.geometry(R.SCRFD, box, size) == want, (box, size)
        assert R.scrfd_scale(box, size) == np.float32(scale), (box, size)
    assert R.geometry(R.RTDETR, (0, 17, 131, 81), 64) == (64, 64, 64, 64, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        R.network_u8(R.SCRFD, FRAME, (0, 96, 131, 97), (64, 64))      # int(64 / 131) = 0 rows


def test_library_geometry_agrees_with_the_reference():
    from ffp_amd import _lib, build
    build.build(verbose=False)
    for (box, imgsz), want in YOLO_GEOMETRY.items():
        nw, nh, top, bottom, left, right = _lib.letterbox_geometry(box[3] - box[1], box[2] - box[0], imgsz)
        assert (nh + top + bottom, nw + left + right, nh, nw, top, bottom, left, right) == want, (box, imgsz)
    import ctypes as C
    for (box, size), (want, scale) in SCRFD_GEOMETRY.items():
        out, s = np.zeros(2, np.int32), C.c_float(0)
        assert _lib.lib().ffp_scrfd_geometry(box[3] - box[1], box[2] - box[0], size[0], size[1], _lib._ip(out), C.byref(s)) == 0
        assert (int(out[1]), int(out[0])) == want[2:4] and np.float32(s.value) == np.float32(scale), (box, size)


def test_pad_areas_and_values():
    assert R.pad_value(R.YOLO) == np.float32(114) / np.float32(255) and R.pad_value(R.SCRFD) == np.float32(-127.5 / 128)
    for (kind, box, size), n_pad in {(R.YOLO, (0, 0, 131, 97), 64): 17 * 64, (R.YOLO, (5, 0, 6, 97), 64): 31 * 64, (R.RTDETR, (0, 0, 131, 97), 64): 0,
                                     (R.SCRFD, (0, 0, 131, 97), (96, 64)): 10 * 64}.items():
        m = R.pad_mask(kind, box, size)
        assert int(m.sum()) == n_pad
        rec = R.records(kind, FRAME, box, size, False)
        assert np.all(rec[m][:, :3] == R.pad_value(kind)) and np.all(rec[..., 3:] == 0)
    m = R.pad_mask(R.YOLO, (0, 0, 131, 97), 64)
    assert m[:8].all() and not m[8:55].any() and m[55:].all()      # 8 rows above, 9 below


def test_hand_checked_pixels():
    """An exact 2x down-scale weighs its four sources 1024 / 2048 each: a 0 / 255 checkerboard becomes ((255 + 255 + 2) >> 2) = 128 everywhere; an
    unresized box is the crop itself; the flip is a channel reversal and nothing else."""
    u = R.network_u8(R.YOLO, CHECKER, (0, 0, 128, 96), 64)
    assert u.shape == (64, 64, 3) and np.all(u[8:56] == 128) and np.all(u[:8] == 114) and np.all(u[56:] == 114)
    assert np.array_equal(R.network_u8(R.YOLO, FRAME, (67, 33, 131, 97), 64), FRAME[33:97, 67:131])
    assert np.array_equal(R.network_u8(R.SCRFD, FRAME, (3, 1, 67, 65), (96, 64))[:, :64], FRAME[1:65, 3:67])
    assert np.array_equal(R.network_u8(R.RTDETR, FRAME, (34, 17, 98, 81), 64), FRAME[17:81, 34:98])
    a, b = R.records(R.YOLO, FRAME, (0, 0, 131, 97), 64, False), R.records(R.YOLO, FRAME, (0, 0, 131, 97), 64, True)
    assert np.array_equal(a[..., :3], b[..., 2::-1]) and a.shape == (64, 64, 4)
    h = R.records(R.YOLO, FRAME, (0, 0, 131, 97), 64, False, half=True)
    assert h.shape == (64, 64, 8) and np.array_equal(h[..., :3], a[..., :3].astype(np.float16).astype(np.float32)) and np.all(h[..., 3:] == 0)


@pytest.mark.parametrize("box", [(0, 0, 131, 97), (10, 20, 40, 40), (3, 1, 67, 65), (5, 0, 6, 97), (0, 17, 131, 81)])
def test_compositions_equal_the_oracles_end_to_end(box):
    src = R.crop(FRAME, box)
    want = ultra_post.preprocess(src, 64)[0].permute(1, 2, 0).numpy()
    assert np.array_equal(R.records(R.YOLO, FRAME, box, 64, True)[..., :3], want)
    want = rtdetr_ref.preprocess(src, 64)[0].permute(1, 2, 0).numpy()
    assert np.array_equal(R.records(R.RTDETR, FRAME, box, 64, True)[..., :3], want)
    if box != (5, 0, 6, 97):      # one column of 97 rows resizes to no column at all
        for flip in (False, True):
            blob, scale = scrfd_ref.blob(src, 96, 64, flip)
            assert np.array_equal(R.records(R.SCRFD, FRAME, box, (96, 64), flip)[..., :3], blob[0].transpose(1, 2, 0))
            assert np.float32(scale) == R.scrfd_scale(box, (96, 64))


def _taps(s, c0, c1, n_src):
    """What a destination index reads: the clamped source index of each of its two weights, the index ignored where the weight is zero."""
    a, b = np.clip(s, 0, n_src - 1), np.clip(s + 1, 0, n_src - 1)
    return np.stack([np.where(c0 == 0, -1, a), c0, np.where(c1 == 0, -1, b), c1])


def test_scale_forms_give_the_same_taps():
    """cv2 forms the scale of an axis as 1. / ((double)dst / src) (the oracle's form); lin_coef (csrc/letterbox.hpp) takes (double)src / dst. The two
    doubles differ in the last bit for about a sixth of these pairs. Every long side 1..4096 resized to 256, 512, 640 and 1024, both axis rules:
    each destination index gets the same source index and the same 11-bit weight for both of its taps (an index compared only where its weight is
    not zero) — more than the identity of the effective taps, which merges two weights on one clamped index. So the kernels keep their form."""
    differ = 0
    for dst in (256, 512, 640, 1024):
        for src in range(1, 4097):
            kernel, cv2 = src / dst, 1.0 / (dst / src)
            if kernel == cv2:
                continue
            differ += 1
            for border in (True, False):
                a, b = _taps(*ultra_post.linear_axis(dst, src, kernel, border), src), _taps(*ultra_post.linear_axis(dst, src, cv2, border), src)
                assert np.array_equal(a, b), (src, dst, border, np.nonzero((a != b).any(0))[0][:4])
    assert differ > 2000      # the sweep did compare something

"""utils.visualization.build_overlay_prims against its oracle: for every case, the two primitive kinds of include/ffp.h restated in numpy
(overlay_ref.apply) and painted from the builder's list leave EXACTLY the pixels `_render` — the Pillow drawing the shim has always done —
leaves on the same image. No device: what the kernel does with such a list is tests/test_gpu_overlay.py's business."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

import ffp_amd  # noqa: F401
from ffp_amd import _lib
from ffp_amd.compat.utils import visualization as V

import overlay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(show_confidence=True, show_keypoints=True, box_color=(0, 255, 0), text_color=(0, 0, 0), kpt_conf_threshold=0.3, draw_skeleton=False)


def det(box, score=0.87, kpts=None):
    d = SimpleNamespace(bbox=SimpleNamespace(to_xyxy=lambda: list(box)), score=SimpleNamespace(value=score))
    if kpts is not None:
        d.keypoints = kpts
    return d


def result(*dets):
    return SimpleNamespace(object_prediction_list=list(dets))


def face_kpts(x, y, s=10.0, conf=(0.9, 0.9, 0.9, 0.9, 0.9)):
    pts = [(x - s, y - s), (x + s, y - s), (x, y), (x - 0.7 * s, y + s), (x + 0.7 * s, y + s)]
    return [[px, py, c] for (px, py), c in zip(pts, conf)]


def noise(h, w, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def check(img, res, **kw):
    """the builder's list under overlay_ref == _render, on the BGR image `img`"""
    o = dict(OPTS, **kw)
    pil = Image.fromarray(np.ascontiguousarray(img[..., ::-1]))
    found = V._render(pil, res, o["show_confidence"], o["show_keypoints"], o["box_color"], o["text_color"], o["kpt_conf_threshold"], o["draw_skeleton"], False)
    want = np.asarray(pil)[..., ::-1]
    prims, masks, found2 = V.build_overlay_prims(res, img.shape[1], img.shape[0], **o)
    assert prims.dtype == _lib.OVERLAY_PRIM_DTYPE and masks.dtype == np.uint8
    got = overlay_ref.apply(img, prims, masks)
    assert found2 == found
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    return prims, masks, want


def test_the_ctypes_mirror_has_the_size_the_header_states():
    hdr = open(os.path.join(ROOT, "include", "ffp.h")).read()
    stated = int(re.search(r"#define FFP_OVERLAY_PRIM_BYTES (\d+)", hdr).group(1))
    assert C.sizeof(_lib.OverlayPrim) == stated == _lib.OVERLAY_PRIM_BYTES == _lib.OVERLAY_PRIM_DTYPE.itemsize
    assert int(re.search(r"#define FFP_OVERLAY_MAX_PRIMS (\d+)", hdr).group(1)) == _lib.OVERLAY_MAX_PRIMS
    fields = re.search(r"typedef struct ffp_overlay_prim \{(.*?)\} ffp_overlay_prim;", hdr, re.S).group(1)
    names = [n for line in fields.splitlines() for n in re.findall(r"(\w+)(?:\[\d+\])?[,;]", line.split("/*")[0])]
    assert names == [f[0] for f in _lib.OverlayPrim._fields_]


def test_a_bad_list_is_refused_before_a_device_is_asked_for():
    """every check of ffp_overlay_draw comes before the device is chosen, so a machine without one refuses the same lists with FFP_ERR_ARG, and an empty
    list is FFP_OK there too"""
    img = noise(12, 16)
    keep = img.copy()
    rec = lambda *rows: np.array(list(rows), _lib.OVERLAY_PRIM_DTYPE)
    assert _lib.overlay_draw(img, rec()) is img and np.array_equal(img, keep)
    for prims, masks in ((rec((1, 0, 0, 4, 4, 4, 1, (1, 2, 3, 0))), np.zeros(16, np.uint8)), (rec((1, 0, 0, 4, 4, 3, 0, (1, 2, 3, 0))), np.zeros(16, np.uint8)),
                         (rec((1, 0, 0, 4, 4, 4, 0, (1, 2, 3, 0))), None), (rec((7, 0, 0, 4, 4, 0, 0, (1, 2, 3, 0))), None), (rec((0, 0, 0, 4, 4, -2, 0, (1, 2, 3, 0))), None),
                         (rec((1, 0, 0, -1, 4, 4, 0, (1, 2, 3, 0))), np.zeros(16, np.uint8))):
        with pytest.raises(_lib.FfpError) as e:
            _lib.overlay_draw(img, prims, masks)
        assert e.value.code == _lib.FFP_ERR_ARG and "primitive 0" in str(e.value)
        assert np.array_equal(img, keep)
    assert _lib.lib().ffp_overlay_draw_dev(0, None, 12, 16, 48, None, 0, None, 0) == _lib.FFP_ERR_ARG            # a null image
    assert _lib.lib().ffp_overlay_draw(0, img.ctypes.data, 12, 16, 48, None, 1, None, 0) == _lib.FFP_ERR_ARG      # a null list of one
    assert _lib.lib().ffp_overlay_draw(0, img.ctypes.data, 12, 16, 48, None, -1, None, 0) == _lib.FFP_ERR_ARG
    assert _lib.lib().ffp_overlay_draw(0, img.ctypes.data, 12, 16, 48, None, _lib.OVERLAY_MAX_PRIMS + 1, None, 0) == _lib.FFP_ERR_ARG
    assert np.array_equal(img, keep)


def test_ordinary_boxes_with_labels_and_landmarks():
    img = noise(240, 320)
    res = result(det((30, 60, 120, 170), 0.91, face_kpts(75, 110, 20)), det((180, 40, 250.9, 130.2), 0.5, face_kpts(215, 80, 14)), det((140, 150, 143, 153), 0.33))
    prims, masks, want = check(img, res)
    assert not np.array_equal(want, img) and len(prims) == 3 * 3 + 2 * 10
    assert masks.size < 4096                                   # one ring, one disc and one mask per distinct label


def test_skeleton_lines_are_rasterised_where_they_lie():
    img = noise(240, 320, 2)
    res = result(det((30, 60, 120, 170), 0.91, face_kpts(75, 110, 20)), det((11, 41, 101, 151), 0.91, face_kpts(56, 91, 20)), det((200, 30, 300, 230), 0.7, face_kpts(250.5, 130.5, 37.3)))
    check(img, res, draw_skeleton=True)
    check(img, result(det((100, 100, 140, 140), 0.6, [[120, 120, 1], [120, 120, 1], [139, 264, 1], [-30, 80, 1], [400, 90, 1]])), draw_skeleton=True)


@pytest.mark.parametrize("bw", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("bh", [1, 2, 3, 4, 5])
def test_boxes_a_few_pixels_wide_or_high(bw, bh):
    img = noise(60, 80, 3)
    check(img, result(det((20, 30, 20 + bw - 1, 30 + bh - 1), 0.4), det((0, 0, bw - 1, bh - 1), 0.4), det((80 - bw, 60 - bh, 79, 59), 0.4)), show_confidence=False)
    check(img, result(det((40, 30, 40 + bw - 1, 30 + bh - 1), 0.4)))


def test_a_box_at_the_origin_has_its_label_above_the_frame():
    check(noise(90, 120, 4), result(det((0, 0, 50, 40), 0.66), det((-20, -30, 30, 8), 0.99), det((100, 3, 119, 30), 0.12)))


def test_boxes_reaching_past_the_right_and_bottom_edges():
    check(noise(90, 120, 5), result(det((90, 60, 140, 110), 0.8), det((-15, 70, 20, 89), 0.8), det((60, 85, 100, 200), 0.8), det((300, 300, 340, 340), 0.8),
                                    det((119, 89, 125, 95), 0.8), det((-50, -50, 200, 200), 0.8)))


def test_landmarks_at_the_corners_and_outside():
    pts = [[0, 0, 1], [119, 0, 1], [0, 89, 1], [119, 89, 1], [60, 45, 1], [-2, 30, 1], [121, 30, 1], [50, -3, 1], [50, 92, 1], [-40, -40, 1], [1, 1, 1], [118, 88, 1]]
    check(noise(90, 120, 6), result(det((10, 20, 100, 80), 0.5, pts)))
    check(noise(90, 120, 6), result(det((10, 20, 100, 80), 0.5, pts[:5])), draw_skeleton=True)


def test_keypoint_confidences_on_both_sides_of_the_threshold():
    k = face_kpts(60, 50, 15, conf=(0.31, 0.9, 0.29, 0.3, 0.0))      # 0.3 itself is not above the threshold
    img = noise(100, 120, 7)
    p_on, _, _ = check(img, result(det((20, 10, 100, 90), 0.5, k)), draw_skeleton=True)
    assert len(p_on) == 3 + 1 + 2 * 2                          # box, label, text; the eye-to-eye line; two landmarks
    p_all, _, _ = check(img, result(det((20, 10, 100, 90), 0.5, k)), draw_skeleton=True, kpt_conf_threshold=-1.0)
    assert len(p_all) == 3 + 6 + 5 * 2
    check(img, result(det((20, 10, 100, 90), 0.5, [])))
    check(img, result(det((20, 10, 100, 90), 0.5, None)))


def test_two_overlapping_detections_where_order_decides():
    img = noise(120, 160, 8)
    a, b = det((20, 40, 90, 100), 0.9, face_kpts(55, 70, 12)), det((22, 24, 92, 84), 0.8, face_kpts(57, 54, 12))
    _, _, ab = check(img, result(a, b), draw_skeleton=True)
    _, _, ba = check(img, result(b, a), draw_skeleton=True)
    assert not np.array_equal(ab, ba)


def test_labels_and_keypoints_switched_off_and_other_colours():
    img = noise(120, 160, 9)
    res = result(det((20, 40, 90, 100), 0.9, face_kpts(55, 70, 12)))
    p, _, _ = check(img, res, show_confidence=False)
    assert len(p) == 1 + 10
    p, _, _ = check(img, res, show_keypoints=False)
    assert len(p) == 3
    check(img, res, box_color=(255, 10, 20), text_color=(255, 255, 255))


def test_an_empty_result_gives_an_empty_list():
    prims, masks, _ = check(noise(40, 50, 10), result())
    assert len(prims) == 0 and masks.size == 0


def test_three_hundred_random_detections_on_noise():
    rng = np.random.default_rng(11)
    dets = []
    for _ in range(300):
        x, y = rng.uniform(-20, 320), rng.uniform(-20, 200)
        w, h = rng.uniform(0, 70), rng.uniform(0, 70)
        k = None
        if rng.random() < 0.8:
            k = [[x + rng.uniform(-5, w + 5), y + rng.uniform(-5, h + 5), rng.random()] for _ in range(5)]
        dets.append(det((x, y, x + w, y + h), float(rng.random()), k))
    prims, masks, _ = check(noise(200, 320, 12), result(*dets), draw_skeleton=True)
    assert len(prims) > 1500


def test_the_verbose_lines_are_the_ones_render_prints(capsys):
    res = result(det((20, 40, 90, 100), 0.9, face_kpts(55, 70, 12)), det((1, 2, 30, 40), 0.2))
    pil = Image.new("RGB", (160, 120))
    V._render(pil, res, True, True, (0, 255, 0), (0, 0, 0), 0.3, False, True)
    printed = capsys.readouterr().out.splitlines()
    log = []
    V.build_overlay_prims(res, 160, 120, log=log)
    assert log == printed and len(log) == 2

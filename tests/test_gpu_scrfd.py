"""GPU parity of the SCRFD face detector (C-ABI ffp_scrfd_*) against the tests-side reference (tests/scrfd_ref.py) on a synthetic
SCRFD-10G-KPS-shaped graph: raw outputs, detections, bit-exact post-processing, batch independence and graph replay."""
import numpy as np
import pytest

import scrfd_ref
from util import iou_xyxy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from ffp_amd import synth
    return synth.scrfd_onnx(0, style="unfolded")


@pytest.fixture(scope="module", params=["f32", "f32x3"])
def det(request, gpu_lib, model):
    prec = gpu_lib.PREC_F32 if request.param == "f32" else gpu_lib.PREC_F32X3
    return gpu_lib.FaceDetector(model[0], precision=prec)


@pytest.fixture(scope="module")
def frame():
    from ffp_amd import synth
    return synth.synthetic_frame(720, 1280, seed=11)


def _real():
    import os
    from PIL import Image
    p = os.path.join(os.path.dirname(__file__), "golden", "real", "det_family.png")
    return np.asarray(Image.open(p).convert("RGB"))


TILES = [[0, 0, 512, 512], [400, 100, 912, 612], [0, 0, 1280, 720], [700, 300, 1000, 700]]


@pytest.mark.parametrize("size", [(640, 640), (512, 384)])
def test_forward_raw_matches_interpreter(det, model, frame, size):
    g = model[1]
    got = det.forward_raw(frame, TILES[:2], size)
    for t, outs in zip(TILES[:2], got):
        x0, y0, x1, y1 = t
        x, _ = scrfd_ref.blob(frame[y0:y1, x0:x1], size[0], size[1])
        ref = scrfd_ref.run_graph(g, x)
        for k in range(9):
            tol = 2e-4 if k < 3 else 2e-2
            np.testing.assert_allclose(outs[k].ravel(), ref[k].ravel(), atol=tol, err_msg=f"output {k}")


def _check_dets(det, ref_det, thr=0.5):
    """The issue's bar: counts equal except for candidates within 1e-4 of the threshold; every other reference box has a partner with
    IoU >= 0.999 and a score within 2e-4; >= 97 % agree on the exact integer box after truncation."""
    near = int(np.sum(np.abs(ref_det[:, 4] - thr) < 1e-4))
    assert abs(len(det) - len(ref_det)) <= near, (len(det), len(ref_det), near)
    exact = n_cmp = 0
    for r in ref_det:
        if abs(r[4] - thr) < 1e-4:
            continue
        n_cmp += 1
        assert len(det)
        assert r[2] - r[0] > 1 and r[3] - r[1] > 1, r                  # the calibrated head gives positive, non-degenerate boxes
        j = int(np.argmin(np.abs(det[:, :4] - r[:4]).max(axis=1)))
        iou = iou_xyxy(r[None, :4], det[j:j + 1, :4])[0]
        assert iou >= 0.999, (iou, r, det[j])
        assert abs(det[j, 4] - r[4]) <= 2e-4, (det[j, 4], r[4])
        exact += int(np.array_equal(det[j, :4].astype(int), r[:4].astype(int)))
    assert exact >= 0.97 * max(n_cmp, 1), (exact, n_cmp)


@pytest.mark.parametrize("size", [(640, 640), (512, 384)])
@pytest.mark.parametrize("src", ["synthetic", "real"])
def test_infer_tiles_matches_reference(det, model, frame, size, src):
    img = frame if src == "synthetic" else _real()
    H, W = img.shape[:2]
    tiles = [[0, 0, min(512, W), min(512, H)], [0, 0, W, H]]
    got = det.infer_tiles(img, tiles, size, 0.5, 0.4)
    suppressed = 0
    for t, d in zip(tiles, got):
        x0, y0, x1, y1 = t
        (rdet, rkps), outs = scrfd_ref.detect(model[1], img[y0:y1, x0:x1], size[0], size[1])
        assert len(rdet) >= 5, len(rdet)
        n_pos = sum(int(np.sum(outs[k] >= np.float32(0.5))) for k in range(3))
        suppressed += n_pos - len(rdet)
        _check_dets(d, rdet)
    assert suppressed > 0


def test_postprocess_bit_exact(det, frame):
    tiles = TILES
    raw = det.forward_raw(frame, tiles, (640, 640))
    got = det.infer_tiles(frame, tiles, (640, 640), 0.5, 0.4)
    for t, outs, d in zip(tiles, raw, got):
        x0, y0, x1, y1 = t
        _, _, ds = scrfd_ref.geometry(y1 - y0, x1 - x0, 640, 640)
        rdet, rkps = scrfd_ref.post(outs, ds, 640, 640, 0.5, 0.4)
        assert len(rdet) > 0
        np.testing.assert_array_equal(d[:, :5], rdet)
        np.testing.assert_array_equal(d[:, 6:].reshape(-1, 5, 3)[:, :, :2], rkps)


@pytest.mark.parametrize("prec", ["f32", "f32x3"])
def test_batch_independence_and_replay(gpu_lib, model, frame, prec):
    d = gpu_lib.FaceDetector(model[0], precision=gpu_lib.PREC_F32 if prec == "f32" else gpu_lib.PREC_F32X3)
    from ffp_amd._lib import slice_bboxes
    tiles = [list(map(int, t)) for t in slice_bboxes(frame.shape[0], frame.shape[1], 512, 512, 0.2, 0.2)]
    tiles = (tiles * 61)[:60] + [[0, 0, frame.shape[1], frame.shape[0]]]
    alone = d.infer_tiles(frame, [tiles[3]], (640, 640))[0]
    first = d.infer_tiles(frame, tiles, (640, 640))
    second = d.infer_tiles(frame, tiles, (640, 640))
    assert len(alone) > 0
    np.testing.assert_array_equal(alone, first[3])
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)


def test_zero_width_tile_refused(det, frame):
    with pytest.raises(RuntimeError, match="resizes to 0x640"):
        det.infer_tiles(frame, [[0, 0, 1, 720]], (640, 640))

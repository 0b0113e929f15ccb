"""GPU parity of YOLO11m-pose and YOLO11l-pose (C-ABI ffp_det_*) against the tests-side CPU reference of the larger scales
(tests/yolo11_scales_ref.py), at the bars of test_gpu_detector.py, plus the 64-channel stem path, graph replay / lanes,
full-size composition and the compat loader on an m checkpoint file."""
import os
import sys

import numpy as np
import pytest

from util import match_by_iou
from yolo11_scales_ref import Yolo11ScalesRef

pytestmark = pytest.mark.gpu

TILES = [(0, 0, 384, 384), (100, 50, 484, 434), (0, 0, 640, 480), (20, 30, 320, 230), (256, 96, 640, 480)]
IMGSZ = 384


@pytest.fixture(scope="module", params=["m-f32", "l-f32", "m-f32x3", "l-f32x3"])
def models(request, gpu_lib):
    from ffp_amd import synth
    sc, mode = request.param.split("-")
    W = synth.yolo11_pose_weights(sc)
    prec = gpu_lib.PREC_F32 if mode == "f32" else gpu_lib.PREC_F32X3
    return sc, Yolo11ScalesRef(W, sc), gpu_lib.Detector(W, arch=sc, precision=prec), W


@pytest.fixture(scope="module")
def frame():
    from ffp_amd import synth
    return synth.synthetic_frame(480, 640, seed=7)


def _ref_raw(ref, crop, imgsz=IMGSZ):
    from oracle import ultra_post
    return ref.forward(ultra_post.preprocess(np.ascontiguousarray(crop), imgsz))[0].numpy()


def test_forward_raw_matches_reference(models, frame):
    sc, ref, det, _ = models
    outs = det.forward_raw(frame, TILES, IMGSZ)
    for t, o in zip(TILES, outs):
        r = _ref_raw(ref, frame[t[1]:t[3], t[0]:t[2]])
        assert o.shape == r.shape, (t, o.shape, r.shape)
        np.testing.assert_allclose(o[4], r[4], atol=2e-4, rtol=0)            # class sigmoid
        np.testing.assert_allclose(o[:4], r[:4], atol=2e-2, rtol=0)          # cx,cy,w,h in net pixels
        np.testing.assert_allclose(o[5:], r[5:], atol=2e-2, rtol=1e-4)       # keypoints


@pytest.mark.parametrize("conf", [0.5, 0.05])
def test_infer_tiles_matches_reference(models, frame, conf):
    from oracle import ultra_post
    sc, ref, det, _ = models
    res = det.infer_tiles(frame, TILES, IMGSZ, conf, 0.7, 300)
    total, same_total = 0, 0
    for t, d in zip(TILES, res):
        r = ultra_post.predict(ref, frame[t[1]:t[3], t[0]:t[2]], IMGSZ, conf, 0.7, 300)
        assert d.shape[0] == len(r), (t, d.shape[0], len(r))
        if len(r) == 0:
            continue
        total += len(r)
        m = match_by_iou(r.xyxy, d[:, :4])
        ious = np.array([x[2] for x in m])
        assert ious.min() >= 0.999, (t, ious.min())
        j = np.array([x[1] for x in m])
        np.testing.assert_allclose(d[j, 4], r.conf, atol=2e-4)
        assert np.array_equal(d[j, 5].astype(int), r.cls.astype(int))
        np.testing.assert_allclose(d[j, 6:].reshape(-1, 5, 3), r.kpts, atol=5e-2, rtol=1e-4)
        same_total += int((d[j, :4].astype(int) == r.xyxy.astype(int)).all(1).sum())
    assert total > 0
    assert same_total >= 0.97 * total, (same_total, total)


def test_fp16_mode_close(models, frame, gpu_lib):
    from util import iou_xyxy
    sc, ref, _, W = models
    det16 = gpu_lib.Detector(W, arch=sc, precision=gpu_lib.PREC_F16)
    outs = det16.forward_raw(frame, TILES[:2], IMGSZ)
    for t, o in zip(TILES[:2], outs):
        r = _ref_raw(ref, frame[t[1]:t[3], t[0]:t[2]])
        np.testing.assert_allclose(o[4], r[4], atol=3e-2)
        hot = r[4] > 0.25
        if hot.any():
            a = np.stack([r[0] - r[2] / 2, r[1] - r[3] / 2, r[0] + r[2] / 2, r[1] + r[3] / 2], 1)[hot]
            b = np.stack([o[0] - o[2] / 2, o[1] - o[3] / 2, o[0] + o[2] / 2, o[1] + o[3] / 2], 1)[hot]
            assert np.median(iou_xyxy(a, b)) >= 0.97


@pytest.mark.parametrize("arch", ["m", "l"])
@pytest.mark.parametrize("order", [0, 1], ids=["as_bgr", "as_rgb"])
def test_64_channel_stem_two_kernel_path(gpu_lib, order, arch):
    """m and l run their 64-channel model.0 straight from the frame (fused with the letterbox) and model.1 as an MFMA conv of its own:
    the stem-fused loader of n/s is not used for them (a four-chunk form measured no faster, profiles/r05_stem_ab_yolo11m.txt). The
    profile names a stand-alone model.1.conv; native-size, interior, down-scaled (letterbox padding), up-scaled and odd-offset slices
    meet the usual bars in both channel orders."""
    from ffp_amd import synth
    W = synth.yolo11_pose_weights(arch)
    ref = Yolo11ScalesRef(W, arch)
    det = gpu_lib.Detector(W, arch=arch, precision=gpu_lib.PREC_F32X3)
    frame = synth.synthetic_frame(301, 421, seed=33)              # 301 x 421 x 3 bytes is not a whole number of dwords
    tiles = [(0, 0, 256, 256), (165, 45, 421, 301), (0, 0, 421, 301), (30, 40, 190, 140), (5, 7, 261, 263)]
    det.set_profile(True)
    outs = det.forward_raw(frame, tiles, 256, chan_order=order)
    names = [e["name"] for e in det.profile_detail()]
    det.set_profile(False)
    assert not any("stem_fused" in n for n in names), names[:4]
    assert any(n.endswith(" model.1.conv") for n in names)
    for t, o in zip(tiles, outs):
        crop = frame[t[1]:t[3], t[0]:t[2]]
        if order == gpu_lib.CHAN_AS_RGB:
            crop = crop[..., ::-1]
        r = _ref_raw(ref, crop, 256)
        np.testing.assert_allclose(o[4], r[4], atol=2e-4, rtol=0)
        np.testing.assert_allclose(o[:4], r[:4], atol=2e-2, rtol=0)
        np.testing.assert_allclose(o[5:], r[5:], atol=2e-2, rtol=1e-4)


@pytest.mark.parametrize("arch", ["m", "l"])
def test_512_slice_at_imgsz_1024(gpu_lib, arch):
    from ffp_amd import synth
    W = synth.yolo11_pose_weights(arch)
    ref = Yolo11ScalesRef(W, arch)
    frame = synth.synthetic_frame(600, 700, seed=12)
    t = (100, 40, 612, 552)
    for prec in (gpu_lib.PREC_F32X3, gpu_lib.PREC_F32):
        o = gpu_lib.Detector(W, arch=arch, precision=prec).forward_raw(frame, [t], 1024)[0]
        r = _ref_raw(ref, frame[t[1]:t[3], t[0]:t[2]], 1024)
        assert o.shape == r.shape
        np.testing.assert_allclose(o[4], r[4], atol=2e-4, rtol=0)
        np.testing.assert_allclose(o[:4], r[:4], atol=2e-2, rtol=0)
        np.testing.assert_allclose(o[5:], r[5:], atol=2e-2, rtol=1e-4)


@pytest.mark.parametrize("arch", ["m", "l"])
def test_graph_replay_and_lanes_change_nothing(gpu_lib, arch):
    """Graph replays and ffp_det_set_lanes(1) (C3k side lanes forked and joined once per C3k, two C3k back to back in l) give the
    eager run's bits."""
    from ffp_amd import synth
    W = synth.yolo11_pose_weights(arch)
    frame = synth.synthetic_frame(300, 420, seed=41)
    tiles = [(0, 0, 256, 256), (164, 44, 420, 300), (0, 0, 420, 300)]
    det = gpu_lib.Detector(W, arch=arch, precision=gpu_lib.PREC_F32X3)
    base = det.forward_raw(frame, tiles, 256)
    for it in range(3):
        outs = det.forward_raw(frame, tiles, 256)
        for a, b in zip(base, outs):
            assert np.array_equal(a, b), it
    det.set_lanes(1)
    for it in range(4):
        outs = det.forward_raw(frame, tiles, 256)
        for a, b in zip(base, outs):
            assert np.array_equal(a, b), it
    assert det.graph_status() == 1
    det.set_lanes(0)
    outs = det.forward_raw(frame, tiles, 256)
    for a, b in zip(base, outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("arch", ["m", "l"])
def test_4k_fused_equals_tilewise_and_sharded(gpu_lib, arch):
    from ffp_amd import synth
    H, Wf = 2160, 3840
    W = synth.yolo11_pose_weights(arch)
    frame = synth.synthetic_frame(H, Wf, seed=0)
    sl = gpu_lib.slice_bboxes(H, Wf, 512, 512, 0.2, 0.2)
    tiles = [tuple(t) for t in sl] + [(0, 0, Wf, H)]
    half = len(tiles) // 2
    for prec in (gpu_lib.PREC_F32, gpu_lib.PREC_F32X3):
        det = gpu_lib.Detector(W, arch=arch, precision=prec)
        per = det.infer_tiles(frame, tiles, 512, 0.25, 0.7, 300)
        sharded = det.infer_tiles(frame, tiles[:half], 512, 0.25, 0.7, 300) + det.infer_tiles(frame, tiles[half:], 512, 0.25, 0.7, 300)
        assert sum(x.shape[0] for x in per) > 0
        for k, (x, y) in enumerate(zip(per, sharded)):
            assert np.array_equal(x, y), k
        for k in (0, 31, 60):
            assert np.array_equal(det.infer_tiles(frame, [tiles[k]], 512, 0.25, 0.7, 300)[0], per[k]), k
        fused = det.sliced_predict(frame, 512, 512, 0.2, 0.2, True, 512, 0.25, 0.7, 300, "GREEDYNMM", "IOS", 0.5, False)
        assert fused.shape[0] > 0 and np.array_equal(fused, det.sliced_predict(frame, 512, 512, 0.2, 0.2, True, 512, 0.25, 0.7, 300,
                                                                              "GREEDYNMM", "IOS", 0.5, False))


def test_compat_sliced_prediction_on_an_m_checkpoint_file(gpu_lib, tmp_path):
    """YOLOv11PoseDetectionModel(model_path=<yolo11m>.ffpw): the scale comes from the weights (arch.yolo11_scale_of), and SAHI's
    get_sliced_prediction through it matches the reference pipeline (oracle.sahi_ref over the tests-side m reference)."""
    from ffp_amd import synth, weights_io
    from oracle import sahi_ref, ultra_post
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-detection-with-yolov11-sahi-and-real-esrgan_amd", "compat"))
    from sahi.predict import get_sliced_prediction
    from utils.yolo_wrapper import YOLOv11PoseDetectionModel
    W = synth.yolo11_pose_weights("m")
    p = tmp_path / "yolo11m-pose-face.ffpw"
    weights_io.save(str(p), W)
    model = YOLOv11PoseDetectionModel(model_path=str(p), confidence_threshold=0.5, device="cuda:0", image_size=256, load_at_init=True)
    assert model.model.arch == "m"
    frame = synth.synthetic_frame(420, 560, seed=9)
    res = get_sliced_prediction(frame, model, slice_height=256, slice_width=256, overlap_height_ratio=0.2, overlap_width_ratio=0.2, verbose=0)
    ref = Yolo11ScalesRef(W, "m")
    exp = sahi_ref.get_sliced_prediction(frame, lambda im: ultra_post.predict(ref, im, 256, 0.5, 0.7, 300), 256, 256, 0.2, 0.2)
    got = np.asarray([q.bbox.to_xyxy() for q in res.object_prediction_list], np.float32).reshape(-1, 4)
    eb = np.asarray([d.bbox for d in exp], np.float32).reshape(-1, 4)
    assert abs(len(got) - len(eb)) <= 1 and len(eb) > 0
    assert np.mean([np.array_equal(eb[i], got[j]) for i, j, _ in match_by_iou(eb, got)]) >= 0.95


def test_arch_x_is_refused_without_fault(gpu_lib):
    """YOLO11x is in the structure table but not built: creating a detector for it fails with an argument error naming the built scales,
    and the library keeps working afterwards."""
    from ffp_amd import synth
    from ffp_amd import arch as A
    Wx = {s.name + sfx: np.zeros(s.weight_shape if sfx == ".weight" else (s.c2,), np.float32)
          for s in A.yolo11_pose_convs("x") for sfx in (".weight", ".bias")}
    with pytest.raises(gpu_lib.FfpError, match="n, s, m and l"):
        gpu_lib.Detector(Wx, arch="x", precision=gpu_lib.PREC_F32X3)
    with pytest.raises(gpu_lib.FfpError):
        gpu_lib.Detector(synth.yolo11_pose_weights("m"), arch="x")
    det = gpu_lib.Detector(synth.yolo11_pose_weights("m"), arch="m")
    assert det.forward_raw(synth.synthetic_frame(64, 64, seed=1), [(0, 0, 64, 64)], 64)[0].shape[1] == (8 * 8 + 4 * 4 + 2 * 2)

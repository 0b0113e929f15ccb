"""The detector's two class-tower plans against each other: YOLO11s in FFP_PREC_F32X3 runs each head level's class tower as two launches
(csrc/conv_dwpw.hip); FFP_CLS_FUSE=0, read where a plan is built, keeps the five launches. Both detectors live in one process.

The towers differ only in the class logits (the fused one splits its depthwise outputs at a bound's exponent and closes with an fp32 dot
product), so box and keypoint values must be the same bytes, class scores agree to the project's class-score bar 2e-4, and, with conf kept
1e-3 away from every score, the same anchors pass and the same detections come out."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCORE_BAR = 2e-4
MARGIN = 1e-3
# net inputs 64 x 64 and 64 x 32 (imgsz 64) and 96 x 64 (imgsz 96): one-tile maps, a partial tile, maps of 8^2 .. 2 x 1
CALLS = [(64, [(0, 0, 64, 64), (100, 40, 164, 72)]), (96, [(30, 20, 126, 84)])]


@pytest.fixture(scope="module")
def pair(gpu_lib):
    from ffp_amd import synth
    W = synth.yolo11_pose_weights("s")
    frame = synth.synthetic_frame(160, 224, seed=11)
    dets = {}
    old = os.environ.get("FFP_CLS_FUSE")
    try:
        for name, env in (("five", "0"), ("fused", None)):
            if env is None:
                os.environ.pop("FFP_CLS_FUSE", None)
            else:
                os.environ["FFP_CLS_FUSE"] = env
            d = gpu_lib.Detector(W, arch="s", precision=gpu_lib.PREC_F32X3)
            d.set_gate(True)
            raws = [d.forward_raw(frame, tiles, imgsz) for imgsz, tiles in CALLS]      # builds the plans while the switch is as set
            d.set_profile(True)
            d.forward_raw(frame, CALLS[0][1], CALLS[0][0])
            steps = [x["name"] for x in d.profile_detail()]
            d.set_profile(False)
            dets[name] = {"det": d, "raw": raws, "steps": steps, "mem": d.mem_bytes()["plans"]}
    finally:
        if old is None:
            os.environ.pop("FFP_CLS_FUSE", None)
        else:
            os.environ["FFP_CLS_FUSE"] = old
    return frame, dets


def test_step_lists(pair):
    """The profile lists the conv launches ("<variant> <name>"); the depthwise launches of the five-op tower are not convs and are not listed:
    three conv rows per level there, two rows of the fused variant here."""
    _, dets = pair
    five = [s for s in dets["five"]["steps"] if "model.23.cv3." in s]
    fused = [s for s in dets["fused"]["steps"] if "model.23.cv3." in s]
    assert len(five) == 9 and not any("_dw3" in s for s in five), five
    assert sorted(s.split(" ", 1)[1] for s in five) == sorted(f"model.23.cv3.{l}.{t}" for l in range(3) for t in ("0.1.conv", "1.1.conv", "2"))
    assert len(fused) == 6 and all(s.startswith("f32x3_k1s1_dw3 ") for s in fused), fused
    assert sorted(s.split(" ", 1)[1] for s in fused) == sorted(f"model.23.cv3.{l}.{t}" for l in range(3) for t in ("0", "1+2"))
    rest = lambda steps: [s.split(" ", 1)[1] for s in steps if "model.23.cv3." not in s]      # layer names: the tuner may time two plans differently
    assert rest(dets["five"]["steps"]) == rest(dets["fused"]["steps"])


def _plan_bytes(gpu_lib, W, frame, fuse, reuse):
    old = os.environ.get("FFP_CLS_FUSE")
    try:
        if fuse:
            os.environ.pop("FFP_CLS_FUSE", None)
        else:
            os.environ["FFP_CLS_FUSE"] = "0"
        d = gpu_lib.Detector(W, arch="s", precision=gpu_lib.PREC_F32X3)
        d.set_buffer_reuse(reuse)
        d.forward_raw(frame, CALLS[0][1], CALLS[0][0])
        return d.mem_bytes()["plans"], d.mem_detail()
    finally:
        if old is None:
            os.environ.pop("FFP_CLS_FUSE", None)
        else:
            os.environ["FFP_CLS_FUSE"] = old


def test_plans_hold_less(gpu_lib, pair):
    """d1, d2 and e2 of every level are no longer allocated. With one allocation per tensor (buffer reuse 0) the plan's bytes drop by exactly
    those tensors. With storage shared by lifetime (the default) the tower's tensors already lived in bytes that the backbone's larger tensors
    had released, and the plan's peak lies in the backbone: there the plan holds the same bytes, not more (measured: 2480128 B both at these
    shapes, 14923533312 B both for the benchmark's two 5-frame plans), while the sum of the tensor sizes drops."""
    from ffp_amd import synth
    frame, dets = pair
    W = synth.yolo11_pose_weights("s")
    print(f"\nplans (shared storage): five-op {dets['five']['mem']} B, fused {dets['fused']['mem']} B")
    assert dets["fused"]["mem"] <= dets["five"]["mem"]
    five, five_d = _plan_bytes(gpu_lib, W, frame, False, 0)
    fused, fused_d = _plan_bytes(gpu_lib, W, frame, True, 0)
    print(f"plans (one allocation per tensor): five-op {five} B, fused {fused} B; sum of tensor sizes {five_d['no_reuse_bytes']} / {fused_d['no_reuse_bytes']}")
    assert fused < five
    assert fused_d["no_reuse_bytes"] < five_d["no_reuse_bytes"]


def test_raw_heads(pair):
    """forward_raw: (4 + nc + 3 * nkpt, anchors) per item, every item active. Rows 0-3 and 5.. come from the box and keypoint towers."""
    _, dets = pair
    worst = 0.0
    for a_call, b_call in zip(dets["five"]["raw"], dets["fused"]["raw"]):
        for a, b in zip(a_call, b_call):
            assert a.shape == b.shape
            assert np.array_equal(a[:4], b[:4]) and np.array_equal(a[5:], b[5:]), "box / keypoint values differ"
            worst = max(worst, float(np.abs(a[4].astype(np.float64) - b[4]).max()))
    print(f"\nlargest class-score difference between the plans: {worst:.3e}")
    assert worst <= SCORE_BAR


def test_detections(pair):
    frame, dets = pair
    for (imgsz, tiles), raw in zip(CALLS, dets["five"]["raw"]):
        scores = np.sort(np.concatenate([r[4] for r in raw]).astype(np.float64))
        # a conf no score of the five-op plan comes within MARGIN of: the middle of the widest gap that leaves anchors above it, or, where the
        # scores crowd together, a value below them all (every anchor a candidate)
        gaps = scores[1:] - scores[:-1]
        k = int(np.argmax(gaps))
        conf = float((scores[k] + scores[k + 1]) / 2) if gaps[k] > 2.5 * MARGIN else float(scores[0] - 2 * MARGIN)
        assert np.abs(scores - conf).min() > MARGIN
        assert (scores > conf).sum() >= 1
        want = dets["five"]["det"].infer_tiles(frame, tiles, imgsz, conf, 0.7, 300)
        for _ in range(2):                                       # eager, then the captured plan
            got = dets["fused"]["det"].infer_tiles(frame, tiles, imgsz, conf, 0.7, 300)
            assert dets["fused"]["det"].last_active() == dets["five"]["det"].last_active()
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.shape == w.shape, (g.shape, w.shape)
                if not len(w):
                    continue
                assert np.array_equal(g[:, 5], w[:, 5])
                assert np.abs(g[:, 4].astype(np.float64) - w[:, 4]).max() <= SCORE_BAR
                x1, y1 = np.maximum(g[:, 0], w[:, 0]), np.maximum(g[:, 1], w[:, 1])
                x2, y2 = np.minimum(g[:, 2], w[:, 2]), np.minimum(g[:, 3], w[:, 3])
                inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
                area = lambda r: (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
                iou = inter / np.maximum(area(g) + area(w) - inter, 1e-12)
                assert iou.min() >= 0.999, iou.min()

"""YOLO11 scales m and l on the CPU side: structure table (Ultralytics parse_model rules), scale detection of a weight dict, the
tests-side reference of the larger scales (tests/yolo11_scales_ref.py) and their synthetic weights. No GPU needed."""
import numpy as np
import pytest
import torch

from yolo11_scales_ref import Yolo11ScalesRef, conv_flops, forward_counting_reads


@pytest.mark.parametrize("scale,count", [("n", 2_624_080), ("s", 9_458_752), ("m", 20_114_688), ("l", 25_372_160), ("x", 56_966_176)])
def test_detect_head_param_counts_match_ultralytics(scale, count):
    """Ultralytics' yolo11.yaml summary lines (Detect head, nc=80): unfused parameters per scale."""
    from ffp_amd import arch
    assert arch.yolo11_unfused_param_count(scale, 80, None) == count


@pytest.mark.parametrize("scale,count", [("n", 2_662_416), ("s", 9_715_744), ("m", 20_905_344), ("l", 26_162_816)])
def test_pose_face_param_counts(scale, count):
    from ffp_amd import arch
    assert arch.yolo11_unfused_param_count(scale, 1, (5, 3)) == count


def test_structure_rules_of_m_and_l():
    """m: forced C3k, one repeat; l: forced C3k, two repeats chained (cv2 takes (2 + n) * c), two PSABlocks; P5 512 channels."""
    from ffp_amd import arch
    for sc, n in (("m", 1), ("l", 2)):
        S = {s.name: s for s in arch.yolo11_pose_convs(sc)}
        assert S["model.0.conv"].c2 == 64 and S["model.1.conv"].c2 == 128
        assert S["model.2.m.0.cv1.conv"].k == 1 and S["model.2.m.0.m.1.cv2.conv"].weight_shape == (32, 32, 3, 3)
        assert S["model.2.cv2.conv"].c1 == (2 + n) * 64
        assert ("model.2.m.1.m.0.cv1.conv" in S) == (n == 2) and ("model.10.m.1.attn.qkv.conv" in S) == (n == 2)
        assert S["model.10.m.0.attn.qkv.conv"].weight_shape == (512, 256, 1, 1)         # nh = 4, kd = 32, hd = 64 as for s
        assert S["model.23.cv2.0.0.conv"].c2 == 64 and S["model.23.cv3.0.0.1.conv"].c2 == 256 and S["model.23.cv4.0.0.conv"].c2 == 64
        assert max(s.c2 for s in S.values()) == 512 and S["model.22.cv2.conv"].c2 == 512         # max_channels 512
    names = {s.name for s in arch.yolo11_pose_convs("l")}
    for k in ("model.2.m.1.m.0.cv1.conv", "model.4.m.1.cv3.conv", "model.10.m.1.attn.qkv.conv", "model.10.m.1.ffn.1.conv"):
        assert k in names


def test_n_and_s_inventories_unchanged():
    """n/s keep their C3k2 layout (C3k only in model.6 / 8 / 22) and their tensor order — every synthetic n/s weight depends on it."""
    from ffp_amd import arch
    for sc in "ns":
        S = arch.yolo11_pose_convs(sc)
        assert len(S) == 96
        c3k = sorted({s.name.split(".")[1] for s in S if ".m.0.m.0." in s.name})
        assert c3k == ["22", "6", "8"]
        assert not any(".m.1." in s.name and not s.name.startswith(("model.6.m.0", "model.8.m.0", "model.22.m.0")) for s in S)


def _dict(scale, nc=1, kpt_shape=(5, 3)):
    from ffp_amd import arch
    return {s.name + sfx: np.zeros(s.weight_shape if sfx == ".weight" else (s.c2,), np.float32)
            for s in arch.yolo11_pose_convs(scale, nc, kpt_shape) for sfx in (".weight", ".bias")}


@pytest.mark.parametrize("scale", list("nsmlx"))
def test_scale_of_standard_dicts(scale):
    from ffp_amd import arch
    assert arch.yolo11_scale_of(_dict(scale)) == scale
    assert arch.yolo11_scale_of(_dict(scale, 80, None)) == scale             # plain Detect head
    assert arch.yolo11_scale_of(_dict(scale, 2, (17, 3))) == scale           # other classes / keypoints


def test_scale_of_rejects_renamed_and_reshaped_tensors():
    from ffp_amd import arch
    W = _dict("m")
    W["model.4.m.0.cv3.convX.weight"] = W.pop("model.4.m.0.cv3.conv.weight")
    with pytest.raises(ValueError, match=r"model\.4\.m\.0\.cv3\.conv\.weight"):
        arch.yolo11_scale_of(W)
    W = _dict("l")
    W["model.13.m.1.cv2.conv.weight"] = np.zeros((128, 64, 3, 3), np.float32)
    with pytest.raises(ValueError, match=r"model\.13\.m\.1\.cv2\.conv\.weight"):
        arch.yolo11_scale_of(W)
    W = _dict("s")                                                            # an extra P2 level, as in a custom "p2p3p4" head
    W["model.23.cv2.3.0.conv.weight"] = np.zeros((64, 64, 3, 3), np.float32)
    with pytest.raises(ValueError, match=r"model\.23\.cv2\.3\.0\.conv\.weight"):
        arch.yolo11_scale_of(W)
    W = _dict("n")
    W["model.0.conv.weight"] = np.zeros((24, 3, 3, 3), np.float32)
    with pytest.raises(ValueError, match="model.0.conv"):
        arch.yolo11_scale_of(W)


@pytest.mark.parametrize("scale", ["n", "s"])
def test_scales_reference_is_the_oracle_on_n_and_s(scale):
    from ffp_amd import synth
    from oracle import ultra_post
    from oracle.yolo11_ref import Yolo11PoseRef
    from oracle import yolo11_ref
    W = synth.yolo11_pose_weights(scale)
    x = ultra_post.preprocess(synth.synthetic_frame(200, 300, seed=4), 256)
    assert torch.equal(Yolo11ScalesRef(W, scale).forward(x), Yolo11PoseRef(W, scale).forward(x))
    assert conv_flops(W, scale, 256, 256) == yolo11_ref.conv_flops(W, scale, 256, 256)


@pytest.mark.parametrize("scale", ["m", "l"])
def test_every_weight_tensor_read_exactly_once(scale):
    from ffp_amd import synth
    W = synth.yolo11_pose_weights(scale)
    reads = forward_counting_reads(W, scale)
    assert set(reads) == set(W)
    assert set(reads.values()) == {1}


@pytest.mark.parametrize("scale", ["m", "l"])
def test_synthetic_weights_detect_something(scale):
    """The m/l calibration (tests/golden/make_synth_calibration_scales.py) keeps the head's scores in the n/s regime: a non-empty
    detection set at conf 0.5 on the frame the GPU parity tests use, and no saturated scores."""
    from ffp_amd import arch, synth
    from oracle import ultra_post
    W = synth.yolo11_pose_weights(scale)
    assert arch.yolo11_scale_of(W) == scale
    ref = Yolo11ScalesRef(W, scale)
    frame = synth.synthetic_frame(480, 640, seed=7)
    r = ref.forward(ultra_post.preprocess(frame[50:434, 100:484], 384))[0]
    frac = float((r[4] > 0.5).float().mean())
    assert 0.0 < frac < 0.2, frac
    assert len(ultra_post.predict(ref, frame[50:434, 100:484], 384, 0.5, 0.7, 300)) > 0


def test_calibration_keeps_existing_keys():
    """synth_calib.json gained the m/l entries; the n/s/ESRGAN entries are the ones every existing golden was made from."""
    import json
    import os
    import ffp_amd
    with open(os.path.join(os.path.dirname(ffp_amd.__file__), "synth_calib.json")) as f:
        cal = json.load(f)
    assert list(cal) == ["yolo11n-pose", "yolo11s-pose", "rrdbnet_x4", "rrdbnet_x2", "yolo11m-pose", "yolo11l-pose"]
    from ffp_amd import arch
    for sc in "ml":
        assert set(cal[f"yolo11{sc}-pose"]) == {s.name for s in arch.yolo11_pose_convs(sc)}

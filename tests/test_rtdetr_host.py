"""CPU tests of RT-DETR-l support: the checkpoint converter (BatchNorm fold, RepConv fold, in_proj split) against the tests-side
reference on the unfused tensors, the constant tables (position embedding, anchors, valid mask), the stretch resize, the synthetic
weights' detection count and the compat loader's refusal of pickled checkpoints."""
import numpy as np
import pytest
import torch

import rtdetr_ref as R


@pytest.fixture(scope="module")
def sd():
    from ffp_amd import synth
    return synth.rtdetr_l_state_dict(1, seed=0)


def test_converter_folds_match_unfused_fp64(sd):
    from ffp_amd import synth, weights_io
    conv = weights_io.from_ultralytics_rtdetr_state_dict(sd, dtype=np.float64)
    assert not any(".bn." in k or "in_proj" in k or "denoising_class_embed" in k or k.startswith("model.16.m.0.conv1") for k in conv)
    assert conv["model.16.m.0.conv.weight"].shape == (256, 256, 3, 3)
    assert conv["model.11.ma.q_proj.weight"].shape == (256, 256)
    assert "model.28.input_proj.0.0.bias" in conv
    frame = synth.synthetic_frame(200, 260, seed=2)
    x = R.preprocess(frame, 160)
    with torch.no_grad():
        a = R.Ref(sd, torch.float64).forward(x)
        b = R.Ref(conv, torch.float64).forward(x)
    assert torch.equal(a["topk"], b["topk"])
    for k in ("boxes", "scores"):
        rel = ((a[k] - b[k]).abs() / a[k].abs().clamp(min=1e-30)).max().item()
        assert rel < 1e-9, (k, rel)
    f32 = weights_io.from_ultralytics_rtdetr_state_dict(sd)
    assert all(v.dtype == np.float32 for v in f32.values())


def test_converter_repconv_is_3x3_plus_centre(sd):
    from ffp_amd import weights_io
    conv = weights_io.from_ultralytics_rtdetr_state_dict(sd, dtype=np.float64)
    x = torch.randn(1, 256, 6, 7, dtype=torch.float64)
    p = "model.21.m.1"
    ref = R.Ref(sd).repconv(p, x)
    got = R.Ref(conv).repconv(p, x)
    assert torch.allclose(ref, got, rtol=1e-10, atol=1e-12)


def test_position_embedding_quirk():
    """Checks the tests-side reference (rtdetr_ref.pos_embed) against the formula; the engine's own table (rtdetr_pos_embed in
    csrc/rtdetr.cpp) is checked through the GPU parity tests, whose AIFI output depends on it."""
    pe = R.pos_embed(3, 2, 8, torch.float64)[0]        # w = 3, h = 2
    # meshgrid(grid_w, grid_h, indexing="ij") flattened: token t gets (w index t // h, h index t % h)
    for t in range(6):
        gw, gh = t // 2, t % 2
        om = 1.0 / (10000.0 ** (np.arange(2) / 2))
        exp = np.concatenate([np.sin(gw * om), np.cos(gw * om), np.sin(gh * om), np.cos(gh * om)])
        np.testing.assert_allclose(pe[t].numpy(), exp, atol=1e-6)


def test_anchors_and_valid_mask():
    """Checks the tests-side reference's anchors and valid mask; the engine's table (rtdetr_anchors in csrc/rtdetr.cpp) is checked through
    the GPU parity tests (the top-300 tokens and the encoder boxes depend on it)."""
    a, v = R.generate_anchors([[80, 80], [40, 40], [20, 20]])
    assert a.shape == (1, 8400, 4) and v.shape == (1, 8400, 1)
    v0 = v[0, :6400, 0].view(80, 80)
    assert not v0[0].any() and not v0[:, 0].any() and not v0[-1].any() and v0[1:-1, 1:-1].all()
    assert v[0, 6400:, 0].all()
    assert torch.isinf(a[0, :80]).all()
    np.testing.assert_allclose(torch.sigmoid(a[0, 6400 + 41]).numpy(), [1.5 / 40, 1.5 / 40, 0.1, 0.1], rtol=1e-12)


def test_stretch_resize_geometry():
    """Checks the tests-side reference's pre- and post-processing geometry; the device's stretch and decode are checked by the GPU
    end-to-end tests."""
    from oracle.ultra_post import resize_linear_u8
    img = (np.arange(30 * 50 * 3) % 251).astype(np.uint8).reshape(30, 50, 3)
    x = R.preprocess(img, 64)
    assert x.shape == (1, 3, 64, 64)
    st = resize_linear_u8(img, 64, 64)
    np.testing.assert_array_equal((x[0].numpy().transpose(1, 2, 0)[..., ::-1] * 255).round().astype(np.uint8), st)
    same = R.preprocess(resize_linear_u8(img, 64, 64), 64)              # already imgsz x imgsz: no resize
    assert torch.equal(same, x)
    d = R.postprocess(np.array([[0.5, 0.5, 0.2, 0.4]], np.float32), np.array([[0.9]], np.float32), (300, 400), 0.25)
    np.testing.assert_allclose(d, [[160, 90, 240, 210, 0.9, 0]], rtol=1e-6)


def test_synthetic_weights_give_detections():
    from ffp_amd import synth
    w = synth.rtdetr_l_weights(1)
    ref = R.Ref(w, torch.float32)
    frame = synth.synthetic_frame(480, 640, seed=5)
    with torch.no_grad():
        d = R.predict(ref, frame, 640, 0.25)
    assert 20 <= len(d) < 300, len(d)
    assert d[:, 4].max() - d[:, 4].min() > 0.2


def test_rtdetr_pt_raises():
    import ffp_amd.compat as compat
    compat.install()
    import ultralytics
    with pytest.raises(ValueError, match="from_ultralytics_rtdetr_state_dict"):
        ultralytics.RTDETR("x.pt")
    m = ultralytics.RTDETR("synthetic:rtdetr-l")
    with pytest.raises(NotImplementedError):
        m.predict(np.zeros((8, 8, 3), np.uint8), stream=True)
    with pytest.raises(NotImplementedError):
        m.predict("clip.mp4")
    with pytest.raises(NotImplementedError, match="show"):
        m.predict(np.zeros((8, 8, 3), np.uint8), show=True)

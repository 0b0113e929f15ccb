"""CPU checks of tests/ops_ref.py — the float64 references tests/test_gpu_ops.py holds the HIP kernels to — against
independent implementations: torch.nn.functional, the oracle's Ultralytics restatement, torch.topk."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x)).permute(2, 0, 1)[None]


@pytest.mark.parametrize("h,w", [(1, 1), (1, 13), (7, 5), (20, 20), (33, 32)])
def test_sppf_matches_chained_max_pool2d(h, w):
    rng = np.random.default_rng(h * 100 + w)
    x = rng.standard_normal((h, w, 8)) - 50.0          # all negative: a 0 standing in for the -inf padding would win
    y = _nchw(x)
    for got in ops_ref.sppf_pool(x):
        y = F.max_pool2d(y, 5, 1, 2)
        assert np.array_equal(got, y[0].permute(1, 2, 0).numpy())


def test_upsample_matches_interpolate():
    x = np.random.default_rng(0).standard_normal((3, 5, 4))
    want = F.interpolate(_nchw(x), scale_factor=2, mode="nearest")[0].permute(1, 2, 0).numpy()
    assert np.array_equal(ops_ref.upsample2x(x), want)


@pytest.mark.parametrize("h,w,nh,gain", [(1, 1, 2, 1.0), (3, 11, 2, 1.0), (13, 20, 4, 1.0), (5, 13, 2, 9.0)])
def test_attention_matches_scaled_dot_product_attention(h, w, nh, gain):
    rng = np.random.default_rng(h + w)
    qkv = rng.standard_normal((h, w, nh * 128))
    qkv[..., :] *= np.tile(np.r_[np.full(64, gain), np.ones(64)], nh)       # gain 9: logits of +-80 and beyond
    t = torch.from_numpy(qkv).reshape(h * w, nh, 128).permute(1, 0, 2)[None]  # (1, nh, N, 128)
    want = F.scaled_dot_product_attention(t[..., :32], t[..., 32:64], t[..., 64:])  # default scale = 32^-0.5
    want = want[0].permute(1, 0, 2).reshape(h, w, nh * 64).numpy()
    got = ops_ref.psa_attention(qkv, nh)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    # the float32 yardstick evaluates the same formula
    y32 = ops_ref.psa_attention(qkv.astype(np.float32), nh, dtype=np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - got).max() <= 1e-4 * np.abs(got).max()


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_dwconv_matches_grouped_conv2d(act):
    rng = np.random.default_rng(act)
    c = 8
    x, res = rng.standard_normal((9, 7, c)), rng.standard_normal((9, 7, c))
    w, b = rng.standard_normal((c, 3, 3)), rng.standard_normal(c)
    y = F.conv2d(_nchw(x), torch.from_numpy(w)[:, None], torch.from_numpy(b), padding=1, groups=c)
    y = [lambda v: v, F.silu, lambda v: F.leaky_relu(v, 0.2), F.relu][act](y) + _nchw(res)
    np.testing.assert_allclose(ops_ref.dwconv3x3(x, w, b, act, res), y[0].permute(1, 2, 0).numpy(), rtol=1e-12, atol=1e-12)


def test_grouped_gather_reads_v_of_the_psa_records():
    # two heads of [q(32) | k(32) | v(64)]: the positional conv's 128 channels are the two v blocks
    x = np.arange(2 * 3 * 260, dtype=np.float64).reshape(2, 3, 260)
    got = ops_ref.grouped_gather(x, 128, coff=4, grp=64, grp_stride=128, grp_off=64)
    want = np.concatenate([x[..., 4 + 64:4 + 128], x[..., 4 + 128 + 64:4 + 256]], -1)
    assert np.array_equal(got, want)
    assert np.array_equal(ops_ref.grouped_gather(x, 8, coff=12), x[..., 12:20])


@pytest.fixture(scope="module")
def oracle_forward():
    import ffp_amd  # noqa: F401
    from ffp_amd import synth
    from oracle import ultra_post
    from oracle.yolo11_ref import Yolo11PoseRef
    torch.set_num_threads(4)
    ref = Yolo11PoseRef(synth.yolo11_pose_weights("n"), "n")
    img = synth.synthetic_frame(160, 224, seed=21)                     # letterboxed to 96 x 128 at imgsz 128
    x = ultra_post.preprocess(img, 128)
    with torch.no_grad():
        raws = ref.forward_raw(x)
        out = ref.decode(raws)[0]
    levels = [r[0].permute(1, 2, 0).numpy() for r in raws]
    return ref, img, x, levels, out


def test_head_decode_matches_oracle_decode(oracle_forward):
    ref, _, _, levels, out = oracle_forward
    got = ops_ref.head_decode(levels, ref.nc, ref.kpt_shape[0])
    assert got.shape == tuple(out.shape)
    np.testing.assert_allclose(got, out.numpy(), rtol=2e-5, atol=2e-4)     # the oracle computes in float32
    got32 = ops_ref.head_decode(levels, ref.nc, ref.kpt_shape[0], dtype=np.float32)
    assert got32.dtype == np.float32
    np.testing.assert_allclose(got32, got, rtol=2e-5, atol=2e-4)


@pytest.mark.parametrize("conf,max_det", [(0.01, 300), (0.01, 7), (0.25, 300)])
def test_nms_and_scaling_match_oracle(oracle_forward, conf, max_det):
    from oracle import ultra_post
    ref, img, x, _, out = oracle_forward
    nk = ref.kpt_shape[0]
    det = ultra_post.non_max_suppression(out, conf, 0.7, max_det, nc=ref.nc)
    keep, cls, margins = ops_ref.nms(out.numpy(), ref.nc, conf, 0.7, max_det)
    assert margins["iou"] > 1e-5 and margins["conf"] > 1e-7, margins      # float32 (oracle) and float64 decide alike
    assert len(keep) == det.shape[0] and (conf > 0.2 or len(keep) >= min(max_det, 10))
    raw = out.numpy().astype(np.float64)
    assert np.array_equal(raw[4, keep].astype(np.float32), det[:, 4].numpy())             # same anchors, same order
    gain = min(x.shape[2] / img.shape[0], x.shape[3] / img.shape[1])
    pad_x = round((x.shape[3] - img.shape[1] * gain) / 2 - 0.1)
    pad_y = round((x.shape[2] - img.shape[0] * gain) / 2 - 0.1)
    geom = (gain, pad_x, pad_y, img.shape[1], img.shape[0], 0, 0)
    rows = ops_ref.det_rows(raw, keep, cls, ref.nc, nk, geom)
    np.testing.assert_allclose(rows[:, :4], ultra_post.scale_boxes(x.shape[2:], det[:, :4], img.shape[:2]).numpy(), atol=1e-3)
    kp = ultra_post.scale_coords(x.shape[2:], det[:, 6:].reshape(-1, nk, 3), img.shape[:2]).numpy()
    np.testing.assert_allclose(rows[:, 6:].reshape(-1, nk, 3), kp, atol=1e-3)
    assert np.array_equal(rows[:, 5], det[:, 5].numpy())


def test_nms_class_offset_and_ties():
    # two classes on the same box are both kept; equal scores are visited in anchor order
    raw = np.zeros((6, 4))
    raw[:4] = np.array([[50, 50, 20, 20]] * 4).T
    raw[4] = [0.9, 0.2, 0.5, 0.5]
    raw[5] = [0.1, 0.9, 0.1, 0.1]
    keep, cls, _ = ops_ref.nms(raw, 2, 0.25, 0.5, 300)
    assert keep.tolist() == [0, 1] and cls.tolist() == [0, 1, 0, 0]
    raw[:2, 2:] += 100                                                   # anchors 2, 3 now far from 0, 1 but on each other
    keep, _, _ = ops_ref.nms(raw, 2, 0.25, 0.5, 300)
    assert keep.tolist() == [0, 1, 2]


def test_truncate_shift():
    rows = np.array([[-0.5, 3.9, 130.2, 99.9, 0.5, 0, 7.25, 8.5, 0.9]])
    got = ops_ref.truncate_shift(rows, 1, (1, 0, 0, 128, 128, 10, 20), 100, 120)
    assert got[0].tolist() == [10, 23, 130, 119, 0.5, 0, 17.25, 28.5, 0.9]


def test_stable_topk_matches_torch_topk_without_ties():
    rng = np.random.default_rng(3)
    s = rng.permutation(8400).astype(np.float32) - 4000.5               # distinct values, both signs
    want = torch.topk(torch.from_numpy(s), 300).indices.numpy()
    assert np.array_equal(ops_ref.stable_topk(s), want)
    assert np.array_equal(ops_ref.stable_topk(s, signed_zero=False), want)


def test_stable_topk_ties_and_signed_zero():
    s = np.zeros(400, np.float32)
    assert ops_ref.stable_topk(s).tolist() == list(range(300))
    s[100:] = -0.0
    s[350:] = 0.0
    assert ops_ref.stable_topk(s).tolist() == list(range(100)) + list(range(350, 400)) + list(range(100, 250))
    assert ops_ref.stable_topk(s, signed_zero=False).tolist() == list(range(300))
    s = np.array([-np.inf, np.inf, 1.0, -1.0], np.float32)
    assert ops_ref.stable_topk(s, 4).tolist() == [1, 2, 3, 0]

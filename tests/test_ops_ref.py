"""CPU checks of tests/ops_ref.py — the float64 references tests/test_gpu_ops.py, tests/test_gpu_rtdetr_ops.py and
tests/test_gpu_scrfd_ops.py hold the HIP kernels to — against independent implementations: torch.nn.functional, the oracle's
Ultralytics restatement, torch.topk, and the grid_sample / predictor / RetinaFace restatements of rtdetr_ref.py and scrfd_ref.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref
from rt_deform_cases import DEFORM_SHAPES, deform_inputs


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


# ---- RT-DETR operators --------------------------------------------------------------------------------------------------------

def _hwc(t):
    return t[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("k,s,act", [(5, 1, 3), (3, 2, 0)])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 2), (6, 5), (5, 4), (6, 7)])
def test_rt_dwconv_matches_grouped_conv2d(h, w, k, s, act):
    rng = np.random.default_rng(h * 10 + w + k)
    c = 8
    x, wt, b = rng.standard_normal((h, w, c)), rng.standard_normal((c, k, k)), rng.standard_normal(c)
    y = F.conv2d(_nchw(x), torch.from_numpy(wt)[:, None], torch.from_numpy(b), stride=s, padding=k // 2, groups=c)
    if act == 3:
        y = F.relu(y)
    got = ops_ref.rt_dwconv(x, wt, b, k, s, act)
    assert got.shape == tuple(_hwc(y).shape)
    np.testing.assert_allclose(got, _hwc(y), rtol=1e-12, atol=1e-12)
    y32 = ops_ref.rt_dwconv(x.astype(np.float32), wt, b, k, s, act, dtype=np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - got).max() <= 1e-5 * max(1.0, np.abs(got).max())


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (4, 1), (5, 7)])
@pytest.mark.parametrize("shift", [-50.0, 0.0])
def test_rt_maxpool2_matches_padded_ceil_mode_max_pool(h, w, shift):
    x = np.random.default_rng(h + w).standard_normal((h, w, 4)) + shift      # all negative: the zero padding wins at the far edges
    want = F.max_pool2d(F.pad(_nchw(x), [0, 1, 0, 1]), 2, 1, ceil_mode=True)
    got = ops_ref.rt_maxpool2(x)
    assert np.array_equal(got, _hwc(want))
    if shift < 0:
        assert (got[-1] == 0).all() and (got[:, -1] == 0).all() and (got[:-1, :-1] < 0).all()


def test_layer_norm_and_gelu_match_torch():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((7, 256))
    x[1] += 1e4
    x[2] = 3.25
    x[3] *= 1e-4
    x[4, 17] = 1e4
    g, b = rng.standard_normal(256), rng.standard_normal(256)
    want = F.layer_norm(torch.from_numpy(x), (256,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    got = ops_ref.layer_norm(x, g, b)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)
    assert np.array_equal(got[2], b)                                         # a constant token: exactly beta
    assert ops_ref.layer_norm(x.astype(np.float32), g, b, dtype=np.float32).dtype == np.float32
    v = np.r_[np.linspace(-10, 10, 401), 0.0, -0.0, 30.0, -30.0, 1e-8]
    np.testing.assert_allclose(ops_ref.gelu(v), F.gelu(torch.from_numpy(v)).numpy(), rtol=1e-12, atol=1e-300)
    g32 = ops_ref.gelu(v.astype(np.float32), dtype=np.float32)
    assert g32.dtype == np.float32 and np.abs(g32 - ops_ref.gelu(v.astype(np.float32))).max() <= 1e-6 * 30


@pytest.mark.parametrize("L,gain", [(1, 1.0), (65, 1.0), (130, 30.0)])
def test_rt_attention_matches_scaled_dot_product_attention(L, gain):
    rng = np.random.default_rng(L)
    qk, v = rng.standard_normal((L, 512)) * np.sqrt(gain), rng.standard_normal((L, 256))
    t = lambda a: torch.from_numpy(a).reshape(L, 8, 32).permute(1, 0, 2)[None]
    want = F.scaled_dot_product_attention(t(qk[:, :256].copy()), t(qk[:, 256:].copy()), t(v))[0].permute(1, 0, 2).reshape(L, 256).numpy()
    got = ops_ref.rt_attention(qk, v)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11)
    y32 = ops_ref.rt_attention(qk.astype(np.float32), v.astype(np.float32), dtype=np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - got).max() <= 1e-3 * np.abs(got).max()


def test_rt_enc_prep_and_gather():
    rng = np.random.default_rng(1)
    levels = [rng.standard_normal(s + (256,)) for s in ((6, 4), (3, 2), (2, 1))]
    valid = (rng.random(32) > 0.3).astype(np.float64)
    t, tm = ops_ref.rt_enc_prep(levels, valid)
    want = torch.cat([_nchw(a).flatten(2).permute(0, 2, 1) for a in levels], 1)[0]          # _get_encoder_input
    assert np.array_equal(t, want.numpy()) and np.array_equal(tm, (torch.from_numpy(valid)[:, None] * want).numpy())
    anchors = rng.standard_normal((32, 4))
    e, a = ops_ref.rt_gather(t, [0, 31, 31, -1, 32, 5], anchors)
    assert np.array_equal(e, t[[0, 31, 31, 0, 31, 5]]) and np.array_equal(a, anchors[[0, 31, 31, 0, 31, 5]])


def test_rt_ref_matches_inverse_sigmoid():
    import rtdetr_ref
    r = np.array([0.0, 1.0, 1e-7, 1 - 1e-7, 0.5, -0.1, 1.1, 0.3])
    np.testing.assert_allclose(ops_ref.inverse_sigmoid(r), rtdetr_ref.inverse_sigmoid(torch.from_numpy(r)).numpy(), rtol=1e-14)
    d = np.array([0.0, 20.0, -20.0, 100.0, -100.0, 0.5, -0.5, 1.0])
    want = torch.sigmoid(torch.from_numpy(d) + rtdetr_ref.inverse_sigmoid(torch.from_numpy(r))).numpy()
    np.testing.assert_allclose(ops_ref.rt_ref(d, ref=r), want, rtol=1e-13, atol=1e-300)
    assert ops_ref.rt_ref(d, anc=np.full(8, np.inf)).tolist() == [1.0] * 8
    assert ops_ref.rt_ref(d.astype(np.float32), ref=r.astype(np.float32), dtype=np.float32).dtype == np.float32


@pytest.mark.parametrize("shapes", [[(5, 7), (3, 4), (2, 2)], [(7, 5), (4, 3), (2, 2)], [(4, 4), (2, 2), (1, 1)]])
def test_rt_deform_matches_grid_sample(shapes):
    """Against rtdetr_ref.multi_scale_deformable_attn (F.grid_sample) with the location formula of Ref.ms_deform_attn; the maps
    are not square, and the offsets push a good part of the points over every edge."""
    import rtdetr_ref
    rng = np.random.default_rng(len(shapes) + shapes[0][0])
    nt, Q = sum(h * w for h, w in shapes), 40
    val = rng.standard_normal((nt, 256))
    oa = np.concatenate([rng.standard_normal((Q, 192)) * 6, rng.standard_normal((Q, 96)) * 3], 1)
    ref = np.concatenate([rng.random((Q, 2)), rng.random((Q, 2)) * 0.6], 1)
    ref[3, 2:] = 0
    value = torch.from_numpy(val).view(1, nt, 8, 32)
    off = torch.from_numpy(oa[:, :192]).view(1, Q, 8, 3, 4, 2)
    aw = torch.softmax(torch.from_numpy(oa[:, 192:]).view(1, Q, 8, 12), -1).view(1, Q, 8, 3, 4)
    r = torch.from_numpy(ref)[None, :, None, :]
    loc = r[:, :, None, :, None, :2] + off / 4 * r[:, :, None, :, None, 2:] * 0.5
    want = rtdetr_ref.multi_scale_deformable_attn(value, [list(s) for s in shapes], loc, aw)[0].numpy()
    got = ops_ref.rt_deform(val, shapes, oa, ref)
    X, Y = ops_ref.rt_deform_locations(oa, ref, shapes)
    assert (X < -1).any() and (Y < -1).any() and ((X > -1) & (X < 0)).any() and ((Y > -1) & (Y < 0)).any()
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11)
    y32 = ops_ref.rt_deform(val.astype(np.float32), shapes, oa.astype(np.float32), ref.astype(np.float32), dtype=np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - got).max() <= 1e-3 * np.abs(got).max()
    if shapes[0][0] != shapes[0][1]:                       # the transposed geometry is another function of the same data
        assert np.abs(ops_ref.rt_deform(val, [(w, h) for h, w in shapes], oa, ref) - got).max() > 0.1


def test_rt_deform_inputs_cover_every_kind_of_sample_point():
    """A condition on the inputs, evaluated with the float32 location formula: every head meets every kind."""
    for val, oa, ref, kind in (deform_inputs(11 + i, w) for i, w in enumerate(["unit", "pm80"])):
        for i in range(2):
            X, Y = ops_ref.rt_deform_locations(oa[i], ref[i], DEFORM_SHAPES, dtype=np.float32)
            W = np.asarray([s[1] for s in DEFORM_SHAPES], np.float32)[None, None, :, None]
            H = np.asarray([s[0] for s in DEFORM_SHAPES], np.float32)[None, None, :, None]
            live = (ref[i][:, 2] > 0)[:, None, None, None] & (ref[i][:, 3] > 0)[:, None, None, None]
            conds = {
                "centre": (X == np.floor(X)) & (Y == np.floor(Y)) & (X >= 0) & (X < W) & (Y >= 0) & (Y < H),
                "x in [-1, 0)": (X >= -1) & (X < 0) & (Y >= 0) & (Y <= H - 1), "y in [-1, 0)": (Y >= -1) & (Y < 0) & (X >= 0) & (X <= W - 1),
                "x in [W-1, W)": (X >= W - 1) & (X < W), "y in [H-1, H)": (Y >= H - 1) & (Y < H),
                "x == -1": X == -1, "x == W": X == W, "far +": (X > 1e5) & (Y > 1e5), "far -": (X < -1e5) & (Y < -1e5),
                "width 0": np.broadcast_to((ref[i][:, 2] == 0)[:, None, None, None], X.shape),
            }
            for name, m in conds.items():
                per_head = (m & (live | (name == "width 0"))).sum((0, 2, 3))
                assert (per_head > 0).all(), f"image {i}: heads {np.flatnonzero(per_head == 0)} never meet '{name}'"


@pytest.mark.parametrize("nc", [1, 3, 80])
def test_rt_post_matches_the_predictor_restatement(nc):
    import rtdetr_ref
    rng = np.random.default_rng(nc)
    ref = rng.random((300, 4))
    logits = rng.standard_normal((300, nc)) * 2
    logits[5, :] = logits[5].max()                         # a tie over every class: the first one
    best = np.sort(ops_ref.sigmoid(logits).max(1))
    conf = float(best[149] + best[150]) / 2                # half of the queries pass
    rows, margin = ops_ref.rt_post(ref, logits, conf, (333, 200))
    assert margin > 1e-6
    want = rtdetr_ref.postprocess(ref, ops_ref.sigmoid(logits), (200, 333), conf)
    assert 0 < len(rows) < 300 and rows.shape == want.shape
    np.testing.assert_allclose(rows, want, rtol=1e-12, atol=1e-12)
    raw = ops_ref.rt_raw(ref, logits)
    assert raw.shape == (300, 4 + nc) and np.array_equal(raw[:, :4], ref)
    np.testing.assert_allclose(raw[:, 4:], torch.sigmoid(torch.from_numpy(logits)).numpy(), rtol=1e-14)


# ---- SCRFD operators ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (8, 6)])
def test_scrfd_pools_match_torch(h, w):
    x = np.random.default_rng(h).standard_normal((h, w, 3)) - 20.0
    assert np.array_equal(ops_ref.scrfd_maxpool(x), _hwc(F.max_pool2d(_nchw(x), 3, 2, 1)))
    for k in (1, 2, 3):
        want = F.avg_pool2d(_nchw(x), k, k, ceil_mode=True, count_include_pad=False)
        got = ops_ref.scrfd_avgpool(x, k)
        assert got.shape == tuple(_hwc(want).shape)
        np.testing.assert_allclose(got, _hwc(want), rtol=1e-13)
    assert ops_ref.scrfd_avgpool(x.astype(np.float32), 2, dtype=np.float32).dtype == np.float32


@pytest.mark.parametrize("use_kps", [False, True])
def test_scrfd_post_matches_the_retinaface_restatement(use_kps):
    import scrfd_ref
    rng = np.random.default_rng(4)
    net_h, net_w, ds = 64, 96, 0.75
    sizes = [(net_h // s, net_w // s) for s in (8, 16, 32)]
    score = [ops_ref.sigmoid(rng.standard_normal(s + (2,)) * 2).astype(np.float32) for s in sizes]
    bbox = [(rng.random(s + (8,)) * 3).astype(np.float32) for s in sizes]
    kps = [rng.standard_normal(s + (20,)).astype(np.float32) for s in sizes] if use_kps else None
    outs = [a.reshape(-1, 1) for a in score] + [a.reshape(-1, 4) for a in bbox] + ([a.reshape(-1, 10) for a in kps] if use_kps else [])
    det, kpss = scrfd_ref.post(outs, ds, net_w, net_h, 0.5, 0.4)
    keep, boxes, kk, margins = ops_ref.scrfd_post(score, bbox, kps, (net_h, net_w), float(np.float32(ds)), 0.5, 0.4)
    assert margins["score"] > 1e-6 and margins["ovr"] > 1e-5, margins        # float32 and float64 decide alike
    assert 3 < len(keep) < (score[0] >= 0.5).sum() + (score[1] >= 0.5).sum() + (score[2] >= 0.5).sum()      # something was suppressed
    allsc = np.concatenate([a.reshape(-1) for a in score])
    assert np.array_equal(allsc[keep], det[:, 4])
    np.testing.assert_allclose(boxes, det[:, :4], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(kk, kpss, rtol=1e-5, atol=1e-4)

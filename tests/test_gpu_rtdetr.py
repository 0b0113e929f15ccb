"""GPU parity of RT-DETR-l (C-ABI ffp_rtdetr_*) against the tests-side reference (tests/rtdetr_ref.py) on synthetic weights: the raw
model output and the top-300 selection, predict end to end (4K frame, non-square image, batch of 8), nc = 1 and 80, batch independence
and graph replay."""
import numpy as np
import pytest
import torch

import rtdetr_ref as R
from util import iou_xyxy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def w1():
    from ffp_amd import synth
    return synth.rtdetr_l_weights(1)


@pytest.fixture(scope="module")
def ref1(w1):
    return R.Ref(w1, torch.float64)


@pytest.fixture(scope="module", params=["f32", "f32x3"])
def det(request, gpu_lib, w1):
    prec = gpu_lib.PREC_F32 if request.param == "f32" else gpu_lib.PREC_F32X3
    return gpu_lib.RTDETRDetector(w1, precision=prec)


def _frame(h, w, seed):
    from ffp_amd import synth
    return synth.synthetic_frame(h, w, seed=seed)


def _check_raw(got, topk, o, tol=1e-4):
    """got [300, 4 + nc], topk [300] from the device; o the reference's outputs of the same image. Returns how many queries were
    compared (0 when the device kept a different boundary token, which changes every query's self-attention)."""
    em = o["enc_max"][0].double().numpy()
    kth = np.sort(em)[::-1][299]
    ref_tok = o["topk"][0].numpy()
    border = set(np.nonzero(np.abs(em - kth) <= 1e-5)[0].tolist())
    assert set(topk.tolist()) - border == set(ref_tok.tolist()) - border
    pos = {int(t): i for i, t in enumerate(ref_tok)}
    rb, rs = o["boxes"][0].double().numpy(), o["scores"][0].double().numpy()
    if set(topk.tolist()) != set(ref_tok.tolist()):
        return 0                                 # a swapped boundary query changes the self-attention of every query: nothing to align
    for q, t in enumerate(topk):
        i = pos[int(t)]
        np.testing.assert_allclose(got[q, :4], rb[i], atol=tol, err_msg=f"query {q} box")
        np.testing.assert_allclose(got[q, 4:], rs[i], atol=tol, err_msg=f"query {q} scores")
    return len(topk)


def test_forward_raw_matches_reference(det, ref1):
    fr = _frame(480, 640, 5)
    raw, topk = det.forward_raw([fr], 640)
    with torch.no_grad():
        o = ref1.forward(R.preprocess(fr, 640))
    assert _check_raw(raw[0], topk[0], o) == 300          # these inputs have no near-tie at the 300th score: every query is compared


def _match(got, exp, conf=0.25):
    """Every reference box matched at IoU >= 0.999 with a score within 1e-4, except detections within 1e-4 of the threshold."""
    near = lambda d: np.abs(d[:, 4] - conf) < 1e-4
    assert abs(len(got) - len(exp)) <= int(near(exp).sum()) + int(near(got).sum())
    used = set()
    for e in exp:
        if abs(e[4] - conf) < 1e-4:
            continue
        ious = iou_xyxy(np.repeat(e[None, :4], len(got), 0), got[:, :4]) if len(got) else np.zeros(0)
        cand = [j for j in np.argsort(-ious) if j not in used and ious[j] >= 0.999 and abs(got[j, 4] - e[4]) < 1e-4 and got[j, 5] == e[5]]
        assert cand, f"reference box {e} unmatched"
        used.add(cand[0])


@pytest.mark.parametrize("shape", [(2160, 3840), (300, 400)])
def test_predict_end_to_end(det, w1, shape):
    fr = _frame(*shape, seed=7)
    got = det.predict([fr], 640, 0.25)[0]
    exp = R.predict(R.Ref(w1, torch.float32), fr, 640, 0.25)
    assert len(exp) >= 20 and len(got) >= 20
    _match(got, exp)


def test_predict_batch_of_8(det, w1):
    frs = [_frame(240 + 40 * i, 320 + 56 * i, seed=20 + i) for i in range(8)]
    got = det.predict(frs, 640, 0.25)
    ref = R.Ref(w1, torch.float32)
    for fr, g in zip(frs, got):
        exp = R.predict(ref, fr, 640, 0.25)
        assert len(g) >= 20
        _match(g, exp)


@pytest.mark.parametrize("prec", ["f32", "f32x3"])
def test_nc80(gpu_lib, prec):
    from ffp_amd import synth
    w = synth.rtdetr_l_weights(80)
    d = gpu_lib.RTDETRDetector(w, precision=gpu_lib.PREC_F32 if prec == "f32" else gpu_lib.PREC_F32X3)
    assert d.nc == 80
    fr = _frame(360, 480, 9)
    raw, topk = d.forward_raw([fr], 320)
    with torch.no_grad():
        o = R.Ref(w, torch.float64).forward(R.preprocess(fr, 320))
    assert _check_raw(raw[0], topk[0], o) == 300


def test_batch_independence_and_replay_f32(gpu_lib, w1):
    d = gpu_lib.RTDETRDetector(w1, precision=gpu_lib.PREC_F32)
    a, b, c = _frame(300, 400, 1), _frame(500, 380, 2), _frame(720, 1280, 3)
    r_eager, t_eager = d.forward_raw([a, b, c], 320)
    assert d.info()["graph_state"] == 0
    r_replay, t_replay = d.forward_raw([a, b, c], 320)
    assert d.info()["graph_state"] == 1
    assert np.array_equal(r_eager, r_replay) and np.array_equal(t_eager, t_replay)
    r_b, t_b = d.forward_raw([b], 320)
    assert np.array_equal(r_b[0], r_eager[1]) and np.array_equal(t_b[0], t_eager[1])
    r_ca, _ = d.forward_raw([c, a, b], 320)
    assert np.array_equal(r_ca[0], r_eager[2]) and np.array_equal(r_ca[1], r_eager[0])
    p1 = d.predict([b], 320, 0.25)[0]
    p3 = d.predict([a, b, c], 320, 0.25)[1]
    assert np.array_equal(p1, p3)

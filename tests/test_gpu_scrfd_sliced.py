"""Device-resident sliced prediction of the SCRFD detector (ffp_scrfd_infer_tiles_ex / _dev, ffp_scrfd_sliced_predict / _dev,
ffp_op_scrfd_sahi_rows, pipeline.DetectionFirstPipeline) on a small synthetic model at det size 128: the operator against the numpy
restatement of tests/scrfd_sahi_common.py, the two modes, chunking in both precisions, the device variants, the fused call against
oracle/sahi_ref's merge, against get_sliced_prediction through compat and against the pure CPU chain, the negative-box error, the
pipeline class and the plan memory entries."""
import ctypes as C
import os

import numpy as np
import pytest

import scrfd_ref
import scrfd_sahi_common as S
from util import match_by_iou

pytestmark = pytest.mark.gpu

DET = (128, 128)
THR, NMS = 0.5, 0.4
SL, OV = 96, 0.2
FRAMES = {"a": (200, 260, 21), "b": (160, 200, 21), "neg": (200, 260, 7)}
PPS = [("NMS", "IOS", 0.5), ("GREEDYNMM", "IOS", 0.5)]


@pytest.fixture(scope="module")
def model():
    from ffp_amd import synth
    return synth.scrfd_onnx(3, style="folded", stem=8, widths=(16, 16, 16, 32), depths=(1, 1, 1, 1), neck=16, head=16, stacked=1, calib_size=64)


@pytest.fixture(scope="module")
def frames():
    from ffp_amd import synth
    return {k: synth.synthetic_frame(h, w, seed) for k, (h, w, seed) in FRAMES.items()}


@pytest.fixture(scope="module")
def det(gpu_lib, model):
    return gpu_lib.FaceDetector(model[0], precision=gpu_lib.PREC_F32)


def _items(gpu_lib, frame):
    H, W = frame.shape[:2]
    t = [[int(v) for v in b] for b in gpu_lib.slice_bboxes(H, W, SL, SL, OV, OV)]
    return t + [[0, 0, W, H]] if len(t) > 1 else t


@pytest.fixture(scope="module")
def local(gpu_lib, det, frames):
    """The baseline, computed once: the existing infer_tiles (ffp_scrfd_infer_tiles) on the items of the two clean frames."""
    return {k: det.infer_tiles(frames[k], _items(gpu_lib, frames[k]), DET, THR, NMS) for k in ("a", "b")}


@pytest.fixture(scope="module")
def sahi(gpu_lib, det, frames):
    return {k: det.infer_tiles(frames[k], _items(gpu_lib, frames[k]), DET, THR, NMS, conf=THR, mode="sahi") for k in ("a", "b")}


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), f"tile {k}"


def _restated(rows, items, frame, conf):
    out = []
    for r, t in zip(rows, items):
        w, bad = S.sahi_rows(r, t, frame.shape[0], frame.shape[1], conf)
        assert not bad
        out.append(w)
    return out


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------

def test_op_sahi_rows(gpu_lib):
    dets, counts = S.hand_rows()
    got, cnt, bad = gpu_lib.op_scrfd_sahi_rows(dets, counts, S.TILES, S.FULL, S.CONF)
    assert bad is None
    for t in range(3):
        want, _ = S.sahi_rows(dets[t, :counts[t]], S.TILES[t], *S.FULL, S.CONF)
        assert cnt[t] == len(want), f"tile {t}"
        assert np.array_equal(got[t, :cnt[t]], want), f"tile {t}"                       # bit for bit, in the tile's order
        assert (got[t, cnt[t]:counts[t]] == 0).all()                                    # vacated rows zeroed (include/ffp.h)
        assert (got[t, counts[t]:] == S.SENTINEL).all()                                 # rows past the old count untouched
    assert list(cnt) == [6, 0, 3]


def test_op_sahi_rows_negative_far_corner(gpu_lib):
    dets, counts = S.hand_rows(negative=True)
    got, cnt, bad = gpu_lib.op_scrfd_sahi_rows(dets, counts, S.TILES, S.FULL, S.CONF)
    assert bad == (2, 1)                                                                # rows (2, 1) and (2, 3) offend: the first is named
    out, c, b = dets.copy(), counts.copy(), C.c_int32(-5)
    rc = gpu_lib.lib().ffp_op_scrfd_sahi_rows(0, 3, S.CAP, gpu_lib._ip(S.TILES), S.FULL[0], S.FULL[1], S.CONF, gpu_lib._fp(out), gpu_lib._ip(c), C.byref(b))
    msg = gpu_lib.lib().ffp_last_error().decode()
    assert rc == 1 and b.value == 2 * S.CAP + 1 and "tile 2 row 1" in msg and "cannot be negative" in msg
    want0, _ = S.sahi_rows(dets[0, :counts[0]], S.TILES[0], *S.FULL, S.CONF)            # the other tiles are converted as usual
    assert cnt[0] == len(want0) and np.array_equal(got[0, :cnt[0]], want0)


def test_op_sahi_rows_many_rounds(gpu_lib):
    """520 rows in one tile: three rounds of the 256-thread workgroup, survivors of a later round land on rows an earlier round read."""
    rng = np.random.default_rng(3)
    cap, n = 600, 520
    dets = np.full((2, cap, S.STRIDE), S.SENTINEL, np.float32)
    dets[:, :n] = rng.uniform(-20, 120, (2, n, S.STRIDE)).astype(np.float32)
    dets[:, :n, 2:4] = np.abs(dets[:, :n, 2:4]) + 1                                     # far corners positive: nothing to flag
    dets[:, :n, 4] = rng.uniform(0.3, 0.9, (2, n)).astype(np.float32)
    dets[1, :n, 4] = 0.9                                                                # the second tile keeps every row
    counts = np.array([n, n], np.int32)
    tiles = np.array([[40, 8, 136, 104], [0, 0, 260, 200]], np.int32)
    got, cnt, bad = gpu_lib.op_scrfd_sahi_rows(dets, counts, tiles, S.FULL, S.CONF)
    assert bad is None
    for t in range(2):
        want, _ = S.sahi_rows(dets[t, :n], tiles[t], *S.FULL, S.CONF)
        assert cnt[t] == len(want) and np.array_equal(got[t, :cnt[t]], want)
        assert (got[t, cnt[t]:n] == 0).all() and (got[t, n:] == S.SENTINEL).all()
    assert 256 < cnt[0] < n and cnt[1] == n


# ---- 2. modes ------------------------------------------------------------------------------------------------------------------------

def test_local_mode_is_infer_tiles(gpu_lib, det, frames, local):
    f = frames["a"]
    items = _items(gpu_lib, f)
    assert len(items) == 13 and sum(len(r) for r in local["a"]) > 100
    _same(det.infer_tiles(f, items, DET, THR, NMS, conf=THR, mode="local"), local["a"])


@pytest.mark.parametrize("conf", [THR, 0.6])
def test_sahi_mode_is_the_restatement(gpu_lib, det, frames, local, conf):
    f = frames["a"]
    items = _items(gpu_lib, f)
    got = det.infer_tiles(f, items, DET, THR, NMS, conf=conf, mode="sahi")
    _same(got, _restated(local["a"], items, f, conf))
    n_local, n_got = sum(len(r) for r in local["a"]), sum(len(r) for r in got)
    assert (n_got == n_local) if conf == THR else (0 < n_got < n_local)               # at 0.6 the compaction drops rows


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["PREC_F32", "PREC_F32X3"])
def test_chunks_give_the_same_bits(gpu_lib, model, frames, precision):
    """13 items at max_batch 5 (chunks 5, 4, 4) and 1 against one batch of 13: a tile's rows do not depend on its batch mates."""
    d = gpu_lib.FaceDetector(model[0], precision=getattr(gpu_lib, precision))
    f = frames["a"]
    items = _items(gpu_lib, f)
    for mode in ("local", "sahi"):
        whole = d.infer_tiles(f, items, DET, THR, NMS, conf=THR, mode=mode, max_batch=0)
        assert sum(len(r) for r in whole) > 100
        for mb in (5, 1):
            _same(d.infer_tiles(f, items, DET, THR, NMS, conf=THR, mode=mode, max_batch=mb), whole)
    assert d.mem_bytes()["plans_resident"] == 4                                        # batches of 13, 5, 4 and 1


# ---- 4. device variants --------------------------------------------------------------------------------------------------------------

def test_device_variants(gpu_lib, det, frames, local, sahi):
    import torch
    f = frames["a"]
    H, W = f.shape[:2]
    items = _items(gpu_lib, f)
    cap = 256
    d_frame = torch.from_numpy(f).cuda()
    d_out = torch.full((len(items), cap, S.STRIDE), S.SENTINEL, dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(len(items), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                          # the engine works on its own stream
    for mode, want in (("local", local["a"]), ("sahi", sahi["a"])):
        det.infer_tiles_dev(d_frame.data_ptr(), H, W, items, d_out.data_ptr(), cap, d_cnt.data_ptr(), DET, THR, NMS, conf=THR, mode=mode, max_batch=5)
        out, cnt = d_out.cpu().numpy(), d_cnt.cpu().numpy()
        _same([out[i, :cnt[i]] for i in range(len(items))], want)
    d_rows = torch.zeros((512, S.STRIDE), dtype=torch.float32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.sliced_predict_dev(d_frame.data_ptr(), H, W, d_rows.data_ptr(), 512, d_n.data_ptr(), SL, SL, OV, OV, True, DET, THR, NMS, THR, max_batch=5)
    host = det.sliced_predict(f, SL, SL, OV, OV, True, DET, THR, NMS, THR, max_batch=0)
    n = int(d_n.item())
    assert n == len(host) > 1 and np.array_equal(d_rows[:n].cpu().numpy(), host)
    # the untruncated count with a short output (the rule of ffp_merge_dev): no error, the first rows written
    d_n.zero_()
    torch.cuda.synchronize()
    det.sliced_predict_dev(d_frame.data_ptr(), H, W, d_rows.data_ptr(), 3, d_n.data_ptr(), SL, SL, OV, OV, True, DET, THR, NMS, THR, max_batch=0)
    assert int(d_n.item()) == len(host) and np.array_equal(d_rows[:3].cpu().numpy(), host[:3])
    with pytest.raises(gpu_lib.FfpError, match=f"{len(host)} merged"):
        det.sliced_predict(f, SL, SL, OV, OV, True, DET, THR, NMS, THR, cap=3)


# ---- 5. the fused call ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["a", "b"])
@pytest.mark.parametrize("pp", PPS)
def test_fused_equals_oracle_merge(gpu_lib, det, frames, sahi, key, pp):
    from oracle import sahi_ref
    rows = np.concatenate(sahi[key], 0)
    # the full-frame prediction is the one sahi does not shift: it keeps its full_shape, and a union it keeps is clipped to the frame
    first_full = len(rows) - len(sahi[key][-1])
    shape = list(frames[key].shape[:2])
    dets = [sahi_ref.Det([float(v) for v in r[:4]], r[4], 0, full_shape=shape if i >= first_full else None, kpts=r[6:].copy(), src=i)
            for i, r in enumerate(rows)]
    want = sahi_ref.postprocess(dets, pp[0], pp[1], pp[2], False)
    got = det.sliced_predict(frames[key], SL, SL, OV, OV, True, DET, THR, NMS, THR, pp[0], pp[1], pp[2], max_batch=5)
    assert 1 < len(want) < len(rows) and len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g[:4], np.float32(w.bbox)) and g[4] == np.float32(w.score) and g[5] == 0
        assert np.array_equal(g[6:], w.kpts)                                           # the keypoints of the (higher-scored) source row
    if pp[0] == "GREEDYNMM":
        assert any(not np.array_equal(g[:4], rows[w.src, :4]) for g, w in zip(got, want))      # some box is a union


@pytest.fixture()
def pack_home(tmp_path, monkeypatch, model):
    d = tmp_path / "home" / ".insightface" / "models" / "buffalo_l"
    os.makedirs(d)
    (d / "det_10g.onnx").write_bytes(model[0])
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    return d


def _compat_model(conf):
    import ffp_amd.compat as compat
    compat.install()
    from utils.insightface_wrapper import InsightFaceDetectionModel
    m = InsightFaceDetectionModel(confidence_threshold=conf)
    m.model.prepare(det_size=DET, det_thresh=conf)                                     # the wrapper prepares at 640; the small model runs at 128
    return m


def _compat_rows(m, rgb, pp):
    from sahi.predict import get_sliced_prediction
    res = get_sliced_prediction(image=rgb, detection_model=m, slice_height=SL, slice_width=SL, overlap_height_ratio=OV, overlap_width_ratio=OV,
                                postprocess_type=pp[0], postprocess_match_metric=pp[1], postprocess_match_threshold=pp[2], verbose=0)
    return np.asarray([p.bbox.to_xyxy() + [p.score.value] for p in res.object_prediction_list], np.float64).reshape(-1, 5)


@pytest.mark.parametrize("pp", PPS)
def test_fused_equals_get_sliced_prediction(gpu_lib, det, frames, pack_home, pp):
    m = _compat_model(THR)
    for key in ("a", "b"):
        py = _compat_rows(m, frames[key], pp)
        got = det.sliced_predict(frames[key], SL, SL, OV, OV, True, DET, THR, NMS, THR, pp[0], pp[1], pp[2], max_batch=0)
        assert len(py) == len(got) > 1
        assert np.array_equal(py[:, :4].astype(np.float32), got[:, :4]) and np.array_equal(py[:, 4].astype(np.float32), got[:, 4])    # row for row


def _cpu_chain(g, rgb):
    """test_gpu_scrfd_compat._cpu_chain at this file's sizes: NumPy RetinaFace.detect per slice -> the wrapper's conversion -> sahi_ref."""
    from oracle import sahi_ref
    from oracle.ultra_post import PredictResult

    def predict_fn(im):
        (d, kps), _ = scrfd_ref.detect(g, im, DET[0], DET[1], THR, NMS, flip=True)
        b = d[:, :4].copy()
        b[:, 0:2] = np.maximum(b[:, 0:2], 0)              # the clip commutes with the truncation: the bounds are integers
        b[:, 2] = np.minimum(b[:, 2], rgb.shape[1])
        b[:, 3] = np.minimum(b[:, 3], rgb.shape[0])
        return PredictResult(b, d[:, 4], np.zeros(len(d)), kps)

    return sahi_ref.get_sliced_prediction(rgb, predict_fn, SL, SL, OV, OV)


@pytest.mark.parametrize("key", ["a", "b"])
def test_fused_against_cpu_chain(gpu_lib, det, model, frames, key):
    """The bars of test_gpu_scrfd_compat.test_app_v1_flow: the count differs by at most 1, >= 95 % of the IoU-matched boxes are equal."""
    ref = _cpu_chain(model[1], frames[key])
    eb = np.asarray([d.bbox for d in ref], np.float64).reshape(-1, 4)
    got = det.sliced_predict(frames[key], SL, SL, OV, OV, True, DET, THR, NMS, THR, max_batch=0).astype(np.float64)
    pairs = match_by_iou(eb, got[:, :4])
    frac = float(np.mean([np.array_equal(eb[i], got[j, :4]) for i, j, _ in pairs]))
    print(f"frame {key}: cpu {len(eb)} fused {len(got)} matched {len(pairs)} equal {frac:.4f}")
    assert abs(len(eb) - len(got)) <= 1, (len(eb), len(got))
    assert frac >= 0.95


def test_single_slice_is_not_merged(gpu_lib, det, frames):
    small = np.ascontiguousarray(frames["a"][:SL, :SL])
    want = det.infer_tiles(small, [[0, 0, SL, SL]], DET, THR, NMS, conf=THR, mode="sahi")[0]
    got = det.sliced_predict(small, SL, SL, OV, OV, True, DET, THR, NMS, THR, "NMS", "IOS", 0.01)
    assert len(want) > 1 and np.array_equal(got, want)
    merged, _ = gpu_lib.merge(want, "NMS", "IOS", 0.01)
    assert len(merged) < len(want)                    # a merge would have shown


# ---- 6. the negative box --------------------------------------------------------------------------------------------------------------

def test_negative_far_corner_fails_the_frame(gpu_lib, det, frames, pack_home):
    f = frames["neg"]
    with pytest.raises(gpu_lib.FfpError, match=r"tile \d+ row \d+.*cannot be negative") as e:
        det.sliced_predict(f, SL, SL, OV, OV, True, DET, THR, NMS, THR)
    assert e.value.code == 1
    m = _compat_model(THR)
    with pytest.raises(Exception, match="cannot be negative"):
        _compat_rows(m, f, PPS[1])
    again = det.sliced_predict(frames["b"], SL, SL, OV, OV, True, DET, THR, NMS, THR)       # the engine is usable after the error
    assert len(again) > 1


# ---- 7. the pipeline class ------------------------------------------------------------------------------------------------------------

def test_detection_first_pipeline(gpu_lib, det, model, frames):
    import torch
    from ffp_amd import pipeline, synth
    rgb = frames["a"]
    H, W = rgb.shape[:2]
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    sr_w = synth.rrdbnet_weights(4, 23)                                                # "synthetic:RealESRGAN_x4plus"
    cfg = pipeline.PipeConfig(slice_h=SL, slice_w=SL, overlap=OV, conf=THR, sr_crops=3, merge_cap=512)
    pipe = pipeline.DetectionFirstPipeline(model[0], sr_w, cfg, det_size=DET, nms_thresh=NMS)
    d_bgr = torch.from_numpy(bgr).cuda()
    torch.cuda.synchronize()
    rows_d, n = pipe.detect(d_bgr, H, W)
    want = det.sliced_predict(rgb, SL, SL, OV, OV, True, DET, THR, NMS, THR, chan_order=gpu_lib.CHAN_AS_BGR, max_batch=0)
    assert n == len(want) > 3 and np.array_equal(rows_d[:n].cpu().numpy(), want)        # BGR resident + no flip == sahi's RGB + swapRB
    boxes = pipe.crop_boxes(rows_d[:n])
    assert boxes.dtype == np.int32 and boxes.shape == (3, 4)
    out, offs = pipe.enhance_crops(d_bgr, H, W, boxes)
    fp = pipeline.FramePipeline(synth.yolo11_pose_weights("n"), sr_w, cfg, arch="n")
    out2, offs2 = fp.enhance_crops(d_bgr, H, W, boxes)
    assert list(offs) == list(offs2) and out.numel() == out2.numel() > 0
    assert torch.equal(out, out2)


# ---- 8. memory ------------------------------------------------------------------------------------------------------------------------

def test_mem_bytes_and_drop_plans(gpu_lib, model, frames):
    d = gpu_lib.FaceDetector(model[0], precision=gpu_lib.PREC_F32)
    assert d.mem_bytes() == {"plans": 0, "plans_resident": 0}
    first = d.sliced_predict(frames["b"], SL, SL, OV, OV, True, DET, THR, NMS, THR, max_batch=3)      # 7 items: chunks 3, 2, 2
    mb = d.mem_bytes()
    assert mb["plans"] > 0 and mb["plans_resident"] == 2
    d.drop_plans()
    assert d.mem_bytes() == {"plans": 0, "plans_resident": 0}
    assert np.array_equal(d.sliced_predict(frames["b"], SL, SL, OV, OV, True, DET, THR, NMS, THR, max_batch=3), first)


def test_ninth_plan_evicts_the_least_recently_used(gpu_lib, model, frames):
    """At most 8 plans per handle, least recently used first out (csrc/plan_cache.hpp): batches of n = 1..9 tiles are nine plans of nine
    different sizes b_n, so the byte sum of the resident plans tells which ones they are."""
    d = gpu_lib.FaceDetector(model[0], precision=gpu_lib.PREC_F32)
    f = frames["a"]
    items = _items(gpu_lib, f)
    run = lambda n: d.infer_tiles(f, items[:n], DET, THR, NMS)
    b = {}
    for n in range(1, 10):
        d.drop_plans()
        rows = run(n)
        b[n] = d.mem_bytes()["plans"]
        if n == 2:
            first2 = rows
    assert len(set(b.values())) == 9 and min(b.values()) > 0, b
    d.drop_plans()
    for n in range(1, 9):
        run(n)
    assert d.mem_bytes() == {"plans": sum(b[n] for n in range(1, 9)), "plans_resident": 8}
    run(1)                                                                 # a hit: n = 1 becomes the most recently used
    assert d.mem_bytes() == {"plans": sum(b[n] for n in range(1, 9)), "plans_resident": 8}
    run(9)                                                                 # n = 2 goes, not n = 1
    assert d.mem_bytes() == {"plans": sum(b.values()) - b[2], "plans_resident": 8}
    again2 = run(2)                                                        # laid out again; n = 3 goes
    assert d.mem_bytes() == {"plans": sum(b.values()) - b[3], "plans_resident": 8}
    _same(again2, first2)

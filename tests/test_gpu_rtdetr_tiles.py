"""RT-DETR-l over tiles of one frame (ffp_rtdetr_infer_tiles, ffp_rtdetr_sliced_predict, ffp_op_rt_post_tiles) on synthetic weights: tiles
equal host crops through the existing predict (FP32: bit for bit), channel order, the SAHI box rules against a float32 numpy restatement, the
fused call against the staged one, the single-slice case, F32X3 against the CPU reference, and the argument errors."""
import numpy as np
import pytest
import torch

import rtdetr_ref as R
import rtdetr_tiles_common as T
from test_gpu_rtdetr import _match

pytestmark = pytest.mark.gpu

NQ = 300


@pytest.fixture(scope="module")
def w1():
    from ffp_amd import synth
    return synth.rtdetr_l_weights(1)


@pytest.fixture(scope="module")
def det(gpu_lib, w1):
    return gpu_lib.RTDETRDetector(w1, precision=gpu_lib.PREC_F32)


@pytest.fixture(scope="module")
def frame():
    return T.frame_bgr()


@pytest.fixture(scope="module")
def tl(gpu_lib):
    return T.tiles(gpu_lib)


@pytest.fixture(scope="module")
def conf(det, frame, tl):
    return T.median_conf(det, frame, tl)


@pytest.fixture(scope="module")
def by_crop(det, frame, tl, conf):
    """The baseline: the existing predict() on the host crops, computed once."""
    rows = det.predict(T.crops(frame, tl), T.IMGSZ, conf)
    n = sum(len(r) for r in rows)
    assert 0 < n < len(tl) * NQ                       # the median keeps some and drops some
    return rows


@pytest.fixture(scope="module")
def local(det, frame, tl, conf):
    return det.infer_tiles(frame, tl, T.IMGSZ, conf, "local", max_batch=3)


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), f"tile {k}"


def test_chunk_sizes_run(det, local, by_crop):
    """max_batch = 3 over seven tiles: chunks of 3, 2, 2 (two plans); the rows equal predict() on the crops bit for bit."""
    _same(local, by_crop)
    assert det.mem_bytes()["plans_resident"] >= 2


def test_tiles_equal_crops_default_batch(det, frame, tl, conf, by_crop):
    _same(det.infer_tiles(frame, tl, T.IMGSZ, conf, "local", max_batch=0), by_crop)


def test_channel_order(gpu_lib, det, frame, tl, conf, local):
    rgb = np.ascontiguousarray(frame[:, :, ::-1])
    _same(det.infer_tiles(rgb, tl, T.IMGSZ, conf, "local", chan_order=gpu_lib.CHAN_AS_RGB, max_batch=3), local)


def _op_inputs():
    """n = 3 tiles, nc = 2, record widths 8 (boxes at 4) and 4 (logits at 1). Boxes are cx, cy, w, h times the tile size; logits far from
    the threshold except the one that sits on it."""
    tiles = np.array([[40, 8, 136, 104], [168, 104, 264, 200], [0, 0, 264, 200]], np.int32)      # 96 x 96, 96 x 96 at the corner, full frame
    ref = np.zeros((3, NQ, 8), np.float32)
    lg = np.full((3, NQ, 4), -6.0, np.float32)                    # sigmoid 0.0025: dropped
    rng = np.random.default_rng(5)
    ref[..., 4:8] = rng.uniform(0.2, 0.6, (3, NQ, 4)).astype(np.float32) * np.float32([1, 1, 0.5, 0.5])
    q = {}
    def put(name, tile, query, box, logits):
        ref[tile, query, 4:8] = box
        lg[tile, query, 1:3] = logits
        q[name] = (tile, query)
    put("plain", 0, 3, [0.5, 0.5, 0.25, 0.25], [3.0, -3.0])
    put("neg_corner", 0, 7, [0.05, 0.03, 0.3, 0.2], [2.0, -1.0])              # x1, y1 < 0: clamped to 0
    put("left_of_crop", 0, 20, [-0.3, 0.5, 0.2, 0.2], [2.5, 0.0])             # x2 < 0: dropped in SAHI mode, kept in LOCAL
    put("zero_width", 0, 41, [0.5, 0.5, 0.0, 0.3], [2.5, 0.0])                # x1 == x2: dropped
    put("on_conf", 0, 55, [0.4, 0.4, 0.2, 0.2], [0.0, -4.0])                  # sigmoid(0) = 0.5 = conf exactly: strict >
    put("second_class", 0, 299, [0.6, 0.4, 0.2, 0.2], [-1.0, 4.0])
    put("past_full", 1, 0, [0.9, 0.95, 0.4, 0.3], [3.0, 1.0])                 # reaches past the crop, but the clip is against the FULL shape
    put("past_full_frame", 2, 150, [0.97, 0.98, 0.2, 0.2], [1.0, 3.5])        # full-frame tile: x2 > full_w, y2 > full_h, clamped
    put("neg_full_frame", 2, 151, [0.01, 0.5, 0.1, 0.1], [1.5, -2.0])
    for k in range(100, 140):                                                  # more than one wavefront of survivors, in order
        lg[0, k, 1] = 1.0 + 0.01 * k
    lg[1, 1:, :] = -6.0                                                        # tile 1: one survivor in LOCAL
    return tiles, ref, lg, q


def _op_expected(ref, sig, tiles, conf, mode, full):
    out = []
    for i, t in enumerate(tiles):
        w, h = np.float32(t[2] - t[0]), np.float32(t[3] - t[1])
        b = ref[i, :, 4:8]
        best = sig[i].max(-1)
        cls = sig[i].argmax(-1).astype(np.float32)                 # first maximum, as the kernel's strict >
        dw, dh = b[:, 2] / np.float32(2), b[:, 3] / np.float32(2)
        rows = np.stack([(b[:, 0] - dw) * w, (b[:, 1] - dh) * h, (b[:, 0] + dw) * w, (b[:, 1] + dh) * h, best, cls], 1).astype(np.float32)
        rows = rows[best > np.float32(conf)]
        out.append(T.sahi_rows(rows, t, *full) if mode == "sahi" else rows)
    return out


@pytest.mark.parametrize("mode", ["local", "sahi"])
def test_op_rt_post_tiles(gpu_lib, mode):
    tiles, ref, lg, q = _op_inputs()
    full, conf = (200, 264), 0.5
    raw, _, _ = gpu_lib.op_rt_decode(ref, 4, lg, 1, 2, raw=np.zeros((3, NQ, 6), np.float32))      # the device's own sigmoid of every logit
    sig = raw[..., 4:]
    assert sig[q["on_conf"]][0] == np.float32(0.5)
    sent = np.full((3, NQ, 6), -7.0, np.float32)
    det, counts = gpu_lib.op_rt_post_tiles(ref, 4, lg, 1, 2, conf, tiles, full, mode, det=sent)
    want = _op_expected(ref, sig, tiles, conf, mode, full)
    for i in range(3):
        assert counts[i] == len(want[i]), f"tile {i}"
        assert np.array_equal(det[i, :counts[i]], want[i]), f"tile {i}"            # bit for bit, query order
        assert (det[i, counts[i]:] == -7.0).all()                                  # rows past the count untouched
    # the branches the inputs were built for
    loc = _op_expected(ref, sig, tiles, conf, "local", full)
    kept_local = lambda name: int((np.flatnonzero(sig[q[name][0]].max(-1) > np.float32(conf)) == q[name][1]).any())
    assert kept_local("left_of_crop") and kept_local("zero_width") and not kept_local("on_conf")
    if mode == "sahi":
        assert len(want[0]) == len(loc[0]) - 2                                     # left_of_crop and zero_width dropped, nothing else
        assert len(want[1]) == 1 and want[1][0, 2] > 264 - 1 and want[1][0, 2] <= 264 + 96     # not clipped to the crop; shifted, no second clip
        r0 = want[0]
        assert (r0[:, 0] >= 40).all() and (r0[:, 0] == 40).any() and (r0[:, 1] == 8).any()     # negative corners clamped to 0, then shifted
        ff = want[2]
        assert (ff[:, 2] == 264).any() and (ff[:, 3] == 200).any() and (ff[:, 0] == 0).any()
    else:
        assert (loc[0][:, 0] < 0).any() and (loc[0][:, 2] < 0).any()
    assert (want[0][:, 5] == 1).sum() == 1 and len(want[0]) > 40
    # a tile without survivors
    lg0 = lg.copy()
    lg0[1] = -6.0
    _, c0 = gpu_lib.op_rt_post_tiles(ref, 4, lg0, 1, 2, conf, tiles, full, mode)
    assert c0[1] == 0 and c0[0] == counts[0] and c0[2] == counts[2]


def test_sahi_mode_on_the_network(det, frame, tl, conf, local):
    got = det.infer_tiles(frame, tl, T.IMGSZ, conf, "sahi", max_batch=3)
    _same(got, [T.sahi_rows(r, t, T.H, T.W) for r, t in zip(local, tl)])


@pytest.fixture(scope="module")
def grid_rows(gpu_lib, det, frame, conf):
    g = [[int(v) for v in t] for t in gpu_lib.slice_bboxes(T.H, T.W, 96, 96, 0.25, 0.25)] + [[0, 0, T.W, T.H]]
    rows = det.infer_tiles(frame, g, T.IMGSZ, conf, "sahi")
    return np.concatenate(rows, 0)


@pytest.mark.parametrize("pp", [("NMS", "IOU", 0.5), ("GREEDYNMM", "IOS", 0.5)])
def test_fused_equals_staged(gpu_lib, det, frame, conf, grid_rows, pp):
    want, _ = gpu_lib.merge(grid_rows, pp[0], pp[1], pp[2])
    got = det.sliced_predict(frame, 96, 96, 0.25, 0.25, True, T.IMGSZ, conf, pp[0], pp[1], pp[2])
    assert 1 < len(want) < len(grid_rows)
    assert got.shape == want.shape and np.array_equal(got, want)
    again = det.sliced_predict(frame, 96, 96, 0.25, 0.25, True, T.IMGSZ, conf, pp[0], pp[1], pp[2])       # graph replay
    assert np.array_equal(again, got)


def test_single_slice(det, frame, conf):
    """One slice: no full-frame pass and no merge (a merge at threshold 0.01 would remove boxes and order the rest by score)."""
    small = np.ascontiguousarray(frame[:96, :96])
    got = det.sliced_predict(small, 96, 96, 0.25, 0.25, True, T.IMGSZ, conf, "NMS", "IOU", 0.01)
    want = det.infer_tiles(small, [[0, 0, 96, 96]], T.IMGSZ, conf, "sahi")[0]
    assert len(want) > 1 and np.array_equal(got, want)
    merged, _ = det_merge(want)
    assert len(merged) < len(want)                    # the inputs would have shown a merge


def det_merge(rows):
    from ffp_amd import _lib
    return _lib.merge(rows, "NMS", "IOU", 0.01)


def test_f32x3_against_reference(gpu_lib, w1, frame, tl, conf):
    """FFP_PREC_F32X3 per tile against rtdetr_ref.predict on the host crop, by the criteria of test_gpu_rtdetr._match. The frame seed was
    checked on the CPU for near-ties at the 300th encoder score (rtdetr_tiles_common.SEED)."""
    d = gpu_lib.RTDETRDetector(w1, precision=gpu_lib.PREC_F32X3)
    got = d.infer_tiles(frame, tl, T.IMGSZ, conf, "local", max_batch=3)
    ref = R.Ref(w1, torch.float32)
    total = 0
    for g, c in zip(got, T.crops(frame, tl)):
        exp = R.predict(ref, c, T.IMGSZ, conf)
        total += len(exp)
        _match(g, exp, conf)
    assert total >= 20


def _err(gpu_lib, fn, *needles):
    with pytest.raises(gpu_lib.FfpError) as e:
        fn()
    assert e.value.code == 1, e.value
    for s in needles:
        assert s in str(e.value), str(e.value)
    return e.value


def test_argument_errors(gpu_lib, det, frame, conf, grid_rows):
    _err(gpu_lib, lambda: det.infer_tiles(frame, [[0, 0, 96, 96], [200, 0, T.W + 1, 96]], T.IMGSZ, conf), "tile 1")      # x1 > W
    _err(gpu_lib, lambda: det.infer_tiles(frame, [[10, 10, 10, 50]], T.IMGSZ, conf), "tile 0")                            # empty
    _err(gpu_lib, lambda: det.infer_tiles(frame, [[0, 0, 96, 96], [0, 0, 96, 96], [50, 60, 40, 90]], T.IMGSZ, conf), "tile 2")   # inverted
    _err(gpu_lib, lambda: det.infer_tiles(frame, np.zeros((0, 4), np.int32), T.IMGSZ, conf), "tile", "n_tiles 0")
    _err(gpu_lib, lambda: det.infer_tiles(frame, [[0, 0, 96, 96]], 300, conf), "imgsz")
    merged, _ = gpu_lib.merge(grid_rows, "GREEDYNMM", "IOS", 0.5)
    assert len(merged) >= 2
    e = _err(gpu_lib, lambda: det.sliced_predict(frame, 96, 96, 0.25, 0.25, True, T.IMGSZ, conf, cap=len(merged) - 1), f"{len(merged)} merged")
    # the untruncated count reaches the caller of the C entry
    import ctypes as C
    out, n = np.zeros((1, 6), np.float32), C.c_int32(0)
    rc = gpu_lib.lib().ffp_rtdetr_sliced_predict(det._h, frame.ctypes.data, T.H, T.W, gpu_lib.CHAN_AS_BGR, 96, 96, 0.25, 0.25, 1, T.IMGSZ, conf, 0,
                                                 gpu_lib.PP_GREEDYNMM, gpu_lib.METRIC_IOS, 0.5, 0, gpu_lib._fp(out), 1, C.byref(n))
    assert rc == 1 and n.value == len(merged)


def test_device_variant_and_chunk_plans(gpu_lib, w1, frame, tl, conf, local):
    """ffp_rtdetr_infer_tiles_dev: frame and outputs as device pointers, same rows as the host variant; seven tiles at max_batch 3 run as
    chunks of 3, 2, 2, i.e. exactly two plans on a fresh engine."""
    d = gpu_lib.RTDETRDetector(w1, precision=gpu_lib.PREC_F32)
    t = np.ascontiguousarray(np.asarray(tl, np.int32))
    d_frame = torch.from_numpy(frame).cuda()
    d_out = torch.zeros((len(tl), NQ, 6), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(len(tl), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                          # the engine works on its own stream
    for _ in range(2):                                # eager, then the captured graphs
        gpu_lib._check(gpu_lib.lib().ffp_rtdetr_infer_tiles_dev(d._h, d_frame.data_ptr(), T.H, T.W, gpu_lib.CHAN_AS_BGR, gpu_lib._ip(t), len(tl),
                                                                T.IMGSZ, conf, 0, 3, d_out.data_ptr(), d_cnt.data_ptr()))
        out, cnt = d_out.cpu().numpy(), d_cnt.cpu().numpy()
        _same([out[i, :cnt[i]] for i in range(len(tl))], local)
    assert d.mem_bytes()["plans_resident"] == 2
    d.drop_plans()
    assert d.mem_bytes() == {"plans": 0, "plans_resident": 0}


def test_fifth_plan_evicts_the_least_recently_used(gpu_lib, w1, frame, tl):
    """At most 4 plans per handle, least recently used first out (csrc/plan_cache.hpp): batches of n = 1..5 images at imgsz 128 (the smallest
    multiple of 32 with 300 encoder tokens: 256 + 64 + 16) are five plans; b_n is what the n-th adds to the resident bytes."""
    d = gpu_lib.RTDETRDetector(w1, precision=gpu_lib.PREC_F32)
    imgs = T.crops(frame, tl)
    total, b = [0], {}
    for n in range(1, 6):
        d.predict(imgs[:n], 128, 0.5)
        total.append(d.mem_bytes()["plans"])
        if n <= 4:
            assert d.mem_bytes()["plans_resident"] == n
            b[n] = total[n] - total[n - 1]
    assert d.mem_bytes()["plans_resident"] == 4                            # n = 1 went
    assert 0 < b[1] < b[2] < b[3] < b[4], b
    d.predict(imgs[:1], 128, 0.5)                                          # so this lays n = 1 out again, and n = 2 goes
    mb = d.mem_bytes()
    assert mb["plans_resident"] == 4 and mb["plans"] - total[5] == b[1] - b[2], (mb, total, b)
    d.drop_plans()
    assert d.mem_bytes() == {"plans": 0, "plans_resident": 0}

"""Operator-level parity of the SCRFD HIP kernels (csrc/scrfd_ops.hip: pools, decode, NMS) through ffp_op_scrfd_pool and
ffp_op_scrfd_post, against tests/ops_ref.py and the RetinaFace restatement of tests/scrfd_ref.py. The entry points call the launch
functions the plans call.

The engine tests run two net sizes whose maps stay even down to stride 32 and feed the pools post-ReLU values: here the maps are
odd, so the clipped ceil-mode average windows run, and all-negative, so a padding value that wins shows. The decode / NMS cases
are designed candidate by candidate. Batches are ragged (pools) or of three images with different det_scale (post), views are
channel slices of wider records, and output buffers are pre-filled with sentinels.

Error bounds follow the rule of tests/test_gpu_ops.py (exact where float32 is exact, else at most 4 x the float32 yardstick with
F32_FLOOR as the floor)."""
import numpy as np
import pytest

import ops_ref
import scrfd_ref

pytestmark = pytest.mark.gpu

F32_FLOOR = 2e-6


def _sent(rng, shape):
    return rng.integers(-1000, 1000, shape).astype(np.float32)


def _untouched(got, before, coff, c, what):
    mask = np.ones(before[0].shape[-1], bool)
    mask[coff:coff + c] = False
    for g, b in zip(got, before):
        assert np.array_equal(g[..., mask], b[..., mask]), f"{what}: values outside the output slice changed"


# ---- pools ------------------------------------------------------------------------------------------------------------------------

# ragged: the smallest image comes first and the last one has more output elements (10 x 10 x 6 for max and k = 2, 7 x 7 x 6 for
# k = 3) than the 256 one workgroup covers, so a grid sized from image 0 leaves sentinels in it
POOL_SHAPES = [(1, 1), (5, 7), (8, 6), (20, 20)]


def _pool_inputs(rng, c, cs, coff):
    xs = [(-np.abs(rng.standard_normal((h, w, c))) - 1).astype(np.float32) for h, w in POOL_SHAPES]       # all negative
    x = [np.full((h, w, cs), 9e4, np.float32) for h, w in POOL_SHAPES]
    for a, b in zip(x, xs):
        a[..., coff:coff + c] = b
    return xs, x


@pytest.mark.parametrize("px_align", [1, 32])
def test_scrfd_maxpool(gpu_lib, px_align):
    rng = np.random.default_rng(px_align)
    c, cs, coff, y_cs, y_coff = 6, 10, 2, 9, 1
    xs, x = _pool_inputs(rng, c, cs, coff)
    want = [ops_ref.scrfd_maxpool(a) for a in xs]
    assert [w.shape[:2] for w in want] == [(1, 1), (3, 4), (4, 3), (10, 10)]
    assert want[-1].size > 256 >= want[0].size
    y0 = [_sent(rng, w.shape[:2] + (y_cs,)) for w in want]
    got = gpu_lib.op_scrfd_pool(x, c, coff, y0, y_coff, True, px_align=px_align)
    _untouched(got, y0, y_coff, c, "scrfd maxpool")
    for i, (g, w) in enumerate(zip(got, want)):
        o = g[..., y_coff:y_coff + c]
        assert np.array_equal(o, w), f"image {i}"
        assert (o < 0).all()                               # the padding never wins


@pytest.mark.parametrize("px_align", [1, 32])
@pytest.mark.parametrize("k", [2, 3])
def test_scrfd_avgpool(gpu_lib, k, px_align):
    """k = 2 on 5x7 -> 3x4 has windows of 4, 2 and 1 pixels; k = 3 (the lowering takes any k up to 8) of 9, 6, 3 and 2."""
    rng = np.random.default_rng(k * 40 + px_align)
    c, cs, coff, y_cs, y_coff = 6, 10, 2, 9, 1
    xs, x = _pool_inputs(rng, c, cs, coff)
    ref = [ops_ref.scrfd_avgpool(a, k) for a in xs]
    y32 = [ops_ref.scrfd_avgpool(a, k, dtype=np.float32) for a in xs]
    if k == 2:
        assert [r.shape[:2] for r in ref] == [(1, 1), (3, 4), (4, 3), (10, 10)]
    assert ref[-1].size > 256 >= ref[0].size
    y0 = [_sent(rng, r.shape[:2] + (y_cs,)) for r in ref]
    got = gpu_lib.op_scrfd_pool(x, c, coff, y0, y_coff, False, k=k, px_align=px_align)
    _untouched(got, y0, y_coff, c, "scrfd avgpool")
    scale = max(np.abs(r).max() for r in ref)
    yard = max(np.abs(a.astype(np.float64) - r).max() for a, r in zip(y32, ref)) / scale
    err = max(np.abs(g[..., y_coff:y_coff + c].astype(np.float64) - r).max() for g, r in zip(got, ref)) / scale
    bound = max(4 * yard, F32_FLOOR)
    print(f"scrfd avgpool k{k}: float32 yardstick {yard:.3g}, device error {err:.3g}, bound {bound:.3g}")
    assert err <= bound, f"scrfd avgpool k{k}: device error {err:.3g} > bound {bound:.3g} (float32 yardstick {yard:.3g})"
    # a constant map stays constant: a clipped window divides by the pixels it has
    flat = [np.full_like(a, 3.0) for a in x]
    got = gpu_lib.op_scrfd_pool(flat, c, coff, y0, y_coff, False, k=k, px_align=px_align)
    assert all((g[..., y_coff:y_coff + c] == 3.0).all() for g in got)


# ---- decode + NMS -------------------------------------------------------------------------------------------------------------------

NET_H, NET_W, A, STRIDES = 64, 96, 2, (8, 16, 32)
SIZES = [(NET_H // s, NET_W // s) for s in STRIDES]
A_OFF = np.cumsum([0] + [h * w * A for h, w in SIZES])
S_CS, S_OFF, B_CS, B_OFF, K_CS, K_OFF = A + 6, 3, 4 * A + 4, 2, 10 * A + 5, 1
DET_SCALE = np.array([1.0, 0.5, 1.5], np.float32)
THRESH, NMS_THRESH = 0.5, 0.3


class _Heads:
    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        n = 3
        self.score = [np.full((n, h, w, S_CS), 9e4, np.float32) for h, w in SIZES]
        self.bbox = [np.full((n, h, w, B_CS), 9e4, np.float32) for h, w in SIZES]
        self.kps = [np.full((n, h, w, K_CS), 9e4, np.float32) for h, w in SIZES]
        for l, (h, w) in enumerate(SIZES):
            self.score[l][..., S_OFF:S_OFF + A] = -6 - rng.random((n, h, w, A))            # nothing passes until put()
            self.bbox[l][..., B_OFF:B_OFF + 4 * A] = rng.random((n, h, w, 4 * A)) * 3
            self.kps[l][..., K_OFF:K_OFF + 10 * A] = rng.standard_normal((n, h, w, 10 * A))
        self.rng = rng

    def put(self, im, l, y, x, a, logit, box=None, dist=None):
        """Anchor a of pixel (y, x) of level l: its logit and either the box it decodes to (crop pixels at det_scale 1, exact for
        coordinates that are multiples of stride / 8) or its four distances. Returns its anchor number."""
        s = STRIDES[l]
        self.score[l][im, y, x, S_OFF + a] = logit
        if box is not None:
            dist = [(x * s - box[0]) / s, (y * s - box[1]) / s, (box[2] - x * s) / s, (box[3] - y * s) / s]
        if dist is not None:
            self.bbox[l][im, y, x, B_OFF + 4 * a:B_OFF + 4 * a + 4] = dist
        return int(A_OFF[l] + (y * SIZES[l][1] + x) * A + a)

    def outs(self, im, raw, use_kps):
        """The graph outputs scrfd_ref.post reads, with the decode's own sigmoid as the scores."""
        o = [raw[im, A_OFF[l]:A_OFF[l + 1]].reshape(-1, 1) for l in range(3)]
        o += [self.bbox[l][im, ..., B_OFF:B_OFF + 4 * A].reshape(-1, 4) for l in range(3)]
        if use_kps:
            o += [self.kps[l][im, ..., K_OFF:K_OFF + 10 * A].reshape(-1, 10) for l in range(3)]
        return o

    def logits(self, im):
        return np.concatenate([self.score[l][im, ..., S_OFF:S_OFF + A].reshape(-1) for l in range(3)])


def _designed():
    H = _Heads(5)
    ids = {}
    # image 0 (det_scale 1): every designed group sits away from the others
    ids["pair_plus1_a"] = H.put(0, 0, 5, 5, 0, 3.0, box=[40, 40, 49, 49])     # with "+1": 50 / 150 = 0.333 > 0.3 -> the second goes;
    ids["pair_plus1_b"] = H.put(0, 0, 5, 5, 1, 2.9, box=[45, 40, 54, 49])     # without: 36 / 126 = 0.286 <= 0.3 -> it would stay
    ids["thin_a"] = H.put(0, 0, 1, 10, 0, 2.5, box=[80, 8, 80, 18])           # two boxes of width 0, 3 px apart. With "+1": areas 11, no
    ids["thin_b"] = H.put(0, 0, 1, 10, 1, 2.4, box=[83, 8, 83, 18])           # overlap, both stay; without: 0 / 0, not <= thresh -> the second goes
    ids["tie"] = [H.put(0, 0, 4, 0, 1, 2.0, box=[0, 32, 4, 36]), H.put(0, 0, 0, 0, 0, 2.0, box=[0, 0, 4, 4]), H.put(0, 0, 0, 6, 0, 2.0, box=[48, 0, 52, 4])]
    ids["half"] = H.put(0, 0, 7, 11, 1, 0.0, box=[88, 56, 92, 60])            # sigmoid(0) = 0.5 = thresh: kept (>=)
    # image 1 (det_scale 0.5): 120 boxes of 480 px on centres at most 88 x 56 px apart overlap each other by > 0.56; three small ones elsewhere
    for j in range(120):
        y, x, a = np.unravel_index(j, (8, 12, A))
        H.put(1, 0, y, x, a, 4.0 - 0.01 * j, dist=[30, 30, 30, 30])
    H.put(1, 1, 0, 0, 0, 1.0, dist=[0.1, 0.1, 0.2, 0.2]); H.put(1, 1, 3, 5, 1, 1.1, dist=[0.1, 0.1, 0.2, 0.2]); H.put(1, 2, 1, 2, 0, 1.2, dist=[0.05, 0.05, 0.1, 0.1])
    # image 2 (det_scale 1.5): 40 random candidates over the three levels
    for j in range(40):
        l = j % 3
        H.put(2, l, H.rng.integers(SIZES[l][0]), H.rng.integers(SIZES[l][1]), H.rng.integers(A), 0.1 + 3 * H.rng.random(), dist=H.rng.random(4) * 3)
    return H, ids


@pytest.fixture(scope="module")
def designed():
    return _designed()


def _run(lib, H, use_kps, cap, px_align=1):
    out0 = _sent(np.random.default_rng(cap), (3, cap, 21))
    out, counts, raw = lib.op_scrfd_post((NET_H, NET_W), A, H.score, H.bbox, H.kps if use_kps else None, (S_OFF, B_OFF, K_OFF), DET_SCALE, THRESH,
                                         NMS_THRESH, out0, strides=STRIDES, px_align=px_align, raw_scores=True)
    return out0, out, counts, raw


@pytest.mark.parametrize("px_align", [1, 32])
@pytest.mark.parametrize("use_kps", [True, False], ids=["kps", "no_kps"])
def test_scrfd_post_matches_retinaface_bit_for_bit(gpu_lib, designed, use_kps, px_align):
    """scrfd_ref.post reads sigmoid scores: it gets the decode's own (checked against the float64 sigmoid by the yardstick rule, and a
    logit of 0 must give exactly 0.5); boxes, keypoints, order and the kept set are then compared bit for bit."""
    H, ids = designed
    out0, out, counts, raw = _run(gpu_lib, H, use_kps, 64, px_align)
    for im in range(3):
        lg = H.logits(im)
        ref, y32 = ops_ref.sigmoid(lg), ops_ref.sigmoid(lg, np.float32)
        yard, err = np.abs(y32 - ref).max(), np.abs(raw[im] - ref).max()              # max |ref| <= 1
        assert err <= max(4 * yard, F32_FLOOR), f"image {im}: sigmoid error {err:.3g}, float32 yardstick {yard:.3g}"
        assert (raw[im][lg == 0] == 0.5).all() and (raw[im][lg == lg[ids['tie'][0]]] == raw[im][ids['tie'][0]]).all()
        det, kpss = scrfd_ref.post(H.outs(im, raw, use_kps), float(DET_SCALE[im]), NET_W, NET_H, THRESH, NMS_THRESH)
        k = counts[im]
        assert k == len(det), f"image {im}: kept {k}, reference {len(det)}"
        np.testing.assert_array_equal(out[im, :k, :5], det)
        np.testing.assert_array_equal(out[im, :k, 5], 0)
        kp = out[im, :k, 6:].reshape(k, 5, 3)
        np.testing.assert_array_equal(kp[..., :2], kpss if use_kps else 0)
        np.testing.assert_array_equal(kp[..., 2], 1)
        assert np.array_equal(out[im, k:], out0[im, k:]), f"image {im}: rows past the count changed"
        # the float64 restatement from the definition agrees wherever no decision is close
        keep, _, _, margins = ops_ref.scrfd_post([raw[im, A_OFF[l]:A_OFF[l + 1]] for l in range(3)], H.outs(im, raw, False)[3:6], None,
                                                 (NET_H, NET_W), float(DET_SCALE[im]), THRESH, NMS_THRESH)
        assert margins["ovr"] > 1e-5 and margins["score"] > 1e-6, f"image {im}: a decision within {margins}"      # condition on the inputs
        assert np.array_equal(raw[im][keep], det[:, 4])
    # image 0: the designed decisions
    s = lambda name: raw[0][ids[name]]
    want0 = [s("pair_plus1_a"), s("thin_a"), s("thin_b")] + [raw[0][i] for i in sorted(ids["tie"])] + [np.float32(0.5)]
    assert out[0, :counts[0], 4].tolist() == want0            # pair_plus1_b suppressed, both thin boxes kept, ties in anchor order, 0.5 kept
    tie_rows = out[0, 3:6, :4]
    assert tie_rows.tolist() == [[0, 0, 4, 4], [48, 0, 52, 4], [0, 32, 4, 36]]          # ascending anchor number, not insertion order
    assert counts[1] == 4 and out[1, 0, 4] == raw[1][0]       # the cluster of 120 collapses onto its best box
    assert counts[2] > 10


def test_scrfd_post_cap_below_the_number_kept(gpu_lib, designed):
    """Pinned: with cap below the number kept the kernel writes the first cap rows and out_counts still reports how many faces the NMS
    KEPT (7 here), so a caller sees that the list was cut (ScrfdEngine::infer_tiles turns that into FFP_ERR_ARG)."""
    H, _ = designed
    _, full, full_counts, _ = _run(gpu_lib, H, True, 64)
    out0, out, counts, _ = _run(gpu_lib, H, True, 3)
    assert full_counts.tolist()[:2] == [7, 4] and counts.tolist() == full_counts.tolist()
    for im in range(3):
        k = min(3, counts[im])
        assert np.array_equal(out[im, :k], full[im, :k]) and np.array_equal(out[im, k:], out0[im, k:])


def test_bad_arguments_are_refused_before_any_launch(gpu_lib, designed):
    H, _ = designed
    z = lambda *s: np.zeros(s, np.float32)
    calls = {
        "average window above 8": lambda: gpu_lib.op_scrfd_pool([z(9, 9, 4)], 4, 0, [z(1, 1, 4)], 0, False, k=9),
        "slice outside the record": lambda: gpu_lib.op_scrfd_pool([z(4, 4, 4)], 4, 2, [z(2, 2, 4)], 0, True),
        "cap 0": lambda: gpu_lib.op_scrfd_post((NET_H, NET_W), A, H.score, H.bbox, None, (S_OFF, B_OFF), DET_SCALE, THRESH, NMS_THRESH, z(3, 0, 21)),
        "det_scale 0": lambda: gpu_lib.op_scrfd_post((NET_H, NET_W), A, H.score, H.bbox, None, (S_OFF, B_OFF), [1.0, 0.0, 1.0], THRESH, NMS_THRESH, z(3, 4, 21)),
        "bbox values outside the record": lambda: gpu_lib.op_scrfd_post((NET_H, NET_W), A, H.score, H.bbox, None, (S_OFF, B_OFF + 5), DET_SCALE, THRESH, NMS_THRESH,
                                                                         z(3, 4, 21)),
    }
    for what, call in calls.items():
        with pytest.raises(gpu_lib.FfpError) as e:
            call()
        assert e.value.code == 1, what

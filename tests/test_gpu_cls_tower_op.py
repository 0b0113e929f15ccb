"""The fused class tower alone (ffp_op_cls_tower, csrc/conv_dwpw.hip): two launches,
    e1 = SiLU(pw0(SiLU(dw0(x))))        logits = fin(SiLU(pw1(SiLU(dw1(e1)))))
each depthwise 3x3 computed inside the loader of the 1x1 conv behind it. The depthwise outputs are never stored, so no kernel has seen their
max |value|: their fp16 hi/lo split takes its exponent from a per-image bound amax(input) * max_c sum|w_c| + max|b| (csrc/dw_bound.hpp).
The depthwise weights here are N(0, 1) * 2, an L1 norm of ~14-20 per channel: the bound sits 3-5 binades above the real maximum.

Reference: tests/ops_ref.py composed in float64. Yardstick of the error: the same composition run unfused on the device, image by image
(op_dwconv3x3 + op_conv2d in FFP_PREC_F32X3: the kernels the five-launch plan runs).

Bounds, from the arithmetic and not from what the kernel gives:
  (a) |sigmoid(logit) - sigmoid(reference)| <= 2e-4, the project's class-score bar (test_gpu_detector.py).
  (b) e1: a bound k binades above the true maximum only changes an element whose lo part becomes an fp16 subnormal; its absolute error is then
      at most 2^-25 in scaled units = 2^-38 of the bound, i.e. 2^(k - 38) of the tensor's maximum: with k <= 6 that is 2^-32, 1/256 of one fp32
      rounding of the largest element. So on the well-scaled images the fused error may exceed the unfused one only by rounding noise: factor
      1.25 on the unfused error of the same image, no absolute floor. Logits: with nc <= 4 the closing conv is an fp32 fmaf chain over 128 terms
      instead of a split-fp16 MFMA sum; both are fp32-grade but not the same sum, so the factor there is 4 (sqrt(128) roundings of 2^-24 against
      the split's 2^-22 per product). Relative to max |reference| of the image.
      Measured on MI355X (profiles/cls_tower_fused_ab.txt holds the table this test prints):
      outlier image (N(0, 1) * 2^-16 with six values of +-16), fused / unfused: e1 3.227e-07 / 3.227e-07 (128 -> 128 -> 1), 9.119e-07 / 9.119e-07
      (512 -> 128 -> 5); logits 2.442e-07 / 1.936e-07 and 4.910e-07 / 4.910e-07. On every image of every case the e1 errors agree to the printed
      digits; the largest logit ratio is 1.26 (image 7, 128 -> 128 -> 1), the largest class-score error 3.7e-06.
  (c) an image's outputs are the same bytes alone and inside the batch; (d) two runs give the same bytes;
  (e) head channels outside [64, 64 + nc) come back as they went in, and no word of the padding pixels of e1, of the stored second tensor (nc = 5)
      or of the head record changed: the images 5 x 7, 17 x 33 and 9 x 9 leave 29, 15 and 15 pixels of padding behind them under
      px_align 32, which the op entry fills with a pattern and reads back (its `stray` count). With nc = 5 the head record
      is written by the plain 1x1 conv, whose flat-pixel kernels compute padding pixels like any pixel (Level::build): the count then covers e1 and e2."""
import numpy as np
import pytest

import ops_ref

pytestmark = pytest.mark.gpu

SCORE_BAR = 2e-4
E1_FACTOR, LOGIT_FACTOR = 1.25, 4.0
C3 = 128

# smaller than a 16 x 16 tile; exactly one tile; one row and one column past a tile edge; several tiles
PLAIN = [(5, 7), (16, 16), (17, 33), (32, 48)]


def _batch(rng, cin):
    """-> (images, kinds). kinds: 'plain' N(0, 1); 'zero'; 'small' / 'large' the same values 2^20 apart; 'outlier' N(0, 1) * 2^-16 with a few 2^4."""
    xs = [rng.standard_normal((h, w, cin)).astype(np.float32) for h, w in PLAIN]
    kinds = ["plain"] * len(PLAIN)
    xs.append(np.zeros((8, 8, cin), np.float32)); kinds.append("zero")
    base = rng.standard_normal((9, 9, cin)).astype(np.float32)
    xs.append(base * np.float32(2.0 ** -20)); kinds.append("small")
    xs.append(base.copy()); kinds.append("large")
    o = (rng.standard_normal((16, 20, cin)) * 2.0 ** -16).astype(np.float32)
    idx = rng.integers(0, o.size, 6)
    o.reshape(-1)[idx] = np.float32(16.0) * rng.choice([-1.0, 1.0], 6).astype(np.float32)
    xs.append(o); kinds.append("outlier")
    return xs, kinds


def _weights(rng, cin, nc):
    dw = lambda c: ((rng.standard_normal((c, 3, 3)) * 2.0).astype(np.float32), (rng.standard_normal(c) * 0.1).astype(np.float32))
    pw = lambda co, ci: ((rng.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32), (rng.standard_normal(co) * 0.1).astype(np.float32))
    return {"dw0": dw(cin), "pw0": pw(C3, cin), "dw1": dw(C3), "pw1": pw(C3, C3), "fin": pw(nc, C3)}


def _reference(x, W):
    f = lambda a: np.asarray(a, np.float64)
    d1 = ops_ref.dwconv3x3(x, W["dw0"][0], W["dw0"][1], act=1)
    e1 = ops_ref.act_fn(d1 @ f(W["pw0"][0]).T + f(W["pw0"][1]), 1)
    d2 = ops_ref.dwconv3x3(e1, W["dw1"][0], W["dw1"][1], act=1)
    e2 = ops_ref.act_fn(d2 @ f(W["pw1"][0]).T + f(W["pw1"][1]), 1)
    return e1, e2 @ f(W["fin"][0]).T + f(W["fin"][1])


def _unfused(lib, x, W):
    """One image through today's kernels: depthwise (fp32) + 1x1 (fp32 split), five launches."""
    def dwc(a, w, b):
        c = a.shape[2]
        return lib.op_dwconv3x3([a], c, 0, w, b, [np.zeros_like(a)], 0, act=1)[0]
    def pwc(a, w, b, act):
        return lib.op_conv2d(a[None], w[:, :, None, None], b, act=act, precision=lib.PREC_F32X3)[0]
    e1 = pwc(dwc(x, *W["dw0"]), *W["pw0"], 1)
    e2 = pwc(dwc(e1, *W["dw1"]), *W["pw1"], 1)
    return e1, pwc(e2, *W["fin"], 0)


def _fused(lib, xs, W, heads, nc):
    return lib.op_cls_tower(xs, W["dw0"], W["pw0"], W["dw1"], W["pw1"], W["fin"], heads, 64, px_align=32)


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("cin,nc", [(128, 1), (128, 3), (128, 5), (512, 1), (512, 3), (512, 5)])
def test_cls_tower(gpu_lib, cin, nc):
    rng = np.random.default_rng(1000 * cin + nc)
    xs, kinds = _batch(rng, cin)
    W = _weights(rng, cin, nc)
    head_cs = 64 + nc + 3
    heads0 = [rng.integers(-1000, 1000, (x.shape[0], x.shape[1], head_cs)).astype(np.float32) for x in xs]
    e1, heads, stray = _fused(gpu_lib, xs, W, [h.copy() for h in heads0], nc)
    assert stray == 0, f"{stray} words of padding pixels changed"
    # (d) determinism
    e1_b, heads_b, _ = _fused(gpu_lib, xs, W, [h.copy() for h in heads0], nc)
    for i in range(len(xs)):
        assert np.array_equal(e1[i], e1_b[i]) and np.array_equal(heads[i], heads_b[i]), f"image {i}: two runs differ"
    print(f"\ncls tower {cin} -> 128 -> {nc}: relative max error against float64   e1 fused / unfused      logits fused / unfused      max score error")
    for i, (x, kind) in enumerate(zip(xs, kinds)):
        ref_e1, ref_lg = _reference(x, W)
        un_e1, un_lg = _unfused(gpu_lib, x, W)
        lg = heads[i][..., 64:64 + nc]
        assert np.isfinite(e1[i]).all() and np.isfinite(lg).all(), f"image {i} ({kind})"
        ef, eu = _rel(e1[i], ref_e1), _rel(un_e1, ref_e1)
        lf, lu = _rel(lg, ref_lg), _rel(un_lg, ref_lg)
        score = float(np.abs(ops_ref.sigmoid(lg) - ops_ref.sigmoid(ref_lg)).max())
        print(f"  image {i} {x.shape[0]:2d}x{x.shape[1]:2d} {kind:8s} e1 {ef:.3e} / {eu:.3e}   logits {lf:.3e} / {lu:.3e}   score {score:.3e}")
        # (a)
        assert score <= SCORE_BAR, f"image {i} ({kind}): class score off by {score}"
        # (b) on the well-scaled images; the others are reported above and held by (a)
        if kind in ("plain", "large", "small"):
            assert ef <= E1_FACTOR * eu, f"image {i} ({kind}): e1 error {ef} against {eu} unfused"
            assert lf <= LOGIT_FACTOR * lu, f"image {i} ({kind}): logit error {lf} against {lu} unfused"
        # (e)
        keep = np.ones(head_cs, bool)
        keep[64:64 + nc] = False
        assert np.array_equal(heads[i][..., keep], heads0[i][..., keep]), f"image {i}: head channels outside the class slice changed"
        # (c) the image alone
        a_e1, a_head, a_stray = _fused(gpu_lib, [x], W, [heads0[i].copy()], nc)
        assert a_stray == 0, f"image {i} alone: {a_stray} words of padding pixels changed"
        assert np.array_equal(a_e1[0], e1[i]), f"image {i} ({kind}): e1 depends on the batch mates"
        assert np.array_equal(a_head[0], heads[i]), f"image {i} ({kind}): logits depend on the batch mates"


def test_cls_tower_refuses_what_the_kernel_cannot_run(gpu_lib):
    rng = np.random.default_rng(5)
    W = _weights(rng, 128, 1)
    x = [rng.standard_normal((8, 8, 128)).astype(np.float32)]
    head = [np.zeros((8, 8, 68), np.float32)]
    with pytest.raises(gpu_lib.FfpError) as e:
        gpu_lib.op_cls_tower(x, W["dw0"], W["pw0"], W["dw1"], W["pw1"], W["fin"], head, 64, px_align=1)      # one exponent per image needs aligned images
    assert e.value.code == 1

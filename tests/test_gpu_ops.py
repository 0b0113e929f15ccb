"""Operator-level parity of the detector's non-convolution HIP kernels (csrc/ops_misc.hip, csrc/det_post.hip, rt_topk of
csrc/rtdetr_ops.hip) through the single-operator entry points ffp_op_*, against the float64 references of tests/ops_ref.py.

Every kernel variant runs every case it can take (ffp_op_variant pins it in-process): SPPF LDS / direct, attention MFMA / VALU,
depthwise column-walk / strip. Views are channel slices of wider buffers as in the plans, batches are ragged, and the device
layout pads images to a pixel alignment, so the inter-image addressing is exercised as well.

Error bounds that are not exact follow one rule: the yardstick is a plain float32 numpy evaluation of the same formula against
the float64 reference (max abs error / max |reference|); the device may be at most 4 x the yardstick — the kernels sum in
another order and the online softmax rescales once per 32-key block — with a floor for cases where the yardstick is (almost)
exact. Messages carry both figures."""
import numpy as np
import pytest

import ops_ref

pytestmark = pytest.mark.gpu

F32_FLOOR = 2e-6                     # the fp32-grade floor of test_f32x3_scaled_split_is_fp32_grade_over_ranges
F16_OUT = 2.0 ** -11                 # one rounding of the output to fp16, relative


def _prec(lib, half):
    return lib.PREC_F16 if half else lib.PREC_F32


def _h(a, half):
    """What the device stores of a host array: itself, or its fp16 rounding."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):                 # guard values around a slice become inf in fp16: still guards
        return a.astype(np.float16).astype(np.float32) if half else a


def _sentinel(rng, shapes, cs):
    """Output buffers filled with small integers (exact in fp16): what must come back outside the written slices."""
    return [rng.integers(-1000, 1000, (h, w, cs)).astype(np.float32) for h, w in shapes]


class _variants:
    """Runs the body once per named variant of a family, restoring the automatic choice afterwards."""
    def __init__(self, lib, family, names):
        self.lib, self.family, self.names = lib, family, names

    def __iter__(self):
        try:
            for n in self.names:
                self.lib.op_variant(self.family, n)
                yield n or "auto"
        finally:
            self.lib.op_variant(self.family, 0)


def _untouched(got, before, slices, what):
    mask = np.ones(before[0].shape[2], bool)
    for o, c in slices:
        mask[o:o + c] = False
    for g, b in zip(got, before):
        assert np.array_equal(g[..., mask], b[..., mask]), f"{what}: values outside the output slices changed"


# ---- SPPF -------------------------------------------------------------------------------------------------------------------

def _sppf_input(rng, h, w, c):
    # everything far below zero (a 0 standing in for the -inf padding would win every border window), the border rows and
    # columns hold the maxima of their rows / columns
    x = rng.standard_normal((h, w, c)) * 3 - 1000
    x[0] += 40; x[-1] += 45; x[:, 0] += 50; x[:, -1] += 55
    return x.astype(np.float32)


SPPF_BATCHES = {
    "1x1": [(1, 1)], "1x13": [(1, 13)], "7x5": [(7, 5)], "16x16": [(16, 16)], "20x20": [(20, 20)], "32x32": [(32, 32)],
    "33x32": [(33, 32)], "40x40": [(40, 40)], "ragged": [(7, 5), (16, 16), (1, 13), (32, 32)], "mixed": [(16, 16), (40, 40), (3, 3)],
}


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("c", [4, 256])
@pytest.mark.parametrize("name", list(SPPF_BATCHES))
def test_sppf_pool(gpu_lib, name, c, half):
    shapes = SPPF_BATCHES[name]
    rng = np.random.default_rng(len(name) * 131 + c)
    x_cs, x_coff, y_cs = c + 8, 4, 3 * c + 16
    offs = (c + 8, 4, 2 * c + 12)                    # y1, y2, y3: out of order, gaps of 4 channels around each
    x = [np.concatenate([np.full((h, w, 4), 9e4, np.float32), _sppf_input(rng, h, w, c), np.full((h, w, 4), 9e4, np.float32)], 2) for h, w in shapes]
    y0 = _sentinel(rng, shapes, y_cs)
    want = [ops_ref.sppf_pool(_h(a[..., x_coff:x_coff + c], half)) for a in x]
    lds_ok = max(h * w for h, w in shapes) <= 1024
    outs = {}
    for v in _variants(gpu_lib, gpu_lib.OP_SPPF, (["lds"] if lds_ok else []) + ["direct", 0]):
        got = gpu_lib.op_sppf_pool(x, c, x_coff, y0, offs, px_align=32 if len(shapes) > 1 else 1, precision=_prec(gpu_lib, half))
        _untouched(got, y0, [(o, c) for o in offs], f"sppf {v}")
        for i, g in enumerate(got):
            for k in range(3):
                assert np.array_equal(g[..., offs[k]:offs[k] + c], want[i][k]), f"sppf {v}: image {i} y{k + 1} differs from {k + 1} chained max pools"
        outs[v] = got
    if lds_ok:
        assert all(np.array_equal(a, b) for a, b in zip(outs["lds"], outs["direct"]))
    else:
        gpu_lib.op_variant(gpu_lib.OP_SPPF, "lds")
        try:
            with pytest.raises(gpu_lib.FfpError) as e:     # refused before any launch
                gpu_lib.op_sppf_pool(x, c, x_coff, y0, offs, precision=_prec(gpu_lib, half))
            assert e.value.code == 1
        finally:
            gpu_lib.op_variant(gpu_lib.OP_SPPF, 0)


# ---- nearest x2 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("px_align", [1, 32])
def test_upsample2x(gpu_lib, half, px_align):
    shapes = [(1, 1), (3, 5), (8, 8), (2, 7)]
    rng = np.random.default_rng(7)
    c, x_cs, x_coff, y_cs, y_coff = 8, 24, 8, 32, 16
    x = [_h(rng.standard_normal((h, w, x_cs)), half) for h, w in shapes]
    y0 = _sentinel(rng, [(2 * h, 2 * w) for h, w in shapes], y_cs)
    got = gpu_lib.op_upsample2x(x, c, x_coff, y0, y_coff, px_align=px_align, precision=_prec(gpu_lib, half))
    _untouched(got, y0, [(y_coff, c)], "upsample")
    for a, g in zip(x, got):
        assert np.array_equal(g[..., y_coff:y_coff + c], ops_ref.upsample2x(a[..., x_coff:x_coff + c]))


# ---- depthwise 3x3 --------------------------------------------------------------------------------------------------------

DW_CASES = [
    # id, shapes, C, act, residual
    ("c128_16x16", [(16, 16)] * 2, 128, 1, False), ("c256_9x16_res", [(9, 16)] * 2, 256, 0, True), ("c64_33x17", [(33, 17)] * 2, 64, 1, False),
    ("1x1", [(1, 1)], 8, 1, False), ("1x9", [(1, 9)], 8, 2, True), ("9x1", [(9, 1)], 8, 3, False), ("33x17_relu_res", [(33, 17)], 8, 3, True),
    ("ragged_lrelu", [(5, 7), (1, 1), (16, 16), (3, 21), (9, 2)], 16, 2, True), ("ragged_silu", [(2, 3), (17, 33), (4, 4)], 32, 1, False),
]


def _dw_check(lib, got, want, half, what):
    for i, (g, r) in enumerate(zip(got, want)):
        tol = 2e-3 if half else 2e-5
        err = np.abs(g - r).max()
        assert np.all(np.abs(g - r) <= tol + tol * np.abs(r)), f"{what}: image {i} max abs error {err:.3g} (tolerance {tol:g} abs + rel)"


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("case", DW_CASES, ids=[c[0] for c in DW_CASES])
def test_dwconv3x3(gpu_lib, case, half):
    _, shapes, c, act, has_res = case
    rng = np.random.default_rng(c * 7 + len(shapes))
    x_cs, x_coff, y_cs, y_coff, r_cs, r_coff = c + 8, 4, c + 12, 8, c + 4, 4
    x = [_h(rng.standard_normal((h, w, x_cs)), half) for h, w in shapes]
    res = [_h(rng.standard_normal((h, w, r_cs)), half) for h, w in shapes] if has_res else None
    wt = (rng.standard_normal((c, 3, 3)) / 3).astype(np.float32)
    b = (rng.standard_normal(c) * 0.1).astype(np.float32)
    y0 = _sentinel(rng, shapes, y_cs)
    want = [ops_ref.dwconv3x3(a[..., x_coff:x_coff + c], wt, b, act, res[i][..., r_coff:r_coff + c] if has_res else None) for i, a in enumerate(x)]
    outs = {}
    for v in _variants(gpu_lib, gpu_lib.OP_DWCONV, ["col", "strip", 0]):
        got = gpu_lib.op_dwconv3x3(x, c, x_coff, wt, b, y0, y_coff, act=act, res=res, r_coff=r_coff, px_align=32 if len(shapes) > 2 else 1,
                                   precision=_prec(gpu_lib, half))
        _untouched(got, y0, [(y_coff, c)], f"dwconv {v}")
        _dw_check(gpu_lib, [g[..., y_coff:y_coff + c] for g in got], want, half, f"dwconv {v}")
        outs[v] = got
    # the file header of ops_misc.hip claims the two kernels are bit-identical
    assert all(np.array_equal(a, b_) for a, b_ in zip(outs["col"], outs["strip"]))
    assert all(np.array_equal(a, b_) for a, b_ in zip(outs["col"], outs["auto"]))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("nh", [2, 4])
def test_dwconv3x3_reads_v_in_place_from_the_psa_records(gpu_lib, nh, half):
    """The PSA positional conv: its nh*64 channels are the v blocks of nh [q(32) | k(32) | v(64)] records, read in place
    (grp 64, grp_stride 128, grp_off 64) from a qkv view that itself starts inside a wider buffer; the residual is the
    attention output."""
    shapes = [(13, 20), (1, 1), (4, 8)]
    rng = np.random.default_rng(nh)
    c, x_coff = nh * 64, 8
    x_cs = x_coff + nh * 128 + 4
    x = [_h(rng.standard_normal((h, w, x_cs)), half) for h, w in shapes]
    res = [_h(rng.standard_normal((h, w, c)), half) for h, w in shapes]
    wt = (rng.standard_normal((c, 3, 3)) / 3).astype(np.float32)
    b = (rng.standard_normal(c) * 0.1).astype(np.float32)
    y0 = _sentinel(rng, shapes, c + 4)
    want = [ops_ref.dwconv3x3(ops_ref.grouped_gather(a, c, x_coff, 64, 128, 64), wt, b, 0, r) for a, r in zip(x, res)]
    outs = {}
    for v in _variants(gpu_lib, gpu_lib.OP_DWCONV, ["col", "strip"]):
        got = gpu_lib.op_dwconv3x3(x, c, x_coff, wt, b, y0, 4, grp=64, grp_stride=128, grp_off=64, res=res, px_align=32, precision=_prec(gpu_lib, half))
        _untouched(got, y0, [(4, c)], f"grouped dwconv {v}")
        _dw_check(gpu_lib, [g[..., 4:] for g in got], want, half, f"grouped dwconv {v}")
        outs[v] = got
    assert all(np.array_equal(a, b_) for a, b_ in zip(outs["col"], outs["strip"]))


# ---- attention ----------------------------------------------------------------------------------------------------------------

ATTN_MAPS = {1: (1, 1), 31: (1, 31), 32: (4, 8), 33: (3, 11), 63: (7, 9), 64: (8, 8), 65: (5, 13), 127: (1, 127), 128: (8, 16), 129: (3, 43),
             260: (13, 20), 400: (20, 20), 1024: (32, 32)}
ATTN_KINDS = ["unit", "logits80", "one_key", "v_offset"]
ATTN_TABLE = []                      # (case, variant, precision, yardstick, device error, bound): printed by the last test of the group


def _attn_input(rng, h, w, nh, kind):
    t = rng.standard_normal((h * w, nh, 128))
    if kind == "logits80":           # q, k ~ N(0, 4.5^2): logits q.k / sqrt(32) have sigma 20 and reach +-80 over the N^2 pairs
        t[:, :, :64] *= 4.5
    elif kind == "one_key":          # every query has a component along one key: its logit leads the others by 2 * 1.5 * 32 / sqrt(32) = 17
        j = (h * w) // 2             # (the rest keep a weight of 1e-5 or so: the key dominates without the softmax saturating to exactly 1)
        t[:, :, :32] += 2.0
        t[j, :, 32:64] += 1.5
    elif kind == "v_offset":
        t[:, :, 64:] += 1000.0
    return t.reshape(h, w, nh * 128)


def _attn_run(lib, shapes, nh, kind, seed, label):
    rng = np.random.default_rng(seed)
    q_coff, o_coff = 4, 8
    q_cs, o_cs = nh * 128 + 8, nh * 64 + 12
    fails = []
    for half in (False, True):
        qkv = [_h(np.concatenate([np.full((h, w, 4), 7e4), _attn_input(rng, h, w, nh, kind), np.full((h, w, 4), 7e4)], 2), half) for h, w in shapes]
        ref = [ops_ref.psa_attention(a[..., q_coff:q_coff + nh * 128].astype(np.float64), nh) for a in qkv]
        y32 = [ops_ref.psa_attention(a[..., q_coff:q_coff + nh * 128], nh, dtype=np.float32) for a in qkv]
        assert all(np.isfinite(r).all() for r in ref)
        scale = max(np.abs(r).max() for r in ref)
        yard = max(np.abs(a.astype(np.float64) - r).max() for a, r in zip(y32, ref)) / scale
        bound = max(4 * yard, F32_FLOOR) + (F16_OUT if half else 0.0)
        out0 = _sentinel(rng, shapes, o_cs)
        for v in _variants(lib, lib.OP_ATTENTION, ["mfma", "valu"]):
            got = lib.op_psa_attention(qkv, nh, q_coff, out0, o_coff, px_align=32 if len(shapes) > 1 else 1, precision=_prec(lib, half))
            _untouched(got, out0, [(o_coff, nh * 64)], f"attention {v}")
            o = [g[..., o_coff:o_coff + nh * 64] for g in got]
            assert all(np.isfinite(a).all() for a in o), f"{label} {v}: output not finite"
            err = max(np.abs(a.astype(np.float64) - r).max() for a, r in zip(o, ref)) / scale
            ATTN_TABLE.append((label, v, "f16" if half else "f32", yard, err, bound))
            if not err <= bound:
                fails.append(f"{label} {v} {'f16' if half else 'f32'}: device error {err:.3g} > bound {bound:.3g} (float32 yardstick {yard:.3g})")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", ATTN_KINDS)
@pytest.mark.parametrize("nh", [2, 4])
@pytest.mark.parametrize("n", list(ATTN_MAPS))
def test_psa_attention(gpu_lib, n, nh, kind):
    """Finding of this test, fixed with it: the VALU kernel added the keys to its output accumulator one by one, and at N = 1024
    with one dominating key (a large term early, then hundreds of small ones each rounded at the accumulator's ulp) its fp32
    error was 5.21e-06 (nh 2) / 5.49e-06 (nh 4) of max |ref| against float32 yardsticks of 1.11e-06 / 1.00e-06: 4.7 x and 5.5 x,
    over the 4 x allowed (unit-variance and v-offset inputs sat at 0.98 of the bound). psa_attention_kernel now sums each
    64-key block by itself and folds it into the running sums once per block, like the MFMA kernel; the MFMA kernel, which every
    plan uses, was inside the bound and is unchanged."""
    _attn_run(gpu_lib, [ATTN_MAPS[n]], nh, kind, n * 8 + nh, f"N={n} nh={nh} {kind}")


@pytest.mark.parametrize("kind", ATTN_KINDS)
def test_psa_attention_ragged_batch(gpu_lib, kind):
    _attn_run(gpu_lib, [(3, 11), (20, 20), (1, 1), (3, 11)], 2, kind, 5, f"N=33|400|1|33 nh=2 {kind}")


def test_psa_attention_error_table(gpu_lib):
    """Prints the measured yardstick / device error of every attention case above (run with -s); asserts nothing new."""
    print("\ncase | variant | storage | float32 yardstick | device error | bound")
    for row in ATTN_TABLE:
        print("%s | %s | %s | %.3g | %.3g | %.3g" % row)


# ---- Pose-head decode -----------------------------------------------------------------------------------------------------------

def _geom(sh, sw, imgsz):
    """Ultralytics LetterBox(auto) + scale_boxes geometry of a (sh x sw) crop: (net_h, net_w), (gain, pad_x, pad_y, sw, sh)."""
    r = min(imgsz / sh, imgsz / sw)
    nw, nh_ = int(round(sw * r)), int(round(sh * r))
    dw, dh = (imgsz - nw) % 32, (imgsz - nh_) % 32
    net_h, net_w = nh_ + dh, nw + dw
    gain = min(net_h / sh, net_w / sw)
    return (net_h, net_w), (gain, round((net_w - sw * gain) / 2 - 0.1), round((net_h - sh * gain) / 2 - 0.1), sw, sh)


# (crop h, crop w, imgsz, x0, y0): gains 0.5 (down-scaling, padded rows), 2 (up-scaling, padded rows), 1.25 (up-scaling, padded
# rows, not a power of two), 1 — all exact in fp32, so the reference's float64 gain is the device's
CROPS = [(160, 256, 128, 0, 0), (40, 64, 128, 100, 30), (96, 128, 160, 7, 300), (64, 64, 64, 32, 32)]


def _random_heads(rng, net_hw, nc, nkpt):
    cs = 64 + nc + 3 * nkpt
    return [(rng.standard_normal((net_hw[0] // s, net_hw[1] // s, cs)) * 2).astype(np.float32) for s in (8, 16, 32)]


PX_ROWS_FLOOR = 2.0 ** -13           # one fp32 ulp at 1024 px


def _decode_groups(nc, nkpt):
    px = [0, 1, 2, 3] + [4 + nc + 3 * k + d for k in range(nkpt) for d in (0, 1)]
    pr = list(range(4, 4 + nc)) + [4 + nc + 3 * k + 2 for k in range(nkpt)]
    return np.asarray(px), np.asarray(pr)


def _decode_bounds(levels, nc, nkpt):
    """(ref64, {group: (rows, yardstick abs, bound abs)}): pixel rows (boxes, keypoint x / y) with the floor of one fp32 ulp at
    1024 px; probability rows (class and visibility sigmoids) with the fp32-grade floor — expf and the division are a few ulp
    each on the device, the float32 yardstick is correctly rounded."""
    ref = ops_ref.head_decode(levels, nc, nkpt)
    y32 = ops_ref.head_decode(levels, nc, nkpt, dtype=np.float32).astype(np.float64)
    px, pr = _decode_groups(nc, nkpt)
    out = {}
    for name, rows, floor in (("pixels", px, PX_ROWS_FLOOR), ("probabilities", pr, F32_FLOOR)):
        scale = np.abs(ref[rows]).max()
        yard = np.abs(y32[rows] - ref[rows]).max()
        out[name] = (rows, yard, max(4 * yard, floor if name == "pixels" else floor * scale))
    return ref, out


DECODE_TABLE = []


@pytest.mark.parametrize("px_align", [1, 32])
@pytest.mark.parametrize("nc,nkpt", [(1, 5), (1, 0), (3, 5), (3, 0)])
def test_decode_raw(gpu_lib, nc, nkpt, px_align):
    rng = np.random.default_rng(nc * 10 + nkpt)
    nets = [_geom(*c[:3])[0] for c in CROPS]
    heads = [_random_heads(rng, hw, nc, nkpt) for hw in nets]
    raws, _, _ = gpu_lib.op_det_post(heads, nc, nkpt, [(1, 0, 0, 1, 1, 0, 0)] * len(heads), nms=False, px_align=px_align)
    fails = []
    for i, (lv, got) in enumerate(zip(heads, raws)):
        ref, groups = _decode_bounds(lv, nc, nkpt)
        assert got.shape == ref.shape
        for name, (rows, yard, bound) in groups.items():
            err = np.abs(got[rows].astype(np.float64) - ref[rows]).max()
            DECODE_TABLE.append((f"nc={nc} nkpt={nkpt} align={px_align} image {i} ({nets[i][1]}x{nets[i][0]})", name, yard, err, bound))
            if not err <= bound:
                fails.append(f"image {i} {name}: device error {err:.3g} > bound {bound:.3g} (float32 yardstick {yard:.3g})")
    assert not fails, "\n".join(fails)


def test_decode_raw_error_table(gpu_lib):
    """Prints the measured yardstick / device error (absolute) of the decode cases above (run with -s); asserts nothing new."""
    print("\ncase | rows | float32 yardstick | device error | bound")
    for row in DECODE_TABLE:
        print("%s | %s | %.3g | %.3g | %.3g" % row)


# ---- NMS: heads whose decode is exact in fp32, decisions with wide margins, exact agreement required ------------------------------------

LOGITS = np.array([-1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 3.0])     # class logits of candidates: scores tie exactly within a value
COLD = -6.0                                                  # sigmoid = 0.0025: never a candidate at conf 0.25
CONF, IOU = 0.25, 0.7


def exact_heads(rng, net_hw, nc, nkpt, cand, logits, cls, dists):
    """Heads of one image. cand: anchor indices (level-major, row-major) that become candidates; logits / cls: their class logit
    and class; dists (len(cand), 4): integer DFL bins left, top, right, bottom, one-hot at +30 over -30: the softmax expectation
    is the bin exactly in float32 and in float64, so box sides are integers times the stride. Every other anchor is cold."""
    cs = 64 + nc + 3 * nkpt
    sizes = [(net_hw[0] // s) * (net_hw[1] // s) for s in (8, 16, 32)]
    A = sum(sizes)
    flat = np.full((A, cs), -30.0, np.float32)
    flat[:, 0:64:16] = 30.0                                   # bin 0 on every side of the cold anchors
    flat[:, 64:64 + nc] = COLD - 2.0
    flat[:, 64] = COLD
    if nkpt:
        flat[:, 64 + nc:] = (rng.standard_normal((A, 3 * nkpt)) * 2).astype(np.float32)
    cand = np.asarray(cand)
    for k in range(4):
        flat[cand, 16 * k] = -30.0
        flat[cand, 16 * k + np.asarray(dists)[:, k]] = 30.0
    flat[cand, 64:64 + nc] = COLD - 2.0
    flat[cand, 64 + np.asarray(cls)] = np.asarray(logits, np.float32)
    out, p = [], 0
    for s, n in zip((8, 16, 32), sizes):
        out.append(flat[p:p + n].reshape(net_hw[0] // s, net_hw[1] // s, cs))
        p += n
    return out


def scenario(name, seed, net_hw, nc, nkpt, n_cand):
    """Builds one image's heads for a named structure of candidates."""
    rng = np.random.default_rng(seed)
    sizes = [(net_hw[0] // s) * (net_hw[1] // s) for s in (8, 16, 32)]
    A = sum(sizes)
    if name == "none":
        cand = np.zeros(0, np.int64)
    elif name == "one_box_kills_all":                     # a 5 x 5 block of stride-32 anchors with 960 px boxes: IoU >= 0.77 with the centre
        h32, w32 = net_hw[0] // 32, net_hw[1] // 32
        yy, xx = np.mgrid[h32 // 2 - 2:h32 // 2 + 3, w32 // 2 - 2:w32 // 2 + 3]
        cand = sizes[0] + sizes[1] + (yy * w32 + xx).ravel()
    else:
        cand = np.sort(rng.choice(A, n_cand, replace=False))
    n = len(cand)
    cls = rng.integers(0, nc, n)
    logits = rng.choice(LOGITS, n)
    if name == "one_box_kills_all":
        dists = np.full((n, 4), 15)
        logits[:] = 1.0
        logits[n // 2] = 3.0                                  # the centre wins
    elif name == "sparse":                                    # 2 x 2 anchor cells: neighbours overlap with IoU 1/3, everything survives
        dists = np.ones((n, 4), np.int64)
    elif name == "all_tied":                                  # one score for every candidate: the kept order is the anchor order
        dists = np.ones((n, 4), np.int64)
        logits[:] = 0.5
    else:                                                     # "dense": boxes of 4..8 cells; "crowded": 8..14 cells, for a low IoU threshold
        d = rng.integers(4, 8, (n, 2)) if name == "crowded" else rng.integers(2, 5, (n, 2))
        dists = np.stack([d[:, 0], d[:, 1], d[:, 0], d[:, 1]], 1)
    if name in ("dense", "crowded", "sparse") and n:
        logits[-1] = 4.0                                      # the last candidate (the highest position of the compacted list) wins first
    return exact_heads(rng, net_hw, nc, nkpt, cand, logits, cls, dists), n


def _reference_rows(levels, nc, nkpt, geom, conf, iou, max_det, round_boxes, shift, full_hw):
    ref = ops_ref.head_decode(levels, nc, nkpt)
    keep, cls, margins = ops_ref.nms(ref, nc, conf, iou, max_det)
    rows = ops_ref.det_rows(ref, keep, cls, nc, nkpt, geom, round_boxes)
    if shift:
        rows = ops_ref.truncate_shift(rows, nkpt, geom, *full_hw)
    return ref, keep, rows, margins


def _check_nms(lib, heads, nc, nkpt, geoms, max_det, round_boxes=False, shift=False, full_hw=(0, 0), conf=CONF, iou=IOU, exact_boxes=True):
    """Runs the device post-processing and compares with the float64 reference. Returns per image (keep, candidate positions of the
    kept anchors, number of candidates)."""
    _, dets, counts = lib.op_det_post(heads, nc, nkpt, geoms, conf=conf, iou=iou, max_det=max_det, round_boxes=round_boxes, shift=shift,
                                      full_hw=full_hw, raw=False)
    info = []
    for i, lv in enumerate(heads):
        ref, keep, rows, margins = _reference_rows(lv, nc, nkpt, geoms[i], conf, iou, max_det, round_boxes, shift, full_hw)
        # the condition under which exact agreement is demanded: no decision of the reference is close
        assert margins["iou"] >= 1e-4 and margins["conf"] >= 1e-6, f"image {i}: inputs too close to a threshold {margins}"
        assert counts[i] == len(keep), f"image {i}: {counts[i]} kept, reference keeps {len(keep)}"
        d = dets[i, :len(keep)].astype(np.float64)
        assert not dets[i, len(keep):].any(), f"image {i}: rows past the count were written"
        assert np.array_equal(d[:, 5], rows[:, 5]), f"image {i}: classes differ"
        _, groups = _decode_bounds(lv, nc, nkpt)
        gain = geoms[i][0]
        if exact_boxes or round_boxes or shift:
            bad = np.flatnonzero((d[:, :4] != rows[:, :4].astype(np.float32)).any(1))
            assert bad.size == 0, f"image {i}: first differing kept row {bad[0]}: device {d[bad[0], :6]} reference {rows[bad[0], :6]}"
        else:
            assert np.abs(d[:, :4] - rows[:, :4]).max(initial=0) <= groups["pixels"][2] / gain
        assert np.abs(d[:, 4] - rows[:, 4]).max(initial=0) <= groups["probabilities"][2], f"image {i}: scores"
        if nkpt:
            k, kr = d[:, 6:].reshape(-1, nkpt, 3), rows[:, 6:].reshape(-1, nkpt, 3)
            tol_px = groups["pixels"][2] / gain + (PX_ROWS_FLOOR * 4 if shift else 0)       # + the fp32 rounding of the shifted coordinate
            assert np.abs(k[..., :2] - kr[..., :2]).max(initial=0) <= tol_px, f"image {i}: keypoints"
            assert np.abs(k[..., 2] - kr[..., 2]).max(initial=0) <= groups["probabilities"][2], f"image {i}: keypoint visibilities"
        cand = np.flatnonzero(ref[4:4 + nc].max(0) > conf)
        info.append((keep, np.searchsorted(cand, keep), len(cand)))
    return info


UNIT = (1.0, 0, 0, 640, 640, 0, 0)


@pytest.mark.parametrize("nc,nkpt", [(1, 5), (3, 0), (3, 5), (1, 0)])
def test_nms_small_cases(gpu_lib, nc, nkpt):
    """Zero candidates; every candidate suppressed by one box; a ragged batch with letterbox padding, down- and up-scaling gains."""
    heads = [scenario("none", 1, (640, 640), nc, nkpt, 0)[0], scenario("one_box_kills_all", 2, (640, 640), nc, nkpt, 0)[0]]
    info = _check_nms(gpu_lib, heads, nc, nkpt, [UNIT, UNIT], 300)
    assert info[0][2] == 0 and len(info[0][0]) == 0
    assert info[1][2] == 25 and (nc > 1 or len(info[1][0]) == 1)          # with several classes: one survivor per class present
    geoms, heads = [], []
    for j, (sh, sw, imgsz, x0, y0) in enumerate(CROPS):
        net, g = _geom(sh, sw, imgsz)
        assert float(np.float32(g[0])) == g[0]
        geoms.append(g + (x0, y0))
        heads.append(scenario("dense", 10 + j, net, nc, nkpt, 60)[0])
    for rb, sh_ in ((False, False), (True, False), (False, True)):
        info = _check_nms(gpu_lib, heads, nc, nkpt, geoms, 300, round_boxes=rb, shift=sh_, full_hw=(400, 300), exact_boxes=False)
        assert all(0 < len(k) <= n for k, _, n in info) and sum(len(k) for k, _, _ in info) < sum(n for _, _, n in info)


def test_nms_identical_boxes_of_two_classes_are_both_kept(gpu_lib):
    """Anchor a with bins (2, 2, 3, 2) and its right neighbour with (3, 2, 2, 2) decode to the same box. In different classes both
    stay (class offset 7680); in one class the later one goes."""
    rng = np.random.default_rng(0)
    a = 80 * 40 + 20
    b = 80 * 60 + 50
    cand = [a, a + 1, b, b + 1]
    dists = [[2, 2, 3, 2], [3, 2, 2, 2]] * 2
    heads = [exact_heads(rng, (640, 640), 3, 5, cand, [1.0, 2.0, 1.0, 2.0], [0, 2, 1, 1], dists)]
    info = _check_nms(gpu_lib, heads, 3, 5, [UNIT], 300)
    assert info[0][0].tolist() == [a + 1, b + 1, a]


CROWDED_IOU = 0.33       # with boxes of 8..14 cells most candidates are suppressed: fewer than 1024 survive, max_det = 1024 cuts nothing


@pytest.mark.parametrize("nc,nkpt", [(1, 5), (3, 0)])
@pytest.mark.parametrize("name,n_cand,iou", [("crowded", 2048, CROWDED_IOU), ("crowded", 2049, CROWDED_IOU), ("crowded", 6000, CROWDED_IOU), ("dense", 6000, IOU),
                                             ("sparse", 2049, IOU), ("sparse", 6000, IOU), ("all_tied", 6000, IOU)])
def test_nms_around_the_lds_capacity(gpu_lib, name, n_cand, iou, nc, nkpt):
    """One 640 x 640 image (8400 anchors) with up to, just over and far over the 2048 candidates the kernel keeps in LDS; the
    candidates past 2048 live in global scratch (scores) and are re-read from the decode output (boxes, classes)."""
    heads, n = scenario(name, n_cand, (640, 640), nc, nkpt, n_cand)
    assert n == n_cand
    # the structure of the case, on the reference without a cut: who survives, who is suppressed, on which side of position 2048
    ref = ops_ref.head_decode(heads, nc, nkpt)
    alive = np.searchsorted(np.flatnonzero(ref[4:4 + nc].max(0) > CONF), ops_ref.nms(ref, nc, CONF, iou, 10 ** 9)[0])
    dead = np.setdiff1d(np.arange(n_cand), alive)
    if name == "crowded":
        assert 100 < len(alive) < 1024 and (dead < 2048).sum() > 100
    if name in ("crowded", "dense") and n_cand == 6000:
        assert (dead >= 2048).sum() > 100 and (alive < 2048).sum() > 50 and (alive >= 2048).sum() > 50
    if name in ("sparse", "all_tied"):
        assert len(dead) == 0
    for max_det in (1, 300, 1024):
        (keep, pos, ncand), = _check_nms(gpu_lib, [heads], nc, nkpt, [UNIT], max_det, iou=iou)
        assert ncand == n_cand
        assert len(keep) == min(max_det, len(alive))              # a smaller max_det cuts the list while live candidates remain
        if name != "all_tied":
            assert pos[0] == n_cand - 1                           # the first winner sits at the highest position
        else:
            assert pos.tolist() == list(range(max_det))           # >= 70 tied scores across wave boundaries: anchor order
        if max_det >= 300 and n_cand > 2048 and name != "all_tied":
            assert (pos < 2048).any() and (pos >= 2048).any()     # winners on both sides of the LDS capacity


def test_nms_batch_where_one_image_spills(gpu_lib):
    nc, nkpt = 3, 5
    specs = [("dense", (640, 640), 1500), ("sparse", (640, 640), 3000), ("dense", (256, 256), 500), ("sparse", (96, 128), 100)]
    heads = [scenario(nm, 40 + j, hw, nc, nkpt, k)[0] for j, (nm, hw, k) in enumerate(specs)]
    geoms = [(1.0, 0, 0, hw[1], hw[0], 10 * j, 20 * j) for j, (_, hw, _) in enumerate(specs)]
    for px_align in (1, 32):
        _, dets, counts = gpu_lib.op_det_post(heads, nc, nkpt, geoms, conf=CONF, iou=IOU, max_det=300, raw=False, px_align=px_align)
        assert counts.tolist() == [len(_reference_rows(h, nc, nkpt, g, CONF, IOU, 300, False, False, (0, 0))[1]) for h, g in zip(heads, geoms)]
    info = _check_nms(gpu_lib, heads, nc, nkpt, geoms, 300, shift=True, full_hw=(700, 700))
    assert [n for _, _, n in info] == [1500, 3000, 500, 100]


# ---- RT-DETR query selection ----------------------------------------------------------------------------------------------------

def _topk_ref(s, nc):
    return np.stack([ops_ref.stable_topk(im[:, :nc].max(1)) for im in s])


@pytest.mark.parametrize("nc", [1, 80])
@pytest.mark.parametrize("nt", [300, 301, 525, 8400])
def test_rt_topk(gpu_lib, nt, nc):
    """The documented order — (logit descending, token index ascending) — is asserted exactly, ties included."""
    rng = np.random.default_rng(nt + nc)
    cs = nc + 3                                               # the class logits are a slice of wider records
    def run(mx, label):
        s = np.full((mx.shape[0], nt, cs), np.inf, np.float32)   # a kernel reading outside the slice would see +inf
        s[:, :, 2:2 + nc] = -np.inf
        hot = rng.integers(0, nc, mx.shape)
        np.put_along_axis(s[:, :, 2:2 + nc], hot[..., None], mx[..., None].astype(np.float32), 2)
        if nc > 1:                                            # below the maximum everywhere else (never the other zero: see the -0.0 test)
            low = np.where(np.isfinite(mx), mx - 1 - rng.random(mx.shape), -np.inf).astype(np.float32)
            rest = np.broadcast_to(low[..., None], s[:, :, 2:2 + nc].shape).copy()
            np.put_along_axis(rest, hot[..., None], mx[..., None].astype(np.float32), 2)
            s[:, :, 2:2 + nc] = rest
        got = gpu_lib.op_rt_topk(s, nc, 2)
        want = np.stack([ops_ref.stable_topk(m) for m in mx.astype(np.float32)])
        assert np.array_equal(got, want), f"{label}: first difference at rank {np.flatnonzero((got != want).any(0))[0]}"
    run(rng.standard_normal((3, nt)), "random")
    run(np.full((2, nt), -1.25), "all equal")                                 # the first 300 indices win
    tie = rng.standard_normal((2, nt))
    if nt > 300:
        order = np.argsort(-tie[0])
        tie[:, order[250:min(nt, 380)]] = tie[0, order[250]]                  # a block of equal values straddling rank 300
    run(tie, "tie block across rank 300")
    inf = rng.standard_normal((2, nt))
    inf[:, rng.choice(nt, 40, replace=False)] = np.inf
    inf[:, rng.choice(nt, nt // 2, replace=False)] = -np.inf
    run(inf, "+-inf")
    run(np.round(rng.standard_normal((2, nt)) * 2) + 0.5, "heavy ties over a few values")


def test_rt_topk_orders_negative_zero_below_positive_zero(gpu_lib):
    """rt_topk compares the order-preserving bit patterns of the logits, a total order: -0.0 ranks below +0.0, where float
    comparison (torch.topk) calls them equal and would rank them by index alone. Either is a valid top-k of the values; the kernel's
    choice is the documented one (include/ffp.h) and is pinned here on single-class data (with several classes the maximum of a
    -0.0 and a +0.0 is whichever fmaxf returns)."""
    nt = 525
    s = np.full((1, nt, 1), -1.0, np.float32)
    s[0, 100:500, 0] = -0.0
    s[0, 350:450, 0] = 0.0
    got = gpu_lib.op_rt_topk(s)
    assert got[0].tolist() == list(range(350, 450)) + list(range(100, 300))
    assert np.array_equal(got[0], ops_ref.stable_topk(s[0, :, 0]))
    assert not np.array_equal(got[0], ops_ref.stable_topk(s[0, :, 0], signed_zero=False))

"""Operator-level parity of the RT-DETR non-convolution HIP kernels (csrc/rtdetr_ops.hip) through the single-operator entry points
ffp_op_rt_*, against the float64 references of tests/ops_ref.py. The entry points call the launch functions the plans call.

What the end-to-end tests cannot see is built into the inputs here: maps that are not square, LayerNorm tokens with a large mean,
attention with a late dominant key, deformable sampling points on and over every edge, all-negative pool inputs, token counts on
both sides of the block sizes. Every case has at least two images with different content, views are channel slices of wider
records, and output buffers are pre-filled with sentinels that must come back unchanged outside the written slice.

Error bounds follow the rule of tests/test_gpu_ops.py: exact where the operation is exact in float32 (copies, maxima, a single add,
arithmetic that -ffp-contract=off makes reproducible in a float32 numpy restatement); otherwise the yardstick is the plain float32
evaluation of the same formula against the float64 reference (max abs error / max |reference|), the device may be at most 4 x the
yardstick with F32_FLOOR as the floor, and messages carry both figures.

Max-|value| slots: every kernel that raises one is started at 0 — the returned bits must equal the bits of max |stored output|
exactly (a maximum has no order dependence) — and above that value, which must come back unchanged."""
import numpy as np
import pytest

import ops_ref
from rt_deform_cases import DEFORM_SHAPES, DEFORM_SHAPES_T, deform_inputs

pytestmark = pytest.mark.gpu

F32_FLOOR = 2e-6
NQ = 300


def _bits(v):
    return int(np.asarray([v], np.float32).view(np.uint32)[0])


def _sent(rng, shape):
    return rng.integers(-1000, 1000, shape).astype(np.float32)


def _untouched(got, before, coff, c, what):
    mask = np.ones(before.shape[-1], bool)
    mask[coff:coff + c] = False
    assert np.array_equal(got[..., mask], before[..., mask]), f"{what}: values outside the output slice changed"


def _bounded(got, ref, y32, what):
    ref = np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), f"{what}: output not finite"
    scale = np.abs(ref).max()
    yard = np.abs(np.asarray(y32, np.float64) - ref).max() / scale
    err = np.abs(np.asarray(got, np.float64) - ref).max() / scale
    bound = max(4 * yard, F32_FLOOR)
    print(f"{what}: float32 yardstick {yard:.3g}, device error {err:.3g}, bound {bound:.3g}")
    assert err <= bound, f"{what}: device error {err:.3g} > bound {bound:.3g} (float32 yardstick {yard:.3g})"


def _slot(run, stored, what):
    """run(amax) -> (outputs, final slot bits); stored(outputs) -> the values the kernel stored. Returns the outputs of the run from 0."""
    out, bits = run(0.0)
    m = np.float32(np.abs(stored(out)).max())
    assert bits == _bits(m), f"{what}: slot from 0 came back as {bits:#010x}, max |stored output| = {m!r} is {_bits(m):#010x}"
    high = np.float32(m * 2 + 1)
    out2, bits2 = run(high)
    assert bits2 == _bits(high), f"{what}: a slot above the output's maximum changed ({_bits(high):#010x} -> {bits2:#010x})"
    assert np.array_equal(stored(out2), stored(out), equal_nan=True)
    return out


# ---- depthwise k5 s1 / k3 s2 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,x_cs,x_coff,y_cs,y_coff", [(4, 4, 0, 8, 4), (12, 20, 4, 20, 4)], ids=["c4", "c12_of_20"])
@pytest.mark.parametrize("k,s,act,hw", [(5, 1, 3, (1, 1)), (5, 1, 3, (3, 2)), (5, 1, 3, (6, 5)), (3, 2, 0, (1, 1)), (3, 2, 0, (5, 4)), (3, 2, 0, (6, 7))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rt_dwconv(gpu_lib, k, s, act, hw, c, x_cs, x_coff, y_cs, y_coff):
    rng = np.random.default_rng(k * 100 + hw[0] * 10 + hw[1] + c)
    n, (h, w) = 3, hw
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    assert (ho, wo) == (hw if s == 1 else {(1, 1): (1, 1), (5, 4): (3, 2), (6, 7): (3, 4)}[hw])
    x = rng.standard_normal((n, h, w, x_cs)).astype(np.float32)                 # both signs: the ReLU clips about half of the sums
    x[..., :x_coff] = 9e4; x[..., x_coff + c:] = 9e4
    wt = (rng.standard_normal((c, k, k)) / k).astype(np.float32)
    b = (rng.standard_normal(c) * 0.1).astype(np.float32)
    y0 = _sent(rng, (n, ho, wo, y_cs))
    ref = np.stack([ops_ref.rt_dwconv(a[..., x_coff:x_coff + c], wt, b, k, s, act) for a in x])
    y32 = np.stack([ops_ref.rt_dwconv(a[..., x_coff:x_coff + c], wt, b, k, s, act, dtype=np.float32) for a in x])
    if act == 3:
        assert (ref == 0).any() and (ref > 0).any()
    what = f"rt_dwconv k{k} s{s} {h}x{w} c{c}"
    got = _slot(lambda a: gpu_lib.op_rt_dwconv(x, c, x_coff, wt, b, y0, y_coff, k, s, act, amax=a), lambda y: y[..., y_coff:y_coff + c], what)
    _untouched(got, y0, y_coff, c, what)
    _bounded(got[..., y_coff:y_coff + c], ref, y32, what)
    if act == 3:
        assert (got[..., y_coff:y_coff + c] >= 0).all()


# ---- HGStem's pool ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign", ["negative", "mixed"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (4, 1), (5, 7)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_rt_maxpool2(gpu_lib, hw, sign):
    rng = np.random.default_rng(hw[0] * 10 + hw[1])
    n, (h, w), c, x_cs, x_coff, y_cs, y_coff = 2, hw, 8, 16, 4, 12, 4
    x = rng.standard_normal((n, h, w, x_cs)).astype(np.float32)
    if sign == "negative":
        x = -np.abs(x) - 1
    x[..., :x_coff] = 9e4; x[..., x_coff + c:] = 9e4
    y0 = _sent(rng, (n, h, w, y_cs))
    want = np.stack([ops_ref.rt_maxpool2(a[..., x_coff:x_coff + c]) for a in x])
    what = f"rt_maxpool2 {h}x{w} {sign}"
    got = _slot(lambda a: gpu_lib.op_rt_maxpool2(x, c, x_coff, y0, y_coff, amax=a), lambda y: y[..., y_coff:y_coff + c], what)
    _untouched(got, y0, y_coff, c, what)
    o = got[..., y_coff:y_coff + c]
    assert np.array_equal(o, want), what
    if sign == "negative":                               # the window reaches the zero padding in the last row and column, nowhere else
        assert (o[:, -1] == 0).all() and (o[:, :, -1] == 0).all() and (o[:, :-1, :-1] < 0).all()


# ---- add ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", [0, 7])
def test_rt_add(gpu_lib, period):
    rng = np.random.default_rng(period)
    n, L, c = 3, 7, 12
    npx = n * L
    a = rng.standard_normal((npx, 20)).astype(np.float32)
    b = rng.standard_normal((period or npx, 16)).astype(np.float32)         # b_cs != a_cs
    y0 = _sent(rng, (npx, 24))
    want = a[:, 4:16] + (np.tile(b, (n, 1)) if period else b)[:, 0:12]
    what = f"rt_add period {period}"
    got = _slot(lambda m: gpu_lib.op_rt_add(a, c, 4, b, 0, y0, 8, period=period, amax=m), lambda y: y[:, 8:20], what)
    _untouched(got, y0, 8, c, what)
    assert np.array_equal(got[:, 8:20], want), what


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------

LN_KINDS = ["unit", "mean1e4", "constant", "tiny", "spike"]


def _ln_tokens(rng, nt, kind):
    x = rng.standard_normal((nt, 256))
    special = sorted({0, nt // 2, nt - 1})                # next to ordinary tokens wherever there is more than one
    for i in special:
        if kind == "mean1e4":
            x[i] += 1e4
        elif kind == "constant":
            x[i] = 3.25 * (i + 1)
        elif kind == "tiny":
            x[i] *= 1e-4
        elif kind == "spike":
            x[i, (17 * (i + 1)) % 256] = 1e4
    return x.astype(np.float32), special


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("nt", [1, 5, 301])
def test_rt_layernorm(gpu_lib, nt, kind, inplace):
    """Finding of this test, fixed with it: with a token mean of 1e4 and std 1 the kernel's mean, a float32 tree sum of 256 values rounded
    at the ulp of the SUM (0.25 at 2.56e6), was off by up to 1.2e-3 of the std: at 5 tokens the device error was 4.02e-4 of max |ref|
    against a float32 yardstick of 3.78e-5 (bound 1.51e-4). rt_layernorm_kernel now corrects the mean once by the mean of the
    residuals x - mean (small numbers, summed accurately); the same cases then measure 8.9e-8 to 1.6e-7."""
    rng = np.random.default_rng(nt * 7 + LN_KINDS.index(kind))
    xs, special = _ln_tokens(rng, nt, kind)
    g = (1 + 0.5 * rng.standard_normal(256)).astype(np.float32)
    b = rng.standard_normal(256).astype(np.float32)
    cs, coff = 320, 32
    y0 = _sent(rng, (nt, cs))
    what = f"rt_layernorm {nt} tokens {kind} {'in place' if inplace else 'out of place'}"
    if inplace:
        y0[:, coff:coff + 256] = xs
        run = lambda a: gpu_lib.op_rt_layernorm(None, 0, g, b, y0, coff, amax=a)
    else:
        x = np.full((nt, cs), 9e4, np.float32)
        x[:, coff:coff + 256] = xs
        run = lambda a: gpu_lib.op_rt_layernorm(x, coff, g, b, y0, coff, amax=a)
    got = _slot(run, lambda y: y[:, coff:coff + 256], what)
    _untouched(got, y0, coff, 256, what)
    o = got[:, coff:coff + 256]
    _bounded(o, ops_ref.layer_norm(xs, g, b), ops_ref.layer_norm(xs, g, b, dtype=np.float32), what)
    if kind == "constant":
        for i in special:
            assert np.array_equal(o[i], b), f"{what}: a constant token must give beta exactly"


# ---- GELU -------------------------------------------------------------------------------------------------------------------------

def test_rt_gelu(gpu_lib):
    rng = np.random.default_rng(0)
    v = np.r_[np.linspace(-10, 10, 523), 0.0, -0.0, 30.0, -30.0, 1e-8].astype(np.float32)      # 528 values = 66 records of 8
    cs, coff, c = 12, 4, 8
    x = _sent(rng, (v.size // c, cs))
    x[:, coff:coff + c] = rng.permutation(v).reshape(-1, c)
    xs = x[:, coff:coff + c].copy()
    got = _slot(lambda a: gpu_lib.op_rt_gelu(x, c, coff, amax=a), lambda y: y[:, coff:coff + c], "rt_gelu")
    _untouched(got, x, coff, c, "rt_gelu")
    _bounded(got[:, coff:coff + c], ops_ref.gelu(xs), ops_ref.gelu(xs, dtype=np.float32), "rt_gelu")


# ---- attention, 8 heads of 32 -----------------------------------------------------------------------------------------------------

ATTN_KINDS = ["gain1", "gain30", "late_key", "early_key"]


def _attn_inputs(rng, n, L, kind):
    qk = rng.standard_normal((n, L, 512))
    if kind == "gain30":                                 # q . k / sqrt(32) ~ N(0, 30^2): a softmax that is one-hot or nearly so
        qk *= np.sqrt(30.0)
    elif kind in ("late_key", "early_key"):              # every query has a component along one key: its logit leads by 2 * 1.5 * 32 / sqrt(32) = 17;
        j = L - 1 if kind == "late_key" else 0           # in the last key block the running maximum jumps after everything else was summed
        qk[:, :, :256] += 2.0
        qk[:, j, 256:] += 1.5
    return qk.astype(np.float32), rng.standard_normal((n, L, 256)).astype(np.float32)


@pytest.mark.parametrize("kind", ATTN_KINDS)
@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 300])
def test_rt_attention(gpu_lib, L, kind):
    rng = np.random.default_rng(L * 4 + ATTN_KINDS.index(kind))
    n = 2
    qs, vs = _attn_inputs(rng, n, L, kind)
    qk = np.full((n, L, 528), 7e4, np.float32); qk[..., 8:520] = qs
    v = np.full((n, L, 264), 7e4, np.float32); v[..., 4:260] = vs       # v in a buffer of its own record width
    y0 = _sent(rng, (n, L, 272))
    ref = np.stack([ops_ref.rt_attention(a, b) for a, b in zip(qs, vs)])
    y32 = np.stack([ops_ref.rt_attention(a, b, dtype=np.float32) for a, b in zip(qs, vs)])
    what = f"rt_attention L={L} {kind}"
    got = _slot(lambda a: gpu_lib.op_rt_attention(qk, 8, v, 4, y0, 12, amax=a), lambda y: y[..., 12:268], what)
    _untouched(got, y0, 12, 256, what)
    _bounded(got[..., 12:268], ref, y32, what)


# ---- encoder input ----------------------------------------------------------------------------------------------------------------

def test_rt_enc_prep(gpu_lib):
    """The tm slot is by design raised with the maximum of t, an upper bound of max |tm| (masked tokens are zeros): asserted as such."""
    rng = np.random.default_rng(3)
    n, shapes, css, coffs = 3, [(6, 4), (3, 2), (2, 1)], [264, 256, 272], [4, 0, 16]
    srcs = []
    for (h, w), cs, co in zip(shapes, css, coffs):
        a = np.full((n, h, w, cs), 9e4, np.float32)
        a[..., co:co + 256] = rng.standard_normal((n, h, w, 256))
        srcs.append(a)
    nt = sum(h * w for h, w in shapes)
    assert nt == 32
    valid = np.ones(nt, np.float32)
    start = 0
    for h, w in shapes:
        valid[start] = 0; valid[start + h * w - 1] = 0
        start += h * w
    srcs[0][1, 0, 0, coffs[0]] = 50.0                    # the batch maximum sits in a masked token: max |tm| < max |t|
    rows = n * nt + 2
    t0, tm0 = _sent(rng, (rows, 256)), _sent(rng, (rows, 256))
    t, tm, st, stm = gpu_lib.op_rt_enc_prep(srcs, coffs, valid, t0, tm0, amax_t=0.0, amax_tm=0.0)
    for i in range(n):
        wt, wtm = ops_ref.rt_enc_prep([a[i, ..., co:co + 256] for a, co in zip(srcs, coffs)], valid)
        assert np.array_equal(t[i * nt:(i + 1) * nt], wt) and np.array_equal(tm[i * nt:(i + 1) * nt], wtm), f"image {i}"
    assert np.array_equal(t[n * nt:], t0[n * nt:]) and np.array_equal(tm[n * nt:], tm0[n * nt:]), "records behind the last token changed"
    assert st == _bits(np.abs(t[:n * nt]).max()) == _bits(50.0)
    assert stm == st and np.abs(tm[:n * nt]).max() < 50.0                 # the documented upper bound
    _, _, st2, stm2 = gpu_lib.op_rt_enc_prep(srcs, coffs, valid, t0, tm0, amax_t=77.0, amax_tm=1e-3)
    assert st2 == _bits(77.0) and stm2 == _bits(50.0)


# ---- gather -----------------------------------------------------------------------------------------------------------------------

def test_rt_gather(gpu_lib):
    rng = np.random.default_rng(4)
    n, nt = 2, 32
    es = rng.standard_normal((n, nt, 256)).astype(np.float32)
    e = np.full((n, nt, 272), 9e4, np.float32); e[..., 8:264] = es
    idx = rng.integers(0, nt, (n, NQ)).astype(np.int32)                  # 300 draws of 32: repeats everywhere
    idx[:, :6] = [0, nt - 1, nt - 1, -1, nt, 0]
    idx[1, 6:9] = [-7, nt + 100, 5]
    anchors = rng.standard_normal((nt, 4)).astype(np.float32)
    anchors[3] = np.inf
    idx[0, 10] = 3
    q0, a0 = _sent(rng, (n, NQ, 264)), _sent(rng, (n, NQ, 4))
    q, anc = _slot(lambda m: (lambda r: (r[:2], r[2]))(gpu_lib.op_rt_gather(e, 8, idx, anchors, q0, 4, a0, amax=m)), lambda o: o[0][..., 4:260], "rt_gather")
    _untouched(q, q0, 4, 256, "rt_gather")
    for i in range(n):
        we, wa = ops_ref.rt_gather(es[i], idx[i], anchors)
        assert np.array_equal(q[i, :, 4:260], we) and np.array_equal(anc[i], wa), f"image {i}"
    assert np.isinf(anc[0, 10]).all()


# ---- reference boxes --------------------------------------------------------------------------------------------------------------

def test_rt_ref_init(gpu_lib):
    rng = np.random.default_rng(5)
    nq = 2 * NQ
    ds = (rng.standard_normal((nq, 4)) * 3).astype(np.float32)
    anc = (rng.standard_normal((nq, 4)) * 2).astype(np.float32)
    anc[7] = np.inf; anc[301, 2] = np.inf
    delta = np.full((nq, 8), 9e4, np.float32); delta[:, 4:] = ds
    r0 = _sent(rng, (nq, 12))
    got = _slot(lambda a: gpu_lib.op_rt_ref(delta, 4, r0, 4, anc=anc, amax=a), lambda y: y[:, 4:8], "rt_ref init")
    _untouched(got, r0, 4, 4, "rt_ref init")
    _bounded(got[:, 4:8], ops_ref.rt_ref(ds, anc=anc), ops_ref.rt_ref(ds, anc=anc, dtype=np.float32), "rt_ref init")
    assert (got[7, 4:8] == 1).all() and got[301, 6] == 1


def test_rt_ref_refine(gpu_lib):
    rng = np.random.default_rng(6)
    refs = np.array([0.0, 1.0, 1e-7, 1 - 1e-7, 0.5, -0.1, 1.1], np.float32)
    dels = np.array([0.0, 20.0, -20.0, 100.0, -100.0], np.float32)
    grid = np.stack(np.meshgrid(refs, dels, indexing="ij"), -1).reshape(-1, 2)           # 35 (ref, delta) pairs
    nq = 2 * NQ
    rs = rng.random((nq, 4)).astype(np.float32)
    ds = rng.standard_normal((nq, 4)).astype(np.float32)
    rs.reshape(-1)[:35], ds.reshape(-1)[:35] = grid[:, 0], grid[:, 1]
    rs.reshape(-1)[1300:1335], ds.reshape(-1)[1300:1335] = grid[:, 0], grid[:, 1]       # and in the second image
    delta = np.full((nq, 8), 9e4, np.float32); delta[:, :4] = ds
    r0 = _sent(rng, (nq, 8)); r0[:, 4:] = rs
    got = _slot(lambda a: gpu_lib.op_rt_ref(delta, 0, r0, 4, amax=a), lambda y: y[:, 4:], "rt_ref refine")
    _untouched(got, r0, 4, 4, "rt_ref refine")
    _bounded(got[:, 4:], ops_ref.rt_ref(ds, ref=rs), ops_ref.rt_ref(ds, ref=rs, dtype=np.float32), "rt_ref refine")


# ---- deformable sampling ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deform_cases():
    return {w: deform_inputs(11 + i, w) for i, w in enumerate(["unit", "pm80"])}


@pytest.mark.parametrize("shapes", [DEFORM_SHAPES, DEFORM_SHAPES_T], ids=["5x7_3x4_2x2", "7x5_4x3_2x2"])
@pytest.mark.parametrize("weights", ["unit", "pm80"])
def test_rt_deform(gpu_lib, deform_cases, weights, shapes):
    """The second geometry reads the same arrays with every level transposed: a swapped H / W gives the other answer."""
    vs, oas, rs, _ = deform_cases[weights]
    rng = np.random.default_rng(9)
    n, nt = vs.shape[:2]
    val = np.full((n, nt, 264), 9e4, np.float32); val[..., 4:260] = vs
    oa = np.full((n, NQ, 296), 9e4, np.float32); oa[..., 8:] = oas
    rf = np.full((n, NQ, 8), 9e4, np.float32); rf[..., :4] = rs
    y0 = _sent(rng, (n, NQ, 268))
    ref = np.stack([ops_ref.rt_deform(vs[i], shapes, oas[i], rs[i]) for i in range(n)])
    y32 = np.stack([ops_ref.rt_deform(vs[i], shapes, oas[i], rs[i], dtype=np.float32) for i in range(n)])
    other = np.stack([ops_ref.rt_deform(vs[i], [(w, h) for h, w in shapes], oas[i], rs[i]) for i in range(n)])
    assert np.abs(other - ref).max() > 0.5                 # the transposed geometry is another function of the same data
    what = f"rt_deform {shapes} weights {weights}"
    got = _slot(lambda a: gpu_lib.op_rt_deform(shapes, val, 4, oa, 8, rf, 0, y0, 8, amax=a), lambda y: y[..., 8:264], what)
    _untouched(got, y0, 8, 256, what)
    _bounded(got[..., 8:264], ref, y32, what)


# ---- raw output and RTDETRPredictor.postprocess -----------------------------------------------------------------------------------

def _decode_inputs(nc):
    rng = np.random.default_rng(nc)
    n = 3
    rs = rng.random((n, NQ, 4)).astype(np.float32)
    lg = (rng.standard_normal((n, NQ, nc)) * 2).astype(np.float32)
    lg[1] = np.abs(lg[1]) + 0.1                            # image 1: every query passes conf 0.5
    lg[2] = -np.abs(lg[2]) - 0.1                           # image 2: none does
    lg[0, 10] = -1.0; lg[0, 10, nc // 2] = 0.0             # a best logit of exactly 0: sigmoid 0.5, not above conf 0.5
    lg[0, 11] = 1.5                                        # every class ties: the first one
    if nc > 1:
        lg[0, 12] = -2.0; lg[0, 12, 1:] = 0.75             # first maximum at class 1
    ref = np.full((n, NQ, 8), 9e4, np.float32); ref[..., 4:] = rs
    sc = np.full((n, NQ, nc + 8), 9e4, np.float32); sc[..., 4:4 + nc] = lg
    return rs, lg, ref, sc


@pytest.mark.parametrize("nc", [1, 3, 80])
def test_rt_decode_raw(gpu_lib, nc):
    rs, lg, ref, sc = _decode_inputs(nc)
    raw0 = _sent(np.random.default_rng(0), (3, NQ, 4 + nc))
    raw, _, _ = gpu_lib.op_rt_decode(ref, 4, sc, 4, nc, raw=raw0)
    assert np.array_equal(raw[..., :4], rs)
    _bounded(raw[..., 4:], ops_ref.sigmoid(lg), ops_ref.sigmoid(lg, np.float32), f"rt_raw nc={nc}")


@pytest.mark.parametrize("nc", [1, 3, 80])
def test_rt_decode_post(gpu_lib, nc):
    rs, lg, ref, sc = _decode_inputs(nc)
    conf = 0.5
    wh = np.array([[333, 200], [64, 480], [1920, 1080]], np.float32)            # (width, height), none square
    det0 = _sent(np.random.default_rng(1), (3, NQ, 6))
    _, det, counts = gpu_lib.op_rt_decode(ref, 4, sc, 4, nc, conf=conf, orig_wh=wh, det=det0)
    want_counts = []
    for i in range(3):
        rows, margin = ops_ref.rt_post(rs[i], lg[i], conf, wh[i])
        assert margin >= 1e-5, f"image {i}: a score within {margin:.3g} of conf"          # condition on the inputs
        if nc > 1:                                          # and the two best classes differ in float32 too, unless their logits are equal
            top = np.sort(lg[i], -1)[:, -2:]
            s32 = ops_ref.sigmoid(top, np.float32)
            assert ((s32[:, 1] > s32[:, 0]) | (top[:, 1] == top[:, 0])).all()
        want_counts.append(len(rows))
        k = counts[i]
        assert k == len(rows), f"image {i}: {k} rows, reference {len(rows)}"
        assert np.array_equal(det[i, k:], det0[i, k:]), f"image {i}: rows past the count changed"
        assert np.array_equal(det[i, :k, 5], rows[:, 5]), f"image {i}: classes (the first maximum) or the query order differ"
        keep = ops_ref.sigmoid(lg[i]).max(-1) > conf
        b = rs[i][keep]                                     # the predictor's arithmetic restated in float32: reproducible without contraction
        dw, dh = b[:, 2] / np.float32(2), b[:, 3] / np.float32(2)
        box32 = np.stack([(b[:, 0] - dw) * wh[i, 0], (b[:, 1] - dh) * wh[i, 1], (b[:, 0] + dw) * wh[i, 0], (b[:, 1] + dh) * wh[i, 1]], 1)
        assert np.array_equal(det[i, :k, :4], box32), f"image {i}: boxes"
        if k:
            _bounded(det[i, :k, 4], rows[:, 4], ops_ref.sigmoid(lg[i], np.float32).max(-1)[keep], f"rt_post nc={nc} image {i} scores")
    assert 0 < want_counts[0] < NQ and want_counts[1] == NQ and want_counts[2] == 0
    keep0 = np.flatnonzero(ops_ref.sigmoid(lg[0]).max(-1) > conf)
    assert 10 not in keep0 and 11 in keep0                  # strict >: the logit of exactly 0 is dropped
    assert det[0, list(keep0).index(11), 5] == 0
    if nc > 1:
        assert det[0, list(keep0).index(12), 5] == 1


# ---- argument checks --------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(gpu_lib):
    z = lambda *s: np.zeros(s, np.float32)
    calls = {
        "dwconv C % 4": lambda: gpu_lib.op_rt_dwconv(z(1, 3, 3, 8), 6, 0, z(6, 3, 3), z(6), z(1, 2, 2, 8), 0, 3, 2),
        "dwconv k3 s1": lambda: gpu_lib.op_rt_dwconv(z(1, 3, 3, 4), 4, 0, z(4, 3, 3), z(4), z(1, 3, 3, 4), 0, 3, 1),
        "dwconv offset % 4": lambda: gpu_lib.op_rt_dwconv(z(1, 3, 3, 8), 4, 2, z(4, 5, 5), z(4), z(1, 3, 3, 8), 0, 5, 1),
        "maxpool slice outside the record": lambda: gpu_lib.op_rt_maxpool2(z(1, 2, 2, 8), 8, 4, z(1, 2, 2, 8), 0),
        "layernorm needs 256 channels": lambda: gpu_lib.op_rt_layernorm(z(5, 200), 0, z(256), z(256), z(5, 256), 0),
        "attention needs q | k of 512": lambda: gpu_lib.op_rt_attention(z(1, 4, 500), 0, z(1, 4, 256), 0, z(1, 4, 256), 0),
        "deform needs 288 offsets and weights": lambda: gpu_lib.op_rt_deform([(1, 1)] * 3, z(1, 3, 256), 0, z(1, NQ, 280), 0, z(1, NQ, 4), 0, z(1, NQ, 256), 0),
        "enc_prep needs n * tokens records": lambda: gpu_lib.op_rt_enc_prep([z(2, 1, 1, 256)] * 3, [0, 0, 0], z(3), z(5, 256), z(5, 256)),
        "add period above the record count": lambda: gpu_lib.op_rt_add(z(3, 4), 4, 0, z(7, 4), 0, z(3, 4), 0, period=7),
        "decode nc outside the record": lambda: gpu_lib.op_rt_decode(z(1, NQ, 4), 0, z(1, NQ, 3), 0, 4, raw=z(1, NQ, 8)),
    }
    for what, call in calls.items():
        with pytest.raises(gpu_lib.FfpError) as e:
            call()
        assert e.value.code == 1, what

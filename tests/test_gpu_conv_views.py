"""The conv kernel families on the operands the plans give them (ffp_op_conv2d_views): ragged batches aligned to 32 pixels, channel slices of
wider records, two residual terms, per-image exponent slots and the gate — every shape number of tests/test_gpu_conv.py's tables, pinned through
ffp_op_conv2d_shape. Reference: float64 F.conv2d per image (operands rounded to fp16 first for PREC_F16), then act -> v * s1 + res1 -> v * s2 + res2
-> act_post. Tolerances are test_gpu_conv.py's: 2e-5 (f32), 2e-3 (f16), 3e-5 (f32x3) on unit-scale outputs, and for scaled images the per-output-channel
relative form of test_f32x3_scaled_split_is_fp32_grade_over_ranges. A forced call matches, or is the library's argument error (code 1): a wrong tensor
is the only failure."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import ACTS, EPI_GENERIC, EPI_ROWS, K3D_SHAPES, PW_SHAPES, _epi_k3d_cases, _epi_pw_cases, pw_can_run

pytestmark = pytest.mark.gpu

# output sizes of the base batch: ragged tile edges both ways, a one-pixel image that owns a whole 32-pixel fragment of padding, an image narrower than a tile
BASE_OUT = ((9, 17), (16, 16), (1, 1), (20, 5), (33, 31))
X_PAD, X_COFF, Y_PAD, Y_COFF = 48, 16, 24, 8      # input: slice at 16 of records of cin + 48; output: slice at 8 of records of cout + 24 (every fast path stays eligible)
S1 = S2 = float(np.float32(0.2))
SLOT0 = 0x00000101                                # initial output slot pattern (+ image index): small, nonzero, below any stored maximum


def _tol(P):
    return {P.PREC_F32: 2e-5, P.PREC_F16: 2e-3, P.PREC_F32X3: 3e-5}


def _pname(P, prec):
    return {P.PREC_F32: "f32", P.PREC_F16: "f16", P.PREC_F32X3: "f32x3"}[prec]


def _plan(P):
    """(family, precision, (shape, cin, cout, k, stride)) of every shape number, as test_conv_epilogue_contract_every_kernel lists them: the generic numbers
    in all three precisions on every case of EPI_GENERIC, the others in their family's precision on the smallest case of their table they can run."""
    out = [("generic", prec, c) for prec in (P.PREC_F32, P.PREC_F16, P.PREC_F32X3) for c in EPI_GENERIC
           if not (prec == P.PREC_F32X3 and c[3] == 3 and c[4] == 2 and c[0] in (0, 1))]      # the split's wide 3x3 stride-2 stages do not fit the LDS: not among the valid ones
    out += [(P.op_conv2d_shape_name(c[0]).split()[0], P.PREC_F16, c) for c in EPI_ROWS]
    out += [("pw", P.PREC_F32X3, c) for c in _epi_pw_cases()] + [("k3d", P.PREC_F32X3, c) for c in _epi_k3d_cases()]
    assert sorted({c[0] for _, _, c in out}) == list(range(26))
    return out


def _in_sizes(out_sizes, stride):
    return tuple((h, w) if stride == 1 else (2 * h - 1, 2 * w - 1) for h, w in out_sizes)      # k 3, pad 1, stride 2: (2h - 1 - 1) // 2 + 1 = h


@functools.lru_cache(maxsize=None)
def _case(cin, cout, k, stride, out_sizes=BASE_OUT, residuals=True):
    """standard-normal inputs, weights of unit output variance, bias and two residuals, once per case"""
    rng = np.random.default_rng([20261101, cin, cout, k, stride, len(out_sizes)])
    xs = tuple(rng.standard_normal((h, w, cin), dtype=np.float32) for h, w in _in_sizes(out_sizes, stride))
    wt = (rng.standard_normal((cout, cin, k, k), dtype=np.float32) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout, dtype=np.float32) * np.float32(0.1)
    r1 = tuple(rng.standard_normal((h, w, cout), dtype=np.float32) for h, w in out_sizes) if residuals else None
    r2 = tuple(rng.standard_normal((h, w, cout), dtype=np.float32) for h, w in out_sizes) if residuals else None
    return xs, wt, b, r1, r2


def _conv64(xs, wt, b, stride, half):
    w64 = torch.from_numpy(wt)
    w64 = (w64.half() if half else w64).double()
    out = []
    for x in xs:
        xt = torch.from_numpy(np.ascontiguousarray(x)).permute(2, 0, 1)[None]
        xt = (xt.half() if half else xt).double()
        out.append(F.conv2d(xt, w64, torch.from_numpy(b).double(), stride=stride, padding=wt.shape[2] // 2)[0].permute(1, 2, 0).contiguous())
    return out


@functools.lru_cache(maxsize=None)
def _base_conv64(cin, cout, k, stride, half):
    xs, wt, b, _, _ = _case(cin, cout, k, stride)
    return _conv64(xs, wt, b, stride, half)


def _epilogue(conv, act, r1, r2, post, half):
    """act -> v * s1 + res1 -> v * s2 + res2 -> act_post on the float64 conv sums"""
    out = []
    for i, v in enumerate(conv):
        v = ACTS[act](v)
        for r, s in ((r1, S1), (r2, S2)):
            if r is not None:
                rt = torch.from_numpy(r[i])
                v = v * s + (rt.half() if half else rt).double()
        out.append(ACTS[post](v).numpy())
    return out


def _pattern(shape, salt=0):
    """finite, different from element to element, exact in fp16"""
    n = int(np.prod(shape))
    return (((np.arange(n, dtype=np.int64) + salt) * 7919 % 2039).astype(np.float32) * np.float32(0.25) - np.float32(100.0)).reshape(shape)


def _embed(imgs, cs, coff, fill):
    """records of cs channels with imgs at [coff, coff + C): the other channels NaN ('nan': a read of a neighbour channel shows) or the pattern"""
    out = []
    for i, a in enumerate(imgs):
        rec = np.full(a.shape[:2] + (cs,), np.nan, np.float32) if fill == "nan" else _pattern(a.shape[:2] + (cs,), 131 * i)
        rec[..., coff:coff + a.shape[2]] = a
        out.append(rec)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _Tally:
    def __init__(self, name):
        self.name, self.ran, self.refused, self.wrong = name, {}, {}, []

    def call(self, P, family, f):
        """f() or None when the library refuses the op with its argument error"""
        try:
            r = f()
        except P.FfpError as e:
            assert e.code == 1, (self.name, family, str(e))
            self.refused[family] = self.refused.get(family, 0) + 1
            return None
        self.ran[family] = self.ran.get(family, 0) + 1
        return r

    def bad(self, *what):
        self.wrong.append(what)

    def report(self, minimum=(), generic_refuses_nothing=True):
        print(f"{self.name}: ran {sum(self.ran.values())} {dict(sorted(self.ran.items()))}, refused {sum(self.refused.values())} "
              f"{dict(sorted(self.refused.items()))}, wrong {len(self.wrong)}")
        for w in self.wrong[:40]:
            print("  wrong:", *w)
        assert not self.wrong, self.wrong[:10]
        if generic_refuses_nothing:
            assert not self.refused.get("generic"), self.refused
        for fam in minimum:
            assert self.ran.get(fam, 0) >= 1, (self.name, fam, "no shape of the family ran")


def _y0(out_sizes, cout):
    return [_pattern((h, w, cout + Y_PAD), 977 * i) for i, (h, w) in enumerate(out_sizes)]


def _check_written(t, tag, y, y0, ref, tol, coff, cout):
    """the slice matches the reference, everything else in the records is what went up"""
    for i in range(len(y)):
        got = y[i][..., coff:coff + cout]
        if not np.allclose(got, ref[i], rtol=tol, atol=tol):
            t.bad(*tag, f"image {i}", float(np.nanmax(np.abs(got - ref[i]))) if np.isfinite(got).all() else "not finite")
        keep = np.ones(y[i].shape[2], bool)
        keep[coff:coff + cout] = False
        if not _same_bits(y[i][..., keep], y0[i][..., keep]):
            t.bad(*tag, f"image {i}", "channels outside the slice changed")


# ---- a. slices ----------------------------------------------------------------------------------------------------------------------
def test_slices_of_wider_records_every_shape(gpu_lib):
    """Input = channels [16, 16 + cin) of records of cin + 48 (the others NaN), output = channels [8, 8 + cout) of records of cout + 24 (the others a
    finite per-element pattern), SiLU, five ragged images aligned to 32 pixels — and to 1 for the 3x3 families. The slice matches the reference; the other
    channels of y come back bit for bit; `stray` (the slack behind y, y's padding pixels — for a 1x1 conv those outside its own slice) is 0; the op that
    ran reports the pinned number's variant."""
    P = gpu_lib
    t = _Tally("slices")
    try:
        for family, prec, (shape, cin, cout, k, stride) in _plan(P):
            half = prec == P.PREC_F16
            xs, wt, b, _, _ = _case(cin, cout, k, stride)
            ref = _epilogue(_base_conv64(cin, cout, k, stride, half), 1, None, None, 0, half)
            xr, y0 = _embed(xs, cin + X_PAD, X_COFF, "nan"), _y0(BASE_OUT, cout)
            P.op_conv2d_shape(shape)
            for align in (32, 1) if k == 3 else (32,):
                tag = (family, _pname(P, prec), shape, f"{cin}->{cout} k{k}s{stride} align{align}")
                r = t.call(P, family, lambda: P.op_conv2d_views(xr, X_COFF, wt, b, y0, Y_COFF, stride=stride, act=1, px_align=align, precision=prec))
                if r is None:
                    continue
                y, _, stray = r
                _check_written(t, tag, y, y0, ref, _tol(P)[prec], Y_COFF, cout)
                if stray != 0:
                    t.bad(*tag, f"stray {stray}")
                suffix = P.op_conv2d_shape_name(shape).split()[1]
                if not P.op_conv2d_last_variant().endswith("_" + suffix):
                    t.bad(*tag, "variant", P.op_conv2d_last_variant())
    finally:
        P.op_conv2d_shape(-1)
    t.report(minimum=("pw", "k3d", "rows", "rows16", "rows16pc"))


def test_pose_head_slices_of_an_80_channel_record(gpu_lib):
    """The two head slices of a one-class pose record (yolo11.cpp: 64 box | 1 class | 15 keypoint channels): cout = 15 at offset 65 — not divisible by 4,
    so vec_ok and fast_out are off and every store is a dword or an element — and cout = 1 at offset 64, through the generic shapes in all three
    precisions and every pw shape that can run them. Channels 0..63 and the other slice stay intact."""
    P = gpu_lib
    t = _Tally("head slices")
    cin = 64
    try:
        for cout, coff in ((15, 65), (1, 64)):
            xs, wt, b, _, _ = _case(cin, cout, 1, 1)
            xr = _embed(xs, cin + X_PAD, X_COFF, "nan")
            y0 = [_pattern((h, w, 80), 613 * i) for i, (h, w) in enumerate(BASE_OUT)]
            runs = [("generic", prec, s_) for prec in (P.PREC_F32, P.PREC_F16, P.PREC_F32X3) for s_ in range(6)]
            runs += [("pw", P.PREC_F32X3, s_) for s_ in sorted(PW_SHAPES) if pw_can_run(s_, cin, cout)]
            for family, prec, shape in runs:
                half = prec == P.PREC_F16
                ref = _epilogue(_base_conv64(cin, cout, 1, 1, half), 0, None, None, 0, half)
                P.op_conv2d_shape(shape)
                tag = (family, _pname(P, prec), shape, f"{cin}->{cout} at {coff} of 80")
                r = t.call(P, family, lambda: P.op_conv2d_views(xr, X_COFF, wt, b, y0, coff, act=0, px_align=32, precision=prec))
                if r is None:
                    continue
                _check_written(t, tag, r[0], y0, ref, _tol(P)[prec], coff, cout)
                if r[2] != 0:
                    t.bad(*tag, f"stray {r[2]}")
    finally:
        P.op_conv2d_shape(-1)
    t.report(minimum=("pw",))


# ---- b. two residual terms ------------------------------------------------------------------------------------------------------------
def test_two_residual_terms_every_shape(gpu_lib):
    """LeakyReLU, then v * 0.2 + res1, then v * 0.2 + res2 (rrdb.cpp's has_res2), res1 and res2 from differently laid out buffers, without and with a ReLU
    behind them, through every shape number. Standard-normal data: a swapped order or a dropped term is an O(0.1..1) error. conv_pw has no residual inputs
    (kEpiPw) and refuses; the families that have them (generic, rows, rows16, rows16pc, trunk, k3d) run or refuse by act_post."""
    P = gpu_lib
    t = _Tally("two residuals")
    try:
        for family, prec, (shape, cin, cout, k, stride) in _plan(P):
            half = prec == P.PREC_F16
            xs, wt, b, r1, r2 = _case(cin, cout, k, stride)
            conv = _base_conv64(cin, cout, k, stride, half)
            xr, y0 = _embed(xs, cin + X_PAD, X_COFF, "nan"), _y0(BASE_OUT, cout)
            r1r, r2r = _embed(r1, cout + 8, 8, "nan"), _embed(r2, 2 * cout + 16, cout + 8, "nan")
            P.op_conv2d_shape(shape)
            for post in (0, 3):
                ref = _epilogue(conv, 2, r1, r2, post, half)
                tag = (family, _pname(P, prec), shape, f"{cin}->{cout} k{k}s{stride} post{post}")
                r = t.call(P, family, lambda: P.op_conv2d_views(xr, X_COFF, wt, b, y0, Y_COFF, stride=stride, act=2, act_post=post, res1=r1r, r1_coff=8, s1=S1,
                                                                res2=r2r, r2_coff=cout + 8, s2=S2, px_align=32, precision=prec))
                if r is None:
                    continue
                _check_written(t, tag, r[0], y0, ref, _tol(P)[prec], Y_COFF, cout)
                if r[2] != 0:
                    t.bad(*tag, f"stray {r[2]}")
    finally:
        P.op_conv2d_shape(-1)
    assert not t.ran.get("pw"), t.ran
    t.report(minimum=("k3d", "rows", "rows16", "rows16pc"))


# ---- c. per-image exponents ------------------------------------------------------------------------------------------------------------
def _rel_err(y, ref):
    """Largest error of an image relative to each output channel's own magnitude in that image (the largest |reference| of the channel over the image's
    pixels, as in the range test). On a one-pixel image that maximum is a single sum, not a magnitude: where the sum cancels to a hundredth of its terms
    the exact-fp32 kernel itself measures 1.0e-5 .. 1.4e-5 (MI355X, image 2 of the base batch at x3e4) against the 1e-5 bar. The rows of the weights are
    drawn alike, so the channels of such an image share one magnitude: there, and only there, a channel's scale is not taken below the median of the
    image's channel scales. Every image of two pixels and more is measured as stated."""
    c = ref.shape[-1]
    scale = np.abs(ref).reshape(-1, c).max(0)
    if ref.shape[0] * ref.shape[1] == 1:
        scale = np.maximum(scale, np.median(scale))
    return float((np.abs(y - ref).reshape(-1, c).max(0) / (scale + 1e-30)).max())


def _check_slots(t, tag, slots, y, coff, cout, skip=()):
    """every slot finite and EQUAL to the largest |stored value| of its image's real pixels: the generic kernel (amax_run over the values it stores),
    conv_pw (`am` over real pixels and channels) and conv_k3d raise the slot to the stored maximum, none documents a bound."""
    for i in range(len(y)):
        if i in skip:
            continue
        got = float(slots[i:i + 1].view(np.float32)[0])
        want = float(np.abs(y[i][..., coff:coff + cout]).max())
        if not np.isfinite(got) or _bits(np.float32(got)) != _bits(np.float32(want)):
            t.bad(*tag, f"slot {i} = {got!r}, stored maximum {want!r}")


IMG_SCALES = (1e-3, 1.0, 3e4, 1.0, 1e-6)


def test_per_image_exponent_slots_every_split_shape(gpu_lib):
    """PREC_F32X3 with one max-|value| slot per image, the images' activations scaled by 1e-3, 1, 3e4, 1, 1e-6: each image's error relative to its own
    output-channel scale meets the bar of test_f32x3_scaled_split_is_fp32_grade_over_ranges (<= max(3 x the exact-f32 kernel's error, 2e-6) and <= 1e-5);
    every image computed alone gives the bits it has in the batch; every returned slot is finite (padding pixels go up as NaN) and equals the largest
    |stored value| of its image's real pixels."""
    P = gpu_lib
    t = _Tally("per-image exponents")
    slot0 = (SLOT0 + np.arange(5)).astype(np.uint32)
    f32_err = {}
    try:
        for family, prec, (shape, cin, cout, k, stride) in _plan(P):
            if prec != P.PREC_F32X3:
                continue
            xs0, wt, b, _, _ = _case(cin, cout, k, stride)
            xs = [x * np.float32(s_) for x, s_ in zip(xs0, IMG_SCALES)]
            key = (cin, cout, k, stride)
            xr, y0 = _embed(xs, cin + X_PAD, X_COFF, "nan"), _y0(BASE_OUT, cout)
            if key not in f32_err:      # the yardstick: the exact-fp32 kernel the route picks, same operands
                P.op_conv2d_shape(-1)
                ref = [v.numpy() for v in _conv64(xs, wt, b, stride, False)]
                y32 = P.op_conv2d_views(xr, X_COFF, wt, b, y0, Y_COFF, stride=stride, px_align=32, precision=P.PREC_F32)[0]
                f32_err[key] = (ref, [_rel_err(y32[i][..., Y_COFF:Y_COFF + cout], ref[i]) for i in range(5)])
            ref, e32 = f32_err[key]
            P.op_conv2d_shape(shape)
            for align in (32, 1) if k == 3 else (32,):
                tag = (family, shape, f"{cin}->{cout} k{k}s{stride} align{align}")
                kw = dict(stride=stride, px_align=align, per_image_amax=True, precision=prec)
                r = t.call(P, family, lambda: P.op_conv2d_views(xr, X_COFF, wt, b, y0, Y_COFF, amax_out=slot0, **kw))
                if r is None:
                    continue
                y, slots, stray = r
                errs = [_rel_err(y[i][..., Y_COFF:Y_COFF + cout], ref[i]) if np.isfinite(y[i][..., Y_COFF:Y_COFF + cout]).all() else np.inf for i in range(5)]
                print(f"  {tag}: f32x3 {['%.2e' % e for e in errs]} f32 {['%.2e' % e for e in e32]}")
                for i in range(5):
                    if not (errs[i] <= max(3.0 * e32[i], 2e-6) and errs[i] <= 1e-5):
                        t.bad(*tag, f"image {i} (x{IMG_SCALES[i]:g})", errs[i], e32[i])
                if stray != 0:
                    t.bad(*tag, f"stray {stray}")
                _check_slots(t, tag, slots, y, Y_COFF, cout)
                for i in range(5):
                    ya, sa, _ = P.op_conv2d_views(xr[i:i + 1], X_COFF, wt, b, y0[i:i + 1], Y_COFF, amax_out=slot0[i:i + 1], **kw)
                    if not _same_bits(ya[0], y[i]) or sa[0] != slots[i]:
                        t.bad(*tag, f"image {i} alone differs from the batch in {int((_bits(ya[0]) != _bits(y[i])).sum())} values, slot {sa[0]:#x} / {slots[i]:#x}")
    finally:
        P.op_conv2d_shape(-1)
    t.report(minimum=("pw", "k3d"))


# ---- d. the gate ---------------------------------------------------------------------------------------------------------------------------
MASKS = ((1, 1, 1, 1, 1), (0, 0, 0, 0, 0), (1, 0, 1, 0, 1), (0, 0, 1, 0, 0), (0, 1, 1, 1, 1))


def _nan_where_off(imgs, mask):
    return [a if m else np.full_like(a, np.nan) for a, m in zip(imgs, mask)]


def _check_gated(t, tag, mask, y, slots, y_ung, slots_ung, y0, slot0):
    """active images: the ungated call's bits, slot included; inactive images: record and slot as they went up. With one slot per buffer (f32 / f16, whose
    kernels raise no slot) the slot is what went up under every mask."""
    for i, m in enumerate(mask):
        if m and not _same_bits(y[i], y_ung[i]):
            t.bad(*tag, f"active image {i} differs from the ungated call in {int((_bits(y[i]) != _bits(y_ung[i])).sum())} values")
        if not m and not _same_bits(y[i], y0[i]):
            t.bad(*tag, f"inactive image {i}: {int((_bits(y[i]) != _bits(y0[i])).sum())} values of its record changed")
        if len(slots) > 1 and slots[i] != (slots_ung[i] if m else slot0[i]):
            t.bad(*tag, f"image {i} ({'active' if m else 'inactive'}): slot {slots[i]:#x}, ungated {slots_ung[i]:#x}, went up as {slot0[i]:#x}")
    if len(slots) == 1 and slots[0] != slot0[0]:
        t.bad(*tag, f"the buffer's slot {slots[0]:#x}, went up as {slot0[0]:#x}")


def test_gate_every_shape(gpu_lib):
    """ConvOp::gate through every shape number on its family's 1x1 / 3x3 stride-1 case (the k3d numbers on their table case at stride 1; the generic
    numbers 0..3, whose table rows are 1x1 and stride 2, also on 64 -> 128 3x3 stride 1), masks 11111, 00000, 10101, 00100, 01111 and 11111 -> 00100 on one
    set of tables (gate_prev: the second run walks a gated table compacted a second time, with the first compaction's entries behind the count). Inactive
    images' inputs and residuals go up as NaN. An active image has the ungated call's bits and slot, an inactive image's whole record and its output slot
    (one per image for f32x3, a small nonzero pattern) are what went up, 00000 writes nothing; `stray` is 0, an inactive image's padding pixels included.
    A shape runs all six gated calls or refuses all six (code 1): 00000 or the rerun cannot be refused alone. Gated and ungated calls are counted apart,
    and the per-family minimum is of gated calls. The residual term is used where the family has one. Forced onto 3x3 stride 1, the generic wide shapes
    (0, 1: not among the valid ones there) may be the launcher's "does not fit the LDS" state error; such a (precision, shape) is skipped and printed."""
    P = gpu_lib
    t = _Tally("gate")
    slot0 = (SLOT0 + np.arange(5)).astype(np.uint32)
    gated_calls = [(m, None) for m in MASKS] + [(MASKS[3], MASKS[0])]
    plan = [e for e in _plan(P) if e[0] == "k3d" or e[2][4] == 1]
    plan += [("generic", prec, (s_, 64, 128, 3, 1)) for prec in (P.PREC_F32, P.PREC_F16, P.PREC_F32X3) for s_ in range(4)]
    unfit = []
    try:
        for family, prec, (shape, cin, cout, k, _) in plan:
            half, per_img = prec == P.PREC_F16, prec == P.PREC_F32X3
            xs, wt, b, r1, _ = _case(cin, cout, k, 1)
            y0 = _y0(BASE_OUT, cout)
            s0 = slot0 if per_img else slot0[:1]
            P.op_conv2d_shape(shape)
            for align in (32, 1) if k == 3 else (32,):
                tag = (family, _pname(P, prec), shape, f"{cin}->{cout} k{k} align{align}")
                kw = dict(act=1, px_align=align, per_image_amax=per_img, amax_out=s0, precision=prec)

                def run(mask, prev=None, res=True):
                    m = mask or (1,) * 5
                    kr = dict(res1=_embed(_nan_where_off(r1, m), cout + 8, 8, "nan"), r1_coff=8, s1=S1) if res else {}
                    return P.op_conv2d_views(_embed(_nan_where_off(xs, m), cin + X_PAD, X_COFF, "nan"), X_COFF, wt, b, y0, Y_COFF, gate=mask, gate_prev=prev, **kw, **kr)

                use_res = family != "pw"      # kEpiPw: no residual inputs
                if (cin, cout, k) == (64, 128, 3) and shape in (0, 1):
                    try:
                        run(None, res=use_res)
                    except P.FfpError as e:
                        if "does not fit the LDS" in str(e):
                            unfit.append(tag)
                            continue
                ung = t.call(P, family + " ungated", lambda: run(None, res=use_res))
                if ung is None:
                    continue
                ref = _epilogue(_base_conv64(cin, cout, k, 1, half), 1, r1 if use_res else None, None, 0, half)
                _check_written(t, tag + ("ungated",), ung[0], y0, ref, _tol(P)[prec], Y_COFF, cout)
                n_ran = 0
                for mask, prev in gated_calls:
                    mt = tag + ("mask " + "".join(map(str, mask)) + (" after " + "".join(map(str, prev)) if prev else ""),)
                    r = t.call(P, family, lambda: run(mask, prev, use_res))
                    if r is None:
                        continue
                    n_ran += 1
                    _check_gated(t, mt, mask, r[0], r[1], ung[0], ung[1], y0, s0)
                    if r[2] != 0:
                        t.bad(*mt, f"stray {r[2]}")
                if n_ran not in (0, len(gated_calls)):
                    t.bad(*tag, f"{n_ran} of {len(gated_calls)} gated calls ran, the others were refused")
    finally:
        P.op_conv2d_shape(-1)
    print("gate: does not fit the LDS:", unfit)
    assert not t.refused.get("generic ungated"), t.refused
    t.report(minimum=("pw", "k3d", "rows", "rows16", "rows16pc"))      # gated calls: the ungated ones are under "<family> ungated"


def test_split_1x1_with_one_slot_per_buffer_runs_ungated(gpu_lib):
    """make_conv_args' one documented exception: a split 1x1 conv whose buffers have ONE max-|value| slot has no fragment table to look an image up in and
    runs ungated. Pinned as exactly that — the gated call's result and slot equal the ungated call's, bit for bit — so that a change there is seen."""
    P = gpu_lib
    cin, cout = 64, 128
    xs, wt, b, _, _ = _case(cin, cout, 1, 1)
    xr, y0 = _embed(xs, cin + X_PAD, X_COFF, "nan"), _y0(BASE_OUT, cout)
    try:
        for shape in (4, 11):      # a generic and a pw shape
            P.op_conv2d_shape(shape)
            kw = dict(act=1, px_align=32, per_image_amax=False, amax_out=np.asarray([SLOT0], np.uint32), precision=P.PREC_F32X3)
            ung = P.op_conv2d_views(xr, X_COFF, wt, b, y0, Y_COFF, **kw)
            got = P.op_conv2d_views(xr, X_COFF, wt, b, y0, Y_COFF, gate=MASKS[2], **kw)
            assert all(_same_bits(a, c) for a, c in zip(got[0], ung[0])) and got[1][0] == ung[1][0] and ung[2] == 0, shape
            # ... down to the padding pixels: the 28 behind the inactive 20 x 5 image (the inactive 16 x 16 one has none) are computed like any pixel
            assert got[2] == 28 * cout, (shape, got[2])
    finally:
        P.op_conv2d_shape(-1)


# ---- e. gate and exponent hand-over across a workgroup's block walk ------------------------------------------------------------------
# conv_pw.hip: a work item is BPX = NW x 32 x MI pixels (NW waves of MI 32-pixel fragments), a launch has nslots = min(PB, max(1, R / n_nblk)) workgroup slots
# per channel block, R = 512 for the 4-wave shapes (two workgroups per CU) and 256 for the 8-wave and streamed ones, n_nblk = (cout / 32) / NT channel
# blocks, PB = ceil(total_px / BPX) pixel blocks dealt in contiguous runs of PB / nslots or one more.  shape -> (NW, MI, NT, streamed)
PW_GEOM = {10: (4, 1, 4, False), 11: (4, 2, 2, False), 12: (4, 2, 1, False), 13: (8, 1, 4, False), 14: (8, 2, 2, False), 15: (8, 2, 1, False),
           16: (7, 1, 4, True), 22: (7, 2, 2, True)}
WALK_CASES = ((64, 64), (96, 128))
# 12 image sizes, 1 pixel to 21 280, repeated: images smaller than a block, block-sized ones and ones of many blocks
WALK_DIMS = ((1, 1), (3, 5), (150, 141), (7, 9), (80, 100), (2, 13), (127, 131), (31, 33), (140, 152), (5, 5), (16, 16), (110, 107))


def _aligned_px(sizes, align=32):
    return sum(-(-h * w // align) * align for h, w in sizes)


def _pw_blocks_per_workgroup(shape, total_px, cout):
    """fewest pixel blocks any workgroup of the shape walks (PwCfg::launch / PwSt::launch and the kernel's pb_begin / pb_end)"""
    nw, mi, nt, streamed = PW_GEOM[shape]
    assert nt == PW_SHAPES[shape][0]
    bpx = nw * 32 * mi
    pb = -(-total_px // bpx)
    n_nblk = (-(-cout // 32)) // nt
    nslots = min(pb, max(1, (256 if streamed or nw == 8 else 512) // n_nblk))
    return pb // nslots


@functools.lru_cache(maxsize=None)
def _walk_sizes(cin, cout):
    """the shortest run of WALK_DIMS, at least 30 images, that gives every pw shape able to run the case three blocks per workgroup:
    64 -> 64: 60 images, 401 230 pixels, blocks per workgroup 11: 3, 12: 6, 14: 3, 15: 6, 22: 3;
    96 -> 128: 31 images, 206 384 pixels, 10: 3, 11: 3, 12: 6, 13: 3, 14: 3, 15: 6.
    On the prefix a shape runs on (_walk_prefix) — 64 -> 64: 11 and 14 all 60 images, 22 the first 53, 12 and 15 the first 31, three blocks each;
    96 -> 128: 10, 11, 13, 14 all 31 images (three blocks), 12 and 15 the first 24 (four). Asserted on the host in test_host_logic.py::test_conv_views_plan_bookkeeping."""
    shapes = [s_ for s_ in sorted(PW_SHAPES) if pw_can_run(s_, cin, cout)]
    sizes = []
    while len(sizes) < 30 or min(_pw_blocks_per_workgroup(s_, _aligned_px(sizes), cout) for s_ in shapes) < 3:
        sizes.append(WALK_DIMS[len(sizes) % len(WALK_DIMS)])
    return tuple(sizes)


def _walk_mask(n):
    """on / off in runs of 1, 2, 3, 1, 2, 3 ... images"""
    m, on, run = [], 1, 0
    while len(m) < n:
        m += [on] * (run % 3 + 1)
        on, run = 1 - on, run + 1
    return tuple(m[:n])


def _walk_prefix(shape, sizes, cout):
    """images of the batch a shape runs on: the shortest prefix, two rounds of WALK_DIMS at least, that gives every workgroup of a pw shape its three
    blocks; the generic shapes (shape None: a workgroup takes one block, there is no walk) run on the two rounds"""
    m = 2 * len(WALK_DIMS)
    while shape is not None and _pw_blocks_per_workgroup(shape, _aligned_px(sizes[:m]), cout) < 3:
        m += 1
    assert m <= len(sizes)
    return m


@pytest.mark.parametrize("cin,cout", WALK_CASES, ids=lambda v: str(v))
def test_gate_and_exponent_hand_over_across_a_block_walk(gpu_lib, cin, cout):
    """1x1 f32x3 with per-image slots on a ragged batch in which every workgroup of every pw shape walks at least three pixel blocks (the counts are in
    _walk_sizes' docstring; a shape that gets there with fewer images runs on that prefix of the batch, _walk_prefix), image scales alternating between
    1e-3 and 1e3 and the mask in runs of 1, 2 and 3 images: off -> on, on -> off and exponent changes fall at block boundaries, inside a block and at the
    last block, so conv_pw's two-blocks-ahead lookups (im_n / im_nn, on_n / on_nn) all run. Every pw shape that can run the case plus the generic
    shapes. Ungated: each image within the range test's bar of its own output-channel scale, slots finite and equal to the stored maximum, and every
    image computed alone gives the batch's bits. Gated: active images have
    the ungated bits and slots, inactive records and slots are what went up.
    Size: 64 -> 64 runs 60 images (401 230 pixels: the 4-wave shapes have 512 workgroup slots of 256 pixels, so three blocks each need 393 216), 96 -> 128
    reaches three blocks with 31 images (206 384 pixels) and stays there: x is 103 / 79 MB, y 116 / 112 MB on the device, and the host holds the float64
    reference and one prefix's packed copies beside them (about 0.7 GB at the peak). On the MI355X a case takes 4 to 5 s."""
    P = gpu_lib
    t = _Tally(f"block walk {cin}->{cout}")
    sizes = _walk_sizes(cin, cout)
    n = len(sizes)
    shapes = [s_ for s_ in sorted(PW_SHAPES) if pw_can_run(s_, cin, cout)]
    assert all(_pw_blocks_per_workgroup(s_, _aligned_px(sizes[:_walk_prefix(s_, sizes, cout)]), cout) >= 3 for s_ in shapes), "the case no longer walks three blocks"
    xs0, wt, b, _, _ = _case.__wrapped__(cin, cout, 1, 1, sizes, residuals=False)      # some hundred MB: not kept
    xs = [x * np.float32(1e-3 if i % 2 == 0 else 1e3) for i, x in enumerate(xs0)]
    del xs0
    ref = [v.numpy() for v in _conv64(xs, wt, b, 1, False)]
    mask = _walk_mask(n)
    slot0 = (SLOT0 + np.arange(n)).astype(np.uint32)
    y0 = [_pattern((h, w, cout + 8), 977 * i) for i, (h, w) in enumerate(sizes)]
    xg = _nan_where_off(xs, mask)
    kw = dict(px_align=32, per_image_amax=True, precision=P.PREC_F32X3)
    packed = {}      # prefix length -> the batches packed once

    def batches(m):
        if m not in packed:
            packed[m] = (P.OpBatch(xs[:m]), P.OpBatch(xg[:m]), P.OpBatch(y0[:m]))
        return packed[m]

    try:
        P.op_conv2d_shape(-1)
        y32 = P.op_conv2d_views(batches(n)[0], 0, wt, b, batches(n)[2], 8, px_align=32, precision=P.PREC_F32)[0]
        e32 = [_rel_err(y32[i][..., 8:], ref[i]) for i in range(n)]
        del y32
        packed.clear()
        runs = [("generic", s_) for s_ in range(6)] + [("pw", s_) for s_ in shapes]
        for family, shape in sorted(runs, key=lambda r: _walk_prefix(r[1] if r[0] == "pw" else None, sizes, cout)):
            m = _walk_prefix(shape if family == "pw" else None, sizes, cout)
            if m not in packed:
                packed.clear()      # one prefix's packed copies at a time
            xb, xgb, yb = batches(m)
            tag = (family, shape, f"{m} images")
            P.op_conv2d_shape(shape)
            ung = t.call(P, family, lambda: P.op_conv2d_views(xb, 0, wt, b, yb, 8, amax_out=slot0[:m], **kw))
            if ung is None:
                continue
            y, slots, stray = ung
            errs = [_rel_err(y[i][..., 8:], ref[i]) if np.isfinite(y[i][..., 8:]).all() else np.inf for i in range(m)]
            print(f"  {tag}: worst f32x3 {max(errs):.2e}, worst f32 {max(e32[:m]):.2e}")
            for i in range(m):
                if not (errs[i] <= max(3.0 * e32[i], 2e-6) and errs[i] <= 1e-5):
                    t.bad(*tag, f"image {i} {sizes[i]}", errs[i], e32[i])
                if not _same_bits(y[i][..., :8], y0[i][..., :8]):
                    t.bad(*tag, f"image {i}", "channels outside the slice changed")
            if stray != 0:
                t.bad(*tag, f"stray {stray}")
            _check_slots(t, tag, slots, y, 8, cout)
            for i in range(m):
                ya, sa, _ = P.op_conv2d_views(xs[i:i + 1], 0, wt, b, y0[i:i + 1], 8, amax_out=slot0[i:i + 1], **kw)
                if not _same_bits(ya[0], y[i]) or sa[0] != slots[i]:
                    t.bad(*tag, f"image {i} alone differs from the batch in {int((_bits(ya[0]) != _bits(y[i])).sum())} values, slot {sa[0]:#x} / {slots[i]:#x}")
            r = t.call(P, family, lambda: P.op_conv2d_views(xgb, 0, wt, b, yb, 8, amax_out=slot0[:m], gate=mask[:m], **kw))
            if r is None:
                continue
            _check_gated(t, tag + ("gated",), mask[:m], r[0], r[1], y, slots, y0, slot0)
            _check_slots(t, tag + ("gated",), r[1], r[0], 8, cout, skip=[i for i in range(m) if not mask[i]])
            if r[2] != 0:
                t.bad(*tag, f"gated stray {r[2]}")
    finally:
        P.op_conv2d_shape(-1)
    t.report(minimum=("pw",))
    assert t.ran.get("pw", 0) == 2 * len(shapes), t.ran

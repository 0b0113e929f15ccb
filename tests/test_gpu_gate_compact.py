"""Compaction of gated tile tables (Level::compact_gated, gate_scan_kernel + gate_scatter_kernel in csrc/det_post.hip) through the op-level conv entry
tests/test_gpu_conv_views.py uses: a gated 3x3 conv (it walks the level's gated tile table) and a gated 1x1 conv on tiny images of 16 channels, sizes
cycling through (1, 3), (3, 20), (17, 5) — one tile, two tiles side by side, two tiles one above the other — in FFP_PREC_F32X3 with one max-|value|
slot per image, as the detector's plans run their gated towers (the 1x1 conv also in plain fp32: _precisions).

n_img runs over 1, 2, 63, 64, 65, 257, 1025: one image, a wave's width and its neighbours, more than one round of the scan's 256-image blocks, more
than four. Masks: none active, all, only the first, only the last, alternating, a seeded random half.

The contract is the gate's existing one:
  * an active image has the ungated call's bits, its slot included;
  * an inactive image's record and slot are what went up (its input goes up as NaN: nothing of it may be read into an active image either);
  * a second run with another mask on the same tables (gate_prev: the tables are compacted again, with the first run's entries still behind the
    count) gives the second mask's result;
  * nothing is written where the conv may not write (`stray` == 0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 16
SIZES = [(1, 3), (3, 20), (17, 5)]
N_IMG = [1, 2, 63, 64, 65, 257, 1025]
SLOT0 = 0x00000101


def _masks(n):
    rng = np.random.default_rng(7000 + n)
    half = np.zeros(n, np.int32)
    half[rng.permutation(n)[:n // 2]] = 1
    first, last = np.zeros(n, np.int32), np.zeros(n, np.int32)
    first[0] = 1
    last[-1] = 1
    return {"none": np.zeros(n, np.int32), "all": np.ones(n, np.int32), "first": first, "last": last,
            "alternating": (np.arange(n) % 2 == 0).astype(np.int32), "half": half}


def _precisions(P, n, k):
    """The split arithmetic with a slot per image, as the plans run their gated towers; the 1x1 conv also in plain fp32 — and only there for a single
    image, where a slot per image is a slot per buffer and the split 1x1 kernels run ungated by design (tests/test_gpu_conv_views.py pins that)."""
    if k == 3:
        return [P.PREC_F32X3]
    return ([P.PREC_F32X3] if n > 1 else []) + [P.PREC_F32]


@pytest.fixture(scope="module")
def cases(gpu_lib):
    """Per (n_img, k, precision): inputs, the records going up, and the ungated call's result — computed once, shared by every mask."""
    P = gpu_lib
    out = {}
    for n in N_IMG:
        rng = np.random.default_rng(100 + n)
        hw = [SIZES[i % len(SIZES)] for i in range(n)]
        xs = [rng.standard_normal((h, w, C)).astype(np.float32) for h, w in hw]
        y0 = [rng.integers(-1000, 1000, (h, w, C + 8)).astype(np.float32) for h, w in hw]
        for k in (3, 1):
            wt = (rng.standard_normal((C, C, k, k)) / np.sqrt(C * k * k)).astype(np.float32)
            b = (rng.standard_normal(C) * 0.1).astype(np.float32)
            for prec in _precisions(P, n, k):
                per_img = prec == P.PREC_F32X3
                slot0 = (SLOT0 + np.arange(n if per_img else 1)).astype(np.uint32)
                kw = dict(act=1, px_align=32, per_image_amax=per_img, amax_out=slot0, precision=prec)
                ung = P.op_conv2d_views(P.OpBatch(xs), 0, wt, b, P.OpBatch(y0), 8, **kw)
                assert ung[2] == 0
                out[n, k, prec] = (xs, y0, slot0, wt, b, kw, ung)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(mask, got, ung, y0, slot0, what):
    y, slots, stray = got
    assert stray == 0, f"{what}: stray {stray}"
    per_img = len(slots) == len(mask)      # the split arithmetic: a slot per image, raised by the conv (a single image's slot too)
    for i, m in enumerate(mask):
        assert np.array_equal(_bits(y[i]), _bits(ung[0][i] if m else y0[i])), f"{what}: {'active' if m else 'inactive'} image {i} differs"
        if per_img:
            want_slot = ung[1][i] if m else slot0[i]
            assert slots[i] == want_slot, f"{what}: {'active' if m else 'inactive'} image {i}: slot {int(slots[i]):#x}, expected {int(want_slot):#x}"
    if not per_img:      # plain fp32 raises no slot: the buffer's is what went up under every mask
        assert slots[0] == slot0[0], f"{what}: the buffer's slot {int(slots[0]):#x}, went up as {int(slot0[0]):#x}"


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("n", N_IMG)
def test_gated_conv_under_every_mask(gpu_lib, cases, n, k):
    P = gpu_lib
    masks = _masks(n)
    names = list(masks)
    for prec in _precisions(P, n, k):
        xs, y0, slot0, wt, b, kw, ung = cases[n, k, prec]
        yb = P.OpBatch(y0)
        for j, name in enumerate(names):
            mask = masks[name]
            what = f"n {n} k {k} precision {prec} mask {name}"
            xg = P.OpBatch([x if m else np.full_like(x, np.nan) for x, m in zip(xs, mask)])
            got = P.op_conv2d_views(xg, 0, wt, b, yb, 8, gate=mask, **kw)
            _check(mask, got, ung, y0, slot0, what)
            # the same tables compacted a second time: the run before used the next mask of the list (its inactive inputs are this mask's)
            prev = masks[names[(j + 1) % len(names)]]
            got = P.op_conv2d_views(xg, 0, wt, b, yb, 8, gate=mask, gate_prev=prev, **kw)
            _check(mask, got, ung, y0, slot0, what + " after " + names[(j + 1) % len(names)])

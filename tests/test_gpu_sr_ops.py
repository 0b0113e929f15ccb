"""Operator-level parity of the kernels around the Real-ESRGAN network — sr_pre_kernel, sr_post_kernel, crop_gather_kernel
(csrc/sr_ops.hip), alpha_linear_kernel (csrc/resize.hip) — and of the tile geometry (csrc/sr_tiles.hpp) that feeds them, through the
ffp_op_sr_* / ffp_op_alpha_linear / ffp_op_crop_gather entries: no weights, no plan, no network.

Every comparison is an equality of bits. The kernels' arithmetic is float32 without contraction and with correctly rounded division, and the
reference performs the same operations in the same order: it is the oracle of tests/realesrgan_formats_ref.py driven with a fake network
(tests/sr_ops_common.py) that records the tensors it is handed — what sr_pre has to write — and returns prescribed tensors, from which
`enhance` computes the canvas sr_post has to write. The fp16 expectation is np.float16 of the float32 value.

The prescribed network outputs hold, in every tile, values below 0 and above 1, -0.0, +-inf, k / range exactly, exact ties k + 0.5 under
`* range` for even and odd k, and ordinary values. NaN is left out: the oracle casts NaN to an integer type, which is undefined. The unused
fourth channel of every network record holds a large finite sentinel.

Buffers are compared whole: flat level buffers and canvases go up filled with a known pattern, and every record or byte that belongs to no
tile of the batch, to no core, to row padding, to the gaps between and before the images or to a channel the selection must not write has to
come back as it went up."""
import ctypes as C

import numpy as np
import pytest

import realesrgan_formats_ref as R
import sr_ops_common as S

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = F32(-7.0)            # exact in fp16 and fp32, negative: no kernel writes it
SENTINEL = F32(3.0e38)      # channel 3 of the network records

# (scale, h, w, tile, tile_pad, pre_pad, strided source / canvas). The smallest that reach each branch: one-pixel sides at x4; odd sizes at x2
# take the mod pad, with pre_pad 1 the double reflect (31 + 1 and 17 + 1 are even: the pre-pad alone; 45 + 1 even, 20 + 1 odd: both); 19x23 under
# three tilings (pad < tile, pad > tile, no pad) has partial last tiles; pre_pad h - 1 is the largest reflect; tight and strided buffers.
GEOMS = [
    (4, 1, 1, 0, 10, 0, True), (4, 1, 7, 0, 10, 0, False), (4, 7, 1, 0, 10, 0, True), (4, 1, 7, 2, 2, 0, True),
    (2, 2, 2, 0, 10, 0, True), (2, 2, 2, 0, 10, 1, False), (2, 3, 5, 0, 10, 0, True), (2, 3, 5, 0, 10, 1, True), (2, 3, 5, 0, 10, 2, False),
    (2, 17, 20, 0, 10, 0, True), (2, 17, 20, 0, 10, 1, True), (2, 17, 20, 0, 10, 3, False), (2, 17, 20, 0, 10, 16, True),
    (2, 31, 45, 0, 10, 1, True), (2, 31, 45, 16, 4, 30, True),
    (4, 19, 23, 8, 4, 0, True), (4, 19, 23, 8, 20, 1, True), (4, 19, 23, 16, 0, 3, False), (4, 19, 23, 8, 4, 18, True),
    (2, 19, 23, 8, 4, 1, True), (2, 19, 23, 8, 20, 0, True), (2, 19, 23, 16, 0, 3, True), (2, 19, 23, 8, 20, 18, False),
]
GEOM_IDS = [f"x{g[0]}-{g[1]}x{g[2]}-t{g[3]}p{g[4]}-pre{g[5]}-{'strided' if g[6] else 'tight'}" for g in GEOMS]

_cases = {}


def case(name, scale, h, w, tile, tile_pad, pre_pad):
    """One oracle run of a layout: (image, max_range, expected canvas, {selection: (recorded inputs, prescribed outputs)})."""
    key = (name, scale, h, w, tile, tile_pad, pre_pad)
    if key not in _cases:
        _, cn, _, max_range = S.layout(name)
        img = S.make_image(name, h, w, 11)
        fake = S.FakeNet(scale, S.prescribed_out(max_range, 3))
        out, ins, outs = S.enhance_with(fake, img, tile, tile_pad, pre_pad)
        sels = S.selections(cn)
        n = len(ins) // len(sels)
        per_sel = {sel: (ins[k * n:(k + 1) * n], outs[k * n:(k + 1) * n]) for k, sel in enumerate(sels)}
        assert out.dtype == (np.uint16 if max_range == 65535 else np.uint8)
        _cases[key] = (img, max_range, out, per_sel)
    return _cases[key]


def put_source(strided, img):
    """The image inside a byte buffer: (Buffer, bytes, item index)."""
    b = S.Buffer(strided)
    a = img[..., None] if img.ndim == 2 else img
    i = b.add(a.shape[0], a.shape[1], a.shape[2], a.dtype)
    buf = b.alloc()
    b.view(buf, i)[...] = a
    return b, buf, i


def f16_of(x, prec, lib):
    return x.astype(np.float16).astype(F32) if prec == lib.PREC_F16 else x


def check_pre(lib, prec, got_tiles, flat, offs, recs, fill_before=None):
    """Tiles equal the recorded tensors, pad channels are +0.0, every other record of the flat buffer holds what it held before."""
    assert len(got_tiles) == len(recs)
    owned = np.zeros(flat.shape[0], bool)
    for t, o, rec in zip(got_tiles, offs.tolist(), recs):
        c = rec.shape[2]
        assert t.shape[:2] == rec.shape[:2] and t.shape[2] >= c
        assert np.array_equal(t[..., :c], f16_of(rec, prec, lib))
        assert np.array_equal(t[..., c:], np.zeros_like(t[..., c:])) and not np.signbit(t[..., c:]).any()
        assert not owned[o:o + rec.shape[0] * rec.shape[1]].any()
        owned[o:o + rec.shape[0] * rec.shape[1]] = True
    before = np.full_like(flat, FILL) if fill_before is None else fill_before
    assert np.array_equal(flat[~owned], before[~owned])
    return owned


def with_sentinel(outs, cs=4):
    res = []
    for o in outs:
        t = np.full(o.shape[:2] + (cs,), SENTINEL, F32)
        t[..., :3] = o
        res.append(t)
    return res


def sel_channels(sel):
    return {S.SEL_BGR: slice(0, 3), S.SEL_GRAY: slice(0, 1), S.SEL_ALPHA: slice(3, 4)}[sel]


def oracle_plane(out, sel):
    o = out[..., None] if out.ndim == 2 else out
    return o[..., sel_channels(sel)]


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_sr_pre_equals_the_tensors_the_oracle_hands_its_network(gpu_lib, geom, prec):
    lib = gpu_lib
    P = lib.PREC_F16 if prec == "f16" else lib.PREC_F32
    scale, h, w, tile, tile_pad, pre_pad, strided = geom
    for name, cn, _, _ in S.LAYOUTS:
        img, max_range, _, per_sel = case(name, scale, h, w, tile, tile_pad, pre_pad)
        b, buf, i = put_source(strided, img)
        for sel, (recs, _) in per_sel.items():
            tiles, flat, offs = lib.op_sr_pre(buf, [b.desc(i, max_range, sel)], scale, tile, tile_pad, pre_pad, P, fill=FILL)
            owned = check_pre(lib, P, tiles, flat, offs, recs)
            assert owned.all()                                    # an exact level has no gaps


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_sr_post_equals_the_oracles_canvas(gpu_lib, geom):
    lib = gpu_lib
    scale, h, w, tile, tile_pad, pre_pad, strided = geom
    for name, cn, _, _ in S.LAYOUTS:
        _, max_range, out, per_sel = case(name, scale, h, w, tile, tile_pad, pre_pad)
        b = S.Buffer(strided, fill_seed=cn)
        i = b.add(scale * h, scale * w, cn, out.dtype)
        before = b.alloc()
        calls = [[sel] for sel in per_sel] + ([list(per_sel)] if len(per_sel) > 1 else [])      # each selection alone; BGRA also as one batch
        for sels in calls:
            want = before.copy()
            for sel in sels:
                b.view(want, i)[..., sel_channels(sel)] = oracle_plane(out, sel)
            descs = [b.desc(i, max_range, sel, h, w) for sel in sels]
            nets = [t for sel in sels for t in with_sentinel(per_sel[sel][1])]
            got = lib.op_sr_post(before, descs, nets, scale, tile, tile_pad, pre_pad)
            # whole buffer: cores, row padding, the bytes before and behind the canvas, and the channels the selection leaves alone
            assert np.array_equal(got, want), (name, sels)


def core_boxes(scale, h, w, tile, pre_pad):
    """(y0, y1, x0, x1) of every tile's core in the canvas, tiles row by row: RealESRGANer.tile_process' output ranges clipped to the
    un-padded output."""
    H, W = h + pre_pad, w + pre_pad
    if scale == 2:
        H, W = H + H % 2, W + W % 2
    t = tile if tile > 0 else max(H, W)
    return [(sy * scale, min(min(sy + t, H) * scale, scale * h), sx * scale, min(min(sx + t, W) * scale, scale * w))
            for sy in range(0, H, t) for sx in range(0, W, t)]


@pytest.mark.parametrize("geom", [g for g in GEOMS if g[3] > 0], ids=[i for g, i in zip(GEOMS, GEOM_IDS) if g[3] > 0])
def test_sr_post_one_tile_writes_its_core_and_nothing_else(gpu_lib, geom):
    """In a whole batch a write outside a tile's core lands in a neighbour's core and is overwritten. With every other core emptied it stays."""
    lib = gpu_lib
    scale, h, w, tile, tile_pad, pre_pad, strided = geom
    for name in ("bgr8", "gray16", "bgra16r255"):
        _, cn, _, _ = S.layout(name)
        _, max_range, out, per_sel = case(name, scale, h, w, tile, tile_pad, pre_pad)
        sel = list(per_sel)[-1]                                   # BGRA: the alpha pass
        b = S.Buffer(strided, fill_seed=cn)
        i = b.add(scale * h, scale * w, cn, out.dtype)
        before = b.alloc()
        nets = with_sentinel(per_sel[sel][1])
        boxes = core_boxes(scale, h, w, tile, pre_pad)
        assert len(boxes) == len(nets) > 1
        painted = np.zeros((scale * h, scale * w), int)
        for k, (y0, y1, x0, x1) in enumerate(boxes):
            want = before.copy()
            if y1 > y0 and x1 > x0:
                b.view(want, i)[y0:y1, x0:x1, sel_channels(sel)] = oracle_plane(out, sel)[y0:y1, x0:x1]
                painted[y0:y1, x0:x1] += 1
            got = lib.op_sr_post(before, [b.desc(i, max_range, sel, h, w)], nets, scale, tile, tile_pad, pre_pad, only_tile=k)
            assert np.array_equal(got, want), (name, k)
        assert (painted == 1).all()


# ---- ragged batches and capacity-mode levels ---------------------------------------------------------------------------------------
RAGGED = [("gray8", 5, 9), ("bgr16", 7, 4), ("bgra8", 6, 6)]          # four images: the BGRA buffer is read twice (colour, alpha)
SMALL = [("bgr8", 3, 5), ("gray16", 4, 4)]


class Batch:
    """Several layouts in one source buffer and one canvas buffer, every image enhanced by its own oracle call."""

    def __init__(self, specs, scale, tile, tile_pad, pre_pad, src=None, dst=None):
        self.src = src or S.Buffer(True)
        self.dst = dst or S.Buffer(True, fill_seed=9)
        self.items = []
        for name, h, w in specs:
            _, cn, dt, max_range = S.layout(name)
            img, _, out, per_sel = case(name, scale, h, w, tile, tile_pad, pre_pad)
            si = self.src.add(h, w, cn, dt)
            di = self.dst.add(scale * h, scale * w, cn, out.dtype)
            self.items.append((img, out, per_sel, si, di, max_range, h, w))

    def fill_source(self, buf):
        for img, _, _, si, *_ in self.items:
            self.src.view(buf, si)[...] = img[..., None] if img.ndim == 2 else img

    def src_descs(self):
        return [self.src.desc(si, mr, sel) for _, _, per_sel, si, _, mr, _, _ in self.items for sel in per_sel]

    def dst_descs(self):
        return [self.dst.desc(di, mr, sel, h, w) for _, _, per_sel, _, di, mr, h, w in self.items for sel in per_sel]

    def recs(self):
        return [r for _, _, per_sel, *_ in self.items for sel in per_sel for r in per_sel[sel][0]]

    def nets(self, cs=4):
        return [t for _, _, per_sel, *_ in self.items for sel in per_sel for t in with_sentinel(per_sel[sel][1], cs)]

    def paint(self, canvas):
        for _, out, per_sel, _, di, *_ in self.items:
            for sel in per_sel:
                self.dst.view(canvas, di)[..., sel_channels(sel)] = oracle_plane(out, sel)


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("scale", [4, 2])
def test_ragged_batch_of_four_layouts(gpu_lib, scale, prec):
    lib = gpu_lib
    P = lib.PREC_F16 if prec == "f16" else lib.PREC_F32
    tile, tile_pad, pre_pad = 4, 2, 1
    bt = Batch(RAGGED, scale, tile, tile_pad, pre_pad)
    assert len(bt.src_descs()) == 4
    buf = bt.src.alloc()
    bt.fill_source(buf)
    tiles, flat, offs = lib.op_sr_pre(buf, bt.src_descs(), scale, tile, tile_pad, pre_pad, P, fill=FILL)
    assert check_pre(lib, P, tiles, flat, offs, bt.recs()).all()
    if prec == "f32":
        before = bt.dst.alloc()
        want = before.copy()
        bt.paint(want)
        assert np.array_equal(lib.op_sr_post(before, bt.dst_descs(), bt.nets(5), scale, tile, tile_pad, pre_pad), want)


@pytest.mark.parametrize("scale", [4, 2])
def test_capacity_mode_level_after_a_larger_batch(gpu_lib, scale):
    """Level::reserve / assign with the capacities a plan gives its levels: the batch alone, and behind a larger batch that has filled the tables
    and the buffers. Records and bytes outside the second batch's tiles and cores keep what the first batch left there."""
    lib = gpu_lib
    tile, tile_pad, pre_pad = 4, 2, 0
    big = Batch(RAGGED, scale, tile, tile_pad, pre_pad)
    small = Batch(SMALL, scale, tile, tile_pad, pre_pad, src=big.src, dst=big.dst)
    buf = big.src.alloc()
    big.fill_source(buf)
    small.fill_source(buf)
    _, t16_big, _ = lib.op_sr_tiles(big.src_descs(), scale, tile, tile_pad, pre_pad)
    _, t16_small, _ = lib.op_sr_tiles(small.src_descs(), scale, tile, tile_pad, pre_pad)
    assert t16_small < t16_big
    cap = t16_big + 5
    for P in (lib.PREC_F32, lib.PREC_F16):
        kw = dict(scale=scale, tile=tile, tile_pad=tile_pad, pre_pad=pre_pad, precision=P, fill=FILL, cap_t16=cap)
        t1, flat1, o1 = lib.op_sr_pre(buf, big.src_descs(), **kw)
        owned1 = check_pre(lib, P, t1, flat1, o1, big.recs())
        assert flat1.shape[0] == 256 * cap and not owned1.all()
        ta, flata, oa = lib.op_sr_pre(buf, small.src_descs(), **kw)
        check_pre(lib, P, ta, flata, oa, small.recs())
        t2, flat2, o2 = lib.op_sr_pre(buf, small.src_descs(), first=big.src_descs(), **kw)
        owned2 = check_pre(lib, P, t2, flat2, o2, small.recs(), fill_before=flat1)
        assert (owned1 & ~owned2).any()                     # records the larger batch wrote and the smaller one must leave alone
    before = big.dst.alloc()
    kw = dict(scale=scale, tile=tile, tile_pad=tile_pad, pre_pad=pre_pad, cap_t16=cap)
    want1 = before.copy()
    big.paint(want1)
    assert np.array_equal(lib.op_sr_post(before, big.dst_descs(), big.nets(), **kw), want1)
    wanta = before.copy()
    small.paint(wanta)
    assert np.array_equal(lib.op_sr_post(before, small.dst_descs(), small.nets(), **kw), wanta)
    want2 = want1.copy()
    small.paint(want2)
    assert np.array_equal(lib.op_sr_post(before, small.dst_descs(), small.nets(), first=(big.dst_descs(), big.nets()), **kw), want2)
    # a level that is exactly full: no padding entry behind the last tile
    kw["cap_t16"] = t16_big
    assert np.array_equal(lib.op_sr_post(before, big.dst_descs(), big.nets(), **kw), want1)
    tf, flatf, of = lib.op_sr_pre(buf, big.src_descs(), scale, tile, tile_pad, pre_pad, lib.PREC_F32, fill=FILL, cap_t16=t16_big)
    check_pre(lib, lib.PREC_F32, tf, flatf, of, big.recs())


def test_bad_arguments_leave_the_buffers_alone(gpu_lib):
    lib = gpu_lib
    l = lib.lib()
    img = np.arange(8 * 8 * 4, dtype=np.uint8)
    d = np.array([[0, 32, 8, 8, 4, 8, 255, S.SEL_BGR]], np.int64)
    dp = d.ctypes.data_as(C.POINTER(C.c_int64))
    flat = np.full((64, 4), FILL, F32)
    offs = np.zeros(4, np.int64)
    op = offs.ctypes.data_as(C.POINTER(C.c_int64))
    net = np.zeros((32 * 32, 4), F32)
    canvas = np.full(32 * 32 * 4, 0x5A, np.uint8)
    dc = np.array([[0, 128, 8, 8, 4, 8, 255, S.SEL_BGR]], np.int64)
    dcp = dc.ctypes.data_as(C.POINTER(C.c_int64))

    def pre(src=img.ctypes.data, n=1, imgs=dp, scale=4, prec=lib.PREC_F32, cap=0, out=flat.ctypes.data, npx=64, off=op):
        return l.ffp_op_sr_pre(0, prec, src, img.size, n, imgs, scale, 0, 10, 0, cap, 0, None, out, npx, off)

    def post(n=1, imgs=dcp, scale=4, nt=net.ctypes.data, cs=4, cap=0, only=-1, out=canvas.ctypes.data):
        return l.ffp_op_sr_post(0, n, imgs, scale, 0, 10, 0, nt, cs, cap, 0, None, None, only, out, canvas.size)

    assert pre() == 0 and post() == 0                                              # the calls themselves are well formed
    flat[...] = FILL
    canvas[...] = 0x5A
    bad = [pre(src=None), pre(imgs=None), pre(out=None), pre(off=None), pre(scale=3), pre(scale=1), pre(prec=7), pre(npx=63),
           post(imgs=None), post(nt=None), post(out=None), post(scale=8), post(cs=2), post(only=1), post(only=-2)]
    # a batch over the capacity: 64 x 64 pixels are 16 body tiles of 16x16
    big = np.array([[0, 192, 64, 64, 3, 8, 255, S.SEL_BGR]], np.int64)
    bigp = big.ctypes.data_as(C.POINTER(C.c_int64))
    src = np.zeros(64 * 64 * 3, np.uint8)
    flat_cap = np.full((256 * 15, 4), FILL, F32)
    bad.append(l.ffp_op_sr_pre(0, lib.PREC_F32, src.ctypes.data, src.size, 1, bigp, 4, 0, 10, 0, 15, 0, None, flat_cap.ctypes.data, 256 * 15, op))
    bigc = np.array([[0, 768, 64, 64, 3, 8, 255, S.SEL_BGR]], np.int64)
    big_canvas = np.full(256 * 256 * 3, 0x5A, np.uint8)
    big_net = np.zeros((256 * 256, 4), F32)
    bad.append(l.ffp_op_sr_post(0, 1, bigc.ctypes.data_as(C.POINTER(C.c_int64)), 4, 0, 10, 0, big_net.ctypes.data, 4, 15, 0, None, None,
                                -1, big_canvas.ctypes.data, big_canvas.size))
    # a description that leaves its buffer, a 16-bit range in 8-bit storage, alpha of a 3-channel image
    for row in ([0, 32, 9, 8, 4, 8, 255, 0], [8, 32, 8, 8, 4, 8, 255, 0], [0, 31, 8, 8, 4, 8, 255, 0], [0, 32, 8, 8, 4, 8, 65535, 0],
                [0, 32, 8, 8, 3, 8, 255, 2], [0, 32, 8, 8, 2, 8, 255, 0], [1, 64, 8, 4, 4, 16, 255, 0]):
        r = np.array([row], np.int64)
        bad.append(pre(imgs=r.ctypes.data_as(C.POINTER(C.c_int64))))
    # the 'cv2' alpha: 8-bit source with a 16-bit canvas, range 65535 into 8 bits; the crop gather: a box that leaves the frame, an offset that leaves the output
    a8, a16 = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint16)
    d8, d16 = np.full((8, 8, 4), 0x5A, np.uint8), np.full((8, 8, 4), 0x5A5A, np.uint16)
    bad += [l.ffp_op_alpha_linear(0, a8.ctypes.data, 4, 4, 8, 255, 8, 8, 16, d16.ctypes.data),
            l.ffp_op_alpha_linear(0, a16.ctypes.data, 4, 4, 16, 65535, 8, 8, 8, d8.ctypes.data),
            l.ffp_op_alpha_linear(0, None, 4, 4, 8, 255, 8, 8, 8, d8.ctypes.data), l.ffp_op_alpha_linear(0, a8.ctypes.data, 4, 4, 8, 255, 8, 8, 8, None),
            l.ffp_op_alpha_linear(0, a8.ctypes.data, 4, 4, 8, 255, 0, 8, 8, d8.ctypes.data)]
    frame = np.zeros((10, 12, 3), np.uint8)
    out = np.full(64, 0x5A, np.uint8)
    for box, off in (([8, 0, 5, 2], 0), ([0, 9, 2, 2], 0), ([0, 0, 4, 4], 32), ([0, 0, 2, 2], -1), ([0, 0, 0, 2], 0)):
        bx, of = np.array(box, np.int32), np.array([off], np.int64)
        bad.append(l.ffp_op_crop_gather(0, frame.ctypes.data, 10, 12, 1, bx.ctypes.data_as(C.POINTER(C.c_int32)), of.ctypes.data_as(C.POINTER(C.c_int64)),
                                        out.ctypes.data, out.size))
    bad.append(l.ffp_op_crop_gather(0, None, 10, 12, 0, None, None, out.ctypes.data, out.size))
    assert bad == [1] * len(bad), bad
    assert (flat == FILL).all() and (flat_cap == FILL).all() and (canvas == 0x5A).all() and (big_canvas == 0x5A).all()
    assert (d8 == 0x5A).all() and (d16 == 0x5A5A).all() and (out == 0x5A).all()


# ---- the 'cv2' alpha upsampler ------------------------------------------------------------------------------------------------------
ALPHA_SIZES = [((1, 1), (4, 4)), ((1, 7), (4, 28)), ((5, 1), (10, 2)), ((9, 13), (36, 52)), ((9, 13), (18, 26)), ((9, 13), (9, 13)), ((12, 10), (5, 7))]


@pytest.mark.parametrize("src_dt,dst_dt,max_range", [(np.uint8, np.uint8, 255), (np.uint16, np.uint8, 255), (np.uint16, np.uint16, 65535)],
                         ids=["u8-u8", "u16-u8", "u16-u16"])
@pytest.mark.parametrize("src_hw,dst_hw", ALPHA_SIZES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in ALPHA_SIZES])
def test_alpha_linear_equals_the_restated_cv2_resize(gpu_lib, src_hw, dst_hw, src_dt, dst_dt, max_range):
    rng = np.random.default_rng([src_hw[0], src_hw[1], dst_hw[0], max_range])
    top = max_range if src_dt == np.uint8 or max_range == 65535 else 256          # 16-bit storage under range 255 holds up to 256: above 1, clipped
    src = rng.integers(0, top, src_hw + (4,), endpoint=True).astype(src_dt)
    src[rng.integers(0, src_hw[0]), rng.integers(0, src_hw[1]), 3] = top
    before = rng.integers(0, np.iinfo(dst_dt).max, dst_hw + (4,), endpoint=True).astype(dst_dt)
    got = gpu_lib.op_alpha_linear(src, before, max_range)
    a = R.resize_linear_f32(src[..., 3].astype(F32) / F32(max_range), dst_hw[1], dst_hw[0])
    want = before.copy()
    want[..., 3] = np.clip(np.rint(a * F32(max_range)), 0, max_range).astype(dst_dt)
    assert got.dtype == dst_dt and np.array_equal(got, want)                       # channels 0-2 keep what they held


# ---- the crop gather ----------------------------------------------------------------------------------------------------------------
def test_crop_gather_equals_slicing(gpu_lib):
    H, W = 37, 53
    rng = np.random.default_rng(41)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    # 1x1; the full frame; flush with the right and bottom edges; 3 * w no multiple of 4; more than 16 * 256 bytes (the grid-stride loop iterates)
    boxes = [(5, 7, 1, 1), (0, 0, W, H), (40, 30, 13, 7), (3, 2, 5, 4), (6, 4, 45, 32)]
    assert boxes[4][2] * boxes[4][3] * 3 > 16 * 256 and (boxes[3][2] * 3) % 4 != 0
    offs, pos = [], 0
    for _, _, w, h in boxes:
        offs.append(pos)
        pos += (w * h * 3 + 15) // 16 * 16
    before = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    want = before.copy()
    for (x0, y0, w, h), o in zip(boxes, offs):
        want[o:o + w * h * 3] = frame[y0:y0 + h, x0:x0 + w].reshape(-1)
    got = gpu_lib.op_crop_gather(frame, boxes, offs, before)
    assert np.array_equal(got, want)                                               # the gaps between the rounded offsets keep what they held
    # the boxes in another order and at unaligned offsets
    order = [4, 0, 3, 2, 1]
    offs2, pos = [], 3
    for k in order:
        offs2.append(pos)
        pos += boxes[k][2] * boxes[k][3] * 3 + 1
    before2 = rng.integers(0, 256, pos + 5, dtype=np.uint8)
    want2 = before2.copy()
    for k, o in zip(order, offs2):
        x0, y0, w, h = boxes[k]
        want2[o:o + w * h * 3] = frame[y0:y0 + h, x0:x0 + w].reshape(-1)
    assert np.array_equal(gpu_lib.op_crop_gather(frame, [boxes[k] for k in order], offs2, before2), want2)
    assert np.array_equal(gpu_lib.op_crop_gather(frame, [], [], before), before)   # n = 0 is accepted and leaves the output alone

"""CPU tests of the host side: the C-ABI library loads and exports every symbol include/ffp.h declares, the pure host
entry points agree with the oracle, compute entry points fail loudly without a GPU, the weight container round-trips."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ffp_amd  # noqa: F401
from ffp_amd import _lib, arch, pipeline, synth, weights_io
from oracle import sahi_ref, ultra_post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ffp_amd import build
    build.build(verbose=False)
    return _lib.lib()


def test_every_declared_symbol_is_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ffp.h")).read()
    declared = set(re.findall(r"\b(ffp_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/ffp.h but not exported by libffp.so"
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    assert lib.ffp_version() >= 200
    # the ctypes table is derived from the header (_abi.parse): a row per prototype, every row set on the loaded library
    assert declared == set(_lib._SIGS) and len(re.findall(r"\bffp_[a-z0-9_]+\s*\([^()]*\)\s*;", hdr)) == len(_lib._SIGS)
    for name, (res, args) in _lib._SIGS.items():
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes) == args, name
    assert _lib._SIGS["ffp_last_error"] == (C.c_char_p, []) and _lib._SIGS["ffp_det_destroy"] == (None, [C.c_void_p])
    assert _lib._SIGS["ffp_op_scrfd_post"][1][7] is C.POINTER(C.POINTER(C.c_float))
    # nothing is skipped: a prototype outside the vocabulary is refused by name
    from ffp_amd import _abi
    for text, what in (("int ffp_x(int (*cb)(int));", "ffp_x"), ("int ffp_y(int a[4]);", "ffp_y"), ("int ffp_z(unsigned a);", "ffp_z"),
                       ("int ffp_ok(int a);\nint ffp_half(int a", "ffp_half")):
        with pytest.raises(ValueError, match=what):
            _abi.parse(text)


def test_conv_shape_table_through_shape_name(lib):
    """The shape numbers of csrc/conv_route.hpp, read without a device: exactly 0..25 have a name, '<family> <suffix>' is unique but for
    the rows configurations (6 / 7 / 8) and the two rows16 forms (9 / 23), whose variant strings have always been shared, and the pw and
    k3d numbers are the keys of the GPU conv tests' PW_SHAPES and K3D_SHAPES."""
    import ast
    names = {}
    for shape in range(-4, 130):
        try:
            names[shape] = tuple(_lib.op_conv2d_shape_name(shape).split())
        except _lib.FfpError as e:
            assert e.code == 1, shape
    assert sorted(names) == list(range(26))
    for bad in (-2, 26, 99):
        with pytest.raises(_lib.FfpError) as e:
            _lib.op_conv2d_shape_name(bad)
        assert e.value.code == 1
    assert all(len(v) == 2 for v in names.values()), names
    groups = {}
    for shape, v in names.items():
        groups.setdefault(v, []).append(shape)
    assert sorted(g for g in groups.values() if len(g) > 1) == [[6, 7, 8], [9, 23]], groups
    assert groups[("rows", "rows")] == [6, 7, 8] and groups[("rows16", "rows16")] == [9, 23]
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_conv.py")).read())
    consts = {t.id: ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) for t in n.targets
              if isinstance(t, ast.Name) and t.id in ("PW_SHAPES", "K3D_SHAPES")}
    assert sorted(consts["PW_SHAPES"]) == sorted(s for s, v in names.items() if v[0] == "pw")
    assert sorted(consts["K3D_SHAPES"]) == sorted(s for s, v in names.items() if v[0] == "k3d")


def test_slice_bboxes_matches_oracle(lib):
    for (H, W, s, o) in [(2160, 3840, 512, 0.2), (4320, 7680, 640, 0.25), (300, 400, 512, 0.2), (513, 1025, 512, 0.0), (1000, 777, 333, 0.37)]:
        assert _lib.slice_bboxes(H, W, s, s, o, o).tolist() == sahi_ref.get_slice_bboxes(H, W, s, s, o, o)
    with pytest.raises(_lib.FfpError):
        _lib.slice_bboxes(100, 100, 0, 10)


def test_letterbox_geometry_matches_oracle(lib):
    rng = np.random.default_rng(0)
    for _ in range(200):
        h, w = int(rng.integers(8, 5000)), int(rng.integers(8, 5000))
        s = int(rng.choice([256, 512, 640, 1024]))
        assert _lib.letterbox_geometry(h, w, s) == ultra_post.letterbox_geometry(h, w, s), (h, w, s)


def test_tile_chunks_are_even_and_larger_first(lib):
    """ffp_tile_chunks, the one statement of how the tile entry points split n items at a positive max_batch: the shapes the engine
    comments and the GPU tests name, then the rule itself (ceil(n / m) chunks, sizes within one of each other, not increasing)."""
    for (n, m), want in {(61, 16): [16, 15, 15, 15], (13, 5): [5, 4, 4], (7, 3): [3, 2, 2], (61, 8): [8, 8, 8, 8, 8, 7, 7, 7], (5, 8): [5],
                         (0, 4): []}.items():
        assert _lib.tile_chunks(n, m) == want, (n, m)
    for n in range(1, 71):
        for m in range(1, 21):
            c = _lib.tile_chunks(n, m)
            assert len(c) == -(-n // m) and sum(c) == n and max(c) <= m and max(c) - min(c) <= 1 and c == sorted(c, reverse=True), (n, m, c)
    k = C.c_int32(-1)
    first = np.zeros(2, np.int32)                                       # fewer than there are: cap sizes written, the full count returned
    assert lib.ffp_tile_chunks(61, 16, first.ctypes.data_as(C.POINTER(C.c_int32)), 2, C.byref(k)) == 0
    assert k.value == 4 and first.tolist() == [16, 15]
    for n, m in ((5, 0), (5, -1), (-1, 4)):
        with pytest.raises(_lib.FfpError) as e:
            _lib.tile_chunks(n, m)
        assert e.value.code == 1, (n, m)


def test_compute_calls_fail_loudly_without_gpu(lib):
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.FfpError) as e:
        _lib.Detector(synth.yolo11_pose_weights("n"), arch="n")
    assert "no HIP device" in str(e.value)
    with pytest.raises(_lib.FfpError):
        _lib.merge(np.zeros((3, 6), np.float32))
    with pytest.raises(_lib.FfpError):
        _lib.Enhancer({"conv_first.weight": np.zeros((64, 3, 3, 3), np.float32)})
    with pytest.raises(_lib.FfpError):
        _lib.op_conv2d(np.zeros((1, 4, 4, 4), np.float32), np.zeros((4, 4, 1, 1), np.float32), None)
    # every family of entries that takes a device number: arguments that are valid up to the device check -> FFP_ERR_HIP (2), said in one way
    f32 = lambda *s: np.zeros(s, np.float32)
    u8 = C.POINTER(C.c_uint8)
    raw = np.zeros(64, np.uint8)              # ffp_jpeg_decode looks at the device before it looks at the bytes
    calls = {
        "merge": lambda: _lib.merge(f32(3, 6)),
        "eval_wider_pr": lambda: _lib.eval_wider_pr([np.zeros((1, 5))], [np.zeros((1, 4))], [np.ones(1, np.uint8)], thresh_num=4),
        "eval_dual_match": lambda: _lib.eval_dual_match([np.zeros((1, 5))], [np.zeros((1, 4))], [np.ones(1, np.uint8)]),
        "eval_coco_bbox": lambda: _lib.eval_coco_bbox(np.zeros((0, 7)), [0, 0], np.zeros((0, 8)), [0, 0], 1, 1, [0.5], [0.0], [[0.0, 1e10]], [100]),
        "jpeg_encode": lambda: _lib.jpeg_encode(np.zeros((8, 8, 3), np.uint8)),
        "jpeg_decode": lambda: _lib._check(lib.ffp_jpeg_decode(0, raw.ctypes.data_as(u8), raw.size, 0, np.zeros(192, np.uint8).ctypes.data_as(u8), 192)),
        "png_encode": lambda: _lib.png_encode(np.zeros((8, 8, 3), np.uint8)),
        "conv2d": lambda: _lib.op_conv2d(f32(1, 4, 4, 4), f32(4, 4, 1, 1), None),
        "conv1x1_up2": lambda: _lib.op_conv1x1_up2(f32(1, 2, 2, 4), f32(1, 4, 4, 4), f32(8, 8), f32(8)),
        "conv2d_time": lambda: _lib.op_conv2d_time(1, 8, 8, 16, 16, iters=1),
        "resize_lanczos4": lambda: _lib.op_resize_lanczos4(np.zeros((4, 4, 3), np.uint8), 6, 5),
        "upsample2x": lambda: _lib.op_upsample2x([f32(2, 2, 8)], 8, 0, [f32(4, 4, 8)], 0),
        "rt_gelu": lambda: _lib.op_rt_gelu(f32(4, 8), 8, 0),
        "image_input": lambda: _lib.op_image_input(_lib.IMAGE_YOLO, np.zeros((40, 40, 3), np.uint8), [(0, 0, 32, 32)], 32),
        "stem": lambda: _lib.op_stem(np.zeros((40, 40, 3), np.uint8), [(0, 0, 32, 32)], 32, f32(16, 3, 3, 3), f32(16), True),
        "stem_conv": lambda: _lib.op_stem_conv(np.zeros((40, 40, 3), np.uint8), [(0, 0, 32, 32)], 32, f32(16, 3, 3, 3), f32(16), f32(32, 16, 3, 3), f32(32)),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.FfpError) as e:
            call()
        assert e.value.code == 2 and "no HIP device" in str(e.value), (name, str(e.value))
        assert f"{name}: no HIP device 0 (no CPU path)" in str(e.value), (name, str(e.value))


def test_bad_arguments_are_reported(lib):
    n = C.c_int32(0)
    assert lib.ffp_slice_bboxes(10, 10, 4, 4, 1.5, 0.2, None, 0, C.byref(n)) == 1
    assert b"overlap" in lib.ffp_last_error()
    assert lib.ffp_letterbox_geometry(0, 10, 512, None) == 1


def test_operator_entry_points_check_arguments_before_touching_the_device(lib):
    """ffp_op_* of the non-convolution kernels: bad views, sizes and variants are FFP_ERR_ARG (code 1) — decided on the host,
    so it holds with or without a GPU — and a well-formed call without a GPU fails loudly instead of computing on the CPU."""
    z = lambda h, w, c: [np.zeros((h, w, c), np.float32)]
    bad = [
        lambda: _lib.op_sppf_pool(z(4, 4, 8), 8, 4, z(4, 4, 32), (0, 8, 16)),                 # input slice past the record
        lambda: _lib.op_sppf_pool(z(4, 4, 8), 8, 0, z(4, 4, 32), (0, 4, 16)),                 # overlapping output slices
        lambda: _lib.op_sppf_pool(z(4, 4, 8), 8, 0, z(4, 4, 32), (0, 8, 28)),                 # output slice past the record
        lambda: _lib.op_sppf_pool(z(4, 4, 8), 8, 0, z(4, 4, 32), (0, 8, 16), precision=_lib.PREC_F32X3),
        lambda: _lib.op_upsample2x(z(2, 2, 8), 8, 0, z(4, 4, 8), 4),
        lambda: _lib.op_psa_attention(z(2, 2, 256), 2, 4, z(2, 2, 128), 0),
        lambda: _lib.op_psa_attention(z(2, 2, 256), 2, 0, z(2, 2, 128), 4),
        lambda: _lib.op_dwconv3x3(z(3, 3, 256), 128, 0, np.zeros((128, 3, 3)), None, z(3, 3, 128), 0, grp=64, grp_stride=128, grp_off=96),
        lambda: _lib.op_dwconv3x3(z(3, 3, 256), 128, 4, np.zeros((128, 3, 3)), None, z(3, 3, 128), 0, grp=64, grp_stride=128, grp_off=64),
        lambda: _lib.op_dwconv3x3(z(3, 3, 8), 8, 0, np.zeros((8, 3, 3)), None, z(3, 3, 8), 0, act=7),
        lambda: _lib.op_det_post([[np.zeros((8, 8, 80), np.float32), np.zeros((4, 4, 80), np.float32), np.zeros((2, 2, 80), np.float32)]], 1, 5,
                                 [(0, 0, 0, 64, 64, 0, 0)]),                                  # no gain
        lambda: _lib.op_det_post([[np.zeros((8, 8, 80), np.float32), np.zeros((4, 4, 80), np.float32), np.zeros((2, 2, 80), np.float32)]], 1, 5,
                                 [(1, 0, 0, 64, 64, 0, 0)], max_det=2000),
        lambda: _lib.op_rt_topk(np.zeros((1, 299, 4), np.float32)),
        lambda: _lib.op_rt_topk(np.zeros((1, 300, 4), np.float32), nc=4, s_coff=1),
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 8, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0),                    # input slice past the record
        lambda: _lib.op_conv2d_views(z(4, 4, 72), 2, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0),                    # input slice not 16-byte aligned
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 40), 16),                   # output slice past the record
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, res1=z(4, 4, 32), r1_coff=8),
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, res2=z(4, 4, 16)),
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, gate_prev=[1]),     # gate_prev without gate
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, act=4),
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, act_post=-1),
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, precision=7),
        lambda: _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, px_align=0),
        lambda: _lib.op_variant(_lib.OP_SPPF, 3),
        lambda: _lib.op_variant(3, 1),
    ]
    # the image-input entries: frame 40 x 48 (h x w), one good box; each call is wrong in one way
    fr, box, f32 = np.zeros((40, 48, 3), np.uint8), [(0, 0, 32, 32)], lambda *s: np.zeros(s, np.float32)
    sw, sb, cw, cb = f32(16, 3, 3, 3), f32(16), f32(32, 16, 3, 3), f32(32)
    l, u8p, ip, fp = _lib.lib(), _lib._u8p, _lib._ip, _lib._fp
    t, o, hw = np.asarray(box, np.int32), f32(32 * 32 * 32), np.zeros(2, np.int32)
    bad += [
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, fr, [(0, 0, 49, 32)], 32),                  # box outside the frame
        lambda: _lib.op_image_input(_lib.IMAGE_RTDETR, fr, [(0, 9, 48, 41)], 32),
        lambda: _lib.op_image_input(_lib.IMAGE_SCRFD, fr, [(-1, 0, 32, 32)], (32, 32)),
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, fr, [(8, 8, 8, 32)], 32),                   # empty box
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, fr, box, 40),                               # imgsz not a multiple of 32
        lambda: _lib.op_image_input(_lib.IMAGE_RTDETR, fr, box, 48),
        lambda: _lib.op_image_input(_lib.IMAGE_SCRFD, fr, box, (64, 40)),
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, fr, box, 0),
        lambda: _lib.op_image_input(3, fr, box, 32),                                             # kind out of range
        lambda: _lib.op_image_input(-1, fr, box, 32),
        lambda: _lib.op_image_input(_lib.IMAGE_SCRFD, fr, box, (32, 32), precision=_lib.PREC_F16),
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, fr, box, 32, precision=_lib.PREC_F32X3),
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, fr, box, 32, chan_order=2),
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, fr, np.zeros((0, 4), np.int32), 32),        # n <= 0
        lambda: _lib.op_image_input(_lib.IMAGE_YOLO, np.zeros((4, 80, 3), np.uint8), [(0, 0, 80, 1)], 32),      # round(32 / 80) = 0 rows: cv2.resize would raise
        lambda: _lib.op_image_input(_lib.IMAGE_SCRFD, fr, [(0, 0, 1, 40)], (32, 32)),
        lambda: _lib._check(l.ffp_op_image_input(0, 0, 0, None, 40, 48, 0, 1, ip(t), 32, 32, fp(o), ip(hw), ip(hw))),     # null pointers
        lambda: _lib._check(l.ffp_op_image_input(0, 0, 0, u8p(fr), 40, 48, 0, 1, None, 32, 32, fp(o), ip(hw), ip(hw))),
        lambda: _lib._check(l.ffp_op_image_input(0, 0, 0, u8p(fr), 40, 48, 0, 1, ip(t), 32, 32, None, ip(hw), ip(hw))),
        lambda: _lib._check(l.ffp_op_image_input(0, 0, 0, u8p(fr), 40, 48, 0, 1, ip(t), 32, 32, fp(o), None, ip(hw))),
        lambda: _lib._check(l.ffp_op_image_input(0, 0, 0, u8p(fr), 40, 48, 0, -1, ip(t), 32, 32, fp(o), ip(hw), ip(hw))),
        lambda: _lib.op_stem(fr, [(0, 0, 49, 32)], 32, sw, sb, True),
        lambda: _lib.op_stem(fr, box, 48, sw, sb, False),
        lambda: _lib.op_stem(fr, box, 32, f32(24, 3, 3, 3), f32(24), True),                      # cout outside 16 / 32 / 64
        lambda: _lib.op_stem(fr, box, 32, sw, sb, True, stride=3),
        lambda: _lib.op_stem(fr, box, 32, sw, sb, True, act=4),
        lambda: _lib.op_stem(fr, box, 32, sw, sb, True, precision=_lib.PREC_F32X3),
        lambda: _lib.op_stem(fr, np.zeros((0, 4), np.int32), 32, sw, sb, True),
        lambda: _lib._check(l.ffp_op_stem(0, 0, 2, u8p(fr), 40, 48, 0, 1, ip(t), 32, fp(sw), fp(sb), 16, 2, 1, fp(o))),       # fused is 0 or 1
        lambda: _lib._check(l.ffp_op_stem(0, 0, 1, None, 40, 48, 0, 1, ip(t), 32, fp(sw), fp(sb), 16, 2, 1, fp(o))),
        lambda: _lib._check(l.ffp_op_stem(0, 0, 1, u8p(fr), 40, 48, 0, 1, ip(t), 32, None, fp(sb), 16, 2, 1, fp(o))),
        lambda: _lib._check(l.ffp_op_stem(0, 0, 1, u8p(fr), 40, 48, 0, 1, ip(t), 32, fp(sw), None, 16, 2, 1, fp(o))),
        lambda: _lib._check(l.ffp_op_stem(0, 0, 1, u8p(fr), 40, 48, 0, 1, ip(t), 32, fp(sw), fp(sb), 16, 2, 1, None)),
        lambda: _lib.op_stem_conv(fr, [(0, 0, 32, 41)], 32, sw, sb, cw, cb),
        lambda: _lib.op_stem_conv(fr, box, 33, sw, sb, cw, cb),
        lambda: _lib.op_stem_conv(fr, box, 32, f32(64, 3, 3, 3), f32(64), f32(128, 64, 3, 3), f32(128)),      # the loader holds one or two 16-channel chunks
        lambda: _lib.op_stem_conv(fr, np.zeros((0, 4), np.int32), 32, sw, sb, cw, cb),
        lambda: _lib.op_stem_conv(fr, box, 32, sw, sb, cw, cb, chan_order=-1),
        lambda: _lib._check(l.ffp_op_stem_conv(0, u8p(fr), 40, 48, 0, 1, ip(t), 32, fp(sw), fp(sb), 16, None, fp(cb), fp(o))),
        lambda: _lib._check(l.ffp_op_stem_conv(0, u8p(fr), 40, 48, 0, 1, ip(t), 32, fp(sw), fp(sb), 16, fp(cw), fp(cb), None)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.FfpError) as e:
            f()
        assert e.value.code == 1, (i, str(e.value))
    if _lib.device_count() == 0:
        with pytest.raises(_lib.FfpError) as e:
            _lib.op_sppf_pool(z(4, 4, 8), 8, 0, z(4, 4, 32), (0, 8, 16))
        assert "no HIP device" in str(e.value)
        with pytest.raises(_lib.FfpError) as e:
            _lib.op_rt_topk(np.zeros((1, 300, 4), np.float32))
        assert "no HIP device" in str(e.value)
        with pytest.raises(_lib.FfpError) as e:
            _lib.op_conv2d_views(z(4, 4, 64), 0, np.zeros((32, 64, 1, 1)), None, z(4, 4, 32), 0, gate=[1], gate_prev=[0])
        assert "no HIP device" in str(e.value)
        for call in (lambda: _lib.op_image_input(_lib.IMAGE_SCRFD, fr, box, (64, 32)), lambda: _lib.op_stem(fr, box, 32, sw, sb, False),
                     lambda: _lib.op_stem_conv(fr, box, 32, sw, sb, cw, cb)):
            with pytest.raises(_lib.FfpError) as e:
                call()
            assert e.value.code == 2 and "no HIP device" in str(e.value)


def test_weights_container_roundtrip():
    W = synth.yolo11_pose_weights("n")
    buf = weights_io.pack(W)
    back = weights_io.unpack(buf)
    assert list(back) == list(W) and all(np.array_equal(back[k], W[k]) for k in W)
    with pytest.raises(ValueError):
        weights_io.unpack(b"nope" + buf[4:])


def test_bn_fold_converter():
    rng = np.random.default_rng(1)
    sd = {"model.0.conv.weight": rng.standard_normal((8, 3, 3, 3)).astype(np.float32), "model.0.bn.weight": rng.uniform(0.5, 2, 8).astype(np.float32),
          "model.0.bn.bias": rng.standard_normal(8).astype(np.float32), "model.0.bn.running_mean": rng.standard_normal(8).astype(np.float32),
          "model.0.bn.running_var": rng.uniform(0.5, 2, 8).astype(np.float32), "model.23.cv2.0.2.weight": rng.standard_normal((64, 8, 1, 1)).astype(np.float32),
          "model.23.cv2.0.2.bias": rng.standard_normal(64).astype(np.float32), "model.23.dfl.conv.weight": np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)}
    out = weights_io.from_ultralytics_state_dict(sd)
    assert set(out) == {"model.0.conv.weight", "model.0.conv.bias", "model.23.cv2.0.2.weight", "model.23.cv2.0.2.bias"}
    import torch
    import torch.nn.functional as F
    x = torch.randn(1, 3, 9, 9)
    y = F.batch_norm(F.conv2d(x, torch.from_numpy(sd["model.0.conv.weight"]), padding=1), torch.from_numpy(sd["model.0.bn.running_mean"]),
                     torch.from_numpy(sd["model.0.bn.running_var"]), torch.from_numpy(sd["model.0.bn.weight"]), torch.from_numpy(sd["model.0.bn.bias"]), eps=1e-3)
    y2 = F.conv2d(x, torch.from_numpy(out["model.0.conv.weight"]), torch.from_numpy(out["model.0.conv.bias"]), padding=1)
    assert torch.allclose(y, y2, atol=1e-5)


def test_frame_items_and_sharding(lib):
    cfg = pipeline.PipeConfig()
    it = pipeline.frame_items(2160, 3840, cfg, 1)
    assert it.shape == (61, 4) and it[-1].tolist() == [0, 0, 3840, 2160]
    it2 = pipeline.frame_items(2160, 3840, cfg, 2)
    assert it2.shape == (122, 4) and it2[61].tolist() == [0, 2160, 512, 2672] and it2[-1].tolist() == [0, 2160, 3840, 4320]
    for world in (1, 2, 3, 4, 8):
        cover = []
        for r in range(world):
            lo, hi, per = pipeline.shard(61, r, world)
            assert hi - lo <= per
            cover += list(range(lo, hi))
        assert cover == list(range(61))
    sizes = pipeline.sr_crop_sizes(32, 0)
    assert set(sizes.tolist()) <= {24, 32, 48, 64, 96}
    b = pipeline.crop_boxes_for_sr(np.zeros((0, 21), np.float32), 2160, 3840, 32, sizes, seed=3)
    assert ((b[:, 2] - b[:, 0]) == sizes).all() and (b[:, 0] >= 0).all() and (b[:, 2] <= 3840).all() and (b[:, 3] <= 2160).all()


def test_pmc_symbol_to_variant_mapping():
    """tools/pmc_traffic.py keys the PMC table by the variant names bench.py reports (roofline.traffic lookup)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("pmc_traffic", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pmc_traffic.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    v = m.variant
    assert v("void ffp::(anonymous namespace)::conv_rows_kernel<1, 2>(ffp::ConvArgs)") == "f16_k3s1_rows"
    assert v("void ffp::conv_mfma_kernel<ffp::X3, 1, 1, 2, 2, 4, 2, 16>(ffp::ConvArgs)") == "f32x3_k1s1_wide"
    assert v("void ffp::conv_mfma_kernel<ffp::X3, 3, 2, 4, 1, 1, 2, 16>(ffp::ConvArgs)") == "f32x3_k3s2_narrow2"
    assert v("void ffp::conv_mfma_kernel<ffp::X3, 3, 1, 4, 1, 1, 1, 16>(ffp::ConvArgs)") == "f32x3_k3s1_narrow1H"
    assert v("_ZN3ffp16conv_mfma_kernelIDF16_Li3ELi1ELi4ELi1ELi2ELi1ELi16EEEvNS_8ConvArgsE") == "f16_k3s1_narrow1"
    assert v("void ffp::conv_mfma_kernel<float, 1, 1, 2, 2, 2, 2, 32>(ffp::ConvArgs)") == "f32_k1s1_wideH"
    assert v("ffp::(anonymous namespace)::conv_rows16_kernel(ffp::ConvArgs)") == "f16_k3s1_rows16"
    assert v("void ffp::(anonymous namespace)::conv_pw_kernel<8, 1, 4, 3, false>(ffp::ConvArgs)") == "f32x3_k1s1_pw1x4w"
    assert v("_ZN3ffp12_GLOBAL__N_114conv_pw_kernelILi4ELi2ELi2ELi2ELb1EEEvNS_8ConvArgsE") == "f32x3_k1s1_pw2x2"
    assert v("void ffp::(anonymous namespace)::conv_pw_kernel<8, 2, 2, 2, true, false>(ffp::ConvArgs)") == "f32x3_k1s1_pw2x2w"
    assert v("void ffp::(anonymous namespace)::conv_pw_kernel<7, 1, 4, 4, false, true>(ffp::ConvArgs)") == "f32x3_k1s1_pw1x4s"
    assert v("_ZN3ffp12_GLOBAL__N_114conv_pw_kernelILi7ELi1ELi4ELi4ELb1ELb1EEEvNS_8ConvArgsE") == "f32x3_k1s1_pw1x4s"
    assert v("__amd_rocclr_copyBuffer") is None


@pytest.mark.parametrize("order", ["torch_first", "libffp_first"])
def test_single_hip_runtime(order):
    """libffp.so, torch and RCCL must share ONE HIP runtime whatever the import order (the wheel bundles a libamdhip64 with
    the same SONAME as the system one; two copies, or the wheel running on the system copy, is the hazard)."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n" % ROOT) + (
        "import torch\nimport ffp_amd\nfrom ffp_amd import _lib\n_lib.lib()\n" if order == "torch_first"
        else "import ffp_amd\nfrom ffp_amd import _lib\n_lib.lib()\nimport torch\n") + (
        "import torch.distributed\n"
        "libs = sorted({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l})\n"
        "print(len(libs), libs)\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    n, libs = out.stdout.strip().split(" ", 1)
    assert n == "1", libs
    import importlib.util
    if importlib.util.find_spec("torch") is not None:
        assert "torch" in libs            # the wheel's own copy, in both orders


def test_bench_lanes_deal_every_group_exactly_once():
    """bench.py --lanes L: detection groups are dealt round-robin, so the lanes together walk exactly the single-lane sequence of steps
    (same frames, crops and seeds); the lane that owns the last group is the one whose final SR batch is event-timed."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for n_steps in (0, 1, 3, 5, 7, 20, 23, 200):
        for db in (1, 4, 5):
            for L in (1, 2, 3, 4):
                lanes = []
                for k in range(L):
                    r = bench.Runner.__new__(bench.Runner)
                    r.DB, r.n_lanes, r.lane = db, L, k
                    lanes.append(r)
                all_groups = lanes[0].groups(n_steps)
                assert sum(g[1] for g in all_groups) == n_steps and all(0 < g[1] <= db for g in all_groups)
                dealt = sorted(g for r in lanes for g in r.my_groups(n_steps))
                assert [(g0, gsz) for _, g0, gsz in dealt] == all_groups and [gi for gi, _, _ in dealt] == list(range(len(all_groups)))
                steps = sorted(s for r in lanes for _, g0, gsz in r.my_groups(n_steps) for s in range(g0, g0 + gsz))
                assert steps == list(range(n_steps))
                if all_groups:
                    owner = (len(all_groups) - 1) % L
                    assert lanes[owner].my_groups(n_steps)[-1][0] == len(all_groups) - 1


def test_bench_full_is_opt_in():
    """bench.py: a plain run measures the headline alone; the profiled pass, secondary rows and CPU baseline need --full, and the
    options that only shape those are refused without it rather than ignored."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.parse([]).full is False
    assert bench.parse(["--full", "--secondary-only", "frame_by_frame", "--cpu-sample"]).full is True
    for extra in (["--secondary-only", "frame_by_frame"], ["--cpu-sample"]):
        with pytest.raises(SystemExit):
            bench.parse(extra)


def test_bench_dump_outputs_reads_the_last_batch_and_keeps_the_budget(tmp_path):
    """bench.py --dump-outputs: the kept frame's crops are cut out of the lane's last SR batch (16-byte aligned entries, boxes clamped
    to the frame, the frame's crops after those of earlier frames in the batch, the frame on another lane); the .npy files are float
    and round-trip the pixels; a budget too small for every crop keeps the same seeded sample on every call."""
    import importlib.util
    import types
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.parse(["--steps", "3", "--dump-outputs", "d"]).dump_outputs == "d"
    rng = np.random.default_rng(1)
    H, W, sc = 200, 300, 4

    def lane(batch, kept_fid):
        r = bench.Runner.__new__(bench.Runner)
        r.H, r.W, r.jpeg_io, r.sub = H, W, False, []
        r.pipe = types.SimpleNamespace(sr=types.SimpleNamespace(scale=sc))
        meta, offs, chunks, want = [], [0], [], None
        for fid, boxes in batch:
            meta.append((fid, len(boxes)))
            crops = []
            for x0, y0, x1, y1 in boxes:
                c = rng.integers(0, 256, ((min(H, y1) - max(0, y0)) * sc, (min(W, x1) - max(0, x0)) * sc, 3), dtype=np.uint8)
                pad = (c.size + 15) // 16 * 16
                chunks.append(np.concatenate([c.reshape(-1), np.full(pad - c.size, 77, np.uint8)]))
                offs.append(offs[-1] + pad)
                crops.append(c)
            if fid == kept_fid:
                want = crops
        r.host_sr = torch.from_numpy(np.concatenate(chunks + [np.zeros(64, np.uint8)]))
        r.last_batch = (meta, np.asarray(offs, np.int64))
        r.kept = {kept_fid: {"rows": rng.random((5, 21)).astype(np.float32), "boxes": np.asarray(dict(batch)[kept_fid], np.int32)}}
        return r, want

    def boxes(n):
        s = rng.choice([24, 32, 48], n)
        x, y = rng.integers(-10, W - 10, n), rng.integers(-10, H - 10, n)
        return [(int(a), int(b), int(a + c), int(b + c)) for a, b, c in zip(x, y, s)]

    r0, want0 = lane([((7, 0), boxes(4)), ((8, 0), boxes(5)), ((9, 0), boxes(3))], (9, 0))
    got = r0.kept_outputs()
    assert len(got["crops"]) == 3 and all(np.array_equal(a, b) for a, b in zip(got["crops"], want0))
    r1, want1 = lane([((3, 0), boxes(2)), ((4, 0), boxes(6))], (4, 0))
    r0.kept, r0.sub = {}, [r1]
    got = r0.kept_outputs()
    assert len(got["rows"]) == 1 and len(got["crops"]) == 6 and all(np.array_equal(a, b) for a, b in zip(got["crops"], want1))

    bench.dump_outputs(str(tmp_path / "all"), got)
    f = {p.stem: np.load(p) for p in (tmp_path / "all").iterdir()}
    assert set(f) == {"detections", "crop_boxes", "enhanced_crops", "enhanced_crop_shapes", "enhanced_crop_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in f.values())
    assert np.array_equal(f["detections"], got["rows"][0]) and f["enhanced_crop_index"].tolist() == list(range(6))
    o = 0
    for c, s in zip(want1, f["enhanced_crop_shapes"].astype(int)):
        assert np.array_equal(f["enhanced_crops"][o:o + s.prod()].reshape(s), c)
        o += s.prod()
    assert o == f["enhanced_crops"].size

    bench.DUMP_BYTES = 200_000
    picks = []
    for k in range(2):
        n = bench.dump_outputs(str(tmp_path / f"small{k}"), got)
        assert n <= 200_000
        picks.append(np.load(tmp_path / f"small{k}" / "enhanced_crop_index.npy").tolist())
    assert 0 < len(picks[0]) < 6 and picks[0] == picks[1]


def test_conv_views_plan_bookkeeping():
    """tests/test_gpu_conv_views.py, the part that needs no device: which shape a case of its plan can run, from the Python predicates alone — every
    pw / k3d case is one its shape can run, the head slices have pw shapes to run on, and the block-walk batches (and the prefix of them each shape runs
    on) give every conv_pw workgroup its three pixel blocks."""
    import test_gpu_conv_views as V
    from test_gpu_conv import K3D_SHAPES, PW_SHAPES, _epi_k3d_cases, _epi_pw_cases, pw_can_run
    for shape, cin, cout, k, stride in _epi_pw_cases():
        assert pw_can_run(shape, cin, cout) and k == 1 and cin % 32 == 0
    for shape, cin, cout, k, stride in _epi_k3d_cases():
        assert -(-cout // 32) >= K3D_SHAPES[shape] and (cin + V.X_PAD) % 4 == 0
    assert [s_ for s_ in sorted(PW_SHAPES) if pw_can_run(s_, 64, 15)] == [12, 15] == [s_ for s_ in sorted(PW_SHAPES) if pw_can_run(s_, 64, 1)]
    for cin, cout in V.WALK_CASES:
        sizes = V._walk_sizes(cin, cout)
        shapes = [s_ for s_ in sorted(PW_SHAPES) if pw_can_run(s_, cin, cout)]
        assert len(shapes) >= 5 and all(V._pw_blocks_per_workgroup(s_, V._aligned_px(sizes), cout) >= 3 for s_ in shapes)
        assert all(V._pw_blocks_per_workgroup(s_, V._aligned_px(sizes[:V._walk_prefix(s_, sizes, cout)]), cout) >= 3 for s_ in shapes)
    assert len(V._walk_sizes(64, 64)) == 60 and len(V._walk_sizes(96, 128)) == 31

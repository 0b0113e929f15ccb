"""Operator-level parity of the four kernels that turn uint8 frame pixels into a network's first tensor: letterbox_kernel and
stem_from_frame_kernel (csrc/ops_misc.hip), scrfd_preproc_kernel (csrc/scrfd_ops.hip) and the STEM loader of conv_mfma_kernel
(csrc/conv_mfma.hip), through ffp_op_image_input, ffp_op_stem and ffp_op_stem_conv. Reference: tests/image_input_ref.py, which composes the
repository's cv2 / Ultralytics / InsightFace oracles (checked on the host by tests/test_image_input_ref.py). The pre-processing is integer work
and one exact float step, so it is compared bit for bit; the convs behind it are held to the bars the conv tests hold their kernels to.

The frame is 97 x 131 (h x w): a row is 393 bytes, so row starts walk through all four byte alignments. ffp_op_image_input lays its one level
out packed (the entry takes no px_align: the engines' image levels of a split plan differ from it only in where an image starts)."""
import functools

import numpy as np
import pytest

import image_input_ref as R

pytestmark = pytest.mark.gpu

_rng = np.random.default_rng(97131)
_yy, _xx = np.mgrid[0:97, 0:131]
FRAMES = {
    "noise": _rng.integers(0, 256, (97, 131, 3), dtype=np.uint8),
    # 0 / 255 per pixel, the three channels out of phase: every interpolated value sits between the clamps and every pad shows
    "checker": np.stack([(((_yy + _xx + c) & 1) * 255).astype(np.uint8) for c in range(3)], -1),
    "big": _rng.integers(0, 256, (131, 259, 3), dtype=np.uint8),
}
NATIVE = [(0, 0, 64, 64), (67, 33, 131, 97), (3, 1, 67, 65), (34, 17, 98, 81)]      # the second ends on the last byte of the frame
ONE_ROW = (0, 96, 131, 97)              # 131 x 1: the YOLO letterbox and SCRFD resize it to no row at all
YOLO_64 = NATIVE + [
    (0, 0, 128, 96),        # exact 2x down-scale, 8 + 8 rows of pad
    (0, 0, 131, 97),        # fractional down-scale, 8 rows above and 9 below
    (10, 20, 40, 40),       # up-scale, 10 rows above and 11 below
    (5, 0, 6, 97),          # one source column: a 64 x 32 network image, 15 + 16 columns of pad
    (4, 96, 131, 97),       # one source row (the widest the letterbox accepts at the frame's last row): 32 x 64, 15 + 16 rows of pad
]
YOLO_96 = [(3, 1, 67, 65)]            # up-scale without pad
RTDETR_64 = YOLO_64 + [ONE_ROW, (0, 17, 131, 81)]      # the last: 64 rows stay, 131 columns shrink; the native boxes are plain copies
SCRFD_BOXES = NATIVE[:3] + [(0, 0, 131, 97), (10, 20, 40, 40), (0, 0, 128, 96), (5, 1, 6, 65)]
ORDERS = ["bgr", "rgb"]


def _order(gpu_lib, name):
    return gpu_lib.CHAN_AS_BGR if name == "bgr" else gpu_lib.CHAN_AS_RGB


@functools.lru_cache(maxsize=None)
def _records(kind, frame, box, size, flip, half):
    a = R.records(kind, FRAMES[frame], box, size, flip, half)
    a.setflags(write=False)
    return a


def _check_image_input(gpu_lib, kind, frame, boxes, size, order, half):
    prec = gpu_lib.PREC_F16 if half else gpu_lib.PREC_F32
    kw = dict(chan_order=_order(gpu_lib, order), precision=prec)
    got = gpu_lib.op_image_input(kind, FRAMES[frame], boxes, size, **kw)
    assert len(got) == len(boxes)
    pad = R.pad_value(kind)
    if half:
        pad = np.float32(np.float16(pad))
    for i, box in enumerate(boxes):
        tag = (frame, box, size, order, half)
        want = _records(kind, frame, box, size, order == "bgr", half)
        net_h, net_w = R.geometry(kind, box, size)[:2]
        assert got[i].shape == want.shape == (net_h, net_w, 8 if half and kind != R.SCRFD else 4), tag
        assert np.array_equal(got[i], want), (tag, np.argwhere(got[i] != want)[:4], got[i][got[i] != want][:4], want[got[i] != want][:4])
        assert np.all(got[i][..., 3:] == 0), tag
        m = R.pad_mask(kind, box, size)
        assert np.all(got[i][m][:, :3] == pad), tag
        # alone, in slot 0 of a level of its own: nothing of an item depends on its batch mates or on where it sits
        alone = gpu_lib.op_image_input(kind, FRAMES[frame], [box], size, **kw)
        assert len(alone) == 1 and np.array_equal(alone[0], got[i]), tag


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("frame", ["noise", "checker"])
def test_image_input_yolo(gpu_lib, frame, order, half):
    """letterbox_kernel on the YOLO geometry (det_tile_geometry): every pixel and channel equal to the oracle's letterbox / 255, pad channels zero, pad
    areas 114 / 255, network sizes the oracle's; a ragged batch (64 x 64, 64 x 32 and 32 x 64 images) and every box alone give the same bits."""
    _check_image_input(gpu_lib, R.YOLO, frame, YOLO_64, 64, order, half)
    _check_image_input(gpu_lib, R.YOLO, frame, YOLO_96, 96, order, half)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("frame", ["noise", "checker"])
def test_image_input_rtdetr(gpu_lib, frame, order, half):
    """letterbox_kernel on the RT-DETR records (rtdetr_tile_records): the same boxes stretched to 64 x 64 — both axes, one axis only, one source
    row or column, and the plain copy."""
    _check_image_input(gpu_lib, R.RTDETR, frame, RTDETR_64, 64, order, half)
    _check_image_input(gpu_lib, R.RTDETR, frame, YOLO_96, 96, order, half)


@pytest.mark.parametrize("size", [(64, 64), (96, 64)], ids=["64x64", "96x64"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("frame", ["noise", "checker"])
def test_image_input_scrfd(gpu_lib, frame, order, size):
    """scrfd_preproc_kernel on the SCRFD records (scrfd_tile_records): the picture at the top-left, zero pad to the right or below, (v - 127.5) / 128."""
    _check_image_input(gpu_lib, R.SCRFD, frame, SCRFD_BOXES, size, order, False)


def test_image_input_refusals(gpu_lib):
    """A box that resizes to nothing is refused where cv2.resize would raise (YOLO_64 and SCRFD_BOXES hold the nearest boxes that are accepted);
    RT-DETR's stretch takes it. SCRFD has no fp16 form."""
    f = FRAMES["noise"]
    for call in (lambda: gpu_lib.op_image_input(R.YOLO, f, [NATIVE[0], ONE_ROW], 64),
                 lambda: gpu_lib.op_image_input(R.SCRFD, f, [ONE_ROW], (64, 64)),
                 lambda: gpu_lib.op_image_input(R.SCRFD, f, [(5, 0, 6, 97)], (64, 64)),
                 lambda: gpu_lib.op_stem_conv(f, [ONE_ROW], 64, np.zeros((16, 3, 3, 3)), np.zeros(16), np.zeros((32, 16, 3, 3)), np.zeros(32)),
                 lambda: gpu_lib.op_image_input(R.SCRFD, f, NATIVE, (64, 64), precision=gpu_lib.PREC_F16)):
        with pytest.raises(gpu_lib.FfpError) as e:
            call()
        assert e.value.code == 1, str(e.value)
    with pytest.raises(ValueError):
        R.network_u8(R.SCRFD, f, ONE_ROW, (64, 64))
    assert R.geometry(R.YOLO, ONE_ROW, 64)[2] == 0


# ---- the image-input conv ----------------------------------------------------------------------------------------------------------------

def _stem_weights(cout, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((cout, 3, 3, 3)) / np.sqrt(27)).astype(np.float32), (0.1 * rng.standard_normal(cout)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _stem_ref(frame, box, imgsz, flip, half, cout, seed, stride, act):
    w, b = _stem_weights(cout, seed)
    return R.conv3x3(_records(R.YOLO, frame, box, imgsz, flip, half)[..., :3], w, b, stride, act)


def _worst(y, ref):
    """max |y - ref| / (1 + |ref|): y meets rtol = atol = t exactly when this is <= t."""
    return float(np.max(np.abs(y.astype(np.float64) - ref) / (1.0 + np.abs(ref))))


def _check_stem(gpu_lib, cout, half, order, stride, act, boxes, imgsz):
    w, b = _stem_weights(cout, cout)
    kw = dict(stride=stride, act=act, chan_order=_order(gpu_lib, order), precision=gpu_lib.PREC_F16 if half else gpu_lib.PREC_F32)
    two = gpu_lib.op_stem(FRAMES["noise"], boxes, imgsz, w, b, False, **kw)
    one = gpu_lib.op_stem(FRAMES["noise"], boxes, imgsz, w, b, True, **kw)
    bar = 2e-3 if half else 2e-5
    for i, box in enumerate(boxes):
        tag = (box, cout, half, order, stride, act)
        ref = _stem_ref("noise", box, imgsz, order == "bgr", half, cout, cout, stride, act)
        assert two[i].shape == one[i].shape == ref.shape, tag
        assert np.array_equal(one[i], two[i]), (tag, np.argwhere(one[i] != two[i])[:4])
        err = _worst(two[i], ref)
        print("stem two-kernel", tag, "worst error / (1 + |ref|): %.3g" % err)
        assert err <= bar, tag


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("cout", [16, 32, 64])
def test_stem_fused_equals_two_kernels(gpu_lib, cout, order, half):
    """stem_from_frame_kernel against letterbox_kernel + the direct conv kernel, stride 2 and SiLU, on the ragged YOLO batch: bit for bit, as
    csrc/ops.hpp promises. The two-kernel result against a float64 conv of the reference network image (for fp16: of its fp16 values; the direct
    kernel keeps fp32 weights and sums in fp32): rtol = atol = 2e-5 / 2e-3, the bars test_gpu_conv.py::test_conv_dense holds the direct kernel to."""
    _check_stem(gpu_lib, cout, half, order, 2, 1, YOLO_64, 64)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("cout,stride,act", [(16, 1, 2), (64, 1, 0), (32, 2, 3)], ids=["c16_s1_lrelu", "c64_s1_none", "c32_s2_relu"])
def test_stem_other_activations_and_stride(gpu_lib, cout, stride, act, half):
    """The same two properties with the direct kernel's other activations (leaky ReLU 0.2 at stride 1 is how the super-resolution network enters it)
    and at imgsz 96."""
    _check_stem(gpu_lib, cout, half, "bgr", stride, act, YOLO_64[3:8], 64)
    _check_stem(gpu_lib, cout, half, "rgb", stride, act, YOLO_96, 96)


# ---- model.0 inside model.1's loader -----------------------------------------------------------------------------------------------------
# (frame, imgsz, boxes): native-size boxes take the loader's dword path (`plain`), the others its letterbox_sample path
STEM_CONV_BATCHES = [
    ("noise", 64, YOLO_64),
    ("noise", 96, [(0, 0, 96, 64), (35, 33, 131, 97), (3, 1, 129, 85), (3, 1, 67, 65)]),      # 64 x 96 images, native twice (24 x 16 outputs: a partial last tile) and resized; 96 x 96 up-scaled
    ("big", 128, [(131, 3, 259, 131), (1, 2, 129, 130), (0, 0, 259, 131)]),                    # 128 x 128 native (flush with the frame's end, and at an odd offset): 32 x 32 outputs, several tile rows
]
F32X3_BAR = 3e-5


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("stem_cout", [16, 32], ids=["16to32", "32to64"])
def test_stem_conv_fused_loader(gpu_lib, stem_cout, order):
    """launch_stem_conv (the default path of YOLO11n / YOLO11s in f32x3) against the float64 reference of both convs on the reference network image:
    stem 3x3 s2 SiLU, conv 3x3 s2 SiLU to twice the channels. Bar: rtol = atol = 3e-5, the project's f32x3 bar (test_conv_dense_f32x3).

    The unfused composition — ffp_op_stem fp32, two kernels, fed to op_conv2d in PREC_F32X3 — is held to the same bar first: measured on an MI355X
    its worst |y - ref| / (1 + |ref|) over all these cases was 2.84e-7 (the fused loader's: 2.84e-7), a hundredth of the bar, so two stacked convs
    on these inputs do not need a wider one. Every figure is printed before it is asserted."""
    rng = np.random.default_rng(1000 + stem_cout)
    sw, sb = _stem_weights(stem_cout, 500 + stem_cout)
    cw = (rng.standard_normal((2 * stem_cout, stem_cout, 3, 3)) / np.sqrt(9 * stem_cout)).astype(np.float32)
    cb = (0.1 * rng.standard_normal(2 * stem_cout)).astype(np.float32)
    co = _order(gpu_lib, order)
    worst_unfused = worst_fused = 0.0
    for frame, imgsz, boxes in STEM_CONV_BATCHES:
        got = gpu_lib.op_stem_conv(FRAMES[frame], boxes, imgsz, sw, sb, cw, cb, chan_order=co)
        x0 = gpu_lib.op_stem(FRAMES[frame], boxes, imgsz, sw, sb, False, chan_order=co)
        assert len(got) == len(boxes)
        for i, box in enumerate(boxes):
            tag = (frame, box, imgsz, stem_cout, order)
            img = _records(R.YOLO, frame, box, imgsz, order == "bgr", False)[..., :3]
            ref = R.conv3x3(R.conv3x3(img, sw, sb, 2, 1), cw, cb, 2, 1)
            unfused = gpu_lib.op_conv2d(x0[i][None], cw, cb, stride=2, act=1, precision=gpu_lib.PREC_F32X3)[0]
            assert got[i].shape == unfused.shape == ref.shape == (img.shape[0] // 4, img.shape[1] // 4, 2 * stem_cout), tag
            eu, ef = _worst(unfused, ref), _worst(got[i], ref)
            print("stem_conv", tag, "unfused %.3g fused %.3g" % (eu, ef))
            worst_unfused, worst_fused = max(worst_unfused, eu), max(worst_fused, ef)
            assert eu <= F32X3_BAR, tag
            assert ef <= F32X3_BAR, (tag, np.argwhere(np.abs(got[i] - ref) > F32X3_BAR * (1 + np.abs(ref)))[:6])
            alone = gpu_lib.op_stem_conv(FRAMES[frame], [box], imgsz, sw, sb, cw, cb, chan_order=co)      # one slot per image: the batch mates do not matter
            assert np.array_equal(alone[0], got[i]), tag
    print("stem_conv worst: unfused %.3g fused %.3g" % (worst_unfused, worst_fused))

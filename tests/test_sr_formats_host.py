"""CPU tests of RealESRGANer.enhance's extra layouts: known answers of the cv2 restatements in the oracle
(tests/realesrgan_formats_ref.py) and the pure layout decision (compat/utils/enhancer.py::enhance_layout)."""
import numpy as np
import pytest

import realesrgan_formats_ref as R


# ---- Lanczos4 / linear known answers ---------------------------------------------------------------------------------------
def test_lanczos4_taps_at_zero_phase():
    c = R.lanczos4_coefs(np.float32(0))
    assert np.array_equal(np.rint(c * np.float32(2048)).astype(int), [0, 0, 0, 2048, 0, 0, 0, 0])
    assert abs(float(c[3]) - 1.0) < 1e-7 and np.abs(np.delete(c, 3)).max() < 1e-20


@pytest.mark.parametrize("fx", [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.875, 0.999, 1e-7, 0.3333333])
def test_lanczos4_weights_sum_to_one(fx):
    c = R.lanczos4_coefs(np.float32(fx))
    assert c.dtype == np.float32 and abs(float(np.sum(c, dtype=np.float64)) - 1.0) < 1e-6


def test_lanczos4_int_weights_stay_inside_int32():
    """The bound the library's int32 sums rely on: over a fine grid of phases a row's positive taps sum to <= 2780 and its
    negative taps to >= -732, so 255 * (2780^2 + 732^2) < 2^31."""
    pos = neg = 0
    for fx in np.linspace(0, 1, 20001, endpoint=False, dtype=np.float32):
        a = np.rint(R.lanczos4_coefs(fx) * np.float32(2048)).astype(np.int64)
        pos, neg = max(pos, int(a[a > 0].sum())), min(neg, int(a[a < 0].sum()))
    assert pos <= 2780 and neg >= -732, (pos, neg)
    assert 255 * (pos * pos + neg * neg) < 2 ** 31


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_lanczos4_same_size_is_a_copy(dtype):
    img = np.random.default_rng(0).integers(0, np.iinfo(dtype).max, (7, 9, 3), endpoint=True).astype(dtype)
    out = R.resize_lanczos4(img, 9, 7)
    assert out.dtype == dtype and np.array_equal(out, img)


@pytest.mark.parametrize("size", [(5, 7), (30, 13), (1, 1), (3, 40)])
def test_lanczos4_constant_u16_stays_constant(size):
    img = np.full((6, 11, 4), 40000, np.uint16)
    out = R.resize_lanczos4(img, *size)
    assert out.shape == (size[1], size[0], 4) and np.all(out == 40000)


def test_lanczos4_constant_u8_stays_constant():
    img = np.full((9, 4), 255, np.uint8)
    assert np.all(R.resize_lanczos4(img, 13, 22) == 255)


def test_lanczos4_u8_grid_hits_the_int32_check():
    img = np.zeros((16, 16), np.uint8)
    img[::2, ::2] = 255                                                          # worst-case sign pattern region
    out = R.resize_lanczos4(img, 37, 29)
    assert out.shape == (29, 37) and out.dtype == np.uint8


def test_linear_x4_phases():
    """x4: fx = (dx + 0.5) / 4 - 0.5 gives 0.625, 0.875, 0.125, 0.375; the first two (sx = -1) reset to sx = 0, fx = 0
    horizontally only."""
    ph_y = R.linear_phases(10, 40, reset=False)[:4]
    assert [float(f) for _, f in ph_y] == [0.625, 0.875, 0.125, 0.375]
    assert [s for s, _ in ph_y] == [-1, -1, 0, 0]
    ph_x = R.linear_phases(10, 40, reset=True)[:4]
    assert [(s, float(f)) for s, f in ph_x] == [(0, 0.0), (0, 0.0), (0, 0.125), (0, 0.375)]
    last = R.linear_phases(10, 40, reset=True)[-1]
    assert last == (9, 0.0)


def test_linear_f32_upsample_of_constant_and_ramp():
    a = np.full((3, 5), 0.25, np.float32)
    assert np.all(R.resize_linear_f32(a, 20, 12) == np.float32(0.25))
    r = np.tile(np.arange(4, dtype=np.float32), (2, 1))
    o = R.resize_linear_f32(r, 8, 4)
    assert np.allclose(o[0], [0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3], atol=0)


def test_bgr2gray_weights():
    px = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    assert np.array_equal(R.bgr2gray(px), np.array([0.114, 0.587, 0.299], np.float32))


# ---- the layout decision ---------------------------------------------------------------------------------------------------
def _layout(shape, dtype=np.uint8, mx=200, scale=4, outscale=None, alpha="realesrgan"):
    from ffp_amd.compat.utils.enhancer import enhance_layout
    return enhance_layout(shape, dtype, mx, scale, outscale, alpha)


def test_layout_modes():
    from ffp_amd import _lib
    assert _layout((10, 12)).mode == "L"
    assert _layout((10, 12, 3)).mode == "RGB"
    lay = _layout((10, 12, 4))
    assert lay.mode == "RGBA" and lay.alpha_mode == _lib.SR_ALPHA_REALESRGAN
    assert _layout((10, 12, 4), alpha="cv2").alpha_mode == _lib.SR_ALPHA_LINEAR
    assert _layout((10, 12, 3)).fast_path
    assert not _layout((10, 12)).fast_path and not _layout((10, 12, 4)).fast_path
    assert not _layout((10, 12, 3), np.uint16).fast_path


def test_layout_16bit_rule():
    lay = _layout((10, 12, 3), np.uint16, 200)                 # uint16 with max <= 256 takes the 8-bit path
    assert lay.max_range == 255 and lay.out_dtype == np.uint8
    assert _layout((10, 12, 3), np.uint16, 256).max_range == 255
    lay = _layout((10, 12, 3), np.uint16, 257)
    assert lay.max_range == 65535 and lay.out_dtype == np.uint16
    assert _layout((10, 12, 4), np.uint16, 256).max_range == 255      # max 256 is fine with the network alpha
    assert _layout((10, 12, 3), np.uint8, 255).max_range == 255


@pytest.mark.parametrize("outscale,hw", [(3.5, (35, 42)), (1.5, (15, 18)), (2, (20, 24)), (5, (50, 60)), (0.35, (3, 4))])
def test_layout_outscale_sizes(outscale, hw):
    lay = _layout((10, 12, 3), outscale=outscale)
    assert (lay.out_h, lay.out_w) == hw and lay.resize and not lay.fast_path


@pytest.mark.parametrize("outscale", [None, 4, 4.0])
def test_layout_net_scale_is_no_resize(outscale):
    lay = _layout((10, 12, 3), outscale=outscale)
    assert (lay.out_h, lay.out_w) == (40, 48) and not lay.resize and lay.fast_path


def test_layout_x2_scale():
    assert not _layout((7, 9), scale=2, outscale=2).resize
    lay = _layout((7, 9), scale=2, outscale=4)
    assert (lay.out_h, lay.out_w) == (28, 36) and lay.resize


@pytest.mark.parametrize("kw", [
    dict(shape=(10, 12, 3), dtype=np.float32),
    dict(shape=(10, 12, 3), dtype=np.int16),
    dict(shape=(10, 12, 3), dtype=np.uint32),
    dict(shape=(10, 12, 2)),
    dict(shape=(10, 12, 1)),
    dict(shape=(10, 12, 5)),
    dict(shape=(10,)),
    dict(shape=(2, 10, 12, 3)),
    dict(shape=(0, 12, 3)),
    dict(shape=(10, 0)),
    dict(shape=(10, 12, 3), outscale=0.05),
    dict(shape=(10, 12, 3), outscale=0),
    dict(shape=(10, 12, 3), outscale=-2),
    dict(shape=(10, 12, 4), dtype=np.uint16, mx=256, alpha="cv2"),
])
def test_layout_rejections(kw):
    shape = kw.pop("shape")
    with pytest.raises(ValueError):
        _layout(shape, **kw)

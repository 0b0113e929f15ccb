"""The fake-network harness of the Real-ESRGAN operator tests (tests/sr_ops_common.py) on the CPU: with an identity-like network the oracle's
enhance() reproduces its input, the network is called for the colour tiles first and the alpha tiles after them, the tile shapes it records are
the ones the library cuts (ffp_op_sr_tiles needs no device), and the prescribed outputs hold every kind of value they promise."""
import numpy as np
import pytest

import realesrgan_formats_ref as R
import sr_ops_common as S

CASES = [(4, 5, 7, 0, 10, 0), (4, 19, 23, 8, 4, 3), (4, 19, 23, 8, 20, 18), (4, 19, 23, 16, 0, 1), (2, 3, 5, 0, 10, 1), (2, 17, 20, 0, 10, 1),
         (2, 19, 23, 8, 4, 0), (2, 31, 45, 16, 2, 30)]


@pytest.mark.parametrize("name", [l[0] for l in S.LAYOUTS])
@pytest.mark.parametrize("scale,h,w,tile,tile_pad,pre_pad", CASES)
def test_identity_network_reproduces_the_input(name, scale, h, w, tile, tile_pad, pre_pad):
    img = S.make_image(name, h, w, 1)
    if img.max() == 256:
        img = np.minimum(img, 255)              # 256 / 255 > 1 is clamped by the network path: not an identity
    fake = S.FakeNet(scale, S.nearest_out(scale))
    out, _ = R.enhance(fake, img, None, "realesrgan", tile=tile, tile_pad=tile_pad, pre_pad=pre_pad)
    want = np.repeat(np.repeat(img, scale, axis=0), scale, axis=1)
    assert out.shape == want.shape
    if img.ndim == 2:
        # BGR2GRAY of three equal channels is v * 0.114f + v * 0.587f + v * 0.299f: within one float32 step of v, so the same integer
        assert np.array_equal(out, want.astype(out.dtype))
    else:
        assert np.array_equal(out[..., :3], want[..., :3].astype(out.dtype))
        if img.shape[2] == 4:
            assert np.array_equal(out[..., 3], want[..., 3].astype(out.dtype))


@pytest.mark.parametrize("scale,h,w,tile,tile_pad,pre_pad", CASES)
def test_colour_tiles_come_before_alpha_tiles(scale, h, w, tile, tile_pad, pre_pad):
    img = S.make_image("bgra8", h, w, 2)
    fake = S.FakeNet(scale, S.nearest_out(scale))
    R.enhance(fake, img, None, "realesrgan", tile=tile, tile_pad=tile_pad, pre_pad=pre_pad)
    n = len(fake.inputs)
    assert n % 2 == 0 and n >= 2
    f = 4 if scale == 2 else 1
    for k, rec in enumerate(fake.inputs):
        planes = [rec[..., c * f:(c + 1) * f] for c in range(3)]
        grey = np.array_equal(planes[0], planes[1]) and np.array_equal(planes[1], planes[2])
        assert grey == (k >= n // 2), (k, n)
    assert [r.shape for r in fake.inputs[:n // 2]] == [r.shape for r in fake.inputs[n // 2:]]
    # the first tile starts at the image's corner: R, G, B of pixel (0, 0), then its alpha
    assert fake.inputs[0][0, 0, 0] == np.float32(img[0, 0, 2]) / np.float32(255) and fake.inputs[0][0, 0, 2 * f] == np.float32(img[0, 0, 0]) / np.float32(255)
    assert fake.inputs[n // 2][0, 0, 0] == np.float32(img[0, 0, 3]) / np.float32(255)


@pytest.mark.parametrize("scale,h,w,tile,tile_pad,pre_pad", CASES + [(4, 1, 1, 0, 10, 0), (4, 1, 7, 2, 2, 0), (2, 2, 2, 0, 10, 1)])
def test_recorded_shapes_are_the_librarys_tiles(ffp, scale, h, w, tile, tile_pad, pre_pad):
    from ffp_amd import _lib
    fake = S.FakeNet(scale, S.nearest_out(scale))
    R.enhance(fake, S.make_image("bgr8", h, w, 3), None, "realesrgan", tile=tile, tile_pad=tile_pad, pre_pad=pre_pad)
    for prec, chans in ((_lib.PREC_F32, {4: 4, 2: 12}), (_lib.PREC_F16, {4: 8, 2: 16})):
        tiles, t16, ch = _lib.op_sr_tiles([(0, w * 3, h, w, 3, 8, 255, S.SEL_BGR)], scale, tile, tile_pad, pre_pad, prec)
        f = 2 if scale == 2 else 1
        assert [(th // f, tw // f) for th, tw in tiles] == [r.shape[:2] for r in fake.inputs]
        assert [(scale * th, scale * tw) for th, tw in tiles] == [o.shape[:2] for o in fake.outputs]
        assert t16 == sum(-(-th // f // 16) * -(-tw // f // 16) for th, tw in tiles)
        assert ch == chans[scale] and ch >= fake.inputs[0].shape[2]


def test_tile_refusals_are_argument_errors(ffp):
    from ffp_amd import _lib
    img = (0, 30, 5, 10, 3, 8, 255, S.SEL_BGR)
    for kw in (dict(scale=4, pre_pad=5), dict(scale=2, tile=3, tile_pad=0), dict(scale=3), dict(scale=4, tile_pad=-1)):
        with pytest.raises(_lib.FfpError) as e:
            _lib.op_sr_tiles([img], **kw)
        assert e.value.code == 1
    with pytest.raises(_lib.FfpError) as e:
        _lib.op_sr_tiles([(0, 3, 1, 1, 3, 8, 255, S.SEL_BGR)], 2)
    assert e.value.code == 1


@pytest.mark.parametrize("max_range", [255, 65535])
def test_prescribed_outputs_hold_every_kind_of_value(max_range):
    v = S.prescribed_out(max_range, 5)(0, None, 4, 4).reshape(-1)
    r = np.float32(max_range)
    assert (v < 0).any() and (v > 1).any() and np.isposinf(v).any() and np.isneginf(v).any() and not np.isnan(v).any()
    assert ((v == 0) & np.signbit(v)).any()
    fin = v[np.isfinite(v) & (v >= 0) & (v <= 1)]
    p = fin * r
    frac = p - np.floor(p)
    ties = p[frac == 0.5]
    assert (np.floor(ties) % 2 == 0).any() and (np.floor(ties) % 2 == 1).any()
    k = np.rint(p)
    assert (k.astype(np.float32) / r == fin).any()

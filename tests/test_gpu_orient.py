"""csrc/orient.hip against its numpy restatement (orient_ref.orient), bit for bit: all eight orientations at 1, 3 and 4 bytes per pixel on the
smallest shapes at which a tiled kernel can go wrong (one pixel, one row and one column longer than a tile, a tile less and a tile more one,
exactly a tile, several tiles with ragged edges both ways), source and destination as views inside sentinel-filled device buffers with padded
pitches and bases at byte offsets 1, 2 and 3 (3-byte pixels against 4-byte words), every byte outside the destination's rows still the sentinel,
the refusals, and a table of five images in one launch."""
import numpy as np
import pytest
import torch

import orient_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def T(gpu_lib):
    return gpu_lib.image_orient_geometry()


def image(h, w, px, seed=0):
    return np.random.default_rng(1000 * h + 10 * w + px + seed).integers(0, 256, (h, w, px)).astype(np.uint8)


def view(buf, lead, h, w, px, pitch):
    return np.lib.stride_tricks.as_strided(buf[lead:], (h, w, px), (pitch, px, 1))


def turn(lib, img, o, src_pad=0, dst_pad=0, src_lead=0, dst_lead=0):
    """img through the kernel between two views -> (result, destination buffer after, mask of the bytes the result owns)"""
    h, w, px = img.shape
    oh, ow = orient_ref.out_shape(h, w, o)
    sp, dp = w * px + src_pad, ow * px + dst_pad
    src = np.full(src_lead + h * sp + 8, SENTINEL, np.uint8)
    view(src, src_lead, h, w, px, sp)[...] = img
    dst = np.full(dst_lead + oh * dp + 8, SENTINEL, np.uint8)
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    torch.cuda.synchronize()
    cap = dst.size - dst_lead
    assert lib.image_orient_dev(d_src.data_ptr() + src_lead, h, w, px, sp, o, d_dst.data_ptr() + dst_lead, dp, cap) == (oh, ow)
    after = d_dst.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy(), src)                      # the source is only read
    owned = np.zeros(dst.size, bool)
    for y in range(oh):
        owned[dst_lead + y * dp: dst_lead + y * dp + ow * px] = True
    return view(after, dst_lead, oh, ow, px, dp).copy(), after, owned


def sizes(T):
    return [(1, 1), (1, T + 1), (T + 1, 1), (T - 1, T + 1), (T, T), (2 * T + 3, T + 5)]


@pytest.mark.parametrize("px", [1, 3, 4])
@pytest.mark.parametrize("o", range(1, 9))
def test_every_orientation_on_the_edge_shapes(gpu_lib, T, o, px):
    for h, w in sizes(T):
        img = image(h, w, px)
        got, after, owned = turn(gpu_lib, img, o)
        assert np.array_equal(got, orient_ref.orient(img, o)), (h, w)
        assert (after[~owned] == SENTINEL).all(), (h, w)


@pytest.mark.parametrize("px", [1, 3, 4])
@pytest.mark.parametrize("o", range(1, 9))
def test_padded_pitches_and_unaligned_bases(gpu_lib, T, o, px):
    h, w = T + 9, 2 * T - 7                                                # more than one tile both ways, ragged
    img = image(h, w, px, seed=7)
    want = orient_ref.orient(img, o)
    cases = [dict(src_pad=5), dict(dst_pad=7), dict(src_pad=1, dst_pad=2)]
    cases += [dict(src_lead=k, dst_lead=(k + 1) % 4, src_pad=k, dst_pad=3 - k) for k in (1, 2, 3)]
    cases += [dict(dst_lead=k) for k in (1, 2, 3)] + [dict(src_lead=k) for k in (1, 2, 3)]
    for kw in cases:
        got, after, owned = turn(gpu_lib, img, o, **kw)
        assert np.array_equal(got, want), kw
        assert (after[~owned] == SENTINEL).all(), kw


def test_the_host_entry_and_gray_arrays(gpu_lib, T):
    img = image(T + 3, T - 2, 3, seed=3)
    for o in (1, 4, 5, 6):
        assert np.array_equal(gpu_lib.image_orient(img, o), orient_ref.orient(img, o))
    rows = img[::2]                                                       # a view with a doubled pitch
    assert np.array_equal(gpu_lib.image_orient(rows, 7), orient_ref.orient(rows, 7))
    gray = image(9, T + 1, 1)[..., 0]
    assert np.array_equal(gpu_lib.image_orient(gray, 8), orient_ref.orient(gray, 8))


def test_refusals_leave_the_destination_untouched(gpu_lib):
    h, w, px = 6, 10, 3
    src = torch.from_numpy(image(h, w, px).reshape(-1)).cuda()
    dst = torch.full((h * w * px + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s, d, row = src.data_ptr(), dst.data_ptr(), w * px
    whole = torch.full((2 * h * row,), SENTINEL, dtype=torch.uint8, device="cuda")      # for the overlap: both images inside one buffer
    calls = {
        "o 0": (s, h, w, px, row, 0, d, row, h * row),
        "o 9": (s, h, w, px, row, 9, d, row, h * row),
        "px 2": (s, h, w, 2, row, 1, d, row, h * row),
        "short source pitch": (s, h, w, px, row - 1, 1, d, row, h * row),
        "short destination pitch": (s, h, w, px, row, 1, d, row - 1, h * row),
        "a turned image at the source's pitch": (s, h, w, px, row, 6, d, row, h * row),      # w rows at that pitch run past a cap that holds h of them
        "short cap": (s, h, w, px, row, 3, d, row, h * row - 1),
        "short cap of a turned image": (s, h, w, px, row, 5, d, h * px, w * h * px - 1),
        "overlap": (whole.data_ptr(), h, w, px, row, 2, whole.data_ptr() + h * row - 1, row, h * row),
        "the same buffer": (whole.data_ptr(), h, w, px, row, 3, whole.data_ptr(), row, h * row),
    }
    images, launches = gpu_lib.image_orient_stats()
    for name, a in calls.items():
        with pytest.raises(gpu_lib.FfpError) as e:
            gpu_lib.image_orient_dev(*a)
        assert e.value.code == gpu_lib.FFP_ERR_ARG, name
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all() and (whole.cpu().numpy() == SENTINEL).all()
    assert gpu_lib.image_orient_stats() == (images, launches)            # nothing was queued
    # and the neighbour of the overlap case, one byte further on, is taken
    gpu_lib.image_orient_dev(whole.data_ptr(), h, w, px, row, 2, whole.data_ptr() + h * row, row, h * row)


def test_five_images_in_one_launch(gpu_lib, T):
    px = 3
    shapes = [(T + 1, 2 * T + 2, 6), (3, 5, 1), (T, T, 8), (2 * T - 1, 7, 3), (1, 3 * T + 1, 5)]
    imgs = [image(h, w, px, seed=i) for i, (h, w, _) in enumerate(shapes)]
    src_off, dst_off, src_pitch, dst_pitch, s_pos, d_pos = [], [], [], [], 1, 2           # odd bases
    for i, (h, w, o) in enumerate(shapes):
        oh, ow = orient_ref.out_shape(h, w, o)
        src_pitch.append(w * px + i)
        dst_pitch.append(ow * px + (4 - i))
        src_off.append(s_pos)
        dst_off.append(d_pos)
        s_pos += h * src_pitch[-1] + 3
        d_pos += oh * dst_pitch[-1] + 5
    src = np.full(s_pos, SENTINEL, np.uint8)
    for im, off, p in zip(imgs, src_off, src_pitch):
        view(src, off, *im.shape, p)[...] = im
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((d_pos,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    images, launches = gpu_lib.image_orient_stats()
    gpu_lib.image_orient_batch_dev(d_src.data_ptr(), src_off, [s[0] for s in shapes], [s[1] for s in shapes], px, src_pitch, [s[2] for s in shapes],
                                   d_dst.data_ptr(), dst_off, dst_pitch, d_pos)
    assert gpu_lib.image_orient_stats() == (images + 5, launches + 1)
    after = d_dst.cpu().numpy()
    owned = np.zeros(d_pos, bool)
    for im, (h, w, o), off, p in zip(imgs, shapes, dst_off, dst_pitch):
        oh, ow = orient_ref.out_shape(h, w, o)
        assert np.array_equal(view(after, off, oh, ow, px, p), orient_ref.orient(im, o)), (h, w, o)
        for y in range(oh):
            owned[off + y * p: off + y * p + ow * px] = True
    assert (after[~owned] == SENTINEL).all()
    # destinations that overlap one another are refused as a whole
    with pytest.raises(gpu_lib.FfpError) as e:
        gpu_lib.image_orient_batch_dev(d_src.data_ptr(), src_off[:2], [3, 3], [5, 5], px, [15, 15], [1, 1], d_dst.data_ptr(), [0, 10], [15, 15], d_pos)
    assert e.value.code == gpu_lib.FFP_ERR_ARG
    # and so is a destination that lies on another image's source: image 0 would be written while image 1 is read
    with pytest.raises(gpu_lib.FfpError) as e:
        gpu_lib.image_orient_batch_dev(d_src.data_ptr(), [0, 200], [3, 3], [5, 5], px, [15, 15], [1, 2], d_src.data_ptr(), [210, 100], [15, 15], s_pos)
    assert e.value.code == gpu_lib.FFP_ERR_ARG
    assert np.array_equal(d_src.cpu().numpy(), src)

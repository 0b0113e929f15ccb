"""JPEG files decoded with their EXIF orientation applied on the device (ffp_jpeg_decode_oriented*, the one decoding routine of
csrc/jpeg_huff.hip followed by csrc/orient.hip): a 40 x 56 crop of a photograph saved by Pillow at 4:2:0, 4:4:4 and grayscale with the tags 1..8.
Bit for bit against orient_ref on the plain decode and against Pillow's exif_transpose; the padding of a padded pitch stays untouched; a forced
orientation overrides the file's; in a batch the turned files cost ONE more launch, a refused file keeps its region, and a batch without a turned
file queues what ffp_jpeg_decode_batch_dev queues."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import orient_ref

pytestmark = pytest.mark.gpu

REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real")
SENTINEL = 0x5A
MODES = {"420": dict(subsampling=2), "444": dict(subsampling=0), "gray": dict()}


@pytest.fixture(scope="module")
def files():
    """{(mode, tag): bytes} and {mode: the plain decode's pixels by Pillow}"""
    crop = Image.open(os.path.join(REAL, "det_family.png")).convert("RGB").crop((100, 60, 156, 100))          # 56 wide, 40 high
    assert crop.size == (56, 40)
    out = {}
    for mode, kw in MODES.items():
        im = crop.convert("L") if mode == "gray" else crop
        for tag in range(1, 9):
            exif = Image.Exif()
            exif[0x0112] = tag
            b = io.BytesIO()
            im.save(b, "JPEG", quality=92, exif=exif, **kw)
            out[(mode, tag)] = b.getvalue()
    b = io.BytesIO()
    exif = Image.Exif()
    exif[0x0112] = 6
    crop.save(b, "JPEG", quality=92, exif=exif, progressive=True)
    out[("progressive", 6)] = b.getvalue()
    return out


def pillow_line(data):
    return np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(data))).convert("RGB"))


@pytest.mark.parametrize("mode", list(MODES))
def test_the_files_own_tag(gpu_lib, files, mode):
    for tag in range(1, 9):
        data = files[(mode, tag)]
        assert gpu_lib.exif_orientation(data) == tag
        plain = gpu_lib.jpeg_decode(data)
        assert plain.shape == (40, 56, 3)
        images = gpu_lib.image_orient_stats()[0]
        got = gpu_lib.jpeg_decode(data, orient=True)
        assert gpu_lib.image_orient_stats()[0] == images + (tag != 1)
        assert got.shape == orient_ref.out_shape(40, 56, tag) + (3,)
        assert np.array_equal(got, orient_ref.orient(plain, tag)), tag
        assert np.array_equal(got, pillow_line(data)), tag
        assert np.array_equal(gpu_lib.jpeg_decode(data, bgr=True, orient=True), got[..., ::-1])


def test_into_a_padded_pitch_on_the_device(gpu_lib, files):
    for tag, lead, pad in ((6, 1, 5), (3, 2, 7), (8, 3, 1), (1, 1, 3)):
        data = files[("420", tag)]
        oh, ow = orient_ref.out_shape(40, 56, tag)
        pitch = ow * 3 + pad
        buf = torch.full((lead + oh * pitch + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        cap = buf.numel() - lead
        assert gpu_lib.jpeg_decode_dev(data, buf.data_ptr() + lead, pitch, cap, bgr=False, orient=True) == (oh, ow)
        after = buf.cpu().numpy()
        got = np.lib.stride_tricks.as_strided(after[lead:], (oh, ow, 3), (pitch, 3, 1))
        assert np.array_equal(got, pillow_line(data)), tag
        owned = np.zeros(after.size, bool)
        for y in range(oh):
            owned[lead + y * pitch: lead + y * pitch + ow * 3] = True
        assert (after[~owned] == SENTINEL).all(), tag
        # one byte short of the oriented image: refused with the buffer as it is
        buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        with pytest.raises(gpu_lib.FfpError) as e:
            gpu_lib.jpeg_decode_dev(data, buf.data_ptr() + lead, pitch, (oh - 1) * pitch + ow * 3 - 1, bgr=False, orient=True)
        assert e.value.code == gpu_lib.FFP_ERR_ARG and (buf.cpu().numpy() == SENTINEL).all()
    # a turned image does not fit the pitch of the stored one
    with pytest.raises(gpu_lib.FfpError):
        gpu_lib.jpeg_decode_dev(files[("420", 6)], buf.data_ptr(), 40 * 3 - 1, buf.numel(), orient=True)


def test_a_forced_orientation_overrides_the_files(gpu_lib, files):
    data = files[("444", 6)]
    plain = gpu_lib.jpeg_decode(data)
    for forced in (1, 3, 5, 8):
        assert np.array_equal(gpu_lib.jpeg_decode(data, orient=forced), orient_ref.orient(plain, forced)), forced
    assert np.array_equal(gpu_lib.jpeg_decode(files[("444", 1)], orient=7), orient_ref.orient(gpu_lib.jpeg_decode(files[("444", 1)]), 7))
    for bad in (-1, 9):
        with pytest.raises(gpu_lib.FfpError) as e:
            gpu_lib.jpeg_decode(data, orient=bad)
        assert e.value.code == gpu_lib.FFP_ERR_ARG


def batch_layout(shapes, pad=0):
    offsets, strides, pos = [], [], 3
    for oh, ow in shapes:
        strides.append(ow * 3 + pad)
        offsets.append(pos)
        pos += oh * strides[-1] + 9
    return offsets, strides, pos


def test_a_batch_of_six(gpu_lib, files):
    tags = [1, 6, 3, 6, 8, 1]
    datas = [files[("420", 1)], files[("444", 6)], files[("gray", 3)], files[("progressive", 6)], files[("420", 8)], files[("444", 1)]]
    shapes = [orient_ref.out_shape(40, 56, t) for t in tags]
    offsets, strides, total = batch_layout(shapes, pad=4)
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    singles = [None if i == 3 else gpu_lib.jpeg_decode(d, orient=True) for i, d in enumerate(datas)]
    images, launches = gpu_lib.image_orient_stats()
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev(datas, buf.data_ptr(), offsets, strides, total, bgr=False, orientations=True)
    assert gpu_lib.image_orient_stats() == (images + 3, launches + 1)       # tags 6, 3 and 8 in one launch; the progressive file never got there
    assert status[3] < 0 and [int(s) for i, s in enumerate(status) if i != 3] == [0] * 5
    after = buf.cpu().numpy()
    owned = np.zeros(total, bool)
    for i, (oh, ow) in enumerate(shapes):
        assert (int(hs[i]), int(ws[i])) == ((0, 0) if i == 3 else (oh, ow))
        if i == 3:
            continue
        got = np.lib.stride_tricks.as_strided(after[offsets[i]:], (oh, ow, 3), (strides[i], 3, 1))
        assert np.array_equal(got, singles[i]), i
        assert np.array_equal(got, pillow_line(datas[i])), i
        for y in range(oh):
            owned[offsets[i] + y * strides[i]: offsets[i] + y * strides[i] + ow * 3] = True
    assert (after[~owned] == SENTINEL).all()                              # the progressive file's region among them
    # per-file values: 0 is the file's own tag, 1..8 forces one
    forced = [5, 0, 1, 1, 0, 2]
    want = [orient_ref.orient(gpu_lib.jpeg_decode(d), o if o else t) for i, (d, o, t) in enumerate(zip(datas, forced, tags)) if i != 3]
    shapes2 = [orient_ref.out_shape(40, 56, o if o else t) for o, t in zip(forced, tags)]
    offsets2, strides2, total2 = batch_layout(shapes2)
    buf2 = torch.full((total2,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev(datas, buf2.data_ptr(), offsets2, strides2, total2, bgr=False, orientations=forced)
    after = buf2.cpu().numpy()
    k = 0
    for i, (oh, ow) in enumerate(shapes2):
        if i == 3:
            continue
        assert (int(hs[i]), int(ws[i])) == (oh, ow)
        assert np.array_equal(np.lib.stride_tricks.as_strided(after[offsets2[i]:], (oh, ow, 3), (strides2[i], 3, 1)), want[k]), i
        k += 1
    with pytest.raises(gpu_lib.FfpError) as e:
        gpu_lib.jpeg_decode_batch_dev(datas, buf2.data_ptr(), offsets2, strides2, total2, orientations=[1, 2, 3, 4, 5, 9])
    assert e.value.code == gpu_lib.FFP_ERR_ARG


def test_a_batch_without_a_turned_file_queues_what_the_plain_entry_queues(gpu_lib, files):
    datas = [files[("420", 1)], files[("444", 1)], files[("gray", 1)], files[("420", 1)]]
    offsets, strides, total = batch_layout([(40, 56)] * 4)
    a = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    b = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_lib.jpeg_decode_batch_dev(datas, a.data_ptr(), offsets, strides, total)
    plain = gpu_lib.jpeg_decode_batch_stats()
    orient_before = gpu_lib.image_orient_stats()
    gpu_lib.jpeg_decode_batch_dev(datas, b.data_ptr(), offsets, strides, total, orientations=True)
    oriented = gpu_lib.jpeg_decode_batch_stats()
    assert oriented[0] == plain[0] + 1 and oriented[1:] == plain[1:]       # one more batch, the same launches and synchronisations
    assert gpu_lib.image_orient_stats() == orient_before
    assert torch.equal(a, b)
    # and with turned files among them: one launch more, however many they are
    turned = [files[("420", 6)], files[("444", 3)], files[("gray", 8)], files[("420", 1)]]
    shapes = [(56, 40), (40, 56), (56, 40), (40, 56)]
    offsets, strides, total = batch_layout(shapes)
    c = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_lib.jpeg_decode_batch_dev(turned, c.data_ptr(), offsets, strides, total, orientations=True)
    assert gpu_lib.jpeg_decode_batch_stats()[1] == plain[1] + 1 and gpu_lib.jpeg_decode_batch_stats()[2] == plain[2]


def test_a_turned_file_the_host_decoder_takes(gpu_lib, files):
    """a stream cut short is flagged by the device decoder and decoded again by the host decoder: status 1, and the same turn afterwards"""
    whole = files[("420", 6)]
    sos = whole.index(b"\xff\xda")
    cut = whole[:sos + 14 + (len(whole) - sos) // 2] + b"\xff\xd9"
    assert gpu_lib.exif_orientation(cut) == 6
    fallbacks = gpu_lib.jpeg_decode_stats()[1]
    plain = gpu_lib.jpeg_decode(cut)
    assert gpu_lib.jpeg_decode_stats()[1] == fallbacks + 1 and plain.shape == (40, 56, 3)
    assert not np.array_equal(plain, gpu_lib.jpeg_decode(whole))           # the cut shows
    datas = [files[("444", 3)], cut, files[("420", 1)]]
    shapes = [(40, 56), (56, 40), (40, 56)]
    offsets, strides, total = batch_layout(shapes, pad=2)
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    images, launches = gpu_lib.image_orient_stats()
    fallbacks = gpu_lib.jpeg_decode_stats()[1]
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev(datas, buf.data_ptr(), offsets, strides, total, bgr=False, orientations=True)
    assert [int(s) for s in status] == [0, 1, 0] and gpu_lib.jpeg_decode_stats()[1] == fallbacks + 1
    assert gpu_lib.image_orient_stats() == (images + 2, launches + 2)       # the sub-batch's launch, and the host-decoded file's own
    assert [(int(a), int(b)) for a, b in zip(hs, ws)] == shapes
    after = buf.cpu().numpy()
    want = [orient_ref.orient(gpu_lib.jpeg_decode(datas[0]), 3), orient_ref.orient(plain, 6), gpu_lib.jpeg_decode(datas[2])]
    owned = np.zeros(total, bool)
    for i, (oh, ow) in enumerate(shapes):
        assert np.array_equal(np.lib.stride_tricks.as_strided(after[offsets[i]:], (oh, ow, 3), (strides[i], 3, 1)), want[i]), i
        for y in range(oh):
            owned[offsets[i] + y * strides[i]: offsets[i] + y * strides[i] + ow * 3] = True
    assert (after[~owned] == SENTINEL).all()
    assert np.array_equal(gpu_lib.jpeg_decode(cut, orient=True), want[1])

"""PNG files read on the device (csrc/png_dec.hip, csrc/png_dec.cpp): one wave per IDAT for files whose IDAT chunks inflate on their own, the host
inflate for every other file, one unfilter kernel for both. Every comparison is exact. The files come from png_seg_ref (Python's zlib, any segment
size / level / strategy), png_ref.write, Pillow and the device encoder; the oracle is png_ref.decode (and the array the file was made from)."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_ref as P
import png_seg_ref as S

pytestmark = pytest.mark.gpu

MIXED = S.SIZES_MIXED
ONE = [16384]


def decode_counted(lib, data, route, **kw):
    """png_decode, and the counters must say which route ran: exactly one decode, on `route`"""
    before = lib.png_decode_stats()
    out = lib.png_decode(data, **kw)
    after = lib.png_decode_stats()
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if route == "parallel" else (0, 1)), (route, before, after)
    return out


# ---- inflate ---------------------------------------------------------------------------------------------------------------------------------
def _inflate_images():
    rng = np.random.default_rng(21)
    h, w = 200, 200
    x = np.arange(w)
    return {
        "noise": rng.integers(0, 64, (h, w, 3)).astype(np.uint8),                              # six bits a byte: Huffman-coded literals, hardly a match
        "constant": np.full((h, w, 3), 85, np.uint8),                                          # 258-byte matches
        "period1": np.repeat(rng.integers(0, 256, (h, 1)).astype(np.uint8), w, 1),             # gray rows of one value: distance 1
        "period3": np.broadcast_to(rng.integers(0, 256, (h, 1, 3)).astype(np.uint8), (h, w, 3)).copy(),   # one colour a row: distance 3
        "ramp": np.broadcast_to(((x * 5) % 251).astype(np.uint8)[None, :, None], (h, w, 3)).copy(),
    }


IMAGES = _inflate_images()
INFLATE_CASES = []
for _sizes, _tag in ((MIXED, "mixed"), (ONE, "16384")):
    INFLATE_CASES += [
        (f"noise-literals-{_tag}", "noise", _sizes, 6, zlib.Z_DEFAULT_STRATEGY),
        (f"constant-258-{_tag}", "constant", _sizes, 6, zlib.Z_DEFAULT_STRATEGY),
        (f"period1-rle-{_tag}", "period1", _sizes, 6, zlib.Z_RLE),
        (f"period3-rle-{_tag}", "period3", _sizes, 6, zlib.Z_RLE),
        (f"period3-overlap-{_tag}", "period3", _sizes, 6, zlib.Z_DEFAULT_STRATEGY),
        (f"fixed-{_tag}", "ramp", _sizes, 6, zlib.Z_FIXED),
        (f"huffman-only-{_tag}", "noise", _sizes, 6, zlib.Z_HUFFMAN_ONLY),
        (f"level6-{_tag}", "ramp", _sizes, 6, zlib.Z_DEFAULT_STRATEGY),
    ]
INFLATE_CASES += [
    ("level0-two-stored-blocks-in-a-span", "noise", [70000], 0, zlib.Z_DEFAULT_STRATEGY),
    ("level6-several-dynamic-blocks-in-a-span", "noise", [120000], 6, zlib.Z_DEFAULT_STRATEGY),
]


@pytest.mark.parametrize("name,image,sizes,level,strategy", INFLATE_CASES, ids=[c[0] for c in INFLATE_CASES])
def test_segmented_files_inflate_on_the_device(gpu_lib, name, image, sizes, level, strategy):
    a = IMAGES[image]
    data = S.write(a, sizes, level, strategy, types=[0] * a.shape[0])         # filter None: the stream is the picture's own bytes, and png_ref unfilters fast
    want = P.decode(data)
    assert np.array_equal(want, a)
    got = decode_counted(gpu_lib, data, "parallel")
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), name


def test_the_span_kinds_the_cases_claim_are_in_the_files():
    """the files above hold what their names say (checked on the raw deflate of single spans)"""
    a = IMAGES["noise"]
    two_stored = S.idat_payloads(S.write(a, [70000], 0, types=[0] * 200))[0][2:]
    assert two_stored[0] == 0 and two_stored[1:3] == b"\xff\xff"                                # a full 65535-byte stored block, then the rest
    assert (S.idat_payloads(S.write(IMAGES["ramp"], ONE, 6, zlib.Z_FIXED, types=[0] * 200))[1][0] >> 1) & 3 == 1
    assert (S.idat_payloads(S.write(a, ONE, 6, zlib.Z_HUFFMAN_ONLY, types=[0] * 200))[1][0] >> 1) & 3 == 2
    several = S.deflate_block_types(S.idat_payloads(S.write(a, [120000], 6, types=[0] * 200))[0][2:])     # how many depends on zlib's symbol buffer: walk them
    assert several.count(2) >= 2, several
    forced = S.deflate_block_types(S.idat_payloads(S.write_blocks(a, 5, types=[0] * 200))[0][2:])
    assert forced.count(2) >= 5, forced


def test_one_span_of_five_dynamic_blocks_that_do_not_end_on_byte_boundaries(gpu_lib):
    """Z_BLOCK ends a block without padding, so the next block header starts in mid-byte: several dynamic blocks in one span, whatever zlib's buffer size"""
    a = IMAGES["noise"]
    data = S.write_blocks(a, 5, types=[0] * 200)
    assert np.array_equal(decode_counted(gpu_lib, data, "parallel"), a)


# ---- round trip through the device encoder ----------------------------------------------------------------------------------------------------------
def _round_trip(lib, a, level=1):
    for bgr in (False, True):
        data = lib.png_encode(a, bgr=bgr, level=level)
        got = decode_counted(lib, data, "parallel", bgr=bgr)
        want = a[..., 0] if a.ndim == 3 and a.shape[2] == 1 else a
        assert got.dtype == a.dtype and got.shape == want.shape and np.array_equal(got, want), (a.shape, a.dtype, bgr)


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_round_trip_channels_and_depths(gpu_lib, ch, dtype):
    rng = np.random.default_rng(ch + 10 * np.dtype(dtype).itemsize)
    hi = 256 if dtype == np.uint8 else 65536
    for (h, w) in [(1, 1), (7, 1), (1, 7), (33, 65), (70, 130)]:
        shape = (h, w) if ch == 1 else (h, w, ch)
        noise = rng.integers(0, hi, shape).astype(dtype)
        half = noise.copy()
        half[:, : w // 2] = hi // 3
        smooth = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5).reshape((h, w) + (1,) * (len(shape) - 2)) * (hi // 256) % hi + np.zeros(shape)).astype(dtype)
        for a in (noise, half, smooth):
            _round_trip(gpu_lib, a)


def test_round_trip_sixteen_bit_colour_at_96x100(gpu_lib):
    rng = np.random.default_rng(5)
    for ch in (3, 4):
        a = rng.integers(0, 65536, (96, 100, ch)).astype(np.uint16)
        a[:, :50] = 30000
        _round_trip(gpu_lib, a)


def test_round_trip_segment_boundaries_in_mid_row(gpu_lib):
    seg = gpu_lib.png_segment_bytes()
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (200, 300, 3)).astype(np.uint8)
    half = noise.copy()
    half[:, :150] = 77
    ramp = np.ascontiguousarray(np.broadcast_to((np.arange(300) * 3 % 256).astype(np.uint8)[None, :, None], (200, 300, 3)))
    assert seg % 901 != 0                                                                           # rows straddle the cuts
    for a in (np.full((200, 300, 3), 85, np.uint8), ramp, noise, half):
        _round_trip(gpu_lib, a)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_round_trip_filtered_size_of_exactly_k_segments(gpu_lib, k):
    seg = gpu_lib.png_segment_bytes()
    rng = np.random.default_rng(k)
    a = rng.integers(0, 256, (k * seg // 256, 255)).astype(np.uint8)
    a[:, 100:] //= 16
    assert a.shape[0] * 256 == k * seg
    _round_trip(gpu_lib, a)


def test_round_trip_level_zero(gpu_lib):
    rng = np.random.default_rng(4)
    _round_trip(gpu_lib, rng.integers(0, 65536, (40, 300, 4)).astype(np.uint16), level=0)
    _round_trip(gpu_lib, rng.integers(0, 256, (47, 54, 3)).astype(np.uint8), level=0)


# ---- the serial route ---------------------------------------------------------------------------------------------------------------------------
def test_files_of_other_writers_take_the_serial_route(gpu_lib):
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, (300, 300, 3)).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(noise).save(b, "PNG")
    pil = b.getvalue()
    cut = S.write_split(noise, 8192)                                                                 # one zlib stream in 8 KiB IDATs, as libpng cuts it
    assert len(S.idat_payloads(cut)) > 10                                                            # (how Pillow cuts its own depends on its buffer size)
    for data in (pil, cut):
        for bgr in (False, True):
            want = noise[..., ::-1] if bgr else noise
            assert np.array_equal(decode_counted(gpu_lib, data, "serial", bgr=bgr), want)
    small = noise[:60, :70]
    for data in (P.write(small), P.write(small, level=0), S.write_split(small, 512), S.write_chained(np.ascontiguousarray(IMAGES["ramp"][:60, :70]), [300])):
        assert np.array_equal(decode_counted(gpu_lib, data, "serial"), P.decode(data))


def test_serial_flag_on_a_segmented_file_gives_the_parallel_routes_bytes(gpu_lib):
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (90, 120, 4)).astype(np.uint8)
    a[20:70, 10:90] = (1, 2, 3, 4)
    for data in (gpu_lib.png_encode(a), S.write(a, MIXED)):
        par = decode_counted(gpu_lib, data, "parallel", bgr=True)
        ser = decode_counted(gpu_lib, data, "serial", bgr=True, flags=gpu_lib.FFP_PNG_DEC_SERIAL)
        assert par.tobytes() == ser.tobytes() and np.array_equal(par[..., [2, 1, 0, 3]], a)


# ---- unfilter ---------------------------------------------------------------------------------------------------------------------------------
def _mixed_types(h):
    return [(3, 4, 1, 0, 2, 4, 3, 2, 1, 4)[r % 10] for r in range(h)]


@pytest.mark.parametrize("ch,dtype", [(1, np.uint8), (1, np.uint16), (3, np.uint8), (4, np.uint8), (3, np.uint16), (4, np.uint16)],
                         ids=["bpp1", "bpp2", "bpp3", "bpp4", "bpp6", "bpp8"])
def test_unfilter_every_type_at_every_path_size(gpu_lib, ch, dtype):
    """the inflated bytes are given (png_ref.write: one zlib stream, host inflate), so these cases test the unfilter kernel alone"""
    rows, cols = gpu_lib.png_unfilter_geometry()
    assert rows >= 64 and cols >= 2
    widths = [1, 2, cols - 1, cols, cols + 1, 2 * cols + 3]
    heights = [1, 2, 63, 64, 65, rows - 1, rows, rows + 1, 2 * rows + 1]
    # wider than the 4 * cols_per_step pixels of the hand-off ring between two waves, under two waves and under all of a band's: the ring wraps
    ring = [(65, 4 * cols + 3), (rows + 1, 4 * cols + 3)]
    sizes = [(3, w) for w in widths] + [(65, cols + 1)] + ring + [(h, w) for h in heights for w in (1, 5)]
    rng = np.random.default_rng(ch * 100 + np.dtype(dtype).itemsize)
    hi = 256 if dtype == np.uint8 else 65536
    for (h, w) in sizes:
        assert (h, w) in ring or h * w <= max(3 * widths[-1], 65 * (cols + 1), heights[-1] * 8)     # the tall cases stay narrow
        a = rng.integers(0, hi, (h, w) if ch == 1 else (h, w, ch)).astype(dtype)
        for types in ([0] * h, [1] * h, [2] * h, [3] * h, [4] * h, _mixed_types(h)):
            data = P.write(a, level=1, types=types)
            for bgr in ((False, True) if ch >= 3 else (False,)):
                got = decode_counted(gpu_lib, data, "serial", bgr=bgr)
                want = a if not bgr else np.concatenate([a[..., 2::-1], a[..., 3:]], axis=2)
                assert got.dtype == a.dtype and np.array_equal(got, want), (h, w, types[:10], bgr)


def test_unfilter_agrees_with_png_ref_and_pillow(gpu_lib):
    """the oracle of the test above is the array the file was made from; here png_ref.decode and Pillow confirm it on one mixed case per pixel size"""
    rng = np.random.default_rng(31)
    for ch, dtype in [(1, np.uint8), (1, np.uint16), (3, np.uint8), (4, np.uint8), (3, np.uint16), (4, np.uint16)]:
        a = rng.integers(0, 256 if dtype == np.uint8 else 65536, (23, 19) if ch == 1 else (23, 19, ch)).astype(dtype)
        data = P.write(a, types=_mixed_types(23))
        got = gpu_lib.png_decode(data)
        assert np.array_equal(got, P.decode(data))
        if dtype == np.uint8:
            assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(data))))


# ---- the device form --------------------------------------------------------------------------------------------------------------------------
def test_device_form_with_a_row_pitch(gpu_lib):
    import torch
    rng = np.random.default_rng(14)
    for ch, dtype in ((3, np.uint8), (4, np.uint16), (1, np.uint8)):
        a = rng.integers(0, 256 if dtype == np.uint8 else 65536, (70, 90, ch)).astype(dtype)
        data = gpu_lib.png_encode(a, bgr=True)
        host = gpu_lib.png_decode(data, bgr=True).reshape(70, 90, ch)
        row = 90 * ch * a.dtype.itemsize
        pitch = row + 37
        buf = torch.full((70 * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        cap = 69 * pitch + row
        assert gpu_lib.png_decode_dev(data, buf.data_ptr(), pitch, cap, bgr=True) == (70, 90, ch, 8 * a.dtype.itemsize)
        back = buf.cpu().numpy().reshape(70, pitch)
        assert back[:, :row].tobytes() == host.tobytes() and np.array_equal(host, a)
        assert (back[:, row:] == 0xA5).all()                                                          # the padding is not touched
        before = gpu_lib.png_decode_stats()
        with pytest.raises(gpu_lib.FfpError) as e:
            gpu_lib.png_decode_dev(data, buf.data_ptr(), pitch, cap - 1, bgr=True)
        assert e.value.code == gpu_lib.FFP_ERR_ARG and gpu_lib.png_decode_stats() == before
    with pytest.raises(gpu_lib.FfpError) as e:
        gpu_lib.png_decode(gpu_lib.png_encode(np.zeros((4, 4), np.uint8)), flags=2)
    assert e.value.code == gpu_lib.FFP_ERR_ARG


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_geometries_are_err_arg_from_png_info(gpu_lib):
    rng = np.random.default_rng(15)
    rgb = rng.integers(0, 256, (20, 30, 3)).astype(np.uint8)
    files = {}
    for mode, field in (("P", "colour type"), ("1", "bit depth"), ("LA", "colour type")):
        b = io.BytesIO()
        Image.fromarray(rgb).convert(mode).save(b, "PNG")
        files[mode] = (b.getvalue(), field)
    files["interlace"] = (S.bad_interlace(), "interlace")
    before = gpu_lib.png_decode_stats()
    for name, (data, field) in files.items():
        for call in (gpu_lib.png_info, gpu_lib.png_decode):
            with pytest.raises(gpu_lib.FfpError, match=field) as e:
                call(data)
            assert e.value.code == gpu_lib.FFP_ERR_ARG, name
    assert gpu_lib.png_decode_stats() == before
    assert gpu_lib.png_info(gpu_lib.png_encode(rgb)) == (20, 30, 3, 8)


# ---- the five hand-made invalid files (each rejected by the same core under the sanitizers first: tests/test_png_decode_host.py) ---------------------
@pytest.mark.parametrize("name", sorted(S.BAD_FILES))
def test_fixed_invalid_files_are_err_arg_and_leave_the_decoder_working(gpu_lib, name):
    build, message = S.BAD_FILES[name]
    before = gpu_lib.png_decode_stats()
    with pytest.raises(gpu_lib.FfpError, match=message) as e:
        gpu_lib.png_decode(build())
    assert e.value.code == gpu_lib.FFP_ERR_ARG and gpu_lib.png_decode_stats() == before
    a = np.random.default_rng(16).integers(0, 256, (40, 50, 3)).astype(np.uint8)
    assert np.array_equal(decode_counted(gpu_lib, S.write(a, [2000]), "parallel"), a)

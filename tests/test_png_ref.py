"""CPU checks of tests/png_ref.py, the numpy restatement the device PNG encoder is held to (tests/test_gpu_png.py): a file written
from its filtered stream decodes, through Pillow, to the input; its unfilterer inverts its filter for all five types, narrow rows and
the first row included. Pillow reduces 16-bit RGB / RGBA to 8 bits on load, so those are decoded with png_ref's own unfilterer."""
import io

import numpy as np
import pytest
from PIL import Image

import png_ref as P


def _img(rng, h, w, ch, dtype):
    shape = (h, w) if ch == 1 else (h, w, ch)
    hi = 256 if dtype == np.uint8 else 65536
    a = rng.integers(0, hi, shape).astype(dtype)
    a[: h // 2] = (a[: h // 2] // 16) * 16                    # smoother top half: more than one filter type gets chosen
    return a


@pytest.mark.parametrize("ch,dtype", [(1, np.uint8), (3, np.uint8), (4, np.uint8), (1, np.uint16)])
def test_pillow_decodes_the_reference_writer(ch, dtype):
    rng = np.random.default_rng(ch * 10 + np.dtype(dtype).itemsize)
    for h, w in ((1, 1), (3, 5), (33, 65)):
        a = _img(rng, h, w, ch, dtype)
        data = P.write(a)
        im = Image.open(io.BytesIO(data))
        im.verify()
        back = np.asarray(Image.open(io.BytesIO(data)))
        assert back.dtype == a.dtype or dtype == np.uint16
        assert np.array_equal(back.astype(a.dtype), a), (h, w, ch, dtype)
        assert np.array_equal(P.decode(data), a)


@pytest.mark.parametrize("ch", [3, 4])
def test_sixteen_bit_colour_round_trips_through_the_reference_unfilterer(ch):
    rng = np.random.default_rng(ch)
    a = _img(rng, 9, 11, ch, np.uint16)
    assert np.array_equal(P.decode(P.write(a)), a)
    assert np.array_equal(P.decode(P.write(a[..., ::-1] if ch == 3 else a[..., [2, 1, 0, 3]], bgr=True)), a)


@pytest.mark.parametrize("ftype", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("h,w,ch,dtype", [(1, 1, 1, np.uint8), (1, 1, 4, np.uint16), (2, 1, 3, np.uint16), (5, 7, 3, np.uint8), (4, 3, 4, np.uint16), (6, 9, 1, np.uint16)])
def test_unfilter_inverts_every_filter_type(ftype, h, w, ch, dtype):
    rng = np.random.default_rng(ftype * 100 + h * 10 + w)
    a = _img(rng, h, w, ch, dtype)
    bpp = ch * np.dtype(dtype).itemsize
    stream = P.filtered_stream(a, types=[ftype] * h)
    assert all(stream[r * (1 + w * bpp)] == ftype for r in range(h))
    assert np.array_equal(P.unfilter(stream, h, w * bpp, bpp), P.raw_rows(a))


def test_filter_choice_rule_on_known_rows():
    zeros = np.zeros(12, np.uint8)
    ramp = np.arange(12, dtype=np.uint8) * 3
    assert P.choose_filter(zeros, zeros, 1) == 0                                 # all sums zero: the lowest type
    assert P.choose_filter(ramp, zeros, 1) == 1                                  # Sub leaves threes; None, Up leave the ramp
    assert P.choose_filter(ramp, ramp, 1) == 2                                   # Up leaves zeros
    # signed counting: 255 counts as 1, so a row of 255s over zeros sums to 12 under None and to 1 under Sub
    assert P.choose_filter(np.full(12, 255, np.uint8), zeros, 1) == 1
    assert P.choose_filter(np.full(12, 200, np.uint8), zeros, 1) == 1            # 56 * 12 against 56


def test_chunk_parser_catches_a_bad_crc():
    a = np.arange(60, dtype=np.uint8).reshape(4, 5, 3)
    data = bytearray(P.write(a))
    P.parse(bytes(data))
    bad = bytearray(data)
    bad[-5] ^= 1                                                                  # IEND's CRC
    with pytest.raises(AssertionError):
        P.parse(bytes(bad))

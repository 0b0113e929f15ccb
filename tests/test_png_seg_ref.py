"""The segmented writer of tests/png_seg_ref.py holds what it promises, on the CPU: its files decode with png_ref.decode and with Pillow to the
input, and every IDAT payload but the Adler one inflates alone as raw deflate. The deliberately non-segmented variants decode too, and their
payloads do not all inflate alone."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_ref as P
import png_seg_ref as S


def _images():
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, (60, 70, 3)).astype(np.uint8)
    flat = np.full((60, 70, 3), 200, np.uint8)
    ramp = np.ascontiguousarray(np.broadcast_to(((np.arange(70) * 5) % 251).astype(np.uint8)[None, :, None], (60, 70, 3)))
    gray16 = (rng.integers(0, 65536, (31, 45)) // 9 * 9).astype(np.uint16)
    rgba = rng.integers(0, 4, (20, 33, 4)).astype(np.uint8) * 60
    return {"noise": noise, "flat": flat, "ramp": ramp, "gray16": gray16, "rgba": rgba}


def _alone(payload, first):
    """raw inflate of one IDAT payload with no history; returns (bytes, the unused tail)"""
    d = zlib.decompressobj(-15)
    out = d.decompress(payload[2:] if first else payload)
    return out, d.unused_data


@pytest.mark.parametrize("sizes", [S.SIZES_MIXED, [16384], [1], [7], [300]], ids=["mixed", "16384", "1", "7", "300"])
@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE], ids=["default", "fixed", "huffman", "rle"])
def test_segmented_files_decode_and_every_idat_inflates_alone(sizes, strategy):
    for name, a in _images().items():
        if sizes in ([1], [7]) and name != "rgba":
            continue                                       # thousands of one-byte segments: the small picture is enough
        data = S.write(a, sizes, 6, strategy)
        assert np.array_equal(P.decode(data), a), name
        if a.dtype == np.uint8:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), a), name
        payloads = S.idat_payloads(data)
        stream = P.filtered_stream(a)
        assert len(payloads) == len(S.cut(stream, sizes)) + 1 and len(payloads[-1]) == 4
        assert payloads[0][:2] == b"\x78\x01"
        got = b""
        for i, p in enumerate(payloads[:-1]):
            out, unused = _alone(p, i == 0)
            assert unused == b"", (name, i)
            if i < len(payloads) - 2:
                assert p.endswith(b"\x00\x00\xff\xff"), (name, i)           # the empty stored block of the sync flush
            got += out
        assert got == stream and int.from_bytes(payloads[-1], "big") == zlib.adler32(stream)


def test_level_zero_and_forced_filter_types():
    a = _images()["noise"]
    for types in (None, [0] * 60, [4] * 60, [r % 5 for r in range(60)]):
        data = S.write(a, [70000], 0, types=types)
        assert np.array_equal(P.decode(data), a)
        assert P.parse(data)["filtered"] == P.filtered_stream(a, types=types)
    two = S.idat_payloads(S.write(np.zeros((200, 200, 3), np.uint8), [70000], 0))[0]
    assert two[2] == 0 and two[3:5] == b"\xff\xff"          # a span of 70 000 stored bytes is two stored blocks


def test_block_walker_and_the_span_of_forced_blocks():
    a = _images()["noise"]
    stream = P.filtered_stream(a)
    assert S.deflate_block_types(zlib.compress(stream, 0)[2:-4]) == [0]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    assert S.deflate_block_types(co.compress(P.filtered_stream(_images()["ramp"])) + co.flush()) == [1]
    data = S.write_blocks(a, 4)
    assert np.array_equal(P.decode(data), a) and len(S.idat_payloads(data)) == 2
    kinds = S.deflate_block_types(S.idat_payloads(data)[0][2:])
    assert len(kinds) >= 4 and set(kinds) <= {0, 2}, kinds           # (noise: zlib may store a block)
    mixed = S.deflate_block_types(S.idat_payloads(S.write(_images()["ramp"], [5000]))[0][2:])
    assert mixed[-1] == 0 and len(mixed) >= 2                        # a segment's own block(s), then the empty stored block of the sync flush


def test_the_non_segmented_variants_decode_but_do_not_inflate_chunk_by_chunk():
    imgs = _images()
    chained = S.write_chained(imgs["ramp"], [300])
    assert np.array_equal(P.decode(chained), imgs["ramp"]) and np.array_equal(np.asarray(Image.open(io.BytesIO(chained))), imgs["ramp"])
    failed = 0
    for i, p in enumerate(S.idat_payloads(chained)[:-1]):
        try:
            _alone(p, i == 0)
        except zlib.error:                                  # "invalid distance too far back": the match reaches into the chunk before
            failed += 1
    assert failed > 0
    split = S.write_split(imgs["noise"], 512)
    assert np.array_equal(P.decode(split), imgs["noise"]) and len(S.idat_payloads(split)) > 4


def test_the_invalid_files_are_invalid_for_png_ref_too():
    """png_ref.parse checks chunk CRCs, the IHDR's fixed fields and, through zlib.decompress, the stream and its Adler-32"""
    for name, (build, _) in S.BAD_FILES.items():
        with pytest.raises((AssertionError, zlib.error)):
            P.parse(build())

"""The EXIF orientation parser (csrc/exif.hpp, plain C++) on the CPU. Through the library: `_lib.exif_orientation` against what Pillow's
getexif() reports (clamped to 1..8, else 1) on files built here — Pillow-written JPEGs with tag values 0..9, hand-built APP1 segments in both
byte orders with the tag as SHORT and as LONG, no tag, APP1 behind a JFIF APP0, an XMP APP1 in front of the Exif one, PNG files with an eXIf
chunk in front of IDAT, behind it and without one — and damaged files, which all give 1. Stand-alone: csrc/exif_host_check.cpp, built with the
HOST compiler under AddressSanitizer + UBSan (`build.py --exif-check`) and run as a child process, hands the parser the same kinds of file, every
prefix of each and seeded single-byte corruptions, each in a heap block of exactly its length. No device anywhere."""
import io
import os
import struct
import subprocess
import zlib

import pytest
from PIL import Image

import ffp_amd  # noqa: F401
from ffp_amd import _lib
from ffp_amd import build as ffp_build


def pillow_says(f: bytes) -> int:
    o = Image.open(io.BytesIO(f)).getexif().get(0x0112, 1)
    return int(o) if isinstance(o, int) and 1 <= o <= 8 else 1


def plain_jpeg() -> bytes:
    b = io.BytesIO()
    Image.new("RGB", (16, 8), (200, 100, 50)).save(b, "JPEG", quality=90)
    return b.getvalue()


def pillow_jpeg(value: int) -> bytes:
    exif = Image.Exif()
    exif[0x0112] = value
    b = io.BytesIO()
    Image.new("RGB", (16, 8), (200, 100, 50)).save(b, "JPEG", quality=90, exif=exif)
    return b.getvalue()


def tiff(le: bool, typ: int, value, ifd_off: int = 8, count=None) -> bytes:
    """TIFF header + IFD0: ImageWidth, then the orientation entry (type 3 SHORT / 4 LONG) unless value is None"""
    e = "<" if le else ">"
    entries = [struct.pack(e + "HHII", 0x0100, 4, 1, 640)]
    if value is not None:
        entries.append(struct.pack(e + "HHI", 0x0112, typ, 1) + (struct.pack(e + "HH", value, 0) if typ == 3 else struct.pack(e + "I", value)))
    head = (b"II" if le else b"MM") + struct.pack(e + "HI", 42, ifd_off)
    return head + b"\0" * max(min(ifd_off, 64) - 8, 0) + struct.pack(e + "H", len(entries) if count is None else count) + b"".join(entries) + b"\0\0\0\0"


def segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def exif_app1(t: bytes) -> bytes:
    return segment(0xE1, b"Exif\0\0" + t)


XMP = segment(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta xmlns:x=\"adobe:ns:meta/\"><rdf:RDF/></x:xmpmeta>")


def jpeg_with(*segs: bytes, after_app0: bool = True) -> bytes:
    """the plain file with the segments put behind its JFIF APP0 (or straight behind SOI)"""
    f = plain_jpeg()
    assert f[2:4] == b"\xff\xe0"
    at = 4 + struct.unpack(">H", f[4:6])[0] if after_app0 else 2
    return f[:at] + b"".join(segs) + f[at:]


def chunk(typ: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def png_with(before=None, after=None) -> bytes:
    b = io.BytesIO()
    Image.new("RGB", (5, 3), (1, 2, 3)).save(b, "PNG")
    f = b.getvalue()
    i, j = f.index(b"IDAT") - 4, f.index(b"IEND") - 4
    return f[:i] + (chunk(b"eXIf", before) if before else b"") + f[i:j] + (chunk(b"eXIf", after) if after else b"") + f[j:]


def well_formed():
    files = {f"pillow jpeg, tag {v}": pillow_jpeg(v) for v in range(10)}
    for le in (True, False):
        for typ in (3, 4):
            for v in (1, 3, 6, 8, 0, 9):
                files[f"app1 {'II' if le else 'MM'} {'SHORT' if typ == 3 else 'LONG'} {v}"] = jpeg_with(exif_app1(tiff(le, typ, v)))
    files["no tag in the directory"] = jpeg_with(exif_app1(tiff(True, 3, None)))
    files["no app1"] = plain_jpeg()
    files["app1 behind the JFIF app0"] = jpeg_with(exif_app1(tiff(False, 3, 6)))
    files["app1 in front of the JFIF app0"] = jpeg_with(exif_app1(tiff(True, 3, 5)), after_app0=False)
    files["xmp app1 in front of the exif one"] = jpeg_with(XMP, exif_app1(tiff(True, 3, 8)))
    files["the directory behind a gap"] = jpeg_with(exif_app1(tiff(True, 3, 3, ifd_off=12)))
    files["png, eXIf in front of IDAT"] = png_with(before=tiff(True, 3, 6))
    files["png, eXIf MM LONG in front of IDAT"] = png_with(before=tiff(False, 4, 3))
    files["png, eXIf behind IDAT"] = png_with(after=tiff(True, 3, 6))
    files["png, no chunk"] = png_with()
    return files


def damaged():
    good = jpeg_with(exif_app1(tiff(True, 3, 6)), after_app0=False)
    assert _lib.exif_orientation(good) == 6
    long_seg = bytearray(good)
    long_seg[4:6] = b"\xff\xf0"                                            # the segment's length runs past the file
    body = tiff(True, 3, 6, count=0xFFFF)[:20]                             # 20 bytes that claim 65535 entries
    cut = good[:2 + 4 + 6 + 8 + 2 + 12 + 5]                                # SOI, segment head, "Exif\0\0", TIFF header, count, one entry, five bytes of the tag's
    return {"segment past the file": bytes(long_seg),
            "IFD offset 0xFFFFFFF0": jpeg_with(exif_app1(tiff(True, 3, 6, ifd_off=0xFFFFFFF0))),
            "IFD offset 0xFFFFFFF0, MM": jpeg_with(exif_app1(tiff(False, 3, 6, ifd_off=0xFFFFFFF0))),
            "entry count 0xFFFF in a 20-byte body": jpeg_with(exif_app1(body)),
            "cut inside the entry": cut,
            "neither kind": b"GIF89a" + bytes(20),
            "two bytes": b"\xff\xd8",
            "empty": b""}


def test_the_library_agrees_with_pillow_on_well_formed_files():
    files = well_formed()
    seen = set()
    for name, f in files.items():
        want = pillow_says(f)
        assert _lib.exif_orientation(f) == want, name
        seen.add(want)
    assert seen == set(range(1, 9))
    # what the corpus is meant to hold, said once against Pillow's answers so that a Pillow which read these files differently would show here
    assert [pillow_says(files[f"pillow jpeg, tag {v}"]) for v in range(10)] == [1, 1, 2, 3, 4, 5, 6, 7, 8, 1]
    assert pillow_says(files["app1 II LONG 6"]) == 6 and pillow_says(files["app1 MM SHORT 8"]) == 8
    assert pillow_says(files["xmp app1 in front of the exif one"]) == 8 and pillow_says(files["the directory behind a gap"]) == 3
    assert pillow_says(files["png, eXIf in front of IDAT"]) == 6 and pillow_says(files["png, eXIf MM LONG in front of IDAT"]) == 3
    assert pillow_says(files["png, eXIf behind IDAT"]) == 6 and pillow_says(files["png, no chunk"]) == 1


def test_damaged_files_are_as_stored():
    for name, f in damaged().items():
        assert _lib.exif_orientation(f) == 1, name


def test_every_prefix_of_a_file_gives_a_value():
    for f in (jpeg_with(XMP, exif_app1(tiff(False, 4, 7))), png_with(before=tiff(True, 3, 2))):
        for n in range(len(f) + 1):
            assert 1 <= _lib.exif_orientation(bytes(f[:n])) <= 8


def test_the_parser_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "exif.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_corpus_prefixes_and_corruptions_under_the_sanitizers():
    driver = ffp_build.build_exif_check(verbose=False)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("exif_host_check: ok"), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

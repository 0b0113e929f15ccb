"""The device JPEG decoder (csrc/jpeg_huff.hip, csrc/jpeg_dec.cpp, csrc/jpeg.hip) on hand-built baseline streams — SURVEY.md §8 f2, the read
side of the reference's file boundary (cv2.imread, pipeline_v4_yolo/1_Inference.py:328-330).

The other JPEG tests decode files a libjpeg-family encoder wrote. Cameras, phones, mozjpeg and image editors write legal baseline files that
break every habit of such an encoder, and cv2.imread reads them. The streams here come from tests/jpeg_stream_builder.py: Huffman tables with
1-bit codes next to 16-bit codes, with every symbol at 16 bits, a table per component under ids 0..3; restart segments of exactly 64k, 64k + 1
and 64k - 1 bytes (no tail subsequence, one of a byte, one of 63 bytes), a tail subsequence shorter than a word as thread 0 of a workgroup, segment
starts at clean offsets 0, 1, 63 (mod 64) and 8192; a restart marker and a stuffed byte across the 1024-byte unstuffing tile; DC category 11, AC category 10, two and three ZRL in a row, blocks that end at k = 63 without EOB, r0 symbols as EOB;
every header layout jpeg_dec.cpp lists as supported; zero padding and fill bytes before RSTn and EOI. tests/test_jpeg_stream_builder.py proves
on the CPU that each stream holds the edge it is named after.

The bar: pixels identical to Pillow (libjpeg-turbo), `np.array_equal`, no tolerance anywhere. Conformant streams (padding with ones, no fill
bytes inside the scan) are decoded ON THE DEVICE (ffp_jpeg_decode_stats), and so are streams whose only liberty is fill bytes before RSTn or
EOI. For zero padding the pixels are the bar and the decoder that produced them is reported in the assertion message (DESIGN.md §JPEG decoding
says which it is)."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import jpeg_stream_builder as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = B.families()
# header layouts jpeg_dec.cpp supports: these decode. Any other one either equals Pillow or is refused with FFP_ERR_ARG, nothing written.
MUST_DECODE = [n for n in FAMILIES["headers"] if n not in B.MAY_REFUSE]
_refs = {}


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def reference(name):
    if name not in _refs:
        _refs[name] = pil_decode(B.build_case(name).data)
    return _refs[name]


def decode(gpu_lib, data):
    """-> (pixels, "device" | "host")"""
    d0, f0, _ = gpu_lib.jpeg_decode_stats()
    got = gpu_lib.jpeg_decode(data)
    d1, f1, _ = gpu_lib.jpeg_decode_stats()
    assert (d1 - d0) + (f1 - f0) == 1
    return got, "device" if d1 > d0 else "host"


def check(gpu_lib, name, on_device=True):
    s = B.build_case(name)
    got, where = decode(gpu_lib, s.data)
    ref = reference(name)
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{name}: wrong pixels from the {where} decoder"
    if on_device:
        assert where == "device", f"{name}: went to the host decoder"
    return where


@pytest.mark.parametrize("family", sorted(f for f in FAMILIES if f.startswith("shape-")))
def test_table_shapes_samplings_and_content_decode_on_the_device(gpu_lib, family):
    """Annex K / deep (1, 2, 3, 9..12, 15, 16 bits) / every symbol at 16 bits / unary DC tables x gray, 4:4:4, 4:2:2, 4:2:0 x noise, a 1-pixel
    checkerboard, 0 / 255 blocks, a flat colour x 1x1, 9x23, 17x33; with three components each has its own tables under ids 0..3."""
    assert len(FAMILIES[family]) == 12
    for name in FAMILIES[family]:
        check(gpu_lib, name)


@pytest.mark.parametrize("name", FAMILIES["big"])
def test_streams_of_just_over_two_workgroups(gpu_lib, name):
    """More than 2 * 8192 + 64 clean bytes: three workgroups, states travel across both boundaries. The flat picture under deep tables is two
    bits a block — it never self-synchronises, exact states travel from workgroup to workgroup in extra rounds."""
    _, _, r0 = gpu_lib.jpeg_decode_stats()
    check(gpu_lib, name)
    _, _, r1 = gpu_lib.jpeg_decode_stats()
    if name == "big|big-flat-deep":
        assert r1 > r0, "no extra round was counted"


@pytest.mark.parametrize("name", FAMILIES["alignment"])
def test_restart_segments_and_stuffed_bytes_on_the_decoders_boundaries(gpu_lib, name):
    check(gpu_lib, name)


@pytest.mark.parametrize("name", FAMILIES["extremes"])
def test_symbol_extremes(gpu_lib, name):
    check(gpu_lib, name)


@pytest.mark.parametrize("name", FAMILIES["headers"] + FAMILIES["refused"])
def test_header_layouts(gpu_lib, name):
    """Every layout either equals Pillow — on the device, these streams are conformant — or is refused with FFP_ERR_ARG, nothing written. The
    layouts jpeg_dec.cpp supports decode: component ids 0, 1, 2, several tables in a segment, tables after SOF and defined twice, Tq and
    Td / Ta up to 3, SOF1, COM / APPn / fill bytes between segments, every DRI variant, a lone component with sampling factors."""
    import torch
    s = B.build_case(name)
    ref = reference(name)
    try:
        got, where = decode(gpu_lib, s.data)
    except gpu_lib.FfpError as e:
        assert name not in MUST_DECODE, f"{name}: a supported header layout was refused: {e}"
        print(f"{name}: refused ({e})")
        assert e.code == gpu_lib.FFP_ERR_ARG, name
        canvas = torch.full((s.h * s.w * 3,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(gpu_lib.FfpError) as e2:
            gpu_lib.jpeg_decode_dev(s.data, canvas.data_ptr(), 0, canvas.numel(), bgr=True)
        assert e2.value.code == gpu_lib.FFP_ERR_ARG and (canvas.cpu().numpy() == 0xA5).all(), name
        return
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{name}: wrong pixels from the {where} decoder"
    assert where == "device", f"{name}: a conformant stream went to the host decoder"


def test_what_libjpeg_accepts_beyond_the_spec(gpu_lib):
    """Zero padding, fill bytes before RSTn and before EOI: pixels equal Pillow's. Fill bytes are dropped by the unstuffing kernels, so those
    streams stay on the device; for zero padding the decoder that produced the pixels is reported, not asserted."""
    where = {name: check(gpu_lib, name, on_device=FILL_ONLY(name)) for name in FAMILIES["lenient"]}
    assert sum(FILL_ONLY(n) for n in where) == 4
    print("decoder per lenient stream:", where)


def FILL_ONLY(name):
    return name.endswith(("fill-before-rst", "fill-before-eoi"))


def mixed_batch():
    """the hand-built set among a few Pillow-written files, shuffled with a seed"""
    from ffp_amd import synth
    photo = synth.synthetic_frame(64, 64, seed=3)
    files, refs, names = [], [], []
    for name in B.whole_set():
        files.append(B.build_case(name).data)
        refs.append(reference(name))
        names.append(name)
    for k, (h, w, kw) in enumerate(((47, 60, dict(quality=95)), (17, 33, dict(quality=90, optimize=True, subsampling=0)),
                                    (64, 64, dict(quality=75, restart_marker_blocks=3, subsampling=1)))):
        b = io.BytesIO()
        Image.fromarray(photo[:h, :w]).save(b, "JPEG", **kw)
        files.append(b.getvalue())
        refs.append(pil_decode(b.getvalue()))
        names.append(f"pillow-{k}")
    order = np.random.default_rng(17).permutation(len(files))
    return [files[i] for i in order], [refs[i] for i in order], [names[i] for i in order]


def test_the_hand_built_set_in_one_batch_and_reversed(gpu_lib):
    """Every case of the catalogue (but the 4-megapixel flat picture, which has its own test) among three Pillow-written files in ONE
    jpeg_decode_batch call, and again reversed. Every file has its own tables (jhb_tables_kernel per file); a file's pixels depend neither on
    its neighbours nor on its place, and neither does the decoder that takes it: every conformant file is Huffman-decoded on the device in the
    batch too — wrong per-file tables would flag every file and the host decoder would still deliver the right pixels."""
    files, refs, names = mixed_batch()
    assert len(files) == len(B.whole_set()) + 3 and len(files) > 250
    singles, where = [], []
    for f in files:
        try:
            px, w = decode(gpu_lib, f)
        except gpu_lib.FfpError as e:
            px, w = e, "refused"
        singles.append(px)
        where.append(w)
    conformant = sum(1 for n, w in zip(names, where) if w != "refused" and (n.startswith("pillow-") or B.build_case(n).conformant))
    assert conformant > 230
    for order in (slice(None), slice(None, None, -1)):
        d0, f0, _ = gpu_lib.jpeg_decode_stats()
        b0 = gpu_lib.jpeg_decode_batch_stats()[0]
        got = gpu_lib.jpeg_decode_batch(files[order])[order]
        d1, f1, _ = gpu_lib.jpeg_decode_stats()
        b1 = gpu_lib.jpeg_decode_batch_stats()[0]
        assert b1 - b0 == 1 and len(got) == len(files)
        assert d1 - d0 >= conformant, "conformant files went to the host decoder in the batch"
        assert (d1 - d0, f1 - f0) == (where.count("device"), where.count("host")), "a file's decoder depends on its batch"
        for g, s, r, name in zip(got, singles, refs, names):
            if isinstance(s, gpu_lib.FfpError):
                assert name.startswith("header|") and name not in MUST_DECODE and isinstance(g, gpu_lib.FfpError) and g.code == s.code, name
            else:
                assert isinstance(g, np.ndarray) and np.array_equal(g, s) and np.array_equal(g, r), name


CHILD = """
import io, json, sys
import numpy as np
import torch
from PIL import Image
sys.path.insert(0, "tests")
import ffp_amd
from ffp_amd import _lib
import jpeg_stream_builder as B
_lib.lib()
out = {}
for name in json.loads(sys.stdin.read()):
    data = B.build_case(name).data
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    try:
        got = _lib.jpeg_decode(data)
        out[name] = "equal" if got.shape == ref.shape and np.array_equal(got, ref) else "wrong pixels"
    except _lib.FfpError as e:
        out[name] = "refused %d" % e.code
d, f, _ = _lib.jpeg_decode_stats()
print("RESULT " + json.dumps({"out": out, "device": d, "fallback": f}))
"""


def test_the_host_decoder_on_the_same_set(gpu_lib):
    """jpeg_dec.cpp is the other implementation of the same semantics: the same streams under FFP_JPEG_HOST_HUFFMAN=1. The switch is read once
    per process: ONE fresh child for every case of the catalogue but the 4-megapixel flat picture; it rebuilds the streams from their names."""
    names = B.whole_set()
    assert len(names) > 250 and "big|big-noise-deep" in names
    env = {k: v for k, v in os.environ.items() if not k.startswith("FFP_") or k == "FFP_LIB"}
    env["FFP_JPEG_HOST_HUFFMAN"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD], input=json.dumps(names), capture_output=True, text=True, env=env, cwd=ROOT, timeout=240)
    assert r.returncode == 0 and "RESULT " in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout[r.stdout.index("RESULT ") + 7:])
    assert res["device"] == 0, "the child decoded on the device: the switch did not reach it"
    assert sorted(res["out"]) == sorted(names)
    for name, what in res["out"].items():
        if what.startswith("refused"):
            assert name.startswith("header|") and name not in MUST_DECODE and what == f"refused {gpu_lib.FFP_ERR_ARG}", (name, what)
        else:
            assert what == "equal", (name, what)

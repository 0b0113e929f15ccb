"""The four codecs on the one workspace pool (csrc/ws_pool.hpp behind csrc/jpeg.hip, jpeg_huff.hip, png.hip, png_dec.hip): every call borrows a
workspace for its length, so encodes and decodes of every kind run side by side, two encodes of one kind included; a workspace grows while
its neighbours are in flight; a decode that is refused half-way gives its workspace back usable; and the counters say what they said before.
The expected results are computed first, on one thread, and pinned as the codecs' own suites pin them: the JPEG encoder's bytes against
Pillow's, the PNG encoder's file against zlib, tests/png_ref.py's filter rule and Pillow, the decoders' pixels against Pillow. The sizes are
the smallest at which the paths differ: 1x1 (one workgroup), 17x33 (odd, a partial MCU, a partial segment), 200x264 (many workgroups, several
PNG segments)."""
import io
import threading

import numpy as np
import pytest
from PIL import Image

import png_ref as P
import png_seg_ref as S

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (17, 33), (200, 264))
PASSES = 5


def pil_save(img, fmt, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, fmt, **kw)
    return b.getvalue()


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def outcome(fn, *a, **kw):
    """("ok", pixels) or ("refused", message): what a decode gave, comparable across threads"""
    try:
        return ("ok", fn(*a, **kw))
    except RuntimeError as e:
        return ("refused", str(e))


def same(a, b):
    return a[0] == b[0] and (np.array_equal(a[1], b[1]) if a[0] == "ok" else a[1] == b[1])


def damaged_streams():
    """test_damaged_streams_go_to_the_host_decoder's three (cut short, bytes flipped, a restart marker removed): the markers are fine, the device
    decoder flags the stream, the host decoder decodes it as libjpeg would or refuses it"""
    from ffp_amd import synth
    img = synth.synthetic_frame(240, 320, seed=9)
    good = pil_save(img, "JPEG", quality=90)
    sos = good.index(b"\xff\xda")
    cut = good[:sos + 14 + (len(good) - sos) // 2] + b"\xff\xd9"
    flipped = bytearray(good)
    for k in range(sos + 200, sos + 260):
        flipped[k] ^= 0x5A
    rst = pil_save(img, "JPEG", quality=90, restart_marker_blocks=4)
    k = rst.index(b"\xff\xd3", rst.index(b"\xff\xda"))
    no_marker = rst[:k] + rst[k + 2:]
    return {"cut": cut, "flipped": bytes(flipped), "marker removed": no_marker}


@pytest.fixture(scope="module")
def cases(gpu_lib):
    """Everything the tests below compare with, computed once on this thread and left unchanged"""
    from ffp_amd import synth
    lib = gpu_lib
    photo = synth.synthetic_frame(64, 64, seed=3)
    noise = np.random.default_rng(21).integers(0, 256, (200, 264, 3), dtype=np.uint8)
    images = [np.ascontiguousarray(photo[:1, :1]), np.ascontiguousarray(photo[:17, :33]), noise]
    assert tuple(a.shape[:2] for a in images) == SIZES
    assert 200 * (1 + 264 * 3) > lib.png_segment_bytes() > 17 * (1 + 33 * 3)
    c = {"images": images, "jpeg_files": [], "png_files": [], "pil_png": pil_save(noise[:60, :70], "PNG"), "jpeg_clean": [], "jpeg_pixels": []}
    for a in images:
        data = lib.jpeg_encode(a, 95)
        assert data == pil_save(a, "JPEG", quality=95), a.shape                      # the encoder's bar: Pillow's bytes
        c["jpeg_files"].append(data)
        data = lib.png_encode(a)
        p = P.parse(data)                                                            # every CRC, zlib.decompress with its Adler-32
        assert p["filtered"] == P.filtered_stream(a, False) and np.array_equal(pil_pixels(data), a), a.shape
        c["png_files"].append(data)
        before = lib.png_decode_stats()
        assert np.array_equal(lib.png_decode(data), a)
        after = lib.png_decode_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (1, 0), "a file of this library's takes the parallel route, and counts once"
        clean = pil_save(a, "JPEG", quality=90)
        c["jpeg_clean"].append(clean)
        c["jpeg_pixels"].append(pil_pixels(clean))
        assert np.array_equal(lib.jpeg_decode(clean), c["jpeg_pixels"][-1]), a.shape
    before = lib.png_decode_stats()
    assert np.array_equal(lib.png_decode(c["pil_png"]), noise[:60, :70]) and np.array_equal(pil_pixels(c["pil_png"]), noise[:60, :70])
    after = lib.png_decode_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (0, 1), "a file of Pillow's takes the serial route, and counts once"
    # the damaged streams: each goes to the host decoder (and its JpegDecodeWs), which decodes or refuses it
    c["damaged"] = {}
    for name, data in damaged_streams().items():
        d0, f0, _ = lib.jpeg_decode_stats()
        c["damaged"][name] = (data, outcome(lib.jpeg_decode, data))
        d1, f1, _ = lib.jpeg_decode_stats()
        assert (d1 - d0, f1 - f0) == (0, 1), name
    c["host_jpeg"] = c["damaged"]["cut"]
    # test_a_refused_single_file_decode_leaves_the_buffer_untouched's two, which neither decoder takes
    c["refused_jpegs"] = (pil_save(synth.synthetic_frame(48, 64, seed=9), "JPEG", quality=90, progressive=True),
                          bytes(np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8)))
    return c


def run_side_by_side(targets):
    raised = []

    def guarded(fn):
        def go():
            try:
                fn()
            except BaseException as e:        # an error or a failed assertion in a thread fails the test that started it
                raised.append(repr(e))
        return go

    threads = [threading.Thread(target=guarded(t), daemon=True) for t in targets]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a codec thread did not return"
    assert raised == []


def test_the_four_codecs_run_side_by_side(gpu_lib, cases):
    lib, c, wrong = gpu_lib, cases, []

    def note(what, ok):
        if not ok:
            wrong.append(what)

    def jpeg_enc():
        for k in range(PASSES):
            for i, a in enumerate(c["images"]):
                note(("jpeg_encode", k, i), lib.jpeg_encode(a, 95) == c["jpeg_files"][i])

    def png_enc():
        for k in range(PASSES):
            for i, a in enumerate(c["images"]):
                note(("png_encode", k, i), lib.png_encode(a) == c["png_files"][i])

    def png_dec():
        for k in range(PASSES):
            for i, a in enumerate(c["images"]):
                note(("png_decode", k, i), np.array_equal(lib.png_decode(c["png_files"][i]), a))
                note(("png_decode, Pillow's file", k, i), np.array_equal(lib.png_decode(c["pil_png"]), c["images"][2][:60, :70]))

    def jpeg_dec():
        data, want = c["host_jpeg"]
        for k in range(PASSES):
            for i in range(len(SIZES)):
                note(("jpeg_decode", k, i), np.array_equal(lib.jpeg_decode(c["jpeg_clean"][i]), c["jpeg_pixels"][i]))
                note(("jpeg_decode, damaged", k, i), same(outcome(lib.jpeg_decode, data), want))

    run_side_by_side([jpeg_enc, png_enc, png_dec, jpeg_dec])
    assert wrong == []


@pytest.mark.parametrize("kind", ["png", "jpeg"])
def test_two_encoders_of_one_kind_at_once(gpu_lib, cases, kind):
    """Each thread alternates between the 17x33 and the 200x264 image, so a leased workspace grows while the other thread's encode is in flight"""
    lib, c, wrong = gpu_lib, cases, []
    encode = (lambda a: lib.png_encode(a)) if kind == "png" else (lambda a: lib.jpeg_encode(a, 95))
    want = c["png_files"] if kind == "png" else c["jpeg_files"]

    def worker(first):
        def go():
            for k in range(PASSES):
                for i in ((1, 2) if first == 1 else (2, 1)):
                    if encode(c["images"][i]) != want[i]:
                        wrong.append((kind, first, k, i))
        return go

    run_side_by_side([worker(1), worker(2)])
    assert wrong == []


def test_a_refused_decode_gives_its_workspace_back_usable(gpu_lib, cases):
    lib, c = gpu_lib, cases
    build, message = S.BAD_FILES["adler"]     # both routes run before it is refused: the workspace has been used, and the refusal unwinds through its lease
    bad_png = build()

    def refusals_then_everything():
        for _ in range(2):
            for data in c["refused_jpegs"]:
                with pytest.raises(lib.FfpError) as e:
                    lib.jpeg_decode(data)
                assert e.value.code == lib.FFP_ERR_ARG
            with pytest.raises(lib.FfpError, match=message):
                lib.png_decode(bad_png)
        for i, a in enumerate(c["images"]):
            assert np.array_equal(lib.jpeg_decode(c["jpeg_clean"][i]), c["jpeg_pixels"][i]), i
            assert np.array_equal(lib.png_decode(c["png_files"][i]), a), i
            assert lib.jpeg_encode(a, 95) == c["jpeg_files"][i] and lib.png_encode(a) == c["png_files"][i], i
        assert np.array_equal(lib.png_decode(c["pil_png"]), c["images"][2][:60, :70])
        assert same(outcome(lib.jpeg_decode, c["host_jpeg"][0]), c["host_jpeg"][1])

    refusals_then_everything()
    run_side_by_side([refusals_then_everything])


def test_the_counters_say_what_they_said(gpu_lib, cases):
    """One sub-batch queues the entropy decode's ten launches and the reconstruction's two, and waits for the stream twice (csrc/jpeg.hpp), whatever
    the number of files: what test_launches_and_synchronisations_do_not_depend_on_the_number_of_files finds equal for 3 and for 40 files"""
    lib, c = gpu_lib, cases
    from ffp_amd import synth
    frame = synth.synthetic_frame(128, 160, seed=8)
    rng = np.random.default_rng(6)
    crops = []
    for _ in range(6):
        h, w = int(rng.integers(20, 97)), int(rng.integers(20, 97))
        crops.append(pil_save(np.ascontiguousarray(frame[:h, :w]), "JPEG", quality=95))
    b0 = lib.jpeg_decode_batch_stats()[0]
    got = lib.jpeg_decode_batch(crops)
    batches, launches, syncs = lib.jpeg_decode_batch_stats()
    assert all(np.array_equal(g, pil_pixels(f)) for g, f in zip(got, crops))
    assert (batches - b0, launches, syncs) == (1, 12, 2)
    for data, route in ((c["png_files"][1], (1, 0)), (c["pil_png"], (0, 1)), (c["png_files"][2], (1, 0))):
        before = lib.png_decode_stats()
        lib.png_decode(data)
        after = lib.png_decode_stats()
        assert (after[0] - before[0], after[1] - before[1]) == route

"""`.png` paths read through the cv2 shim and sahi.utils.cv.read_image_as_array: files of the layout the device encoder writes are inflated and
unfiltered on the GPU (csrc/png_dec.hip), and the shims return exactly what their Pillow line returned before; every other file still goes through
that line. Which files go where follows the measurement (profiles/png_decode_mi355x.json, _lib.png_read_rgb8): both routes beat Pillow on every
frame, so segmented files count as one parallel decode and the one-stream files of other writers as one serial decode; 16-bit, palette and tRNS
files stay with Pillow and move no counter."""
import io

import numpy as np
import pytest
from PIL import Image

import png_seg_ref as S

pytestmark = pytest.mark.gpu

EXIF_ORIENTATION_6 = b"MM\x00\x2a\x00\x00\x00\x08" + b"\x00\x01" + b"\x01\x12\x00\x03\x00\x00\x00\x01\x00\x06\x00\x00" + b"\x00\x00\x00\x00"


@pytest.fixture(scope="module")
def compat(gpu_lib):
    from ffp_amd import compat as c
    c.install()
    return c


def _pillow_bgr(path):
    """the shim's line for every file before the device decoder, and still its line for the files that stay with Pillow"""
    return np.asarray(Image.open(path).convert("RGB"))[..., ::-1]


def _pictures():
    rng = np.random.default_rng(41)
    rgb = rng.integers(0, 256, (67, 91, 3)).astype(np.uint8)
    rgb[10:40, 20:70] = np.linspace(0, 255, 50, dtype=np.uint8)[None, :, None]
    rgba = np.dstack([rgb, rng.integers(0, 256, (67, 91)).astype(np.uint8)])
    return {"gray": np.ascontiguousarray(rgb[..., 1]), "rgb": rgb, "rgba": rgba}


def test_imread_and_read_image_as_array_equal_the_pillow_line(compat, gpu_lib, tmp_path):
    import cv2
    from sahi.utils.cv import read_image_as_array, read_image_as_pil
    for name, a in _pictures().items():
        dev = tmp_path / f"{name}_dev.png"
        dev.write_bytes(gpu_lib.png_encode(a))
        pil = tmp_path / f"{name}_pil.png"
        Image.fromarray(a).save(pil)
        for path, moved in ((str(dev), (1, 0)), (str(pil), (0, 1))):
            want = _pillow_bgr(path)
            before = gpu_lib.png_decode_stats()
            got = cv2.imread(path)
            after = gpu_lib.png_decode_stats()
            assert got.dtype == np.uint8 and got.shape == (67, 91, 3) and np.array_equal(got, want), (name, path)
            assert (after[0] - before[0], after[1] - before[1]) == moved, (name, path)
            before = after
            rgb = read_image_as_array(path)
            after = gpu_lib.png_decode_stats()
            assert np.array_equal(rgb, np.asarray(read_image_as_pil(path))) and np.array_equal(rgb, want[..., ::-1]), (name, path)
            assert (after[0] - before[0], after[1] - before[1]) == moved, (name, path)


def test_sixteen_bit_palette_and_trns_files_return_what_pillow_returns(compat, gpu_lib, tmp_path):
    import cv2
    rng = np.random.default_rng(42)
    g16 = (rng.integers(0, 65536, (33, 47)) // 7 * 7).astype(np.uint16)
    rgb = _pictures()["rgb"]
    files = {"g16_dev": gpu_lib.png_encode(g16), "rgb16_dev": gpu_lib.png_encode(rng.integers(0, 65536, (20, 30, 3)).astype(np.uint16))}
    b = io.BytesIO()
    Image.fromarray(rgb).convert("P").save(b, "PNG")
    files["palette"] = b.getvalue()
    files["trns"] = S.write(rgb, [3000], extra=(S.chunk(b"tRNS", b"\x00\x10\x00\x20\x00\x30"),))
    before = gpu_lib.png_decode_stats()
    for name, data in files.items():
        path = tmp_path / f"{name}.png"
        path.write_bytes(data)
        got = cv2.imread(str(path))
        assert got.dtype == np.uint8 and np.array_equal(got, _pillow_bgr(str(path))), name
    assert gpu_lib.png_decode_stats() == before


def test_exif_orientation_six_comes_back_rotated_as_the_pillow_path_rotates_it(compat, gpu_lib, tmp_path):
    import cv2
    from sahi.utils.cv import read_image_as_array, read_image_as_pil
    a = _pictures()["rgb"]
    path = str(tmp_path / "turned.png")
    with open(path, "wb") as fh:
        fh.write(S.write(a, [16384], extra=(S.chunk(b"eXIf", EXIF_ORIENTATION_6),)))
    with Image.open(path) as im:
        assert im.getexif().get(0x0112) == 6
    want = np.ascontiguousarray(_pillow_bgr(path).transpose(1, 0, 2)[:, ::-1])          # what the shim's _oriented does with 6, on the Pillow line's pixels
    before = gpu_lib.png_decode_stats()
    got = cv2.imread(path)
    assert got.shape == (91, 67, 3) and np.array_equal(got, want)
    assert np.array_equal(got, np.rot90(a[..., ::-1], -1))
    assert gpu_lib.png_decode_stats()[0] == before[0] + 1
    assert np.array_equal(cv2.imread(path, cv2.IMREAD_UNCHANGED), a[..., ::-1])           # no orientation with IMREAD_UNCHANGED, as before
    assert np.array_equal(read_image_as_array(path), np.asarray(read_image_as_pil(path)))  # not a plain file: the PIL path, transposed


def test_sliced_prediction_on_a_png_path_equals_the_decoded_array(compat, gpu_lib, tmp_path):
    from sahi.predict import get_sliced_prediction
    from utils.yolo_wrapper import YOLOv11PoseDetectionModel
    from ffp_amd import synth
    f = synth.synthetic_frame(700, 900, seed=4, n_blobs=20)
    p = tmp_path / "temp_enhanced.png"
    p.write_bytes(gpu_lib.png_encode(f))
    m = YOLOv11PoseDetectionModel(model_path="synthetic:yolo11n-pose", confidence_threshold=0.25, device="cuda:0", image_size=512)
    kw = dict(slice_height=512, slice_width=512, overlap_height_ratio=0.2, overlap_width_ratio=0.2, verbose=0)
    before = gpu_lib.png_decode_stats()
    r_path = get_sliced_prediction(str(p), m, **kw)
    assert gpu_lib.png_decode_stats()[0] == before[0] + 1
    r_arr = get_sliced_prediction(np.asarray(Image.open(str(p)).convert("RGB")), m, **kw)
    key = lambda r: [(o.bbox.to_xyxy(), round(o.score.value, 6)) for o in r.object_prediction_list]
    assert len(key(r_path)) > 0 and key(r_path) == key(r_arr)
    assert (r_path.image_width, r_path.image_height) == (900, 700)


def test_the_enhance_first_hand_off_reads_back_what_imwrite_wrote(compat, gpu_lib, tmp_path):
    """pipeline_v2_enhancement_first/app_v2.py:104-112: the enhanced frame is written to temp_enhanced.png and read back by path. Segmented files go to
    the device (the measurement put them there), so the read is one parallel decode."""
    import cv2
    from ffp_amd import synth
    a = np.ascontiguousarray(synth.synthetic_frame(300, 420, seed=3)[..., ::-1])
    path = str(tmp_path / "t.png")
    assert cv2.imwrite(path, a) is True
    before = gpu_lib.png_decode_stats()
    got = cv2.imread(path)
    after = gpu_lib.png_decode_stats()
    assert np.array_equal(got, a)
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0)

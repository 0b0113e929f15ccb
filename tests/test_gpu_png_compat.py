"""`.png` paths of the cv2 shim and of its callers (utils.visualization.draw_detections, utils.enhancer.FaceEnhancer.enhance_face_crop)
go through the device PNG encoder (csrc/png.hip): other bytes than libpng's, the same pixels. pipeline.CropEnhancerMixin.encode_png does the
same for an image that is already on the device."""
import io
import os
import types

import numpy as np
import pytest
from PIL import Image

import png_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def compat(gpu_lib):
    from ffp_amd import compat as c
    c.install()
    return c


def _device_wrote(path, gpu_lib):
    """the device encoder's layout: one IDAT per segment and the Adler-32's own (Pillow writes the Adler-32 inside its last IDAT)"""
    data = open(path, "rb").read()
    p = P.parse(data)
    S = gpu_lib.png_segment_bytes()
    return p["n_idat"] == -(-len(p["filtered"]) // S) + 1 and len(P.chunks(data)[-2][1]) == 4


def test_imwrite_then_imread_returns_the_bgr_picture(compat, gpu_lib, tmp_path):
    import cv2
    from ffp_amd import synth
    a = np.ascontiguousarray(synth.synthetic_frame(150, 210, seed=3)[..., ::-1])
    path = str(tmp_path / "x.png")
    assert cv2.imwrite(path, a) is True
    assert _device_wrote(path, gpu_lib)
    assert np.array_equal(cv2.imread(path), a)
    assert cv2.imwrite(path, a, [cv2.IMWRITE_PNG_COMPRESSION, 0]) is True
    assert os.path.getsize(path) > a.nbytes and np.array_equal(cv2.imread(path), a)          # stored blocks


def test_bgra_and_sixteen_bit_gray_decode_to_the_same_pixels_through_pillow(compat, gpu_lib, tmp_path):
    import cv2
    rng = np.random.default_rng(8)
    bgra = rng.integers(0, 256, (40, 52, 4)).astype(np.uint8)
    bgra[:20] = (10, 200, 90, 128)
    path = str(tmp_path / "a.png")
    assert cv2.imwrite(path, bgra) and _device_wrote(path, gpu_lib)
    im = Image.open(path)
    assert im.mode == "RGBA" and np.array_equal(np.asarray(im), bgra[..., [2, 1, 0, 3]])
    g16 = (rng.integers(0, 65536, (33, 47)) // 7 * 7).astype(np.uint16)
    path = str(tmp_path / "g.png")
    assert cv2.imwrite(path, g16) and _device_wrote(path, gpu_lib)
    assert np.array_equal(np.asarray(Image.open(path)).astype(np.uint16), g16)


def test_draw_detections_writes_a_png_pillow_accepts(compat, gpu_lib, tmp_path):
    from ffp_amd import synth
    from utils.visualization import draw_detections
    src = str(tmp_path / "in.jpg")
    Image.fromarray(synth.synthetic_frame(200, 260, seed=4)).save(src, quality=95)
    det = types.SimpleNamespace(bbox=types.SimpleNamespace(to_xyxy=lambda: [40.0, 50.0, 120.0, 150.0]), score=types.SimpleNamespace(value=0.87),
                                keypoints=np.asarray([[60, 80, 0.9], [100, 80, 0.9], [80, 100, 0.9], [65, 125, 0.9], [95, 125, 0.9]], np.float32))
    result = types.SimpleNamespace(object_prediction_list=[det])
    out = str(tmp_path / "vis" / "visual_in.png")
    draw_detections(src, result, out)
    Image.open(out).verify()
    assert Image.open(out).size == (260, 200) and _device_wrote(out, gpu_lib)
    px = np.asarray(Image.open(out).convert("RGB"))
    assert tuple(px[150, 80]) == (0, 255, 0)                                             # the box's bottom edge


def test_enhance_face_crop_to_png_writes_the_in_memory_result(compat, gpu_lib, tmp_path):
    import cv2
    from ffp_amd import synth
    from utils.enhancer import FaceEnhancer
    crop = np.ascontiguousarray(synth.synthetic_frame(96, 96, seed=6)[30:54, 40:60, ::-1])
    src = str(tmp_path / "crop.png")
    assert cv2.imwrite(src, crop)
    enh = FaceEnhancer(model_name="RealESRGAN_x4plus", model_path="synthetic:RealESRGAN_x4plus", scale=4, tile=400, half=True)
    want, ok = enh.enhance_image(cv2.imread(src))
    assert ok and want.shape == (96, 80, 3)
    dst = str(tmp_path / "out" / "enhanced.png")
    done, info = enh.enhance_face_crop(src, dst)
    assert done and info["enhanced_size"] == (80, 96) and _device_wrote(dst, gpu_lib)
    assert np.array_equal(np.asarray(Image.open(dst).convert("RGB"))[..., ::-1], want)


def test_mixin_encode_png_leaves_a_resident_frame_as_a_file(gpu_lib):
    import torch
    from ffp_amd import pipeline, synth

    class Stage(pipeline.CropEnhancerMixin):
        pass

    stage = Stage()
    stage.torch, stage.dev, stage._bufs = torch, torch.device("cuda", 0), {}
    bgr = np.ascontiguousarray(synth.synthetic_frame(120, 200, seed=7)[..., ::-1])
    d = torch.from_numpy(bgr).cuda()
    g16 = torch.from_numpy((np.arange(50 * 60, dtype=np.int64).reshape(50, 60) * 21 % 65536).astype(np.uint16).view(np.int16)).cuda()
    torch.cuda.synchronize()
    data = stage.encode_png(d, 120, 200)
    assert data == gpu_lib.png_encode(bgr, bgr=True)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), bgr[..., ::-1])
    assert stage.encode_png(g16, 50, 60, channels=1) == gpu_lib.png_encode(g16.cpu().numpy().view(np.uint16))

"""Image reading helper used by sahi.predict / PredictionResult (PIL; EXIF transposed, RGB)."""
import numpy as np
from PIL import Image, ImageOps

# A baseline RGB .jpg whose EXIF orientation is 2..8 is decoded and turned on the device (csrc/orient.hip) instead of going to Pillow for the whole
# decode. False: such files stay with Pillow, as before (tools/orient_probe.py -> profiles/orient_mi355x.json measures both).
ORIENT_DEVICE_ROUTE = True


def read_image_as_pil(image, exif_fix: bool = True) -> Image.Image:
    Image.MAX_IMAGE_PIXELS = None
    if isinstance(image, Image.Image):
        pil = image
    elif isinstance(image, str):
        pil = Image.open(image)
        if exif_fix:
            pil = ImageOps.exif_transpose(pil)
        pil = pil.convert("RGB")
    elif isinstance(image, np.ndarray):
        if image.ndim == 3 and image.shape[0] < 5 and image.shape[2] > 4:   # CHW -> HWC
            image = image.transpose(1, 2, 0)
        pil = Image.fromarray(image)
    else:
        raise TypeError("read image with 'pillow' using 'Image.open()'")
    return pil


def read_image_as_array(image) -> np.ndarray:
    """HxWx3 uint8 RGB ndarray of what read_image_as_pil would return, without the PIL round trip where none is needed: an ndarray is
    used as it is (SAHI's own np.asarray(read_image_as_pil(ndarray)) is the same bytes), a baseline .jpg is decoded by this build's codec
    (on the GPU; same pixels as libjpeg — tests/test_gpu_jpeg.py) and, when it carries an EXIF rotation, turned there as exif_transpose turns it."""
    if isinstance(image, np.ndarray) and image.ndim == 3 and image.shape[2] == 3 and image.dtype == np.uint8:
        return image
    if isinstance(image, str) and image.lower().endswith((".jpg", ".jpeg")):
        try:
            from ffp_amd import _lib
            if _lib.device_count() > 0:
                with Image.open(image) as im:             # headers only: the mode, and the tag exactly as exif_transpose would see it
                    o = im.getexif().get(0x0112, 1)
                    rgb = im.mode == "RGB"
                turned = o in (2, 3, 4, 5, 6, 7, 8)
                if rgb and (ORIENT_DEVICE_ROUTE if turned else o in (0, 1)):
                    with open(image, "rb") as fh:
                        return _lib.jpeg_decode(fh.read(), bgr=False, orient=int(o) if turned else False)
        except Exception:        # noqa: BLE001 — progressive / CMYK / truncated files: PIL decides
            pass
    if isinstance(image, str) and image.lower().endswith(".png"):
        # 8-bit gray / RGB / RGBA files go through this build's decoder (_lib.png_read_rgb8): the ones its encoder wrote (the enhanced frame of
        # pipeline_v2_enhancement_first/app_v2.py:104-112) are inflated on the GPU, others on the host, all unfiltered on the GPU; every other file stays with PIL
        try:
            from ffp_amd import _lib
            if _lib.device_count() > 0:
                with Image.open(image) as im:
                    plain = im.getexif().get(0x0112, 1) in (0, 1)
                if plain:
                    with open(image, "rb") as fh:
                        a = _lib.png_read_rgb8(fh.read(), bgr=False)
                    if a is not None:
                        return a
        except Exception:        # noqa: BLE001 — PIL decides
            pass
    return np.asarray(read_image_as_pil(image))

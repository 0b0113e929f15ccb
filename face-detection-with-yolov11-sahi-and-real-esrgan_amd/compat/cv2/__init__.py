"""Minimal `cv2` stand-in for the reference's scripts when OpenCV is not installed (it is not a dependency of this
build): the image-file calls they make — `cv2.imread` for the image size (pipeline_v4_yolo/app_yolo_sahi.py:37-42),
`cv2.imwrite` with `[cv2.IMWRITE_JPEG_QUALITY, q]` (utils/enhancer.py:273-278), `cv2.cvtColor` BGR<->RGB, `cv2.resize` —
on Pillow + numpy, BGR arrays like OpenCV's. A real OpenCV further down sys.path always wins: this module then
re-exports it untouched. Drawing: `cv2.rectangle` (pixel-exact for thickness 1, 2 and filled) and `cv2.putText` (through Pillow,
not OpenCV's glyphs) for pipeline_v3_RTDETR/inference.py; utils.visualization of this build draws with Pillow.

`.jpg` files go through this build's JPEG codec on the GPU (csrc/jpeg.hip: ffp_jpeg_decode / ffp_jpeg_encode) whenever a device is
visible; its output is byte-identical (files) and pixel-identical (decoded arrays) to the libjpeg-turbo inside OpenCV and Pillow
(tests/test_gpu_jpeg.py) for YCbCr / grayscale baseline files, so the choice changes the time, not one bit of the result. `.png`
files are written by the device encoder too (csrc/png.hip: ffp_png_encode; uint8 / uint16, gray, BGR or BGRA): other bytes than
libpng's, the same pixels (tests/test_gpu_png.py), 10 to 100 times sooner than Pillow at compress_level=1 (profiles/png_encode_mi355x.json);
8-bit gray / RGB / RGBA `.png` files are read by the device decoder (csrc/png_dec.hip: ffp_png_decode) and come back as Pillow's
`convert("RGB")` gives them; 16-bit, palette, tRNS, gray+alpha and interlaced files stay with Pillow (profiles/png_decode_mi355x.json). Files the
device codec does not read (progressive, RGB-coded with Adobe transform 0 or R/G/B component ids) and machines without a GPU use
Pillow, and say so once on stderr. Like `cv2.imread`, `imread` applies the EXIF orientation tag (not with IMREAD_UNCHANGED): for `.jpg` files on
the device, before the frame comes down, when ORIENT_DEVICE_ROUTE is set (csrc/orient.hip; off by default).
"""
import importlib.machinery
import importlib.util
import os
import sys

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _real_cv2():
    for p in sys.path:
        if not p or os.path.abspath(p) == _here:
            continue
        spec = importlib.machinery.PathFinder.find_spec("cv2", [p])
        if spec is not None and spec.origin and os.path.dirname(os.path.dirname(os.path.abspath(spec.origin))) != _here:
            return spec
    return None


_spec = _real_cv2()
if _spec is not None:                                   # OpenCV is installed: be it
    _mod = importlib.util.module_from_spec(_spec)
    sys.modules[__name__] = _mod
    _spec.loader.exec_module(_mod)
else:
    import numpy as np
    from PIL import Image

    __version__ = "0.0-ffp-shim"
    IMREAD_COLOR, IMREAD_UNCHANGED = 1, -1
    IMWRITE_JPEG_QUALITY, IMWRITE_PNG_COMPRESSION = 1, 16
    COLOR_BGR2RGB, COLOR_RGB2BGR = 4, 4
    INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4

    _state = {"gpu": None, "told": False, "told_png": False}

    # .jpg / .jpeg, True: the EXIF orientation is read from the file's bytes and applied on the device before the frame comes down (csrc/exif.hpp,
    # csrc/orient.hip). False: the tag through Pillow and a numpy transpose-and-copy on the host, as before. Off by default: the device route's
    # median is 9 to 11 times lower, but in one of two visits its slowest sample (31.7 ms) did not beat the host route's fastest (24.5 ms), and a
    # route is on only where it does (README, profiles/orient_mi355x.json).
    ORIENT_DEVICE_ROUTE = False

    def _gpu_codec():
        if _state["gpu"] is None:
            try:
                from ffp_amd import _lib
                _state["gpu"] = _lib if _lib.device_count() > 0 else False
            except Exception:
                _state["gpu"] = False
        return _state["gpu"]

    def _tell(why):
        if not _state["told"]:
            _state["told"] = True
            print(f"cv2 shim: JPEG through Pillow ({why}); same bytes, host speed", file=sys.stderr)

    def _tell_png(why):
        if not _state["told_png"]:
            _state["told_png"] = True
            print(f"cv2 shim: PNG through Pillow ({why}); same pixels, host speed", file=sys.stderr)

    def _is_png(path):
        return os.path.splitext(str(path))[1].lower() == ".png"

    def _is_jpeg(path):
        return os.path.splitext(str(path))[1].lower() in (".jpg", ".jpeg")

    def _exif_orientation(path):
        """EXIF orientation tag (1..8; 1 = as stored). Reads the APP1 segment only, no pixel decoding."""
        try:
            with Image.open(path) as im:
                o = int(im.getexif().get(0x0112, 1))
            return o if 1 <= o <= 8 else 1
        except Exception:
            return 1

    def _oriented(a, o):
        """What OpenCV's imread does with the EXIF orientation unless IMREAD_IGNORE_ORIENTATION / IMREAD_UNCHANGED is set."""
        if o == 2:
            a = a[:, ::-1]
        elif o == 3:
            a = a[::-1, ::-1]
        elif o == 4:
            a = a[::-1]
        elif o == 5:
            a = a.transpose(1, 0, 2)
        elif o == 6:
            a = a.transpose(1, 0, 2)[:, ::-1]
        elif o == 7:
            a = a.transpose(1, 0, 2)[::-1, ::-1]
        elif o == 8:
            a = a.transpose(1, 0, 2)[::-1]
        return np.ascontiguousarray(a)

    def imread(path, flags=IMREAD_COLOR):
        """HxWx3 uint8 BGR with the EXIF orientation applied (OpenCV's default), or None when the file cannot be read (OpenCV's
        convention: no exception)."""
        try:
            turn = flags != IMREAD_UNCHANGED
            tag = lambda: _exif_orientation(path) if turn else 1       # through Pillow, for the host's transpose-and-copy
            if _is_jpeg(path):
                codec = _gpu_codec()
                if codec:
                    with open(path, "rb") as fh:
                        data = fh.read()
                    try:
                        if ORIENT_DEVICE_ROUTE:
                            return codec.jpeg_decode(data, bgr=True, orient=turn)      # the tag from the bytes, the turn on the device
                        return _oriented(codec.jpeg_decode(data, bgr=True), tag())
                    except codec.FfpError as e:               # e.g. a progressive or an RGB-coded (Adobe transform 0) file
                        _tell(str(e))
                else:
                    _tell("no GPU visible")
            elif _is_png(path):
                codec = _gpu_codec()
                if codec:
                    with open(path, "rb") as fh:
                        a = codec.png_read_rgb8(fh.read(), bgr=True)      # None: the file stays with Pillow (16-bit, palette, tRNS, a route left to Pillow)
                    if a is not None:
                        return _oriented(a, tag())
            return _oriented(np.asarray(Image.open(path).convert("RGB"))[..., ::-1], tag())
        except Exception:
            return None

    def imwrite(path, img, params=None):
        """JPEG quality from [IMWRITE_JPEG_QUALITY, q] (OpenCV default 95); [IMWRITE_PNG_COMPRESSION, 0] gives stored blocks, every
        other level the device's one compressor. Returns success like OpenCV."""
        try:
            q, png_level = 95, 1
            if params:
                for k, v in zip(params[0::2], params[1::2]):
                    if k == IMWRITE_JPEG_QUALITY:
                        q = int(v)
                    elif k == IMWRITE_PNG_COMPRESSION:
                        png_level = int(v)
            a = np.ascontiguousarray(img)
            if _is_png(path) and a.dtype in (np.uint8, np.uint16) and a.size > 0 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] in (1, 3, 4))):
                codec = _gpu_codec()
                if codec:
                    data = codec.png_encode(a, 0 if png_level == 0 else 1, bgr=True)
                    with open(path, "wb") as fh:
                        fh.write(data)
                    return True
                _tell_png("no GPU visible")
            if _is_jpeg(path) and a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8:
                codec = _gpu_codec()
                if codec:
                    data = codec.jpeg_encode(a, q, bgr=True)
                    with open(path, "wb") as fh:
                        fh.write(data)
                    return True
                _tell("no GPU visible")
            pil = Image.fromarray(a[..., ::-1] if a.ndim == 3 and a.shape[2] == 3 else a)
            if _is_jpeg(path):
                pil.save(path, quality=q)
            else:
                pil.save(path)
            return True
        except Exception:
            return False

    FONT_HERSHEY_SIMPLEX, LINE_8, FILLED = 0, 8, -1

    def _paint(img, y0, y1, x0, x1, color):
        h, w = img.shape[:2]
        y0, y1, x0, x1 = max(y0, 0), min(y1, h - 1), max(x0, 0), min(x1, w - 1)
        if y0 <= y1 and x0 <= x1:
            c = np.asarray(color, np.float64).reshape(-1)
            img[y0:y1 + 1, x0:x1 + 1] = c[0] if img.ndim == 2 else np.resize(c, img.shape[2])[: img.shape[2]] if c.size < img.shape[2] else c[: img.shape[2]]

    def rectangle(img, pt1, pt2, color, thickness=1, lineType=LINE_8, shift=0):
        """Axis-aligned cv2.rectangle with LINE_8 and shift 0, in place, pixel for pixel as imgproc/drawing.cpp draws it:
        thickness 1 is the one-pixel outline x1..x2 / y1..y2; thickness 2 is each edge as a filled polygon one pixel either side of
        the edge (three-pixel bands spanning the edge's own length) plus a radius-1 filled circle (a plus) at every corner, so the
        four outer diagonal corner pixels stay unpainted; thickness < 0 fills x1..x2 x y1..y2. Other thicknesses, anti-aliased lines
        and sub-pixel shifts are not restated and raise NotImplementedError."""
        if shift or lineType not in (LINE_8, 4, 8):
            raise NotImplementedError("cv2 shim: rectangle with shift or anti-aliasing")
        x1, x2 = sorted((int(pt1[0]), int(pt2[0])))
        y1, y2 = sorted((int(pt1[1]), int(pt2[1])))
        t = int(thickness)
        if t < 0:
            _paint(img, y1, y2, x1, x2, color)
        elif t <= 1:
            _paint(img, y1, y1, x1, x2, color); _paint(img, y2, y2, x1, x2, color)
            _paint(img, y1, y2, x1, x1, color); _paint(img, y1, y2, x2, x2, color)
        elif t == 2:
            for y in (y1, y2):
                _paint(img, y - 1, y + 1, x1, x2, color)
            for x in (x1, x2):
                _paint(img, y1, y2, x - 1, x + 1, color)
            for (x, y) in ((x1, y1), (x2, y1), (x2, y2), (x1, y2)):
                _paint(img, y, y, x - 1, x + 1, color); _paint(img, y - 1, y + 1, x, x, color)
        else:
            raise NotImplementedError(f"cv2 shim: rectangle thickness {t} (1, 2 and filled are provided)")
        return img

    def putText(img, text, org, fontFace, fontScale, color, thickness=1, lineType=LINE_8, bottomLeftOrigin=False):
        """Text through Pillow, in place: NOT OpenCV's Hershey glyphs, so the pixels differ from cv2.putText's. DejaVu Sans (Pillow's
        built-in font when it is missing) at about the cap height FONT_HERSHEY_SIMPLEX has at fontScale (22 * fontScale px), with `org`
        the left end of the baseline as in OpenCV; `thickness` widens the strokes."""
        from PIL import ImageDraw, ImageFont
        size = max(int(round(22 * float(fontScale))), 6)
        try:
            font = ImageFont.truetype("DejaVuSans.ttf", size)
        except OSError:
            font = ImageFont.load_default()
        a = np.ascontiguousarray(img)
        pil = Image.fromarray(a)
        c = tuple(int(v) for v in np.asarray(color).reshape(-1)[: (1 if a.ndim == 2 else a.shape[2])])
        ImageDraw.Draw(pil).text((int(org[0]), int(org[1])), str(text), fill=c[0] if a.ndim == 2 else c, font=font, anchor="ls",
                                 stroke_width=max(int(thickness) - 1, 0), stroke_fill=c[0] if a.ndim == 2 else c)
        img[...] = np.asarray(pil)
        return img

    def cvtColor(img, code):
        if code != COLOR_BGR2RGB:
            raise NotImplementedError("cv2 shim: only BGR<->RGB")
        return np.ascontiguousarray(img[..., ::-1])

    def resize(img, dsize, fx=0, fy=0, interpolation=INTER_LINEAR):
        w, h = dsize if dsize and dsize[0] > 0 else (int(round(img.shape[1] * fx)), int(round(img.shape[0] * fy)))
        mode = {INTER_NEAREST: Image.NEAREST, INTER_LINEAR: Image.BILINEAR, INTER_CUBIC: Image.BICUBIC, INTER_AREA: Image.BOX,
                INTER_LANCZOS4: Image.LANCZOS}[interpolation]
        return np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((w, h), mode))

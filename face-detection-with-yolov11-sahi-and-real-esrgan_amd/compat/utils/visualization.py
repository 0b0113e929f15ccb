"""utils.visualization with the reference's surface (/root/reference/utils/visualization.py:37-285) on Pillow + numpy:
`draw_detections`, `draw_detections_on_image`, `draw_keypoints_and_skeleton`, `save_face_crops`, `create_detection_summary`
and the landmark tables, so that the import block of pipeline_v4_yolo/app_yolo_sahi.py:13-17 and
pipeline_v1_detection_first/app_v1.py:12 resolves and the scripts' output files (overlay JPEG, crops, summary text) appear
where the reference puts them. `save_face_crops` is the part ON the hot path (it defines the crops the enhancer sees,
:185-223: int box, clamp to the image, skip empty); drawing is presentation code, rendered with PIL primitives (pixel
values of lines and glyphs are not part of any parity claim). Arrays are BGR like cv2's.

`draw_detections` and `save_face_crops` keep the frame on the device when they can (a visible device, a .jpg / .jpeg / .png input the device
decoders read, no EXIF turn, a .jpg / .jpeg / .png output): decode into device memory, draw with csrc/overlay.hip from the list
`build_overlay_prims` makes (the same pixels as the Pillow drawing, bit for bit) or take the crops as views, encode where the frame lies.
Anything else, and any error on the way, takes the host route; the files are the same bytes either way (tests/test_gpu_overlay_compat.py).
"""
import io
import os

import numpy as np
from PIL import Image, ImageDraw

# 5 face landmarks in WIDER FACE order, their skeleton and per-point colours (BGR), as the reference draws them (:5-35)
FACE_KEYPOINT_NAMES = ["left_eye", "right_eye", "nose", "left_mouth", "right_mouth"]
FACE_SKELETON = [[0, 1], [0, 2], [1, 2], [2, 3], [2, 4], [3, 4]]
FACE_KEYPOINT_COLORS = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255)]
SKELETON_COLOR = (0, 255, 255)


def _rgb(bgr):
    return (int(bgr[2]), int(bgr[1]), int(bgr[0]))


def _imread_bgr(path):
    """cv2.imread (a real OpenCV, or this build's shim: JPEG decoded on the GPU, pixel-identical to libjpeg-turbo): BGR or None."""
    try:
        import cv2
        return cv2.imread(str(path))
    except Exception:
        return None


def _imwrite_bgr(path, img, quality=95):
    """cv2.imwrite with [IMWRITE_JPEG_QUALITY, quality] (the shim encodes .jpg on the GPU, byte-identical to libjpeg-turbo)."""
    try:
        import cv2
        return bool(cv2.imwrite(str(path), np.ascontiguousarray(img), [cv2.IMWRITE_JPEG_QUALITY, int(quality)]))
    except Exception:
        return False


def _draw_kpts(draw, keypoints, thr, skeleton):
    if keypoints is None or len(keypoints) == 0:
        return
    if skeleton:
        for a, b in FACE_SKELETON:
            if a < len(keypoints) and b < len(keypoints) and keypoints[a][2] > thr and keypoints[b][2] > thr:
                draw.line([(int(keypoints[a][0]), int(keypoints[a][1])), (int(keypoints[b][0]), int(keypoints[b][1]))], fill=_rgb(SKELETON_COLOR), width=2)
    for i, (x, y, c) in enumerate(np.asarray(keypoints)[:, :3]):
        if c > thr:
            col = FACE_KEYPOINT_COLORS[i] if i < len(FACE_KEYPOINT_COLORS) else (255, 255, 255)
            x, y = int(x), int(y)
            draw.ellipse([x - 3, y - 3, x + 3, y + 3], outline=(255, 255, 255))
            draw.ellipse([x - 2, y - 2, x + 2, y + 2], fill=_rgb(col))


def draw_keypoints_and_skeleton(image, keypoints, confidence_threshold=0.3, draw_skeleton=True):
    """In the reference this draws into `image` and returns it (:37-76); same here for a BGR ndarray."""
    if keypoints is None or len(keypoints) == 0:
        return image
    pil = Image.fromarray(np.ascontiguousarray(image[..., ::-1]))
    _draw_kpts(ImageDraw.Draw(pil), keypoints, confidence_threshold, draw_skeleton)
    image[...] = np.asarray(pil)[..., ::-1]
    return image


def _render(pil, result, show_confidence, show_keypoints, box_color, text_color, kpt_conf_threshold, draw_skeleton, verbose):
    draw = ImageDraw.Draw(pil)
    found = 0
    for idx, det in enumerate(result.object_prediction_list):
        x1, y1, x2, y2 = [int(c) for c in det.bbox.to_xyxy()]
        draw.rectangle([x1, y1, x2, y2], outline=_rgb(box_color), width=2)
        if show_confidence:
            label = f"Face: {det.score.value:.2f}"
            l, t, r, b = draw.textbbox((0, 0), label)
            draw.rectangle([x1, y1 - (b - t) - 10, x1 + (r - l), y1], fill=_rgb(box_color))
            draw.text((x1, y1 - (b - t) - 7), label, fill=_rgb(text_color))
        if show_keypoints:
            k = getattr(det, "keypoints", None)
            if k is not None:
                found += 1
                if verbose:
                    print(f"   ✓ Face #{idx + 1}: Keypoints shape = {np.asarray(k).shape}")
                _draw_kpts(draw, k, kpt_conf_threshold, draw_skeleton)
            elif verbose:
                print(f"   ⚠️  Face #{idx + 1}: NO keypoints attached!")
    return found


# ---- the same drawing as a list of device primitives (csrc/overlay.hip, _lib.overlay_draw_dev) ----------------------------------------------
# `_render` above is the oracle: build_overlay_prims gives, detection by detection and in `_render`'s order, primitives that leave exactly
# `_render`'s pixels (tests/test_overlay_builder.py). Everything Pillow rasterises is taken from Pillow itself, drawn with ink 255 on a black
# "L" canvas — that canvas IS the 8-bit mask, since Pillow's blend of 0 with 255 under m gives m — and laid on as a STAMP with Pillow's
# blend; what Pillow paints as plain rows and columns (fills, outlines of ordinary boxes) is a RECT.
_STAMP_CACHE = {}          # label / shape key -> (dx, dy, mask array): what a glyph run or a landmark looks like does not depend on where it lies
_STAMP_CACHE_MAX = 4096


def _tight(canvas_arr, ox, oy):
    """(dx, dy, mask) of the non-zero part of a canvas whose pixel (0, 0) lies at (ox, oy); None when nothing was painted"""
    ys, xs = np.nonzero(canvas_arr)
    if ys.size == 0:
        return None
    x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    return ox + x0, oy + y0, np.ascontiguousarray(canvas_arr[y0:y1 + 1, x0:x1 + 1])


def _cached_stamp(key, make):
    s = _STAMP_CACHE.get(key)
    if s is None and key not in _STAMP_CACHE:
        if len(_STAMP_CACHE) >= _STAMP_CACHE_MAX:
            _STAMP_CACHE.clear()
        s = _STAMP_CACHE[key] = make()
    return s


def _label_stamp(label):
    """((text width, text height) as draw.textbbox((0, 0), label) gives them, stamp of draw.text((0, 0), label) or None)"""
    def make():
        probe = ImageDraw.Draw(Image.new("RGB", (1, 1)))
        l, t, r, b = probe.textbbox((0, 0), label)
        pad = 8
        canvas = Image.new("L", (max(int(r), 0) + 2 * pad, max(int(b), 0) + 2 * pad), 0)
        ImageDraw.Draw(canvas).text((pad, pad), label, fill=255)
        return (r - l, b - t), _tight(np.asarray(canvas), -pad, -pad)
    return _cached_stamp(("text", label), make)


def _ellipse_stamp(radius, filled):
    def make():
        canvas = Image.new("L", (2 * radius + 1, 2 * radius + 1), 0)
        ImageDraw.Draw(canvas).ellipse([0, 0, 2 * radius, 2 * radius], **({"fill": 255} if filled else {"outline": 255}))
        return _tight(np.asarray(canvas), -radius, -radius)
    return _cached_stamp(("ellipse", radius, filled), make)


def _small_box_stamp(bw, bh, width):
    """outline of a box under 2*width pixels wide or high, where Pillow's rows and columns reach outside the box"""
    def make():
        pad = width + 2
        canvas = Image.new("L", (bw + 2 * pad, bh + 2 * pad), 0)
        ImageDraw.Draw(canvas).rectangle([pad, pad, pad + bw - 1, pad + bh - 1], outline=255, width=width)
        return _tight(np.asarray(canvas), -pad, -pad)
    return _cached_stamp(("box", bw, bh, width), make)


class _PrimList:
    def __init__(self):
        self.rows, self.masks, self.mask_bytes, self.placed = [], [], 0, {}

    def rect(self, x0, y0, x1, y1, bgr, width=0):
        self.rows += (0, x0, y0, x1, y1, width, 0, bgr)

    def stamp(self, x, y, mask, bgr, key=None):
        off = self.placed.get(key) if key is not None else None
        if off is None:
            off = self.mask_bytes
            self.masks.append(mask.reshape(-1))
            self.mask_bytes += mask.size
            if key is not None:
                self.placed[key] = off
        self.rows += (1, x, y, mask.shape[1], mask.shape[0], mask.shape[1], off, bgr)


def _byte3(bgr):
    """a colour as the record's four colour bytes read as one little-endian int32: [0..2] the channels, [3] zero"""
    c = [min(max(int(v), 0), 255) for v in bgr[:3]]
    return c[0] | (c[1] << 8) | (c[2] << 16)


def build_overlay_prims(result, width, height, show_confidence=True, show_keypoints=True, box_color=(0, 255, 0), text_color=(0, 0, 0),
                        kpt_conf_threshold=0.3, draw_skeleton=False, log=None):
    """draw_detections' drawing on a width x height BGR frame as (records of _lib.OVERLAY_PRIM_DTYPE, uint8 mask pool, faces with keypoints):
    painted in order by _lib.overlay_draw_dev they leave the pixels `_render` leaves. log: a list that receives `_render`'s verbose lines."""
    from ffp_amd import _lib
    out = _PrimList()
    box_c, text_c, white, skel_c = _byte3(box_color), _byte3(text_color), _byte3((255, 255, 255)), _byte3(SKELETON_COLOR)
    kpt_c = [_byte3(c) for c in FACE_KEYPOINT_COLORS]
    ring, disc = _ellipse_stamp(3, False), _ellipse_stamp(2, True)
    canvas = None          # frame-sized: a wide line's pixels depend on its absolute coordinates, so it is rasterised where it lies
    found = 0
    for idx, det in enumerate(result.object_prediction_list):
        x1, y1, x2, y2 = [int(c) for c in det.bbox.to_xyxy()]
        if x2 < x1 or y2 < y1:
            raise ValueError("x1 must be greater than or equal to x0" if x2 < x1 else "y1 must be greater than or equal to y0")      # as ImageDraw.rectangle
        if x2 - x1 + 1 >= 4 and y2 - y1 + 1 >= 4:
            out.rect(x1, y1, x2, y2, box_c, 2)
        else:
            s = _small_box_stamp(x2 - x1 + 1, y2 - y1 + 1, 2)
            if s is not None:
                out.stamp(x1 + s[0], y1 + s[1], s[2], box_c, ("box", x2 - x1, y2 - y1))
        if show_confidence:
            label = f"Face: {det.score.value:.2f}"
            (tw, th), s = _label_stamp(label)
            out.rect(x1, y1 - th - 10, x1 + tw, y1, box_c)
            if s is not None:
                out.stamp(x1 + s[0], y1 - th - 7 + s[1], s[2], text_c, ("text", label))
        if show_keypoints:
            k = getattr(det, "keypoints", None)
            if k is not None:
                found += 1
                if log is not None:
                    log.append(f"   ✓ Face #{idx + 1}: Keypoints shape = {np.asarray(k).shape}")
                if len(k) > 0:
                    if draw_skeleton:
                        for a, b in FACE_SKELETON:
                            if a < len(k) and b < len(k) and k[a][2] > kpt_conf_threshold and k[b][2] > kpt_conf_threshold:
                                ax, ay, bx, by = int(k[a][0]), int(k[a][1]), int(k[b][0]), int(k[b][1])
                                bx0, by0 = max(min(ax, bx) - 4, 0), max(min(ay, by) - 4, 0)
                                bx1, by1 = min(max(ax, bx) + 5, width), min(max(ay, by) + 5, height)
                                if bx0 >= bx1 or by0 >= by1:
                                    continue
                                if canvas is None:
                                    canvas = Image.new("L", (width, height), 0)
                                ImageDraw.Draw(canvas).line([(ax, ay), (bx, by)], fill=255, width=2)
                                s = _tight(np.asarray(canvas.crop((bx0, by0, bx1, by1))), bx0, by0)
                                canvas.paste(0, (bx0, by0, bx1, by1))
                                if s is not None:
                                    out.stamp(s[0], s[1], s[2], skel_c)
                    for i, (x, y, c) in enumerate(np.asarray(k)[:, :3]):
                        if c > kpt_conf_threshold:
                            col = kpt_c[i] if i < len(kpt_c) else white
                            x, y = int(x), int(y)
                            out.stamp(x + ring[0], y + ring[1], ring[2], white, "ring")
                            out.stamp(x + disc[0], y + disc[1], disc[2], col, "disc")
            elif log is not None:
                log.append(f"   ⚠️  Face #{idx + 1}: NO keypoints attached!")
    prims = np.array(out.rows, "<i4").view(_lib.OVERLAY_PRIM_DTYPE)          # eight little-endian int32 per record (a coordinate past int32: OverflowError)
    masks = np.concatenate(out.masks) if out.masks else np.zeros(0, np.uint8)
    return prims, masks, found


# ---- device routes: the frame is decoded into device memory, drawn on or cropped there, and only files come back -----------------------------
# Each switch is set by measurement (tools/overlay_probe.py -> profiles/overlay_mi355x.json): a device route is taken by default only where its
# slowest sample beat the host route's fastest. DRAW_DEVICE_ROUTE False, or CROPS_DEVICE_ROUTE_MIN_CROPS None, forces the host route (the
# code of before, below); ROUTE_CALLS counts which route finished each call — the host routes are the only ones that bring the frame down.
DRAW_DEVICE_ROUTE = True
CROPS_DEVICE_ROUTE_MIN_CROPS = 1
# A file whose EXIF orientation is 2..8 (what phones write) keeps the device routes: the tag is read from the file's bytes (csrc/exif.hpp) and the
# frame is turned where it was decoded (csrc/orient.hip), so h and w below are the oriented frame's, the ones cv2.imread returns. False sends such
# files to the host routes, as before (tools/orient_probe.py -> profiles/orient_mi355x.json measures both).
ORIENT_DEVICE_ROUTE = True
ROUTE_CALLS = {"draw_device": 0, "draw_host": 0, "crops_device": 0, "crops_host": 0}


def _ext(path):
    return os.path.splitext(str(path))[1].lower()


def _frame_on_device(image_path, data=None):
    """(torch uint8 tensor holding the packed BGR frame, h, w, _lib), or None when the file is not one for this route: no device, not a .jpg /
    .jpeg / .png path, a PNG that is not 8-bit RGB, or any refusal of the decoder (progressive JPEG, ...). The frame is the one cv2.imread
    returns: a file with an EXIF orientation of 2..8 is turned on the device (h, w are the turned frame's), or is not one for this route when
    ORIENT_DEVICE_ROUTE is off. data: the file's bytes, when the caller has read them."""
    try:
        ext = _ext(image_path)
        if ext not in (".jpg", ".jpeg", ".png"):
            return None
        from ffp_amd import _lib
        if _lib.device_count() <= 0:
            return None
        import torch
        if data is None:
            with open(image_path, "rb") as fh:
                data = fh.read()
        o = _lib.exif_orientation(data)                             # 2..8: the orientations cv2.imread applies
        if o != 1 and not ORIENT_DEVICE_ROUTE:
            return None
        if ext == ".png":
            h, w, ch, depth = _lib.png_info(data)
            if ch != 3 or depth != 8 or _lib._png_has_trns(data):
                return None
        else:
            h, w, _ = _lib.jpeg_info(data)
        oh, ow = (w, h) if o >= 5 else (h, w)
        size = h * w * 3
        frame = torch.empty(size, dtype=torch.uint8, device=torch.device("cuda", 0))
        stored = frame if o == 1 or ext != ".png" else torch.empty(size, dtype=torch.uint8, device=torch.device("cuda", 0))
        torch.cuda.synchronize(0)
        if ext == ".png":
            _lib.png_decode_dev(data, stored.data_ptr(), w * 3, size, bgr=True)
            if o != 1:
                _lib.image_orient_dev(stored.data_ptr(), h, w, 3, w * 3, o, frame.data_ptr(), ow * 3, size)
        else:
            _lib.jpeg_decode_dev(data, frame.data_ptr(), ow * 3, size, bgr=True, orient=o if o != 1 else False)
        return frame, oh, ow, _lib
    except Exception:
        return None


def _draw_on_device(image_path, result, output_path, opts):
    """The device route of draw_detections: the file's bytes (and the lines to print) or None. Nothing is printed or written in here, so the host
    route can still do the whole call."""
    out_ext = _ext(output_path)
    if out_ext not in (".jpg", ".jpeg", ".png"):
        return None
    got = _frame_on_device(image_path)
    if got is None:
        return None
    frame, h, w, _lib = got
    try:
        log = []
        prims, masks, found = build_overlay_prims(result, w, h, *opts, log=log)
        _lib.overlay_draw_dev(frame.data_ptr(), h, w, w * 3, prims, masks)
        if out_ext == ".png":
            data = _lib.png_encode_dev(frame.data_ptr(), h, w, 3, 8, w * 3, 1, bgr=True)
        else:
            data = _lib.jpeg_encode_dev(frame.data_ptr(), h, w, w * 3, 95, bgr=True)
        return data, log, found
    except Exception:
        return None


def draw_detections(image_path, result, output_path, show_confidence=True, show_keypoints=True, box_color=(0, 255, 0), text_color=(0, 0, 0),
                    kpt_conf_threshold=0.3, draw_skeleton=False):
    """Boxes, "Face: 0.xx" labels and landmarks over the image at `image_path`, written to `output_path` (:78-148)."""
    if DRAW_DEVICE_ROUTE:
        done = _draw_on_device(image_path, result, output_path, (show_confidence, show_keypoints, box_color, text_color, kpt_conf_threshold, draw_skeleton))
        if done is not None:
            data, log, found = done
            n = len(result.object_prediction_list)
            print(f"   📊 Jumlah deteksi untuk visualisasi = {n}")
            for line in log:
                print(line)
            print(f"   📍 Total faces with keypoints: {found}/{n}")
            d = os.path.dirname(output_path)
            if d:
                os.makedirs(d, exist_ok=True)
            try:
                with open(output_path, "wb") as fh:
                    fh.write(data)
                print(f"   ✓ Hasil visualisasi disimpan ke: {output_path}")
            except Exception:
                print(f"   ❌ Gagal menyimpan visualisasi ke: {output_path}")
            ROUTE_CALLS["draw_device"] += 1
            return
    ROUTE_CALLS["draw_host"] += 1
    img = _imread_bgr(image_path)
    if img is None:
        print(f"❌ Error: Gagal membaca gambar dari {image_path}")
        return
    n = len(result.object_prediction_list)
    print(f"   📊 Jumlah deteksi untuk visualisasi = {n}")
    pil = Image.fromarray(np.ascontiguousarray(img[..., ::-1]))
    found = _render(pil, result, show_confidence, show_keypoints, box_color, text_color, kpt_conf_threshold, draw_skeleton, True)
    print(f"   📍 Total faces with keypoints: {found}/{n}")
    d = os.path.dirname(output_path)
    if d:
        os.makedirs(d, exist_ok=True)
    if _imwrite_bgr(output_path, np.asarray(pil)[..., ::-1]):
        print(f"   ✓ Hasil visualisasi disimpan ke: {output_path}")
    else:
        print(f"   ❌ Gagal menyimpan visualisasi ke: {output_path}")


def draw_detections_on_image(image, result, show_confidence=True, show_keypoints=True, box_color=(0, 255, 0), text_color=(255, 255, 255),
                             kpt_conf_threshold=0.3, draw_skeleton=False):
    """The same overlay on a BGR ndarray, returned as a new array (:151-183)."""
    pil = Image.fromarray(np.ascontiguousarray(image[..., ::-1]))
    _render(pil, result, show_confidence, show_keypoints, box_color, text_color, kpt_conf_threshold, draw_skeleton, False)
    return np.asarray(pil)[..., ::-1].copy()


def crop_boxes(result, width, height):
    """int box, clamped to the image; empty crops dropped. Returns [(index, x1, y1, x2, y2, score)] (:204-213)."""
    out = []
    for i, det in enumerate(result.object_prediction_list):
        x1, y1, x2, y2 = [int(c) for c in det.bbox.to_xyxy()]
        x1, y1, x2, y2 = max(0, x1), max(0, y1), min(width, x2), min(height, y2)
        if x2 > x1 and y2 > y1:
            out.append((i, x1, y1, x2, y2, det.score.value))
    return out


def _crops_on_device(image_path, result, min_crops):
    """The device route of save_face_crops: [(index, score, bytes of the crop's .jpg)] or None. The frame is decoded once into device memory and
    every crop is a view of it (offset y1*pitch + x1*3, the frame's pitch) for ONE ffp_jpeg_encode_batch_dev pass at quality 95."""
    try:
        ext = _ext(image_path)
        if ext not in (".jpg", ".jpeg", ".png"):
            return None
        from ffp_amd import _lib
        with open(image_path, "rb") as fh:
            data = fh.read()
        h, w = (_lib.png_info(data) if ext == ".png" else _lib.jpeg_info(data))[:2]          # the crop count decides the route: headers first
        if _lib.exif_orientation(data) >= 5:                       # the boxes are the oriented frame's
            h, w = w, h
        boxes = crop_boxes(result, w, h)
        if len(boxes) < min_crops:
            return None
        got = _frame_on_device(image_path, data)
        if got is None or (got[1], got[2]) != (h, w):
            return None
        frame, h, w, _lib = got
        pitch = w * 3
        blobs = _lib.jpeg_encode_batch_dev(frame.data_ptr(), [y1 * pitch + x1 * 3 for _, x1, y1, _, _, _ in boxes], [y2 - y1 for _, _, y1, _, y2, _ in boxes],
                                           [x2 - x1 for _, x1, _, x2, _, _ in boxes], 95, bgr=True, strides=[pitch] * len(boxes))
        return [(i, score, blob) for (i, _, _, _, _, score), blob in zip(boxes, blobs)]
    except Exception:
        return None


def save_face_crops(image_path, result, output_dir, prefix="face_crop"):
    if CROPS_DEVICE_ROUTE_MIN_CROPS is not None:
        crops = _crops_on_device(image_path, result, max(int(CROPS_DEVICE_ROUTE_MIN_CROPS), 1))
        if crops is not None:
            os.makedirs(output_dir, exist_ok=True)
            paths = []
            for i, score, blob in crops:
                p = os.path.join(output_dir, f"{prefix}_{i + 1}_conf_{score:.2f}.jpg")
                try:
                    with open(p, "wb") as fh:
                        fh.write(blob)
                except Exception:
                    pass                                   # as cv2.imwrite's False, which the loop below ignores too
                paths.append(p)
            ROUTE_CALLS["crops_device"] += 1
            return paths
    ROUTE_CALLS["crops_host"] += 1
    img = _imread_bgr(image_path)
    if img is None:
        print(f"Error: Gagal membaca gambar dari {image_path}")
        return []
    os.makedirs(output_dir, exist_ok=True)
    paths = []
    for i, x1, y1, x2, y2, score in crop_boxes(result, img.shape[1], img.shape[0]):
        p = os.path.join(output_dir, f"{prefix}_{i + 1}_conf_{score:.2f}.jpg")
        _imwrite_bgr(p, img[y1:y2, x1:x2])
        paths.append(p)
    return paths


def create_detection_summary(result, image_path, processing_time, output_path, img_width, img_height, slice_width, slice_height):
    """The run's text report, line for line in the reference's layout (:225-285) — other tooling of the reference parses it."""
    preds = result.object_prediction_list
    scores = [p.score.value for p in preds]
    mean = float(np.mean(scores)) if scores else 0
    lines = ["", "=== Ringkasan Deteksi Wajah dengan Keypoints ===", "", "--- Informasi Proses ---",
             f"Gambar Sumber: {os.path.basename(image_path)}", f"Ukuran Gambar Asli: {img_width}x{img_height} px",
             f"Ukuran Slice: {slice_width}x{slice_height} px", f"Waktu Proses Total: {processing_time:.2f} detik", "",
             "--- Statistik Deteksi ---", f"Total Wajah Ditemukan: {len(preds)}", f"Rata-rata Skor Kepercayaan: {mean:.3f}",
             f"Skor Kepercayaan Minimum: {(min(scores) if scores else 0):.3f}", f"Skor Kepercayaan Maksimum: {(max(scores) if scores else 0):.3f}", "",
             "--- Detail Deteksi ---"]
    text = "\n".join(lines) + "\n"
    if not preds:
        text += "Tidak ada wajah yang terdeteksi.\n"
    for i, det in enumerate(preds):
        x1, y1, x2, y2 = [int(c) for c in det.bbox.to_xyxy()]
        text += f"\nWajah #{i + 1}:\n  - Bounding Box: [x1: {x1}, y1: {y1}, x2: {x2}, y2: {y2}]\n  - Skor Kepercayaan: {det.score.value:.3f}\n"
        k = getattr(det, "keypoints", None)
        if k is not None:
            text += "  - Keypoints:\n"
            for j, name in enumerate(FACE_KEYPOINT_NAMES):
                if j < len(k):
                    x, y, c = k[j]
                    text += f"      {name}: ({x:.1f}, {y:.1f}) [conf: {c:.3f}]\n"
    os.makedirs(os.path.dirname(output_path), exist_ok=True)
    with open(output_path, "w", encoding="utf-8") as fh:
        fh.write(text)
    print(f"✓ Summary disimpan ke: {output_path}")

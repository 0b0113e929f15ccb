"""FaceEnhancer / RealESRGANer / RRDBNet with the reference's surface (utils/enhancer.py:21-478) over libffp.so.

`enhance_image` keeps the reference's error convention — it never raises and returns `(image, success)` (:189-235).
File I/O uses Pillow (cv2 is not a dependency of this build): BGR arrays in, BGR arrays out, JPEG quality honoured.
"""
from __future__ import annotations

import os
import time
from typing import NamedTuple

import numpy as np
from PIL import Image

import ffp_amd  # noqa: F401
from ffp_amd import _lib, synth, weights_io


class RRDBNet:
    """Architecture descriptor (basicsr.archs.rrdbnet_arch.RRDBNet signature); the network itself lives in libffp.so."""

    def __init__(self, num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
        if (num_in_ch, num_out_ch, num_feat, num_grow_ch) != (3, 3, 64, 32):
            raise ValueError("only RRDBNet(3, 3, num_feat=64, num_grow_ch=32) is built")
        self.scale, self.num_block = scale, num_block


class RealESRGANer:
    """realesrgan.RealESRGANer(scale, model_path, dni_weight, model, tile, tile_pad, pre_pad, half, gpu_id) -> .enhance()."""

    def __init__(self, scale, model_path, dni_weight=None, model=None, tile=0, tile_pad=10, pre_pad=0, half=False, device=None, gpu_id=None):
        self.scale, self.tile_size, self.tile_pad, self.pre_pad, self.half = scale, tile, tile_pad, pre_pad, half
        if model_path is None:
            raise AttributeError("'NoneType' object has no attribute 'startswith'")   # what realesrgan 0.3.0 does
        nb = model.num_block if model is not None else 23
        if isinstance(model_path, dict):
            W = model_path
        elif str(model_path).startswith("synthetic:"):
            W = synth.rrdbnet_weights(scale, nb)
        elif str(model_path).startswith("https://"):
            raise RuntimeError("weight download is not available offline; pass a local .pth / .ffpw")
        elif str(model_path).endswith(".ffpw"):
            W = weights_io.load(model_path)
        else:
            W = weights_io.load_esrgan_pth(model_path)
        self._sr = _lib.Enhancer(W, scale, nb, device=gpu_id or 0, half=bool(half))

    def enhance(self, img, outscale=None, alpha_upsampler="realesrgan"):
        """realesrgan 0.3.0 RealESRGANer.enhance: gray / BGR / BGRA, 8- or 16-bit, any outscale -> (image, mode)."""
        img = np.asarray(img)
        lay = enhance_layout(img.shape, img.dtype, img.max() if img.size and img.dtype in (np.uint8, np.uint16) else 0, self.scale, outscale,
                             alpha_upsampler)
        img = np.ascontiguousarray(img)
        if lay.fast_path:           # 3-channel uint8 at the net's scale: the path FaceEnhancer takes (utils/enhancer.py:214)
            return self._sr.enhance(img, self.tile_size, self.tile_pad, self.pre_pad), lay.mode
        return self._sr.enhance_ex(img, lay.max_range, lay.alpha_mode, lay.out_h, lay.out_w, self.tile_size, self.tile_pad, self.pre_pad), lay.mode


class EnhanceLayout(NamedTuple):
    mode: str                   # 'L', 'RGB' or 'RGBA'
    max_range: int              # 255 or 65535
    out_dtype: type             # np.uint8 or np.uint16
    out_h: int
    out_w: int
    resize: bool                # out size != scale * input size: a Lanczos4 resize of the result
    alpha_mode: int             # _lib.SR_ALPHA_REALESRGAN / SR_ALPHA_LINEAR (meaningful for 'RGBA')
    fast_path: bool             # 3-channel uint8 without a resize (Enhancer.enhance)


def enhance_layout(shape, dtype, img_max, scale, outscale=None, alpha_upsampler="realesrgan") -> EnhanceLayout:
    """What realesrgan 0.3.0's RealESRGANer.enhance(img, outscale, alpha_upsampler) makes of an input of this shape, dtype and
    maximum (reference call utils/enhancer.py:214). Raises ValueError for what this build does not enhance: other dtypes and
    shapes, an empty image or an outscale that gives an empty output, and a uint16 image with maximum exactly 256 under the
    'cv2' alpha upsampler (its alpha is 256/255 > 1, and realesrgan's uint8 cast of the result is then platform-defined)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.uint8, np.uint16):
        raise ValueError(f"RealESRGANer.enhance takes uint8 or uint16 images, got {dtype}")
    if len(shape) == 2:
        mode = "L"
    elif len(shape) == 3 and shape[2] == 4:
        mode = "RGBA"
    elif len(shape) == 3 and shape[2] == 3:
        mode = "RGB"
    else:
        raise ValueError(f"RealESRGANer.enhance takes HxW, HxWx3 or HxWx4 images, got shape {tuple(shape)}")
    h, w = int(shape[0]), int(shape[1])
    if h < 1 or w < 1:
        raise ValueError(f"empty image {tuple(shape)}")
    max_range = 65535 if float(img_max) > 256 else 255
    alpha_mode = _lib.SR_ALPHA_REALESRGAN if alpha_upsampler == "realesrgan" else _lib.SR_ALPHA_LINEAR
    if mode == "RGBA" and alpha_mode == _lib.SR_ALPHA_LINEAR and dtype == np.uint16 and float(img_max) == 256:
        raise ValueError("uint16 image with maximum 256 and alpha_upsampler 'cv2': realesrgan's result is platform-defined")
    out_h, out_w = h * scale, w * scale
    if outscale is not None and float(outscale) != float(scale):
        out_h, out_w = int(h * outscale), int(w * outscale)
        if out_h < 1 or out_w < 1:
            raise ValueError(f"outscale {outscale} gives an empty {out_w}x{out_h} output for a {w}x{h} image")
    resize = (out_h, out_w) != (h * scale, w * scale)
    return EnhanceLayout(mode, max_range, np.uint16 if max_range == 65535 else np.uint8, out_h, out_w, resize, alpha_mode,
                         mode == "RGB" and dtype == np.uint8 and not resize)


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


class FaceEnhancer:
    def __init__(self, model_name="RealESRGAN_x4plus", model_path=None, scale=4, tile=400, half=True):
        self.model_name, self.scale, self.tile, self.half, self.upsampler = model_name, scale, tile, half, None
        self.device = self._check_device()
        print(f"Using device: {self.device}")
        try:
            self._setup_model(model_name, model_path)
        except Exception as e:
            print(f" Failed to setup model: {e}")
            raise

    def _check_device(self):
        if _lib.device_count() > 0:
            return "cuda"
        return "cpu"

    def _find_model_path(self, model_name):
        for p in (f"models/{model_name}.pth", f"./models/{model_name}.pth", f"../models/{model_name}.pth", f"weights/{model_name}.pth",
                  f"./weights/{model_name}.pth", f"{model_name}.pth", f"./{model_name}.pth"):
            if os.path.exists(p):
                return os.path.abspath(p)
        return None

    def _setup_model(self, model_name, model_path):
        if self.device == "cpu":
            raise RuntimeError("no MI355X visible: this build has no CPU enhancement path")
        if model_path is None:
            model_path = self._find_model_path(model_name)
        if "anime_6B" in model_name:
            model = RRDBNet(3, 3, num_feat=64, num_block=6, num_grow_ch=32, scale=self.scale)
        elif "x2" in model_name:
            model = RRDBNet(3, 3, num_feat=64, num_block=23, num_grow_ch=32, scale=2)
            self.scale = 2                                           # reference quirk kept (utils/enhancer.py:109-119)
        else:
            model = RRDBNet(3, 3, num_feat=64, num_block=23, num_grow_ch=32, scale=self.scale)
        self.upsampler = RealESRGANer(scale=self.scale, model_path=model_path, dni_weight=None, model=model, tile=self.tile, tile_pad=10,
                                      pre_pad=0, half=self.half, gpu_id=0)

    def enhance_image(self, image):
        if self.upsampler is None:
            return image, False
        try:
            if isinstance(image, Image.Image):
                image = np.asarray(image.convert("RGB"))[..., ::-1].copy()
            if image is None or image.size == 0:
                return image, False
            h, w = image.shape[:2]
            if h < 4 or w < 4:
                print(f" Image too small ({w}x{h}), skipping enhancement")
                return image, False
            out, _ = self.upsampler.enhance(image, outscale=self.scale)
            return out, True
        except Exception as e:
            print(f" Enhancement failed: {type(e).__name__}: {e}")
            return image, False

    def enhance_images(self, images):
        """Extension (not in the reference): enhance_image over a list as ONE ragged GPU batch -> [(image, ok)], the same bytes as len(images)
        calls of enhance_image (a crop's result does not depend on its batch: tests/test_gpu_sr_crops.py). enhance_face_crops_batch uses it."""
        out = [(im, False) for im in images]
        if self.upsampler is None or not hasattr(self.upsampler, "_sr"):
            return [self.enhance_image(im) for im in images]
        good = []
        for k, im in enumerate(images):
            if isinstance(im, Image.Image):
                im = np.asarray(im.convert("RGB"))[..., ::-1].copy()
            if im is None or im.size == 0 or im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape[0] < 4 or im.shape[1] < 4:
                if im is not None and im.size and im.ndim == 3 and (im.shape[0] < 4 or im.shape[1] < 4):
                    print(f" Image too small ({im.shape[1]}x{im.shape[0]}), skipping enhancement")
                continue
            if max(im.shape[0], im.shape[1]) > self.tile > 0:          # larger than one tile: the tiled single-image path
                out[k] = self.enhance_image(im)
                continue
            good.append((k, np.ascontiguousarray(im)))
        if good:
            try:
                res = self.upsampler._sr.enhance_batch([im for _, im in good])
                for (k, _), r in zip(good, res):
                    out[k] = (r, True)
            except Exception as e:
                print(f" Enhancement failed: {type(e).__name__}: {e}")
                for k, im in good:
                    out[k] = self.enhance_image(im)
        return out

    def enhance_face_crop(self, crop_path, output_path, quality=95):
        info = {"original_path": crop_path, "output_path": output_path, "original_size": None, "enhanced_size": None,
                "scale_factor": self.scale, "success": False}
        try:
            if not os.path.exists(crop_path):
                return False, info
            img = _imread_bgr(crop_path)
            if img is None:
                return False, info
            info["original_size"] = (img.shape[1], img.shape[0])
            out, ok = self.enhance_image(img)
            if not ok:
                return False, info
            info["enhanced_size"] = (out.shape[1], out.shape[0])
            os.makedirs(os.path.dirname(output_path) or ".", exist_ok=True)
            if not _imwrite_bgr(output_path, out, quality):
                return False, info
            info["success"] = True
            return True, info
        except Exception as e:
            print(f" Error enhancing {os.path.basename(crop_path)}: {e}")
            return False, info

    def get_model_info(self):
        return {"model_name": self.model_name, "scale": self.scale, "tile": self.tile, "half_precision": self.half, "device": self.device,
                "is_loaded": self.upsampler is not None, "backend": f"libffp {_lib.lib().ffp_version()}", "cuda_available": self.device == "cuda"}


# The crops directory from file to file on the device (decode batch -> SR on the atlas -> encode batch) is taken from this many JPEG crops
# on. Set by measurement (tools/jpeg_batch_probe.py -> profiles/jpeg_decode_batch_mi355x.json, "crops_dir"): the smallest measured count at
# which the new route's slowest sample is below the per-file-read route's fastest (4 files: the directory in 4.9..6.1 ms against 9.1..10.2 ms,
# the decode alone in 0.61..0.76 ms against 2.2..2.4 ms; one file is a tie in the decode, 0.57..0.62 ms against 0.56..0.61 ms). None would mean
# that no such count was measured, and keep the old route.
BATCH_ROUTE_MIN_FILES = 4
ATLAS_MAX_WIDTH = 2048


def pack_atlas(sizes, max_width):
    """Shelf packing of images [(h, w), ...] in their order: -> (H, W, [(x, y), ...]). An image goes behind its predecessor on the current
    shelf while it fits into max_width, else it opens a new shelf below; an image wider than max_width gets a shelf of its own (and W
    grows to it). Deterministic, no overlap, everything inside H x W."""
    pos, x, y, shelf_h, W = [], 0, 0, 0, 0
    for h, w in sizes:
        h, w = int(h), int(w)
        if x > 0 and x + w > max_width:
            y += shelf_h
            x, shelf_h = 0, 0
        pos.append((x, y))
        x += w
        shelf_h = max(shelf_h, h)
        W = max(W, x)
    return y + shelf_h, W, pos


def _crops_dir_on_device(crops_dir, files, enhancer):
    """The batch route of enhance_face_crops_batch: {file name: ((w, h), (W, H), bytes of the enhanced .jpg)} for the JPEG crops it
    could take — read once, decoded in ONE pass into a BGR atlas in device memory (ffp_jpeg_decode_batch_dev), enhanced there
    (ffp_sr_enhance_crops_dev with the enhancer's tile), encoded in ONE pass (ffp_jpeg_encode_batch_dev, quality 95). Only the files go up
    and only the enhanced files come down. Every other file, and every failure, is left to the per-file loop."""
    import torch
    sr = enhancer.upsampler._sr
    if enhancer.scale != sr.scale or enhancer.upsampler.scale != sr.scale:      # a resize behind the net: the per-file path knows how
        return {}
    names, datas, sizes = [], [], []
    for f in files:
        if not f.lower().endswith((".jpg", ".jpeg")):
            continue
        try:
            with open(os.path.join(crops_dir, f), "rb") as fh:
                data = fh.read()
            h, w, _ = _lib.jpeg_info(data)
        except Exception:
            continue
        if h < 4 or w < 4:
            continue
        names.append(f); datas.append(data); sizes.append((h, w))
    if not names:
        return {}
    H, W, pos = pack_atlas(sizes, ATLAS_MAX_WIDTH)
    pitch = W * 3
    dev = torch.device("cuda", sr.device)
    atlas = torch.zeros(H * pitch, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hs, ws, status = _lib.jpeg_decode_batch_dev(datas, atlas.data_ptr(), [y * pitch + x * 3 for x, y in pos], [pitch] * len(names), H * pitch,
                                                bgr=True, device=sr.device)
    keep = [i for i in range(len(names)) if status[i] >= 0 and (int(hs[i]), int(ws[i])) == sizes[i]]
    if not keep:
        return {}
    s = sr.scale
    boxes = np.asarray([[pos[i][0], pos[i][1], pos[i][0] + sizes[i][1], pos[i][1] + sizes[i][0]] for i in keep], np.int32)
    cap = int(sum((sizes[i][0] * s * sizes[i][1] * s * 3 + 15) // 16 * 16 for i in keep))
    out = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    offs = sr.enhance_crops_dev([atlas.data_ptr()], H, W, boxes, out.data_ptr(), cap, None, enhancer.tile, 10, True)
    blobs = _lib.jpeg_encode_batch_dev(out.data_ptr(), offs[:len(keep)], [sizes[i][0] * s for i in keep], [sizes[i][1] * s for i in keep], 95, bgr=True,
                                       device=sr.device)
    return {names[i]: ((sizes[i][1], sizes[i][0]), (sizes[i][1] * s, sizes[i][0] * s), blob) for i, blob in zip(keep, blobs)}


def enhance_face_crops_batch(crops_dir, enhancer, prefix="enhanced", progress_callback=None):
    results = {"enhanced_files": [], "failed_files": [], "enhancement_info": [],
               "statistics": {"total_files": 0, "successful": 0, "failed": 0, "total_time": 0}}
    if not os.path.exists(crops_dir):
        return results
    out_dir = os.path.join(os.path.dirname(crops_dir), f"{prefix}_enhanced")
    os.makedirs(out_dir, exist_ok=True)
    files = [f for f in os.listdir(crops_dir) if f.lower().endswith((".png", ".jpg", ".jpeg", ".bmp", ".tiff"))]
    results["statistics"]["total_files"] = len(files)
    t0 = time.time()
    batched, on_device = {}, {}
    n_jpeg = sum(1 for f in files if f.lower().endswith((".jpg", ".jpeg")))
    if type(enhancer) is FaceEnhancer and enhancer.upsampler is not None and BATCH_ROUTE_MIN_FILES is not None and n_jpeg >= BATCH_ROUTE_MIN_FILES:
        try:
            on_device = _crops_dir_on_device(crops_dir, files, enhancer)
        except Exception:
            on_device = {}
    rest = [f for f in files if f not in on_device]
    if type(enhancer) is FaceEnhancer and len(rest) > 1:
        # every readable crop through ONE ragged GPU batch (same bytes as the per-file loop below, which still runs for whatever the batch
        # could not take: unreadable files, failures, an enhancer subclass with its own enhance_face_crop)
        try:
            imgs = [(f, _imread_bgr(os.path.join(crops_dir, f))) for f in rest]
            outs = enhancer.enhance_images([im for _, im in imgs if im is not None])
            it = iter(outs)
            for f, im in imgs:
                if im is not None:
                    o, ok = next(it)
                    if ok:
                        batched[f] = (im, o)
        except Exception:
            batched = {}
    for i, f in enumerate(files, 1):
        name, ext = os.path.splitext(f)
        dst = os.path.join(out_dir, f"{prefix}_{name}{ext}")
        if progress_callback:
            try:
                progress_callback(i, len(files), f)
            except Exception:
                pass
        ok, info = False, None
        if f in on_device:
            (ow, oh), (ew, eh), blob = on_device[f]
            info = {"original_path": os.path.join(crops_dir, f), "output_path": dst, "original_size": (ow, oh), "enhanced_size": (ew, eh),
                    "scale_factor": enhancer.scale, "success": False}
            try:
                os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
                with open(dst, "wb") as fh:
                    fh.write(blob)
                ok = info["success"] = True
            except Exception:
                ok = False
        elif f in batched:
            im, o = batched[f]
            info = {"original_path": os.path.join(crops_dir, f), "output_path": dst, "original_size": (im.shape[1], im.shape[0]),
                    "enhanced_size": (o.shape[1], o.shape[0]), "scale_factor": enhancer.scale, "success": False}
            try:
                os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
                ok = bool(_imwrite_bgr(dst, o, 95))
                info["success"] = ok
            except Exception:
                ok = False
        for _attempt in range(0 if ok else 2):                       # reference retries once (utils/enhancer.py:362-377)
            try:
                ok, info = enhancer.enhance_face_crop(os.path.join(crops_dir, f), dst)
                if ok:
                    break
            except Exception:
                ok = False
        if ok and info:
            results["enhanced_files"].append(dst)
            results["enhancement_info"].append(info)
            results["statistics"]["successful"] += 1
        else:
            results["failed_files"].append(os.path.join(crops_dir, f))
            results["statistics"]["failed"] += 1
    results["statistics"]["total_time"] = time.time() - t0
    return results


def create_enhancement_summary(results, output_path):
    """The batch report in the reference's text layout (utils/enhancer.py:409-452), line for line (pinned by tests/golden/wrapper_expected.json)."""
    import datetime
    st = results["statistics"]
    n = max(st["total_files"], 1)
    lines = ["", "=== LAPORAN ENHANCEMENT WAJAH ===", f"Generated: {datetime.datetime.now().strftime('%Y-%m-%d %H:%M:%S')}", "",
             "--- RINGKASAN STATISTIK ---", f"Total File Diproses: {st['total_files']}", f" Berhasil: {st['successful']}", f" Gagal: {st['failed']}",
             f" Tingkat Keberhasilan: {(st['successful'] / n * 100):.1f}%", f" Waktu Total: {st['total_time']:.2f} detik",
             f" Waktu Rata-rata per File: {(st['total_time'] / n):.2f} detik", "", "--- DETAIL FILE BERHASIL ---"]
    text = "\n".join(lines) + "\n"
    for i, info in enumerate(results["enhancement_info"], 1):
        o, e = info["original_size"], info["enhanced_size"]
        text += (f"\nFile #{i}: {os.path.basename(info['original_path'])}\n   Ukuran Asli: {o[0]}x{o[1]} px\n   Ukuran Enhanced: {e[0]}x{e[1]} px\n"
                 f"   Scale Factor: {info['scale_factor']}x\n   Output: {os.path.basename(info['output_path'])}\n")
    if results["failed_files"]:
        text += f"\n--- FILE GAGAL ({len(results['failed_files'])}) ---\n"
        for i, f in enumerate(results["failed_files"], 1):
            text += f"{i}. {os.path.basename(f)}\n"
    try:
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        with open(output_path, "w", encoding="utf-8") as fh:
            fh.write(text)
        print(f" Enhancement summary saved to: {os.path.basename(output_path)}")
    except Exception as e:
        print(f" Error saving enhancement summary: {e}")


def get_available_models():
    """The reference's model table (utils/enhancer.py:454-480) plus `num_block`, which this build needs to lay the network out."""
    return {
        "RealESRGAN_x4plus": {"description": "Model utama untuk gambar natural (4x)", "scale": 4, "best_for": "Foto natural, potret, wajah", "file_size": "~65MB",
                              "recommended_tile": 400, "num_block": 23},
        "RealESRGAN_x2plus": {"description": "Model untuk enhancement 2x (lebih cepat)", "scale": 2, "best_for": "Enhancement ringan, GPU terbatas", "file_size": "~65MB",
                              "recommended_tile": 600, "num_block": 23},
        "RealESRGAN_x4plus_anime_6B": {"description": "Model khusus untuk anime/kartun (4x)", "scale": 4, "best_for": "Gambar anime, kartun, ilustrasi", "file_size": "~18MB",
                                       "recommended_tile": 400, "num_block": 6},
    }

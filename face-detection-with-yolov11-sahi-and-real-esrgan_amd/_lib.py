"""ctypes binding of libffp.so (include/ffp.h) + thin numpy-facing handles.

The library is the product: if it is missing or cannot be loaded every entry point raises — there is no Python or
PyTorch fallback for any operator.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi, weights_io

_HERE = os.path.dirname(os.path.abspath(__file__))
# FFP_LIB=<path> loads a DIAGNOSTIC build instead (build.build_variant: in-kernel stamps, phase-skip instantiations). Probe scripts set it;
# the shipped libffp.so is never overwritten. Nothing else changes: same symbols, same checks, it is still the only implementation.
LIB_PATH = os.environ.get("FFP_LIB") or os.path.join(_HERE, "libffp.so")

PREC_F32, PREC_F16, PREC_F32X3 = 0, 1, 2
SR_ALPHA_REALESRGAN, SR_ALPHA_LINEAR = 0, 1          # ffp_sr_enhance_ex alpha_mode (include/ffp.h)
CHAN_AS_BGR, CHAN_AS_RGB = 0, 1
IQA_F32_CHW, IQA_U8_HWC = 0, 1                       # ffp_iqa_niqe_features layout
NIQE_FEATURES = 36
PP_NMS, PP_GREEDYNMM = 0, 1
METRIC_IOU, METRIC_IOS = 0, 1
PP_TYPES = {"NMS": PP_NMS, "GREEDYNMM": PP_GREEDYNMM}
METRICS = {"IOU": METRIC_IOU, "IOS": METRIC_IOS}

_lib = None


class FfpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libffp error {code}: {msg}")
        self.code = code


def _p(t):
    return C.POINTER(t)


HEADER_PATH = os.path.join(_HERE, "..", "include", "ffp.h")


def _load_sigs() -> dict:
    """{name: (restype, [argtypes])} of every entry include/ffp.h declares (_abi.parse): the header is the only declaration."""
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes signatures of libffp.so are read from it, so it travels with the package.")
    with open(HEADER_PATH, encoding="utf-8") as f:
        return _abi.parse(f.read())


_SIGS = _load_sigs()
EXPORTED_SYMBOLS = tuple(_SIGS)


def lib() -> C.CDLL:
    """Load libffp.so (in-tree). Raises if it has not been built — the product has no other implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m ffp_amd.build` "
                               "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback.")
        # ONE HIP runtime per process. libffp.so needs `libamdhip64.so.7` and the PyTorch-ROCm wheel bundles a library with
        # that very SONAME (torch/lib/libamdhip64.so, with its own libhsa-runtime64 / librccl next to it): the dynamic loader
        # binds every later user to whichever copy was mapped first. If the system copy (/opt/rocm) came first, a later
        # `import torch` would run the wheel's libraries on a runtime they were not built with (observed: "No HIP GPUs are
        # available"). So when a torch wheel is installed its copy is mapped first — whether or not torch has been imported —
        # and libffp.so, torch and RCCL then share one runtime, one set of device contexts and one allocator view
        # (tests/test_host_logic.py::test_single_hip_runtime checks both load orders).
        if "torch" not in sys.modules:
            try:
                import importlib.util
                spec = importlib.util.find_spec("torch")
                cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else None
                if cand and os.path.exists(cand):
                    C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except Exception:
                pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def _check(rc: int):
    if rc != 0:
        raise FfpError(rc, lib().ffp_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    n = C.c_int(0)
    _check(lib().ffp_device_count(C.byref(n)))
    return n.value


def switches() -> dict:
    """The library's environment switches as this process reads them (csrc/switches.hpp), by name:
    {"value", "source" ("env" | "default"), "when" ("once" | "live"), "accepts", "effect"}. Needs no device.
    FfpError(FFP_ERR_ARG) names the variable whose value its rule refuses."""
    buf = C.create_string_buffer(1 << 16)
    _check(lib().ffp_switches(buf, len(buf)))
    out = {}
    for line in buf.value.decode("utf-8").splitlines():
        head, source, when, accepts, effect = line.split("\t")
        name, value = head.split("=", 1)
        out[name] = {"value": value, "source": source, "when": when, "accepts": accepts, "effect": effect}
    return out


def _ptr_to(ctype):
    """array -> POINTER(ctype) at its first element; None stays None (a NULL argument)."""
    return lambda a: None if a is None else a.ctypes.data_as(_p(ctype))


_fp, _ip, _up, _u8p, _i64p = (_ptr_to(t) for t in (C.c_float, C.c_int32, C.c_uint32, C.c_uint8, C.c_int64))


def slice_bboxes(H: int, W: int, slice_h: int, slice_w: int, overlap_h: float = 0.2, overlap_w: float = 0.2) -> np.ndarray:
    n = C.c_int32(0)
    _check(lib().ffp_slice_bboxes(H, W, slice_h, slice_w, overlap_h, overlap_w, None, 0, C.byref(n)))
    out = np.zeros((n.value, 4), np.int32)
    _check(lib().ffp_slice_bboxes(H, W, slice_h, slice_w, overlap_h, overlap_w, _ip(out), n.value, C.byref(n)))
    return out


def tile_chunks(n: int, max_batch: int) -> List[int]:
    """The sizes of the network batches n tiles run in at a positive max_batch (ffp_tile_chunks)."""
    out, k = np.zeros(max(n, 1), np.int32), C.c_int32(0)               # never more chunks than items
    _check(lib().ffp_tile_chunks(n, max_batch, _ip(out), len(out), C.byref(k)))
    return out[:k.value].tolist()


def _as_tiles(tiles) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(tiles, np.int32).reshape(-1, 4))


def letterbox_geometry(h: int, w: int, imgsz: int) -> Tuple[int, int, int, int, int, int]:
    out = np.zeros(6, np.int32)
    _check(lib().ffp_letterbox_geometry(h, w, imgsz, _ip(out)))
    return tuple(int(v) for v in out)


def _weights_bytes(weights) -> bytes:
    if isinstance(weights, (bytes, bytearray, memoryview)):
        return bytes(weights)
    if isinstance(weights, str):
        with open(weights, "rb") as f:
            return f.read()
    return weights_io.pack(weights)


def _as_frame(frame: np.ndarray) -> np.ndarray:
    f = np.ascontiguousarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"expected an HxWx3 uint8 array, got {f.dtype} {f.shape}")
    return f


def scrfd_describe(onnx_bytes: bytes, n: int = 1, det_w: int = 640, det_h: int = 640) -> str:
    """The lowered step list of an SCRFD ONNX file (host only, no device). Raises FfpError with the refusal message."""
    buf = C.create_string_buffer(bytes(onnx_bytes), len(onnx_bytes))
    out = C.create_string_buffer(1 << 20)
    _check(lib().ffp_scrfd_describe(buf, len(onnx_bytes), n, det_w, det_h, out, len(out)))
    return out.value.decode()


def scrfd_geometry(h: int, w: int, net_w: int, net_h: int) -> Tuple[int, int, float]:
    """RetinaFace.detect's (new_w, new_h, det_scale) of an h x w crop at net size net_w x net_h (host only)."""
    o = np.zeros(2, np.int32)
    s = C.c_float(0)
    _check(lib().ffp_scrfd_geometry(h, w, net_w, net_h, _ip(o), C.byref(s)))
    return int(o[0]), int(o[1]), float(s.value)


class _Handle:
    """Owner of one library handle (self._h, a c_void_p): close() destroys it once, through the entry the subclass names in _DESTROY."""

    _DESTROY = ""

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib(), self._DESTROY)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FaceDetector(_Handle):
    """InsightFace's SCRFD face detector (an ONNX file of a model pack, e.g. buffalo_l/det_10g.onnx) on one GPU (ffp_scrfd_*)."""

    _DESTROY = "ffp_scrfd_destroy"

    STRIDE = 21          # FFP_DET_STRIDE(5)

    def __init__(self, onnx, device: int = 0, precision: int = PREC_F32, n: int = 1):
        buf = _weights_bytes(onnx) if not isinstance(onnx, dict) else None
        if buf is None:
            raise TypeError("FaceDetector takes the ONNX file's bytes or its path")
        self._h = C.c_void_p()
        self.device, self.precision = device, precision
        cbuf = C.create_string_buffer(buf, len(buf))
        _check(lib().ffp_scrfd_create(cbuf, len(buf), n, device, precision, C.byref(self._h)))
        n_out = C.c_int32(0)
        _check(lib().ffp_scrfd_info(self._h, C.byref(n_out), None))
        self.n_outputs = int(n_out.value)

    def last_conv_flops(self) -> float:
        f = C.c_double(0)
        _check(lib().ffp_scrfd_info(self._h, None, C.byref(f)))
        return float(f.value)

    TILE_MODES = {"local": 0, "sahi": 1}         # FFP_SCRFD_TILES_LOCAL, FFP_SCRFD_TILES_SAHI

    def infer_tiles(self, frame: np.ndarray, tiles: Sequence[Sequence[int]], det_size=(640, 640), det_thresh: float = 0.5,
                    nms_thresh: float = 0.4, chan_order: int = CHAN_AS_BGR, cap: int = 1024, *, conf: Optional[float] = None, mode: str = "local",
                    max_batch: int = 0) -> List[np.ndarray]:
        """-> per tile (n_i, 21) float32 rows [x1,y1,x2,y2,score,0, 5 x (x,y,1)] in tile-local pixels (not truncated).
        mode "sahi" (ffp_scrfd_infer_tiles_ex): rows with score < conf (default det_thresh) skipped, boxes int-truncated, clipped against the
        frame and shifted to frame pixels with their keypoints; a box whose far corner is negative raises FfpError, as the reference raises.
        max_batch: items per network batch (0: all tiles in one; < 0: FFP_SCRFD_TILES_DEFAULT_BATCH)."""
        f = _as_frame(frame)
        t = _as_tiles(tiles)
        n = t.shape[0]
        plain = conf is None and mode == "local" and max_batch == 0
        while True:
            dets = np.zeros((max(n, 1), cap, self.STRIDE), np.float32)
            counts = np.zeros(max(n, 1), np.int32)
            if plain:
                rc = lib().ffp_scrfd_infer_tiles(self._h, f.ctypes.data, f.shape[0], f.shape[1], chan_order, _ip(t), n, int(det_size[0]),
                                                 int(det_size[1]), det_thresh, nms_thresh, _fp(dets), cap, _ip(counts))
            else:
                rc = lib().ffp_scrfd_infer_tiles_ex(self._h, f.ctypes.data, f.shape[0], f.shape[1], chan_order, _ip(t), n, int(det_size[0]),
                                                    int(det_size[1]), det_thresh, nms_thresh, det_thresh if conf is None else conf,
                                                    self.TILE_MODES[mode], max_batch, _fp(dets), cap, _ip(counts))
            if rc != 0 and int(counts.max(initial=0)) > cap:
                cap = int(counts.max())                # out_counts are not capped: retry once with room for every face
                continue
            _check(rc)
            return [dets[i, :counts[i]].copy() for i in range(n)]

    def infer_tiles_dev(self, d_frame: int, H: int, W: int, tiles: Sequence[Sequence[int]], d_out: int, cap: int, d_counts: int, det_size=(640, 640),
                        det_thresh: float = 0.5, nms_thresh: float = 0.4, chan_order: int = CHAN_AS_BGR, conf: Optional[float] = None,
                        mode: str = "local", max_batch: int = 0):
        """infer_tiles with the frame (H x W x 3 uint8), d_out [n][cap][21] float32 and d_counts [n] int32 given as device pointers
        (ffp_scrfd_infer_tiles_dev). Returns after the engine's stream has drained."""
        t = _as_tiles(tiles)
        _check(lib().ffp_scrfd_infer_tiles_dev(self._h, d_frame, H, W, chan_order, _ip(t), t.shape[0], int(det_size[0]), int(det_size[1]), det_thresh,
                                               nms_thresh, det_thresh if conf is None else conf, self.TILE_MODES[mode], max_batch, d_out, cap,
                                               d_counts))

    def _sliced_args(self, H, W, slice_h, slice_w, overlap_h, overlap_w, perform_standard_pred, det_size, det_thresh, nms_thresh, conf, max_batch,
                     tile_cap, pp_type, pp_metric, pp_thr, class_agnostic, chan_order):
        return (H, W, chan_order, slice_h, slice_w, overlap_h, overlap_w, int(perform_standard_pred), int(det_size[0]), int(det_size[1]), det_thresh,
                nms_thresh, det_thresh if conf is None else conf, max_batch, tile_cap, PP_TYPES[pp_type], METRICS[pp_metric], float(pp_thr),
                int(class_agnostic))

    def sliced_predict(self, frame: np.ndarray, slice_h: int, slice_w: int, overlap_h: float = 0.2, overlap_w: float = 0.2,
                       perform_standard_pred: bool = True, det_size=(640, 640), det_thresh: float = 0.5, nms_thresh: float = 0.4,
                       conf: Optional[float] = None, pp_type: str = "GREEDYNMM", pp_metric: str = "IOS", pp_thr: float = 0.5,
                       class_agnostic: bool = False, chan_order: int = CHAN_AS_BGR, max_batch: int = -1, tile_cap: int = 1024, cap: int = 4096) -> np.ndarray:
        """Fused get_sliced_prediction over InsightFaceDetectionModel (ffp_scrfd_sliced_predict) -> (k, 21) float32 rows in frame pixels: integer
        boxes stored as floats, score, 0, and the keypoints of the higher-scored source row. conf: the wrapper's confidence_threshold (default
        det_thresh). max_batch: items per network batch (0: all in one; < 0: FFP_SCRFD_TILES_DEFAULT_BATCH)."""
        f = _as_frame(frame)
        H, W = f.shape[:2]
        out = np.zeros((cap, self.STRIDE), np.float32)
        n = C.c_int32(0)
        _check(lib().ffp_scrfd_sliced_predict(self._h, f.ctypes.data, *self._sliced_args(H, W, slice_h, slice_w, overlap_h, overlap_w, perform_standard_pred,
                                                                                         det_size, det_thresh, nms_thresh, conf, max_batch, tile_cap, pp_type,
                                                                                         pp_metric, pp_thr, class_agnostic, chan_order),
                                              _fp(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def sliced_predict_dev(self, d_frame: int, H: int, W: int, d_out: int, cap: int, d_out_n: int, slice_h: int, slice_w: int, overlap_h: float = 0.2,
                           overlap_w: float = 0.2, perform_standard_pred: bool = True, det_size=(640, 640), det_thresh: float = 0.5,
                           nms_thresh: float = 0.4, conf: Optional[float] = None, pp_type: str = "GREEDYNMM", pp_metric: str = "IOS", pp_thr: float = 0.5,
                           class_agnostic: bool = False, chan_order: int = CHAN_AS_BGR, max_batch: int = -1, tile_cap: int = 1024):
        """sliced_predict with the frame, d_out [cap][21] float32 and d_out_n [1] int32 given as device pointers (ffp_scrfd_sliced_predict_dev).
        *d_out_n is the untruncated merged count: above cap the result has overflowed (the rule of ffp_merge_dev)."""
        _check(lib().ffp_scrfd_sliced_predict_dev(self._h, d_frame, *self._sliced_args(H, W, slice_h, slice_w, overlap_h, overlap_w, perform_standard_pred,
                                                                                       det_size, det_thresh, nms_thresh, conf, max_batch, tile_cap, pp_type,
                                                                                       pp_metric, pp_thr, class_agnostic, chan_order),
                                                  d_out, cap, d_out_n))

    def mem_bytes(self) -> dict:
        """Device bytes held by the resident plans, and how many plans are resident."""
        b, n = C.c_uint64(0), C.c_int32(0)
        _check(lib().ffp_scrfd_mem_bytes(self._h, C.byref(b), C.byref(n)))
        return {"plans": int(b.value), "plans_resident": int(n.value)}

    def drop_plans(self):
        _check(lib().ffp_scrfd_drop_plans(self._h))

    def forward_raw(self, frame: np.ndarray, tiles: Sequence[Sequence[int]], det_size=(640, 640),
                    chan_order: int = CHAN_AS_BGR) -> List[List[np.ndarray]]:
        """-> per tile the graph outputs in file order, each (anchors, values) float32 (scores after the sigmoid)."""
        f = _as_frame(frame)
        t = _as_tiles(tiles)
        n = t.shape[0]
        W, H = int(det_size[0]), int(det_size[1])
        per = sum((H // s) * (W // s) * 2 * v for s in (8, 16, 32) for v in (1, 4, 10))
        out = np.zeros(per * n, np.float32)
        sizes = np.zeros(self.n_outputs, np.int64)
        _check(lib().ffp_scrfd_forward_raw(self._h, f.ctypes.data, f.shape[0], f.shape[1], chan_order, _ip(t), n, W, H, _fp(out), out.size,
                                           sizes.ctypes.data_as(_p(C.c_int64))))
        res, o = [], 0
        widths = [1] * 3 + [4] * 3 + [10] * 3
        for i in range(n):
            outs = []
            for k in range(self.n_outputs):
                m = int(sizes[k])
                outs.append(out[o:o + m].reshape(-1, widths[k]).copy())
                o += m
            res.append(outs)
        return res


class RTDETRDetector(_Handle):
    """Ultralytics RT-DETR-l (rtdetr-l.yaml) on one GPU (ffp_rtdetr_*): FFPW weights from weights_io.from_ultralytics_rtdetr_state_dict
    (or synth.rtdetr_l_weights), a path to them, or the tensors as a dict."""

    _DESTROY = "ffp_rtdetr_destroy"

    NQ = 300

    def __init__(self, weights, device: int = 0, precision: int = PREC_F32):
        buf = _weights_bytes(weights)
        self._h = C.c_void_p()
        self.device, self.precision = device, precision
        cbuf = C.create_string_buffer(buf, len(buf))
        _check(lib().ffp_rtdetr_create(cbuf, len(buf), device, precision, C.byref(self._h)))
        nc = C.c_int32(0)
        _check(lib().ffp_rtdetr_info(self._h, C.byref(nc), None, None))
        self.nc = int(nc.value)

    def info(self) -> dict:
        f, g = C.c_double(0), C.c_int32(0)
        _check(lib().ffp_rtdetr_info(self._h, None, C.byref(f), C.byref(g)))
        return {"nc": self.nc, "conv_flops": float(f.value), "graph_state": int(g.value)}

    def profile(self, images: Sequence[np.ndarray], imgsz: int = 640, conf: float = 0.25) -> List[Tuple[str, float]]:
        """One eager predict() with HIP events around every launch: [("<kernel> <layer>", ms)] in launch order."""
        _check(lib().ffp_rtdetr_set_profile(self._h, 1))
        try:
            self.predict(images, imgsz, conf)
        finally:
            _check(lib().ffp_rtdetr_set_profile(self._h, 0))
        n = C.c_int32(0)
        _check(lib().ffp_rtdetr_profile_count(self._h, C.byref(n)))
        out, name, ms = [], C.create_string_buffer(256), C.c_float(0)
        for i in range(n.value):
            _check(lib().ffp_rtdetr_profile_get(self._h, i, name, len(name), C.byref(ms)))
            out.append((name.value.decode(), float(ms.value)))
        return out

    @staticmethod
    def _batch(images):
        ims = [_as_frame(im) for im in images]
        ptrs = (C.c_void_p * len(ims))(*[im.ctypes.data for im in ims])
        hw = np.ascontiguousarray(np.array([im.shape[:2] for im in ims], np.int32).reshape(-1))
        return ims, ptrs, hw

    def predict(self, images: Sequence[np.ndarray], imgsz: int = 640, conf: float = 0.25) -> List[np.ndarray]:
        """BGR uint8 images -> per image (k, 6) float32 rows {x1, y1, x2, y2, score, cls} in original pixels, query order."""
        ims, ptrs, hw = self._batch(images)
        n = len(ims)
        out = np.zeros((n, self.NQ, 6), np.float32)
        counts = np.zeros(n, np.int32)
        _check(lib().ffp_rtdetr_predict(self._h, ptrs, _ip(hw), n, imgsz, conf, _fp(out), _ip(counts)))
        return [out[i, :counts[i]].copy() for i in range(n)]

    def forward_raw(self, images: Sequence[np.ndarray], imgsz: int = 640) -> Tuple[np.ndarray, np.ndarray]:
        """-> ([n, 300, 4 + nc] boxes cxcywh (normalised) ++ sigmoid scores, [n, 300] encoder token of every query)."""
        ims, ptrs, hw = self._batch(images)
        n = len(ims)
        out = np.zeros((n, self.NQ, 4 + self.nc), np.float32)
        topk = np.zeros((n, self.NQ), np.int32)
        _check(lib().ffp_rtdetr_forward_raw(self._h, ptrs, _ip(hw), n, imgsz, _fp(out), _ip(topk)))
        return out, topk

    TILE_MODES = {"local": 0, "sahi": 1}         # FFP_RT_TILES_LOCAL, FFP_RT_TILES_SAHI

    def infer_tiles(self, frame: np.ndarray, tiles: Sequence[Sequence[int]], imgsz: int = 640, conf: float = 0.25, mode: str = "local",
                    chan_order: int = CHAN_AS_BGR, max_batch: int = 0) -> List[np.ndarray]:
        """Tiles [x0, y0, x1, y1] of one frame, each stretched to imgsz -> per tile (k, 6) float32 rows in query order. mode "local": tile-local
        pixels, predict()'s rows of the crop; "sahi": clipped against the frame, invalid boxes dropped, shifted to frame pixels (float boxes).
        max_batch: items per network batch (0: FFP_RT_TILES_DEFAULT_BATCH)."""
        f = _as_frame(frame)
        t = _as_tiles(tiles)
        n = t.shape[0]
        dets = np.zeros((max(n, 1), self.NQ, 6), np.float32)
        counts = np.zeros(max(n, 1), np.int32)
        _check(lib().ffp_rtdetr_infer_tiles(self._h, f.ctypes.data, f.shape[0], f.shape[1], chan_order, _ip(t), n, imgsz, conf, self.TILE_MODES[mode],
                                            max_batch, _fp(dets), _ip(counts)))
        return [dets[i, :counts[i]].copy() for i in range(n)]

    def sliced_predict(self, frame: np.ndarray, slice_h: int, slice_w: int, overlap_h: float = 0.2, overlap_w: float = 0.2,
                       perform_standard_pred: bool = True, imgsz: int = 640, conf: float = 0.25, pp_type: str = "GREEDYNMM", pp_metric: str = "IOS",
                       pp_thr: float = 0.5, class_agnostic: bool = False, chan_order: int = CHAN_AS_BGR, max_batch: int = 0, cap: int = 0) -> np.ndarray:
        """Fused get_sliced_prediction -> (k, 6) float32 rows {x1, y1, x2, y2, score, cls} in frame pixels (float boxes, sahi's rules)."""
        f = _as_frame(frame)
        H, W = f.shape[:2]
        if cap <= 0:
            cap = (len(slice_bboxes(H, W, slice_h, slice_w, overlap_h, overlap_w)) + 1) * self.NQ
        out = np.zeros((cap, 6), np.float32)
        n = C.c_int32(0)
        _check(lib().ffp_rtdetr_sliced_predict(self._h, f.ctypes.data, H, W, chan_order, slice_h, slice_w, overlap_h, overlap_w,
                                               int(perform_standard_pred), imgsz, conf, max_batch, PP_TYPES[pp_type], METRICS[pp_metric], float(pp_thr),
                                               int(class_agnostic), _fp(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def mem_bytes(self) -> dict:
        """Device bytes held by the resident plans' activations, and how many plans are resident."""
        b, n = C.c_uint64(0), C.c_int32(0)
        _check(lib().ffp_rtdetr_mem_bytes(self._h, C.byref(b), C.byref(n)))
        return {"plans": int(b.value), "plans_resident": int(n.value)}

    def drop_plans(self):
        _check(lib().ffp_rtdetr_drop_plans(self._h))


class Detector(_Handle):
    """YOLO11{n,s,m,l}-pose on one GPU (ffp_det_*); `arch` is the scale ("n", "s", "m" or "l", see arch.yolo11_scale_of)."""

    _DESTROY = "ffp_det_destroy"

    def __init__(self, weights, arch: str = "s", nc: int = 1, nkpt: int = 5, device: int = 0, precision: int = PREC_F32):
        buf = _weights_bytes(weights)
        self._h = C.c_void_p()
        self.nc, self.nkpt, self.arch, self.device, self.precision = nc, nkpt, arch, device, precision
        cbuf = C.create_string_buffer(buf, len(buf))
        _check(lib().ffp_det_create(cbuf, len(buf), ord(arch), nc, nkpt, device, precision, C.byref(self._h)))

    @property
    def stride(self) -> int:
        return 6 + 3 * self.nkpt

    @property
    def handle(self):
        return self._h

    def infer_tiles(self, frame: np.ndarray, tiles: Sequence[Sequence[int]], imgsz: int, conf: float, iou: float = 0.7,
                    max_det: int = 300, chan_order: int = CHAN_AS_BGR, round_boxes: bool = False) -> List[np.ndarray]:
        """-> per tile (n_i, 6+3*nkpt) float32 rows [x1,y1,x2,y2,score,cls,kpts] in tile-local pixels (not truncated)."""
        f = _as_frame(frame)
        t = _as_tiles(tiles)
        n = t.shape[0]
        dets = np.zeros((n, max_det, self.stride), np.float32)
        counts = np.zeros(n, np.int32)
        _check(lib().ffp_det_infer_tiles(self._h, f.ctypes.data, f.shape[0], f.shape[1], chan_order, _ip(t), n, imgsz, conf, iou,
                                         max_det, int(round_boxes), _fp(dets), _ip(counts)))
        return [dets[i, :counts[i]].copy() for i in range(n)]

    def forward_raw(self, frame: np.ndarray, tiles: Sequence[Sequence[int]], imgsz: int,
                    chan_order: int = CHAN_AS_BGR) -> List[np.ndarray]:
        """-> per tile the (4+nc+3*nkpt, A) inference-mode head output."""
        f = _as_frame(frame)
        t = _as_tiles(tiles)
        n = t.shape[0]
        no = 4 + self.nc + 3 * self.nkpt
        cap = 0
        for x0, y0, x1, y1 in t:
            sz = imgsz if imgsz > 0 else (max(t[0][2] - t[0][0], t[0][3] - t[0][1]) + 31) // 32 * 32
            cap += no * (sz // 8) ** 2 * 2
        out = np.zeros(cap, np.float32)
        cnt = np.zeros(n, np.int32)
        _check(lib().ffp_det_forward_raw(self._h, f.ctypes.data, f.shape[0], f.shape[1], chan_order, _ip(t), n, imgsz, _fp(out), cap, _ip(cnt)))
        res, o = [], 0
        for i in range(n):
            a = int(cnt[i])
            res.append(out[o:o + no * a].reshape(no, a).copy())
            o += no * a
        return res

    def sliced_predict(self, frame: np.ndarray, slice_h: int, slice_w: int, overlap_h: float = 0.2, overlap_w: float = 0.2,
                       perform_standard_pred: bool = True, imgsz: int = 1024, conf: float = 0.3, iou: float = 0.7, max_det: int = 300,
                       pp_type: str = "GREEDYNMM", pp_metric: str = "IOS", pp_thr: float = 0.5, class_agnostic: bool = False,
                       chan_order: int = CHAN_AS_BGR, round_boxes: bool = False, cap: int = 0) -> np.ndarray:
        """Fused get_sliced_prediction -> (n, 6+3*nkpt) rows in frame coordinates (boxes int-valued)."""
        f = _as_frame(frame)
        H, W = f.shape[:2]
        if cap <= 0:
            cap = (len(slice_bboxes(H, W, slice_h, slice_w, overlap_h, overlap_w)) + 1) * max_det
        out = np.zeros((cap, self.stride), np.float32)
        n = C.c_int32(0)
        _check(lib().ffp_sliced_predict(self._h, f.ctypes.data, H, W, chan_order, slice_h, slice_w, overlap_h, overlap_w,
                                        int(perform_standard_pred), imgsz, conf, iou, max_det, int(round_boxes), PP_TYPES[pp_type],
                                        METRICS[pp_metric], float(pp_thr), int(class_agnostic), _fp(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def last_ms(self) -> dict:
        names = ["total", "preprocess", "network", "decode_nms", "merge"]
        v = C.c_float(0)
        out = {}
        for i, k in enumerate(names):
            _check(lib().ffp_det_last_ms(self._h, i, C.byref(v)))
            out[k] = v.value
        return out

    def graph_status(self) -> int:
        """1: the last call replayed a captured hipGraph, 0: not captured yet, -1: capture failed (eager launches)."""
        v = C.c_int32(0)
        _check(lib().ffp_det_graph_status(self._h, C.byref(v)))
        return v.value

    def mem_bytes(self) -> dict:
        """Device memory held: packed weights, resident plans (activations + tables), number of plans."""
        a, b, n = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        _check(lib().ffp_det_mem_bytes(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return {"weights": int(a.value), "plans": int(b.value), "plans_resident": int(n.value)}

    def drop_plans(self):
        """Release every resident plan now (rebuilt on demand); the packed weights stay."""
        _check(lib().ffp_det_drop_plans(self._h))

    def set_lanes(self, mode: int):
        """0 (default) one stream; 1 head towers and C3k side convs as parallel graph branches (detector-only deployments)."""
        _check(lib().ffp_det_set_lanes(self._h, int(mode)))

    def set_buffer_reuse(self, mode: int):
        """0 one allocation per activation tensor; 1 (default) tensors with disjoint lifetimes share bytes; 2 as 1, released ranges are
        overwritten with 0xFF bytes (diagnostic). Results are bit-identical; the cached plans are dropped."""
        _check(lib().ffp_det_set_buffer_reuse(self._h, int(mode)))

    def set_gate(self, on: bool):
        """Skip the box and keypoint towers of items without a class score above conf (default on); bit-identical results; drops the cached plans."""
        _check(lib().ffp_det_set_gate(self._h, int(on)))

    def last_active(self) -> tuple:
        """(items whose box and keypoint towers ran, items) of the last inference call."""
        a, n = C.c_int32(0), C.c_int32(0)
        _check(lib().ffp_det_last_active(self._h, C.byref(a), C.byref(n)))
        return int(a.value), int(n.value)

    def mem_detail(self) -> dict:
        """Activation storage of the resident plans: bytes held, bytes one allocation per tensor would hold, peak of the bytes live at once."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ffp_det_mem_detail(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"activation_bytes": int(a.value), "no_reuse_bytes": int(b.value), "peak_live_bytes": int(c.value)}

    def fill_steps(self) -> dict:
        """Test hook: 0xFF fill steps in the resident plans, and tensors whose range reached the free list (mode 2: equal and > 0)."""
        a, b = C.c_int32(0), C.c_int32(0)
        _check(lib().ffp_det_fill_steps(self._h, C.byref(a), C.byref(b)))
        return {"fill_steps": int(a.value), "ranges_freed": int(b.value)}

    def stream_wait_event(self, hip_event: int):
        """Order the handle's following work behind a hipEvent_t of this process (torch.cuda.Event.cuda_event)."""
        _check(lib().ffp_det_stream_wait_event(self._h, C.c_void_p(int(hip_event))))

    def set_profile(self, on: bool):
        _check(lib().ffp_det_set_profile(self._h, int(on)))

    def profile(self) -> List[dict]:
        return _profile(self._h, lib().ffp_det_profile_count, lib().ffp_det_profile_get, lib().ffp_det_profile_bytes)

    def profile_detail(self) -> List[dict]:
        return _profile_detail(self._h, lib().ffp_det_profile_detail)

    def conv_stats(self) -> dict:
        fl, ms, n = C.c_double(0), C.c_float(0), C.c_int32(0)
        _check(lib().ffp_det_last_conv_stats(self._h, C.byref(fl), C.byref(ms), C.byref(n)))
        return {"flops": fl.value, "ms": ms.value, "launches": n.value}


def _profile_detail(h, fn) -> List[dict]:
    out, i = [], 0
    while True:
        name = C.create_string_buffer(128)
        fl, ms = C.c_double(0), C.c_float(0)
        if fn(h, i, name, 128, C.byref(fl), C.byref(ms)) != 0:
            return out
        out.append({"name": name.value.decode(), "flops": fl.value, "ms": ms.value})
        i += 1


def _profile(h, count_fn, get_fn, bytes_fn=None) -> List[dict]:
    n = C.c_int32(0)
    _check(count_fn(h, C.byref(n)))
    out = []
    for i in range(n.value):
        name = C.create_string_buffer(64)
        fl, ms, ln, by = C.c_double(0), C.c_float(0), C.c_int32(0), C.c_double(0)
        _check(get_fn(h, i, name, 64, C.byref(fl), C.byref(ms), C.byref(ln)))
        if bytes_fn is not None:
            _check(bytes_fn(h, i, C.byref(by)))
        out.append({"variant": name.value.decode(), "flops": fl.value, "ms": ms.value, "launches": ln.value, "bytes": by.value})
    return out


def conv_totals_enable(on: bool = True):
    """Start (and zero) / stop the process-wide per-variant totals of every plan execution (ffp_conv_totals_*)."""
    _check(lib().ffp_conv_totals_enable(int(on)))


def conv_totals() -> dict:
    """{variant: {"launches", "flops", "bytes"}} since conv_totals_enable(True): algorithmic figures of every launch, graph replays included."""
    n = C.c_int32(0)
    _check(lib().ffp_conv_totals_count(C.byref(n)))
    out = {}
    for i in range(n.value):
        name = C.create_string_buffer(64)
        fl, by, ln = C.c_double(0), C.c_double(0), C.c_int64(0)
        _check(lib().ffp_conv_totals_get(i, name, 64, C.byref(fl), C.byref(by), C.byref(ln)))
        out[name.value.decode()] = {"launches": int(ln.value), "flops": fl.value, "bytes": by.value}
    return out


def merge(rows: np.ndarray, pp_type: str = "GREEDYNMM", metric: str = "IOS", thr: float = 0.5, class_agnostic: bool = False,
          device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """SAHI post-process on (n, stride>=6) float32 rows -> (merged rows, source indices)."""
    r = np.ascontiguousarray(rows, np.float32)
    if r.ndim != 2 or r.shape[1] < 6:
        raise ValueError("rows must be (n, >=6)")
    n, stride = r.shape
    out = np.zeros((max(n, 1), stride), np.float32)
    src = np.zeros(max(n, 1), np.int32)
    k = C.c_int32(0)
    _check(lib().ffp_merge(device, _fp(r), n, stride, PP_TYPES[pp_type], METRICS[metric], float(thr), int(class_agnostic), _fp(out),
                           _ip(src), C.byref(k)))
    return out[:k.value].copy(), src[:k.value].copy()


class Enhancer(_Handle):
    """Real-ESRGAN RRDBNet on one GPU (ffp_sr_*)."""

    _DESTROY = "ffp_sr_destroy"

    def __init__(self, weights, scale: int = 4, num_block: int = 23, device: int = 0, half: bool = True):
        buf = _weights_bytes(weights)
        self._h = C.c_void_p()
        self.scale, self.num_block, self.device, self.half = scale, num_block, device, half
        cbuf = C.create_string_buffer(buf, len(buf))
        _check(lib().ffp_sr_create(cbuf, len(buf), scale, num_block, device, int(half), C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def enhance(self, img_bgr: np.ndarray, tile: int = 0, tile_pad: int = 10, pre_pad: int = 0) -> np.ndarray:
        return self.enhance_batch([img_bgr], tile, tile_pad, pre_pad)[0]

    def enhance_batch(self, imgs: Sequence[np.ndarray], tile: int = 0, tile_pad: int = 10, pre_pad: int = 0) -> List[np.ndarray]:
        ins = [_as_frame(i) for i in imgs]
        n = len(ins)
        outs = [np.zeros((i.shape[0] * self.scale, i.shape[1] * self.scale, 3), np.uint8) for i in ins]
        ip = (C.c_void_p * n)(*[i.ctypes.data for i in ins])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        hs = np.asarray([i.shape[0] for i in ins], np.int32)
        ws = np.asarray([i.shape[1] for i in ins], np.int32)
        _check(lib().ffp_sr_enhance_batch(self._h, n, ip, _ip(hs), _ip(ws), tile, tile_pad, pre_pad, op))
        return outs

    def enhance_ex(self, img: np.ndarray, max_range: int = 255, alpha_mode: int = SR_ALPHA_REALESRGAN, out_h: Optional[int] = None,
                   out_w: Optional[int] = None, tile: int = 0, tile_pad: int = 10, pre_pad: int = 0) -> np.ndarray:
        """ffp_sr_enhance_ex: RealESRGANer.enhance for an HxW (gray), HxWx3 (BGR) or HxWx4 (BGRA) uint8 / uint16 array with the
        given max_range (255 / 65535), alpha upsampler and output size (default scale*h x scale*w; any other size is a Lanczos4
        resize of the result). Returns uint16 when max_range == 65535, else uint8, with the input's number of channels."""
        a = np.ascontiguousarray(img)
        if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)):
            raise ValueError(f"expected an HxW, HxWx3 or HxWx4 uint8 / uint16 array, got {a.dtype} {a.shape}")
        h, w = a.shape[:2]
        oh = h * self.scale if out_h is None else int(out_h)
        ow = w * self.scale if out_w is None else int(out_w)
        out = np.zeros((oh, ow) + a.shape[2:], np.uint16 if max_range == 65535 else np.uint8)
        _check(lib().ffp_sr_enhance_ex(self._h, a.ctypes.data, h, w, 1 if a.ndim == 2 else a.shape[2], 8 * a.itemsize, int(max_range),
                                       int(alpha_mode), oh, ow, tile, tile_pad, pre_pad, out.ctypes.data))
        return out

    def enhance_crops_dev(self, d_frames: Sequence[int], H: int, W: int, boxes: np.ndarray, d_out: int, out_cap: int,
                          frame_of_box: Optional[np.ndarray] = None, tile: int = 400, tile_pad: int = 10, wait: bool = True) -> np.ndarray:
        """Crops of resident BGR frame(s) (device pointers) -> enhanced crops packed in device memory at d_out.
        One frame: ffp_sr_enhance_crops_dev (wait) / _dev_async; several: ffp_sr_enhance_crops_multi_dev_async (+ ffp_sr_wait when
        wait). Returns the n+1 byte offsets (a crop that is empty after clamping has a zero-length entry)."""
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        n = b.shape[0]
        offs = np.zeros(n + 1, np.int64)
        op = offs.ctypes.data_as(_p(C.c_int64))
        if len(d_frames) == 1 and frame_of_box is None:
            fn = lib().ffp_sr_enhance_crops_dev if wait else lib().ffp_sr_enhance_crops_dev_async
            _check(fn(self._h, d_frames[0], H, W, _ip(b), n, tile, tile_pad, d_out, out_cap, op))
        else:
            f = np.ascontiguousarray(frame_of_box if frame_of_box is not None else np.zeros(n, np.int32), np.int32)
            ptrs = (C.c_void_p * len(d_frames))(*d_frames)
            _check(lib().ffp_sr_enhance_crops_multi_dev_async(self._h, len(d_frames), ptrs, _ip(f), H, W, _ip(b), n, tile, tile_pad, d_out,
                                                              out_cap, op))
            if wait:
                self.wait()
        return offs

    def wait(self):
        _check(lib().ffp_sr_wait(self._h))

    def last_ms(self) -> float:
        v = C.c_float(0)
        _check(lib().ffp_sr_last_ms(self._h, C.byref(v)))
        return v.value

    def set_fused_body(self, on: bool):
        """The 345 body convs as ONE persistent launch (default in fp16) or one launch per layer; bit-identical results (drops the plans)."""
        _check(lib().ffp_sr_set_fused_body(self._h, int(on)))

    def mem_bytes(self) -> dict:
        a, b, n = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        _check(lib().ffp_sr_mem_bytes(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return {"weights": int(a.value), "plans": int(b.value), "plans_resident": int(n.value)}

    def drop_plans(self):
        """Release every resident plan now (rebuilt on demand); the packed weights stay."""
        _check(lib().ffp_sr_drop_plans(self._h))

    def plan_state(self) -> dict:
        """plans_built: network layouts built so far (capacity-keyed: varying crop sizes must not grow it);
        last_graph: the last call replayed a captured hipGraph."""
        a, b = C.c_int32(0), C.c_int32(0)
        _check(lib().ffp_sr_plan_state(self._h, C.byref(a), C.byref(b)))
        return {"plans_built": a.value, "last_graph": bool(b.value)}

    def set_profile(self, on: bool):
        _check(lib().ffp_sr_set_profile(self._h, int(on)))

    def profile(self) -> List[dict]:
        return _profile(self._h, lib().ffp_sr_profile_count, lib().ffp_sr_profile_get, lib().ffp_sr_profile_bytes)

    def profile_detail(self) -> List[dict]:
        return _profile_detail(self._h, lib().ffp_sr_profile_detail)

    def conv_stats(self) -> dict:
        fl, ms, n = C.c_double(0), C.c_float(0), C.c_int32(0)
        _check(lib().ffp_sr_last_conv_stats(self._h, C.byref(fl), C.byref(ms), C.byref(n)))
        return {"flops": fl.value, "ms": ms.value, "launches": n.value}


def op_conv2d(x: np.ndarray, w: np.ndarray, b: Optional[np.ndarray], stride: int = 1, groups: int = 1, act: int = 0, up: bool = False,
              res: Optional[np.ndarray] = None, res_scale: float = 1.0, precision: int = PREC_F32, device: int = 0) -> np.ndarray:
    """Single convolution through the HIP kernels. x: (n,h,w,cin) fp32 NHWC, w: (cout, cin/groups, k, k) -> (n,ho,wo,cout)."""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    n, h, wd, cin = x.shape
    cout, _, k, _ = w.shape
    hi, wi = (h * 2, wd * 2) if up else (h, wd)
    ho, wo = (hi + 2 * (k // 2) - k) // stride + 1, (wi + 2 * (k // 2) - k) // stride + 1
    y = np.zeros((n, ho, wo, cout), np.float32)
    bb = np.ascontiguousarray(b, np.float32) if b is not None else None
    rr = np.ascontiguousarray(res, np.float32) if res is not None else None
    _check(lib().ffp_op_conv2d(device, precision, _fp(x), n, h, wd, cin, _fp(w), _fp(bb), cout, k, stride,
                               groups, act, int(up), _fp(rr), res_scale, _fp(y)))
    return y


# ---- the detector's non-convolution kernels one at a time (tests/test_gpu_ops.py). A ragged batch is a list of (h, w, cs) arrays, one
# per image, holding WHOLE pixel records; the operator reads / writes the channel slice the offsets name. Output buffers are passed in
# (`y`, same list form) and come back with the slice written and every other value as it went in.
OP_SPPF, OP_ATTENTION, OP_DWCONV = 0, 1, 2
OP_CLS_TOWER = "cls_tower"      # op_cls_tower: the variant is a tile height, with a workgroup cap beside it (ffp_op_cls_tower_variant)
OP_VARIANTS = {OP_SPPF: {"lds": 1, "direct": 2}, OP_ATTENTION: {"mfma": 1, "valu": 2}, OP_DWCONV: {"col": 1, "strip": 2},
               OP_CLS_TOWER: {"rows16": 16, "rows8": 8}}


def op_variant(family, variant=0, wg_cap: int = 0) -> None:
    """Pin the kernel the following op_sppf_pool / op_psa_attention / op_dwconv3x3 / op_cls_tower calls launch (a name of OP_VARIANTS[family],
    or 0 / None for the automatic choice). OP_CLS_TOWER: the tile height, and with wg_cap > 0 at most that many workgroups, so that a small
    batch walks its tiles persistently."""
    v = OP_VARIANTS[family][variant] if isinstance(variant, str) else int(variant or 0)
    if family == OP_CLS_TOWER:
        _check(lib().ffp_op_cls_tower_variant(v, int(wg_cap)))
        return
    if wg_cap:
        raise ValueError("wg_cap is for OP_CLS_TOWER")
    _check(lib().ffp_op_variant(int(family), v))


class OpBatch:
    """A ragged batch packed once (the images' pixel records back to back), to be passed in place of the list of images to several operator calls."""

    def __init__(self, imgs: Sequence[np.ndarray]):
        self.flat, self.hs, self.ws, self.cs = _op_pack(imgs)


def _op_pack(imgs):
    if isinstance(imgs, OpBatch):
        return imgs.flat, imgs.hs, imgs.ws, imgs.cs
    imgs = [np.asarray(a, np.float32) for a in imgs]
    if not imgs or any(a.ndim != 3 or a.shape[2] != imgs[0].shape[2] for a in imgs):
        raise ValueError("a batch is a non-empty list of (h, w, cs) arrays with one record size")
    hs = np.asarray([a.shape[0] for a in imgs], np.int32)
    ws = np.asarray([a.shape[1] for a in imgs], np.int32)
    cs = int(imgs[0].shape[2])
    flat = np.ascontiguousarray(np.concatenate([a.reshape(-1, cs) for a in imgs], 0))
    return flat, hs, ws, cs


def _op_unpack(flat: np.ndarray, hs, ws) -> List[np.ndarray]:
    out, p = [], 0
    for h, w in zip(hs, ws):
        out.append(flat[p:p + int(h) * int(w)].reshape(int(h), int(w), -1).copy())
        p += int(h) * int(w)
    return out


def _op_same_batch(hs, ws, hs2, ws2, what):
    if not (np.array_equal(hs, hs2) and np.array_equal(ws, ws2)):
        raise ValueError(f"{what}: image sizes differ from the input's")


def op_sppf_pool(x, c: int, x_coff: int, y, y_coffs, px_align: int = 1, precision: int = PREC_F32, device: int = 0) -> List[np.ndarray]:
    """y[..., y_coffs[k] : y_coffs[k] + c] = (k+1) chained MaxPool2d(5, 1, 2) of x[..., x_coff : x_coff + c], k = 0..2."""
    xf, hs, ws, xcs = _op_pack(x)
    yf, hs2, ws2, ycs = _op_pack(y)
    _op_same_batch(hs, ws, hs2, ws2, "sppf_pool")
    o1, o2, o3 = (int(v) for v in y_coffs)
    _check(lib().ffp_op_sppf_pool(device, precision, len(hs), _ip(hs), _ip(ws), px_align, c, _fp(xf), xcs, x_coff, _fp(yf), ycs, o1, o2, o3))
    return _op_unpack(yf, hs, ws)


def op_upsample2x(x, c: int, x_coff: int, y, y_coff: int, px_align: int = 1, precision: int = PREC_F32, device: int = 0) -> List[np.ndarray]:
    """y[..., y_coff : y_coff + c] = nearest x2 of x[..., x_coff : x_coff + c]; the images of y are twice as high and wide."""
    xf, hs, ws, xcs = _op_pack(x)
    yf, hs2, ws2, ycs = _op_pack(y)
    _op_same_batch(hs * 2, ws * 2, hs2, ws2, "upsample2x")
    _check(lib().ffp_op_upsample2x(device, precision, len(hs), _ip(hs), _ip(ws), px_align, c, _fp(xf), xcs, x_coff, _fp(yf), ycs, y_coff))
    return _op_unpack(yf, hs2, ws2)


def op_psa_attention(qkv, nh: int, q_coff: int, out, o_coff: int, px_align: int = 1, precision: int = PREC_F32, device: int = 0) -> List[np.ndarray]:
    """out[..., o_coff : o_coff + nh*64] = attention over each image's pixels of the nh heads [q(32) | k(32) | v(64)] at q_coff of qkv."""
    qf, hs, ws, qcs = _op_pack(qkv)
    of, hs2, ws2, ocs = _op_pack(out)
    _op_same_batch(hs, ws, hs2, ws2, "psa_attention")
    _check(lib().ffp_op_psa_attention(device, precision, len(hs), _ip(hs), _ip(ws), px_align, nh, _fp(qf), qcs, q_coff, _fp(of), ocs, o_coff))
    return _op_unpack(of, hs, ws)


def op_cls_tower(x, dw0, pw0, dw1, pw1, fin, head, head_coff: int, px_align: int = 32, want_e1: bool = True, device: int = 0):
    """The fused class tower (ffp_op_cls_tower). x / head: per image (h, w, cin) / (h, w, head_cs) arrays; dw0 .. fin: (weight, bias) pairs.
    -> (e1 per image (h, w, 128) or None, head per image with the logits in channels [head_coff, head_coff + nc), the number of 32-bit words
    that changed in the device buffers' padding pixels: between the aligned images and behind the last one)."""
    hs, ws = [int(a.shape[0]) for a in x], [int(a.shape[1]) for a in x]
    cin, nc, hcs = int(x[0].shape[2]), int(fin[0].shape[0]), int(head[0].shape[2])
    xf = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1, cin) for a in x]))
    hf = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1, hcs) for a in head]))
    e1 = np.zeros((xf.shape[0], 128), np.float32) if want_e1 else None
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    ws_ = [f32(a) for pair in (dw0, pw0, dw1, pw1, fin) for a in pair]
    stray = C.c_int64(-1)
    _check(lib().ffp_op_cls_tower(device, len(hs), _ip(np.asarray(hs, np.int32)), _ip(np.asarray(ws, np.int32)), px_align, cin, nc, _fp(xf),
                                  *[_fp(a) for a in ws_], _fp(e1) if want_e1 else None, _fp(hf), hcs, head_coff, C.byref(stray)))
    cut = np.cumsum([0] + [h * w for h, w in zip(hs, ws)])
    split = lambda a, c: [a[cut[i]:cut[i + 1]].reshape(hs[i], ws[i], c) for i in range(len(hs))]
    return (split(e1, 128) if want_e1 else None), split(hf, hcs), int(stray.value)


def op_dwconv3x3(x, c: int, x_coff: int, w: np.ndarray, b: Optional[np.ndarray], y, y_coff: int, act: int = 0, grp: int = 0, grp_stride: int = 0,
                 grp_off: int = 0, res=None, r_coff: int = 0, px_align: int = 1, precision: int = PREC_F32, device: int = 0) -> List[np.ndarray]:
    """y[..., y_coff : y_coff + c] = act(depthwise3x3(x) + b) [+ res[..., r_coff : r_coff + c]]; w: (c, 3, 3). grp > 0: input channel ch is
    x[..., x_coff + (ch // grp) * grp_stride + grp_off + ch % grp], else x[..., x_coff + ch]."""
    xf, hs, ws, xcs = _op_pack(x)
    yf, hs2, ws2, ycs = _op_pack(y)
    _op_same_batch(hs, ws, hs2, ws2, "dwconv3x3")
    w = np.ascontiguousarray(w, np.float32)
    if w.shape != (c, 3, 3):
        raise ValueError(f"dwconv3x3: weights {w.shape}, expected {(c, 3, 3)}")
    bb = np.ascontiguousarray(b, np.float32) if b is not None else None
    if bb is not None and bb.shape != (c,):
        raise ValueError(f"dwconv3x3: bias {bb.shape}, expected {(c,)}")
    rf, rcs = None, 0
    if res is not None:
        rf, hs3, ws3, rcs = _op_pack(res)
        _op_same_batch(hs, ws, hs3, ws3, "dwconv3x3 residual")
    _check(lib().ffp_op_dwconv3x3(device, precision, len(hs), _ip(hs), _ip(ws), px_align, c, _fp(xf), xcs, x_coff, grp, grp_stride, grp_off, _fp(w),
                                  _fp(bb), act, _fp(rf), rcs, r_coff, _fp(yf), ycs, y_coff))
    return _op_unpack(yf, hs, ws)


def op_conv2d_views(x, x_coff: int, w: np.ndarray, b: Optional[np.ndarray], y, y_coff: int, stride: int = 1, act: int = 0, act_post: int = 0,
                    up: bool = False, res1=None, r1_coff: int = 0, s1: float = 1.0, res2=None, r2_coff: int = 0, s2: float = 1.0, px_align: int = 32,
                    per_image_amax: bool = False, amax_out=None, gate=None, gate_prev=None, precision: int = PREC_F32, device: int = 0):
    """One dense conv on the operands the plans give it (ffp_op_conv2d_views). x: per image (h, w, x_cs) arrays, read at channels
    [x_coff, x_coff + cin); w: (cout, cin, k, k); y / res1 / res2: per image arrays of the OUTPUT sizes, the conv writes y[..., y_coff : y_coff + cout].
    x, y, res1 and res2 may be OpBatch objects (packed once, reused over calls). amax_out: initial bit patterns of the output's max-|value| slots (n with per_image_amax, else 1; default zeros); gate / gate_prev: per image
    0 / 1. -> (y per image, final slot bit patterns, elements changed where the conv may not write)."""
    xf, hs, ws, xcs = _op_pack(x)
    yf, hs2, ws2, ycs = _op_pack(y)
    if isinstance(y, OpBatch):
        yf = yf.copy()                     # in/out: the packed batch stays what it was
    w = np.ascontiguousarray(w, np.float32)
    if w.ndim != 4 or w.shape[2] != w.shape[3]:
        raise ValueError(f"conv2d_views: weights {w.shape}, expected (cout, cin, k, k)")
    cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    bb = np.ascontiguousarray(b, np.float32) if b is not None else None
    if bb is not None and bb.shape != (cout,):
        raise ValueError(f"conv2d_views: bias {bb.shape}, expected {(cout,)}")
    n = len(hs)
    sc = 2 if up else 1
    pad = k // 2
    _op_same_batch((hs * sc + 2 * pad - k) // stride + 1, (ws * sc + 2 * pad - k) // stride + 1, hs2, ws2, "conv2d_views output")
    rf = [None, None]
    rcs = [0, 0]
    for i, r in enumerate((res1, res2)):
        if r is not None:
            rf[i], hs3, ws3, rcs[i] = _op_pack(r)
            _op_same_batch(hs2, ws2, hs3, ws3, "conv2d_views residual")
    ns = n if per_image_amax else 1
    slots = np.zeros(ns, np.uint32) if amax_out is None else np.ascontiguousarray(amax_out, np.uint32).copy()
    if slots.shape != (ns,):
        raise ValueError(f"conv2d_views: {slots.shape} output slots, expected {(ns,)}")
    g = [None, None]
    for i, m in enumerate((gate, gate_prev)):
        if m is not None:
            g[i] = np.ascontiguousarray(m, np.int32)
            if g[i].shape != (n,):
                raise ValueError(f"conv2d_views: gate {g[i].shape}, expected {(n,)}")
    stray = C.c_int64(-1)
    _check(lib().ffp_op_conv2d_views(device, precision, n, _ip(hs), _ip(ws), px_align, _fp(xf), xcs, x_coff, cin, _fp(w), _fp(bb), cout, k, stride, act,
                                     act_post, int(bool(up)), _fp(rf[0]), rcs[0], r1_coff, s1, _fp(rf[1]), rcs[1], r2_coff, s2, _fp(yf), ycs, y_coff,
                                     int(bool(per_image_amax)), _up(slots), _ip(g[0]),
                                     _ip(g[1]), C.byref(stray)))
    cut = np.cumsum([0] + [int(h) * int(w_) for h, w_ in zip(hs2, ws2)])
    return [yf[cut[i]:cut[i + 1]].reshape(int(hs2[i]), int(ws2[i]), ycs) for i in range(n)], slots, int(stray.value)


def op_det_post(heads, nc: int, nkpt: int, geom, conf: float = 0.25, iou: float = 0.7, max_det: int = 300, round_boxes: bool = False,
                shift: bool = False, full_hw: Tuple[int, int] = (0, 0), raw: bool = True, nms: bool = True, px_align: int = 1, device: int = 0):
    """Pose-head post-processing of given head tensors. heads: per image a triple of (H/s, W/s, 64 + nc + 3*nkpt) arrays for s = 8, 16, 32;
    geom: per image (gain, pad_x, pad_y, crop_w, crop_h, x0, y0). Returns (raws, dets, counts): raws[i] the (4 + nc + 3*nkpt, anchors)
    inference-mode output (None when raw=False); dets (n, max_det, 6 + 3*nkpt) and counts (n,) after NMS (None when nms=False)."""
    n = len(heads)
    cs = 64 + nc + 3 * nkpt
    lv = []
    for l in range(3):
        f, hs, ws, c = _op_pack([h[l] for h in heads])
        if c != cs:
            raise ValueError(f"det_post: head records of {c}, expected {cs}")
        lv.append((f, hs, ws))
    H, Wd = lv[0][1] * 8, lv[0][2] * 8
    for l in (1, 2):
        if not (np.array_equal(lv[l][1] * (8 << l), H) and np.array_equal(lv[l][2] * (8 << l), Wd)):
            raise ValueError("det_post: the three levels must be the net input size over 8, 16 and 32")
    g = np.asarray(geom, np.float64).reshape(n, 7)
    gp = np.ascontiguousarray(g[:, :3], np.float32)
    rc = np.ascontiguousarray(np.rint(g[:, 3:]), np.int32)
    A = [int(sum(int(lv[l][1][i]) * int(lv[l][2][i]) for l in range(3))) for i in range(n)]
    no, stride = 4 + nc + 3 * nkpt, 6 + 3 * nkpt
    o_raw = np.zeros(no * sum(A), np.float32) if raw else None
    o_dets = np.zeros((n, max_det, stride), np.float32) if nms else None
    o_cnt = np.zeros(n, np.int32) if nms else None
    _check(lib().ffp_op_det_post(device, n, _ip(np.ascontiguousarray(H, np.int32)), _ip(np.ascontiguousarray(Wd, np.int32)), px_align, nc, nkpt,
                                 _fp(lv[0][0]), _fp(lv[1][0]), _fp(lv[2][0]), _fp(gp), _ip(rc), conf, iou, max_det, int(round_boxes), int(shift),
                                 int(full_hw[0]), int(full_hw[1]), _fp(o_raw) if raw else None, _fp(o_dets) if nms else None,
                                 _ip(o_cnt) if nms else None))
    raws = None
    if raw:
        raws, p = [], 0
        for a in A:
            raws.append(o_raw[p:p + no * a].reshape(no, a).copy())
            p += no * a
    return raws, o_dets, o_cnt


def op_rt_topk(scores: np.ndarray, nc: Optional[int] = None, s_coff: int = 0, device: int = 0) -> np.ndarray:
    """scores (n, NT, cs) -> (n, 300) token indices by (max over the nc class logits at s_coff descending, index ascending)."""
    s = np.ascontiguousarray(scores, np.float32)
    n, nt, cs = s.shape
    nc = cs - s_coff if nc is None else nc
    out = np.zeros((n, 300), np.int32)
    _check(lib().ffp_op_rt_topk(device, n, nt, nc, _fp(s), cs, s_coff, _ip(out)))
    return out


# ---- the RT-DETR and SCRFD kernels one at a time (tests/test_gpu_rtdetr_ops.py, tests/test_gpu_scrfd_ops.py). Arrays hold whole records
# (..., cs); outputs are passed in and come back with the slice written. `amax`: None (no slot) or the initial value of the output
# buffer's max-|value| slot as a float; the operator then returns (output, final slot bits as int).
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _slot(amax):
    return None if amax is None else np.asarray([np.float32(amax)], np.float32).view(np.uint32).copy()


def _ret(out, s):
    return out if s is None else (out, int(s[0]))


def op_rt_dwconv(x, c: int, x_coff: int, w, b, y, y_coff: int, k: int, s: int, act: int = 0, amax=None, device: int = 0):
    """x (n, h, w, cs) -> y (n, ho, wo, cs') slice = act(depthwise k x k stride s pad k // 2 + b); w (c, k, k)."""
    x, y, w, b = _f32(x), _f32(y).copy(), _f32(w), _f32(b)
    n, h, wd, xcs = x.shape
    if w.shape != (c, k, k) or b.shape != (c,) or y.shape[:3] != (n, (h - 1) // s + 1, (wd - 1) // s + 1):
        raise ValueError("rt_dwconv: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_dwconv(device, n, h, wd, c, k, s, act, _fp(x), xcs, x_coff, _fp(w), _fp(b), _fp(y), y.shape[3], y_coff, _up(sl)))
    return _ret(y, sl)


def op_rt_maxpool2(x, c: int, x_coff: int, y, y_coff: int, amax=None, device: int = 0):
    """HGStem's pool: y slice = max over the 2x2 window at each pixel of x, zeros past the bottom / right edge."""
    x, y = _f32(x), _f32(y).copy()
    n, h, wd, xcs = x.shape
    if y.shape[:3] != (n, h, wd):
        raise ValueError("rt_maxpool2: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_maxpool2(device, n, h, wd, c, _fp(x), xcs, x_coff, _fp(y), y.shape[3], y_coff, _up(sl)))
    return _ret(y, sl)


def op_rt_add(a, c: int, a_coff: int, b, b_coff: int, y, y_coff: int, period: int = 0, amax=None, device: int = 0):
    """a (npx, cs), b (period or npx, cs') -> y slice = a + b[p % period] (period 0: b[p])."""
    a, b, y = _f32(a), _f32(b), _f32(y).copy()
    if b.shape[0] != (period or a.shape[0]) or y.shape[0] != a.shape[0]:
        raise ValueError("rt_add: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_add(device, a.shape[0], c, _fp(a), a.shape[1], a_coff, _fp(b), b.shape[1], b_coff, period, _fp(y), y.shape[1], y_coff, _up(sl)))
    return _ret(y, sl)


def op_rt_layernorm(x, x_coff: int, gamma, beta, y, y_coff: int, amax=None, device: int = 0):
    """LayerNorm over 256 channels, eps 1e-5: x (npx, cs) -> y slice; x None: in place on the slice of y."""
    y, g, b = _f32(y).copy(), _f32(gamma), _f32(beta)
    xx = _f32(x) if x is not None else None
    if g.shape != (256,) or b.shape != (256,) or (xx is not None and xx.shape[0] != y.shape[0]):
        raise ValueError("rt_layernorm: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_layernorm(device, y.shape[0], _fp(xx), xx.shape[1] if xx is not None else 0, x_coff, _fp(g), _fp(b),
                                     _fp(y), y.shape[1], y_coff, _up(sl)))
    return _ret(y, sl)


def op_rt_gelu(x, c: int, coff: int, amax=None, device: int = 0):
    """Exact GELU in place on c channels at coff of x (npx, cs)."""
    x = _f32(x).copy()
    sl = _slot(amax)
    _check(lib().ffp_op_rt_gelu(device, x.shape[0], c, _fp(x), x.shape[1], coff, _up(sl)))
    return _ret(x, sl)


def op_rt_attention(qk, qk_coff: int, v, v_coff: int, y, y_coff: int, amax=None, device: int = 0):
    """qk (n, L, cs) with [q 256 | k 256] at qk_coff, v (n, L, cs') -> y (n, L, cs'') slice of 256: 8 heads of 32 over each image's tokens."""
    qk, v, y = _f32(qk), _f32(v), _f32(y).copy()
    n, L = qk.shape[:2]
    if v.shape[:2] != (n, L) or y.shape[:2] != (n, L):
        raise ValueError("rt_attention: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_attention(device, n, L, _fp(qk), qk.shape[2], qk_coff, _fp(v), v.shape[2], v_coff, _fp(y), y.shape[2], y_coff, _up(sl)))
    return _ret(y, sl)


def op_rt_enc_prep(srcs, src_coffs, valid, t, tm, amax_t=None, amax_tm=None, device: int = 0):
    """srcs: three (n, h_l, w_l, cs_l) arrays with 256 channels at src_coffs[l]; valid (tokens,); t, tm: (rows, 256) with rows >= n * tokens.
    Returns (t, tm, slot bits of t or None, slot bits of tm or None)."""
    srcs = [_f32(a) for a in srcs]
    n = srcs[0].shape[0]
    hs = np.asarray([a.shape[1] for a in srcs], np.int32)
    ws = np.asarray([a.shape[2] for a in srcs], np.int32)
    cs = np.asarray([a.shape[3] for a in srcs], np.int32)
    co = np.asarray(src_coffs, np.int32)
    valid, t, tm = _f32(valid), _f32(t).copy(), _f32(tm).copy()
    if valid.shape != (int((hs * ws).sum()),) or t.shape != tm.shape or t.shape[1] != 256 or any(a.shape[0] != n for a in srcs):
        raise ValueError("rt_enc_prep: shapes")
    s1, s2 = _slot(amax_t), _slot(amax_tm)
    _check(lib().ffp_op_rt_enc_prep(device, n, _ip(hs), _ip(ws), _fp(srcs[0]), _fp(srcs[1]), _fp(srcs[2]), _ip(cs), _ip(co), _fp(valid), t.shape[0],
                                    _fp(t), _fp(tm), _up(s1), _up(s2)))
    return t, tm, None if s1 is None else int(s1[0]), None if s2 is None else int(s2[0])


def op_rt_gather(e, e_coff: int, idx, anchors, q, q_coff: int, anc, amax=None, device: int = 0):
    """e (n, NT, cs), idx (n, 300), anchors (NT, 4) -> (q (n, 300, cs') slice of 256, anc (n, 300, 4)) [, slot bits]."""
    e, q, anchors, anc = _f32(e), _f32(q).copy(), _f32(anchors), _f32(anc).copy()
    idx = np.ascontiguousarray(idx, np.int32)
    n, nt = e.shape[:2]
    if idx.shape != (n, 300) or anchors.shape != (nt, 4) or q.shape[:2] != (n, 300) or anc.shape != (n, 300, 4):
        raise ValueError("rt_gather: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_gather(device, n, nt, _fp(e), e.shape[2], e_coff, _ip(idx), _fp(anchors), _fp(q), q.shape[2], q_coff, _fp(anc), _up(sl)))
    return (q, anc) if sl is None else (q, anc, int(sl[0]))


def op_rt_ref(delta, d_coff: int, ref, r_coff: int, anc=None, amax=None, device: int = 0):
    """delta (nq, cs), ref (nq, cs') -> ref slice of 4 = sigmoid(delta + anc) (anc (nq, 4) given) or sigmoid(delta + inverse_sigmoid(ref))."""
    delta, ref = _f32(delta), _f32(ref).copy()
    an = _f32(anc) if anc is not None else None
    if ref.shape[0] != delta.shape[0] or (an is not None and an.shape != (delta.shape[0], 4)):
        raise ValueError("rt_ref: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_ref(device, delta.shape[0], _fp(delta), delta.shape[1], d_coff, _fp(an), _fp(ref), ref.shape[1],
                               r_coff, _up(sl)))
    return _ret(ref, sl)


def op_rt_deform(shapes, val, v_coff: int, oa, oa_coff: int, ref, r_coff: int, y, y_coff: int, amax=None, device: int = 0):
    """shapes: three (h, w); val (n, tokens, cs) slice of 256, oa (n, 300, cs') slice of 288, ref (n, 300, cs'') slice of 4 -> y (n, 300, cs''')
    slice of 256."""
    val, oa, ref, y = _f32(val), _f32(oa), _f32(ref), _f32(y).copy()
    hs = np.asarray([s[0] for s in shapes], np.int32)
    ws = np.asarray([s[1] for s in shapes], np.int32)
    n = val.shape[0]
    if val.shape[1] != int((hs * ws).sum()) or oa.shape[:2] != (n, 300) or ref.shape[:2] != (n, 300) or y.shape[:2] != (n, 300):
        raise ValueError("rt_deform: shapes")
    sl = _slot(amax)
    _check(lib().ffp_op_rt_deform(device, n, _ip(hs), _ip(ws), _fp(val), val.shape[2], v_coff, _fp(oa), oa.shape[2], oa_coff, _fp(ref), ref.shape[2],
                                  r_coff, _fp(y), y.shape[2], y_coff, _up(sl)))
    return _ret(y, sl)


def op_rt_decode(ref, r_coff: int, scores, s_coff: int, nc: int, conf: Optional[float] = None, orig_wh=None, raw=None, det=None, device: int = 0):
    """ref (n, 300, cs) slice of 4, scores (n, 300, cs') slice of nc logits. raw: (n, 300, 4 + nc) array to fill, or None; det: (n, 300, 6)
    array to fill (needs conf and orig_wh (n, 2) = width, height), or None. Returns (raw, det, counts)."""
    ref, scores = _f32(ref), _f32(scores)
    n = ref.shape[0]
    if ref.shape[:2] != (n, 300) or scores.shape[:2] != (n, 300):
        raise ValueError("rt_decode: shapes")
    o_raw = _f32(raw).copy() if raw is not None else None
    o_det = _f32(det).copy() if det is not None else None
    cnt = np.full(n, -1, np.int32) if det is not None else None
    wh = _f32(orig_wh) if orig_wh is not None else None
    if (o_raw is not None and o_raw.shape != (n, 300, 4 + nc)) or (o_det is not None and (o_det.shape != (n, 300, 6) or wh is None or wh.shape != (n, 2))):
        raise ValueError("rt_decode: output shapes")
    _check(lib().ffp_op_rt_decode(device, n, nc, _fp(ref), ref.shape[2], r_coff, _fp(scores), scores.shape[2], s_coff, float(conf or 0.0),
                                  _fp(wh), _fp(o_raw),
                                  _fp(o_det), _ip(cnt)))
    return o_raw, o_det, cnt


def op_rt_post_tiles(ref, r_coff: int, scores, s_coff: int, nc: int, conf: float, tiles, full_shape, mode: str, det=None, device: int = 0):
    """ref (n, 300, cs) slice of 4, scores (n, 300, cs') slice of nc logits, tiles (n, 4) x0, y0, x1, y1, full_shape (h, w), mode "local" |
    "sahi". det: (n, 300, 6) array to fill (default zeros). Returns (det, counts)."""
    ref, scores = _f32(ref), _f32(scores)
    n = ref.shape[0]
    t = _as_tiles(tiles)
    if ref.shape[:2] != (n, 300) or scores.shape[:2] != (n, 300) or t.shape[0] != n:
        raise ValueError("rt_post_tiles: shapes")
    o = _f32(det).copy() if det is not None else np.zeros((n, 300, 6), np.float32)
    if o.shape != (n, 300, 6):
        raise ValueError("rt_post_tiles: output shape")
    cnt = np.full(n, -1, np.int32)
    _check(lib().ffp_op_rt_post_tiles(device, n, nc, _fp(ref), ref.shape[2], r_coff, _fp(scores), scores.shape[2], s_coff, float(conf), _ip(t),
                                      int(full_shape[0]), int(full_shape[1]), RTDETRDetector.TILE_MODES[mode], _fp(o), _ip(cnt)))
    return o, cnt


def op_scrfd_pool(x, c: int, x_coff: int, y, y_coff: int, maxpool: bool, k: int = 2, px_align: int = 1, device: int = 0) -> List[np.ndarray]:
    """Ragged batch (lists of (h, w, cs) arrays): MaxPool 3x3 s2 p1, or AveragePool k x k stride k ceil_mode count_include_pad=0."""
    xf, hs, ws, xcs = _op_pack(x)
    yf, hs2, ws2, ycs = _op_pack(y)
    want = ((hs - 1) // 2 + 1, (ws - 1) // 2 + 1) if maxpool else (-(-hs // k), -(-ws // k))
    _op_same_batch(want[0], want[1], hs2, ws2, "scrfd_pool")
    _check(lib().ffp_op_scrfd_pool(device, len(hs), _ip(hs), _ip(ws), px_align, c, int(bool(maxpool)), k, _fp(xf), xcs, x_coff, _fp(yf), ycs, y_coff))
    return _op_unpack(yf, hs2, ws2)


def op_scrfd_post(net_hw, A: int, score, bbox, kps, coffs, det_scale, thresh: float, nms_thresh: float, out, strides=(8, 16, 32), px_align: int = 1,
                  raw_scores: bool = False, device: int = 0):
    """score / bbox / kps: per level an (n, h_l, w_l, cs) array (kps None: the 6-output variant) holding A / 4A / 10A values per pixel at
    coffs = (score, bbox, kps offset); scores are logits. out: (n, cap, 21) array to fill. Returns (out, counts[, raw (n, anchors)]):
    counts[i] = faces kept for image i, above cap when the list was cut."""
    net_h, net_w = net_hw
    n = len(det_scale)
    ptrs = (_p(C.c_float) * 9)()
    keep = []
    cs = np.zeros(3, np.int32)
    for kind, lv in enumerate((score, bbox, kps)):
        if lv is None:
            continue
        for l in range(3):
            a = _f32(lv[l])
            if a.shape[:3] != (n, net_h // strides[l], net_w // strides[l]) or (l and a.shape[3] != cs[kind]):
                raise ValueError("scrfd_post: head shapes")
            cs[kind] = a.shape[3]
            keep.append(a)
            ptrs[3 * kind + l] = _fp(a)
    co = np.asarray(list(coffs) + [0] * (3 - len(coffs)), np.int32)
    st = np.asarray(strides, np.int32)
    ds = _f32(det_scale)
    o = _f32(out).copy()
    if o.ndim != 3 or o.shape[0] != n or o.shape[2] != 21:
        raise ValueError("scrfd_post: out must be (n, cap, 21)")
    cnt = np.full(n, -1, np.int32)
    per_img = sum((net_h // s) * (net_w // s) * A for s in strides)
    rs = np.zeros((n, per_img), np.float32) if raw_scores else None
    _check(lib().ffp_op_scrfd_post(device, n, net_h, net_w, A, _ip(st), px_align, ptrs, _ip(cs), _ip(co), _fp(ds), thresh, nms_thresh, o.shape[1], _fp(o),
                                   _ip(cnt), _fp(rs)))
    return (o, cnt, rs) if raw_scores else (o, cnt)


def op_scrfd_sahi_rows(dets: np.ndarray, counts, tiles, full_shape, conf: float, device: int = 0):
    """ffp_op_scrfd_sahi_rows on dets (n, cap, 21) / counts (n) / tiles (n, 4) of a full_shape = (h, w) frame -> (dets, counts, bad): copies
    after the kernel, bad = None or the first (tile, row) whose far corner is negative after the clip (the C entry returns FFP_ERR_ARG there)."""
    d = np.ascontiguousarray(dets, np.float32).copy()
    n, cap = d.shape[0], d.shape[1]
    if d.ndim != 3 or d.shape[2] != FaceDetector.STRIDE:
        raise ValueError(f"dets must be (n, cap, {FaceDetector.STRIDE})")
    c = np.ascontiguousarray(counts, np.int32).copy()
    t = _as_tiles(tiles)
    if c.shape != (n,) or t.shape != (n, 4):
        raise ValueError("counts / tiles do not match dets")
    bad = C.c_int32(-1)
    rc = lib().ffp_op_scrfd_sahi_rows(device, n, cap, _ip(t), int(full_shape[0]), int(full_shape[1]), conf, _fp(d), _ip(c), C.byref(bad))
    if rc != 0 and bad.value < 0:
        _check(rc)
    return d, c, (None if bad.value < 0 else (bad.value // cap, bad.value % cap))


IMAGE_YOLO, IMAGE_RTDETR, IMAGE_SCRFD = 0, 1, 2      # ffp_op_image_input kind


def op_image_input(kind: int, frame: np.ndarray, boxes, size, chan_order: int = CHAN_AS_BGR, precision: int = PREC_F32,
                   device: int = 0) -> List[np.ndarray]:
    """The network image of every box {x0, y0, x1, y1} of an H x W x 3 uint8 frame, as the image-input kernel of `kind` writes it
    (ffp_op_image_input): one (net_h, net_w, 4 or 8) float32 array of whole pixel records per box. size: imgsz, or (det_w, det_h) for
    IMAGE_SCRFD."""
    f, t = _as_frame(frame), _as_tiles(boxes)
    a, b = (int(size[0]), int(size[1])) if kind == IMAGE_SCRFD else (int(size), int(size))
    n = t.shape[0]
    cs = 8 if precision == PREC_F16 and kind != IMAGE_SCRFD else 4
    out = np.zeros((max(n * a * b, 1), cs), np.float32)
    hs, ws = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    _check(lib().ffp_op_image_input(device, kind, precision, _u8p(f), f.shape[0], f.shape[1], chan_order, n, _ip(t), a, b, _fp(out), _ip(hs), _ip(ws)))
    return _op_unpack(out, hs[:n], ws[:n])


def _stem_out_sizes(t: np.ndarray, imgsz: int, stride: int):
    hs, ws = [], []
    for x0, y0, x1, y1 in t.tolist():
        nw, nh, top, bottom, left, right = letterbox_geometry(y1 - y0, x1 - x0, imgsz)
        hs.append((nh + top + bottom - 1) // stride + 1)
        ws.append((nw + left + right - 1) // stride + 1)
    return hs, ws


def op_stem(frame: np.ndarray, boxes, imgsz: int, w, bias, fused: bool, stride: int = 2, act: int = 1, chan_order: int = CHAN_AS_BGR,
            precision: int = PREC_F32, device: int = 0) -> List[np.ndarray]:
    """The image-input 3x3 conv (w (cout, 3, 3, 3), bias (cout,)) on the YOLO letterbox of every box (ffp_op_stem): fused False = the
    letterbox kernel and the direct conv kernel, True = the one kernel that reads the frame. One (ho, wo, cout) float32 array per box."""
    f, t, w, bias = _as_frame(frame), _as_tiles(boxes), _f32(w), _f32(bias)
    if w.ndim != 4 or w.shape[1:] != (3, 3, 3) or bias.shape != (w.shape[0],):
        raise ValueError("stem: w must be (cout, 3, 3, 3) and bias (cout,)")
    n, cout = t.shape[0], int(w.shape[0])
    side = (int(imgsz) - 1) // max(int(stride), 1) + 1
    out = np.zeros((max(n * side * side, 1), cout), np.float32)
    _check(lib().ffp_op_stem(device, precision, int(bool(fused)), _u8p(f), f.shape[0], f.shape[1], chan_order, n, _ip(t), int(imgsz), _fp(w), _fp(bias),
                             cout, int(stride), int(act), _fp(out)))
    return _op_unpack(out, *_stem_out_sizes(t, int(imgsz), int(stride)))


def op_stem_conv(frame: np.ndarray, boxes, imgsz: int, stem_w, stem_b, conv_w, conv_b, chan_order: int = CHAN_AS_BGR, device: int = 0) -> List[np.ndarray]:
    """model.0 inside model.1's loader (ffp_op_stem_conv, PREC_F32X3): stem_w (c, 3, 3, 3) with c 16 or 32, conv_w (2c, c, 3, 3), both stride 2 and
    SiLU. One (net_h / 4, net_w / 4, 2c) float32 array per box."""
    f, t = _as_frame(frame), _as_tiles(boxes)
    sw, sb, cw, cb = _f32(stem_w), _f32(stem_b), _f32(conv_w), _f32(conv_b)
    c = int(sw.shape[0])
    if sw.ndim != 4 or sw.shape[1:] != (3, 3, 3) or sb.shape != (c,) or cw.shape != (2 * c, c, 3, 3) or cb.shape != (2 * c,):
        raise ValueError("stem_conv: stem_w (c, 3, 3, 3), stem_b (c,), conv_w (2c, c, 3, 3), conv_b (2c,)")
    n = t.shape[0]
    side = (int(imgsz) + 3) // 4
    out = np.zeros((max(n * side * side, 1), 2 * c), np.float32)
    _check(lib().ffp_op_stem_conv(device, _u8p(f), f.shape[0], f.shape[1], chan_order, n, _ip(t), int(imgsz), _fp(sw), _fp(sb), c, _fp(cw), _fp(cb),
                                  _fp(out)))
    return _op_unpack(out, *_stem_out_sizes(t, int(imgsz), 4))


def jpeg_encode(img: np.ndarray, quality: int = 95, bgr: bool = False, device: int = 0) -> bytes:
    """Baseline JPEG file (4:2:0, what cv2.imwrite / PIL write at this quality) of an h x w x 3 uint8 image, encoded on the GPU."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    cap = 1024 + h * w * 3
    out = np.empty(cap, np.uint8)
    n = C.c_int64(0)
    _check(lib().ffp_jpeg_encode(device, img.ctypes.data_as(_p(C.c_uint8)), h, w, int(bgr), quality, out.ctypes.data_as(_p(C.c_uint8)), cap, C.byref(n)))
    return out[:n.value].tobytes()


def jpeg_encode_dev(d_ptr: int, h: int, w: int, row_stride: int, quality: int = 95, bgr: bool = True, device: int = 0) -> bytes:
    """Same for an image already in device memory (pointer + row pitch in bytes), e.g. one enhanced crop inside the SR output buffer."""
    cap = 1024 + h * w * 3
    out = np.empty(cap, np.uint8)
    n = C.c_int64(0)
    _check(lib().ffp_jpeg_encode_dev(device, C.c_void_p(d_ptr), h, w, row_stride, int(bgr), quality, out.ctypes.data_as(_p(C.c_uint8)), cap, C.byref(n)))
    return out[:n.value].tobytes()


def jpeg_encode_batch_dev(d_base: int, offsets, hs, ws, quality: int = 95, bgr: bool = True, device: int = 0, strides=None):
    """n device-resident images (d_base + offsets[i], hs[i] x ws[i] x 3, tightly packed rows, or with row pitches of strides[i] bytes: views of one
    frame) -> list of JPEG files, one pass on the GPU."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    hs, ws = np.ascontiguousarray(hs, np.int32), np.ascontiguousarray(ws, np.int32)
    n = len(offsets)
    st = None if strides is None else np.ascontiguousarray(strides, np.int64)
    cap = int(1024 * n + 3 * (hs.astype(np.int64) * ws).sum())
    out = np.empty(max(cap, 1), np.uint8)
    oo = np.zeros(n + 1, np.int64)
    _check(lib().ffp_jpeg_encode_batch_dev(device, C.c_void_p(d_base), n, offsets.ctypes.data_as(_p(C.c_int64)), hs.ctypes.data_as(_p(C.c_int32)),
                                           ws.ctypes.data_as(_p(C.c_int32)), None if st is None else st.ctypes.data_as(_p(C.c_int64)), int(bgr), quality,
                                           out.ctypes.data_as(_p(C.c_uint8)), cap, oo.ctypes.data_as(_p(C.c_int64))))
    return [out[oo[i]:oo[i + 1]].tobytes() for i in range(n)]


OVERLAY_RECT, OVERLAY_STAMP = 0, 1          # include/ffp.h
OVERLAY_MAX_PRIMS = 1 << 20
OVERLAY_PRIM_BYTES = 32


class OverlayPrim(C.Structure):
    """ffp_overlay_prim (include/ffp.h). RECT: corners (x0, y0)..(x1, y1) inclusive, width 0 = fill / >= 1 = frame. STAMP: top-left (x0, y0),
    x1 x y1 the mask's width x height, width its row pitch, mask_off its first byte in the pool."""
    _fields_ = [("kind", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("width", C.c_int32),
                ("mask_off", C.c_int32), ("color", C.c_uint8 * 4)]


OVERLAY_PRIM_DTYPE = np.dtype(OverlayPrim)      # the same 32 bytes as a numpy record: what the primitive builders fill


def _overlay_args(prims, masks):
    prims = np.ascontiguousarray(prims, OVERLAY_PRIM_DTYPE).reshape(-1)
    masks = np.zeros(0, np.uint8) if masks is None else np.ascontiguousarray(masks, np.uint8).reshape(-1)
    return prims, masks, C.c_void_p(prims.ctypes.data if prims.size else None), C.c_void_p(masks.ctypes.data if masks.size else None)


def overlay_draw_dev(d_ptr: int, h: int, w: int, row_stride: int, prims, masks=None, device: int = 0) -> None:
    """Paints `prims` (records of OVERLAY_PRIM_DTYPE, in painter's order) into the h x w x 3 uint8 image in device memory at d_ptr (row pitch
    in bytes, any base alignment), in place (csrc/overlay.hip). masks: the uint8 pool the stamps point into."""
    prims, masks, pp, mp = _overlay_args(prims, masks)
    _check(lib().ffp_overlay_draw_dev(device, C.c_void_p(d_ptr), h, w, row_stride, pp, len(prims), mp, masks.size))


def overlay_draw(img: np.ndarray, prims, masks=None, device: int = 0) -> np.ndarray:
    """The same on a host image (h x w x 3 uint8, rows w*3 bytes apart or further), in place; returns it."""
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.strides[1:] != (3, 1) or img.strides[0] < img.shape[1] * 3 or not img.flags.writeable:
        raise ValueError("overlay_draw: a writeable h x w x 3 uint8 array with contiguous pixels")
    prims, masks, pp, mp = _overlay_args(prims, masks)
    _check(lib().ffp_overlay_draw(device, C.c_void_p(img.ctypes.data), img.shape[0], img.shape[1], img.strides[0], pp, len(prims), mp, masks.size))
    return img


def png_bound(h: int, w: int, channels: int = 3, bit_depth: int = 8) -> int:
    """Worst-case size of the PNG file of an h x w image (every segment stored)."""
    n = lib().ffp_png_bound(h, w, channels, bit_depth)
    if n < 0:
        raise FfpError(1, lib().ffp_last_error().decode("utf-8", "replace"))
    return int(n)


def png_segment_bytes() -> int:
    """Bytes of filtered stream one workgroup compresses on its own (one deflate block, one IDAT chunk)."""
    return int(lib().ffp_png_segment_bytes())


def _png_geometry(img: np.ndarray):
    if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
        raise ValueError(f"png_encode: uint8 or uint16 of shape (H, W), (H, W, 1), (H, W, 3) or (H, W, 4), not {img.dtype} {img.shape}")
    return img.shape[0], img.shape[1], (1 if img.ndim == 2 else img.shape[2]), 8 * img.dtype.itemsize


def png_encode(img: np.ndarray, level: int = 1, bgr: bool = False, device: int = 0, cap: int = None) -> bytes:
    """PNG file of a gray, RGB(A) or BGR(A) uint8 / uint16 image, filtered, compressed and checksummed on the GPU (csrc/png.hip).
    level 0: stored blocks; every level >= 1 is the one device compressor. cap: output capacity, the worst case by default."""
    img = np.ascontiguousarray(img)
    h, w, ch, depth = _png_geometry(img)
    cap = png_bound(h, w, ch, depth) if cap is None else int(cap)
    out = np.empty(max(cap, 1), np.uint8)
    n = C.c_int64(0)
    rc = lib().ffp_png_encode(device, C.c_void_p(img.ctypes.data), h, w, ch, depth, int(bgr), level, out.ctypes.data_as(_p(C.c_uint8)), cap, C.byref(n))
    if rc != 0:
        e = FfpError(rc, lib().ffp_last_error().decode("utf-8", "replace"))
        e.needed = n.value                                   # the size the file has, when the capacity was the trouble
        raise e
    return out[:n.value].tobytes()


def png_encode_dev(d_ptr: int, h: int, w: int, channels: int = 3, bit_depth: int = 8, row_stride: int = None, level: int = 1, bgr: bool = True,
                   device: int = 0) -> bytes:
    """Same for an image already in device memory (pointer + row pitch in bytes): only the file crosses PCIe."""
    if row_stride is None:
        row_stride = w * channels * (bit_depth // 8)
    cap = png_bound(h, w, channels, bit_depth)
    out = np.empty(cap, np.uint8)
    n = C.c_int64(0)
    _check(lib().ffp_png_encode_dev(device, C.c_void_p(d_ptr), h, w, channels, bit_depth, row_stride, int(bgr), level, out.ctypes.data_as(_p(C.c_uint8)), cap,
                                    C.byref(n)))
    return out[:n.value].tobytes()


def png_encode_batch_dev(d_base: int, offsets, hs, ws, channels: int = 3, bit_depth: int = 8, strides=None, level: int = 1, bgr: bool = True, device: int = 0):
    """n device-resident images (d_base + offsets[i] bytes, hs[i] x ws[i], row pitch strides[i] or packed) -> list of PNG files, one pass."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    hs, ws = np.ascontiguousarray(hs, np.int32), np.ascontiguousarray(ws, np.int32)
    n = len(offsets)
    st = None if strides is None else np.ascontiguousarray(strides, np.int64)
    cap = sum(png_bound(int(h), int(w), channels, bit_depth) for h, w in zip(hs, ws))
    out = np.empty(max(cap, 1), np.uint8)
    oo = np.zeros(n + 1, np.int64)
    _check(lib().ffp_png_encode_batch_dev(device, C.c_void_p(d_base), n, offsets.ctypes.data_as(_p(C.c_int64)), hs.ctypes.data_as(_p(C.c_int32)),
                                          ws.ctypes.data_as(_p(C.c_int32)), None if st is None else st.ctypes.data_as(_p(C.c_int64)), channels, bit_depth,
                                          int(bgr), level, out.ctypes.data_as(_p(C.c_uint8)), cap, oo.ctypes.data_as(_p(C.c_int64))))
    return [out[oo[i]:oo[i + 1]].tobytes() for i in range(n)]


def jpeg_info(data: bytes):
    """(height, width, components) from the headers of a JPEG stream."""
    buf = np.frombuffer(data, np.uint8)
    h, w, nc = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(lib().ffp_jpeg_info(buf.ctypes.data_as(_p(C.c_uint8)), len(buf), C.byref(h), C.byref(w), C.byref(nc)))
    return h.value, w.value, nc.value


def _orient_arg(orient) -> int:
    """the `orient` of the decoding entries as the C entries' orientation: True -> 0 (the file's own EXIF tag), 1..8 -> that value"""
    if isinstance(orient, (bool, np.bool_)):
        return 0 if orient else 1
    return int(orient)


def jpeg_decode(data: bytes, bgr: bool = False, device: int = 0, orient=False) -> np.ndarray:
    """JPEG stream -> h x w x 3 uint8 (host Huffman decoding, device IDCT / upsampling / colour conversion), what cv2.imread returns (bgr=True).
    orient: False as stored; True with the file's EXIF orientation applied on the device (the frame cv2.imread returns); 1..8 with that one."""
    h, w, _ = jpeg_info(data)
    buf = np.frombuffer(data, np.uint8)
    out = np.empty((h, w, 3), np.uint8)
    if isinstance(orient, (bool, np.bool_)) and not orient:
        _check(lib().ffp_jpeg_decode(device, buf.ctypes.data_as(_p(C.c_uint8)), len(buf), int(bgr), out.ctypes.data_as(_p(C.c_uint8)), out.size))
        return out
    oh, ow = C.c_int32(0), C.c_int32(0)
    _check(lib().ffp_jpeg_decode_oriented(device, buf.ctypes.data_as(_p(C.c_uint8)), len(buf), int(bgr), _orient_arg(orient), out.ctypes.data_as(_p(C.c_uint8)), out.size,
                                          C.byref(oh), C.byref(ow)))
    return out.reshape(oh.value, ow.value, 3)


def jpeg_decode_dev(data: bytes, d_ptr: int, row_stride: int, cap: int, bgr: bool = True, device: int = 0, orient=False):
    """Same into device memory (pointer, row pitch and capacity in bytes); returns (h, w). orient as in jpeg_decode: the pitch, the capacity and the
    returned size are then the oriented image's."""
    buf = np.frombuffer(data, np.uint8)
    if isinstance(orient, (bool, np.bool_)) and not orient:
        h, w, _ = jpeg_info(data)
        _check(lib().ffp_jpeg_decode_dev(device, buf.ctypes.data_as(_p(C.c_uint8)), len(buf), int(bgr), C.c_void_p(d_ptr), row_stride, cap))
        return h, w
    oh, ow = C.c_int32(0), C.c_int32(0)
    _check(lib().ffp_jpeg_decode_oriented_dev(device, buf.ctypes.data_as(_p(C.c_uint8)), len(buf), int(bgr), _orient_arg(orient), C.c_void_p(d_ptr), row_stride, cap,
                                              C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def exif_orientation(data: bytes) -> int:
    """The EXIF orientation of a JPEG or PNG file from its bytes (csrc/exif.hpp): 1..8, 1 for everything that is not a well-formed tag. No device."""
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    o = C.c_int32(0)
    _check(lib().ffp_exif_orientation(buf.ctypes.data_as(_p(C.c_uint8)), len(data), C.byref(o)))
    return o.value


def image_orient_geometry() -> int:
    """pixels along the side of the tile one workgroup of the orient kernel moves: test hook"""
    t = C.c_int32(0)
    _check(lib().ffp_image_orient_geometry(C.byref(t)))
    return t.value


def image_orient_stats():
    """(images turned, orient launches) since load"""
    a, b = C.c_int64(0), C.c_int64(0)
    _check(lib().ffp_image_orient_stats(C.byref(a), C.byref(b)))
    return a.value, b.value


def image_orient_dev(d_src: int, h: int, w: int, px: int, src_stride: int, orientation: int, d_dst: int, dst_stride: int, cap: int, device: int = 0):
    """The h x w image of px (1, 3, 4) bytes per pixel at device pointer d_src (row pitch in bytes) into d_dst with EXIF orientation 1..8, out of
    place (csrc/orient.hip); cap: the bytes there are from d_dst on. Returns the destination's (h, w): (w, h) for 5..8."""
    _check(lib().ffp_image_orient_dev(device, C.c_void_p(d_src), h, w, px, src_stride, orientation, C.c_void_p(d_dst), dst_stride, cap))
    return (w, h) if orientation >= 5 else (h, w)


def image_orient_time_dev(d_src: int, h: int, w: int, px: int, orientation: int, d_dst: int, cap: int, iters: int = 400, device: int = 0):
    """(microseconds per orient launch, microseconds per device-to-device copy of the same bytes), each over `iters` runs between two events; both
    images packed (tools/orient_probe.py)."""
    k, c = C.c_float(0), C.c_float(0)
    _check(lib().ffp_image_orient_time_dev(device, C.c_void_p(d_src), h, w, px, orientation, C.c_void_p(d_dst), cap, iters, C.byref(k), C.byref(c)))
    return k.value, c.value


def image_orient_batch_dev(d_src_base: int, src_offsets, hs, ws, px: int, src_strides, orientations, d_dst_base: int, dst_offsets, dst_strides, cap: int,
                           device: int = 0) -> None:
    """n images in ONE launch: image i is hs[i] x ws[i] at d_src_base + src_offsets[i] and goes to d_dst_base + dst_offsets[i] with orientations[i];
    cap: the bytes there are from d_dst_base on."""
    i64 = lambda a: np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1))
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
    so, do, ss, ds_, hh, ww, oo = i64(src_offsets), i64(dst_offsets), i64(src_strides), i64(dst_strides), i32(hs), i32(ws), i32(orientations)
    n = len(so)
    if not all(len(a) == n for a in (do, ss, ds_, hh, ww, oo)):
        raise ValueError("image_orient_batch_dev: one entry per image in every table")
    p64 = lambda a: a.ctypes.data_as(_p(C.c_int64))
    p32 = lambda a: a.ctypes.data_as(_p(C.c_int32))
    _check(lib().ffp_image_orient_batch_dev(device, n, C.c_void_p(d_src_base), p64(so), p32(hh), p32(ww), px, p64(ss), p32(oo), C.c_void_p(d_dst_base), p64(do), p64(ds_), cap))


def image_orient(img: np.ndarray, orientation: int, device: int = 0) -> np.ndarray:
    """The same on a host image (h x w or h x w x {1, 3, 4} uint8, rows of any pitch): up, turned on the device, down."""
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or img.size == 0:
        raise ValueError("image_orient: an h x w or h x w x c uint8 array")
    h, w = img.shape[:2]
    px = img.shape[2] if img.ndim == 3 else 1
    if (img.ndim == 3 and px > 1 and img.strides[2] != 1) or (w > 1 and img.strides[1] != px) or (h > 1 and img.strides[0] < w * px):
        raise ValueError("image_orient: pixels contiguous in memory, rows at a pitch of at least a row")
    out = np.empty((w, h) + img.shape[2:] if 5 <= orientation <= 8 else img.shape, np.uint8)
    _check(lib().ffp_image_orient(device, C.c_void_p(img.ctypes.data), h, w, px, img.strides[0] if h > 1 else w * px, orientation, C.c_void_p(out.ctypes.data),
                                  out.strides[0], out.nbytes))
    return out


def _file_table(datas):
    """n byte strings as the (pointer array, sizes, keep-alive list) the batch entries take"""
    bufs = [np.frombuffer(bytes(d), np.uint8) if len(d) else np.zeros(0, np.uint8) for d in datas]
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data if b.size else None for b in bufs])
    sizes = np.asarray([b.size for b in bufs], np.int64).reshape(-1)
    return ptrs, sizes, bufs


def jpeg_decode_batch_dev(datas, d_base: int, offsets, strides, cap: int, bgr: bool = True, device: int = 0, orientations=None):
    """n JPEG streams -> n images in device memory in ONE pass (ffp_jpeg_decode_batch_dev): image i at d_base + offsets[i], row pitch strides[i]
    (None: packed). Returns (hs, ws, status) as int32 arrays; status 0: decoded on the device, 1: by the host decoder, < 0: minus the error code
    of a file that was not decoded (its region is untouched). orientations: None as stored; True every file's own EXIF orientation; or one value
    per file, 0 the file's own and 1..8 that one — applied on the device, and the pitches, the capacity, hs and ws are then the oriented images'."""
    n = len(datas)
    ptrs, sizes, keep = _file_table(datas)
    offsets = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
    if len(offsets) != n:
        raise ValueError("jpeg_decode_batch_dev: one offset per file")
    st = None if strides is None else np.ascontiguousarray(np.asarray(strides, np.int64).reshape(-1))
    if st is not None and len(st) != n:
        raise ValueError("jpeg_decode_batch_dev: one row pitch per file")
    hs, ws, status = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    i64 = lambda a: a.ctypes.data_as(_p(C.c_int64))
    i32 = lambda a: a.ctypes.data_as(_p(C.c_int32))
    if orientations is None:
        _check(lib().ffp_jpeg_decode_batch_dev(device, n, ptrs, i64(np.ascontiguousarray(sizes)) if n else i64(np.zeros(1, np.int64)), int(bgr), C.c_void_p(d_base),
                                               i64(offsets) if n else i64(np.zeros(1, np.int64)), None if st is None else i64(st), cap, i32(hs), i32(ws), i32(status)))
    else:
        oo = None if orientations is True else np.ascontiguousarray(np.asarray(orientations, np.int32).reshape(-1))
        if oo is not None and len(oo) != n:
            raise ValueError("jpeg_decode_batch_dev: one orientation per file")
        _check(lib().ffp_jpeg_decode_batch_oriented_dev(device, n, ptrs, i64(np.ascontiguousarray(sizes)) if n else i64(np.zeros(1, np.int64)), int(bgr),
                                                        None if oo is None or n == 0 else i32(oo), C.c_void_p(d_base), i64(offsets) if n else i64(np.zeros(1, np.int64)),
                                                        None if st is None else i64(st), cap, i32(hs), i32(ws), i32(status)))
    del keep
    return hs[:n], ws[:n], status[:n]


def jpeg_decode_batch(datas, bgr: bool = False, device: int = 0):
    """n JPEG streams in ONE pass -> a list with, per file, the h x w x 3 uint8 array or the FfpError that says why it was not decoded."""
    n = len(datas)
    if n == 0:
        _check(lib().ffp_jpeg_decode_batch(device, 0, None, None, int(bgr), None, None, None, None, None))
        return []
    ptrs, sizes, keep = _file_table(datas)
    res, outs = [], []
    for d in datas:
        try:
            h, w, _ = jpeg_info(d)
            outs.append(np.empty((h, w, 3), np.uint8))
        except FfpError:
            outs.append(np.empty((0, 0, 3), np.uint8))
    optrs = (C.c_void_p * n)(*[o.ctypes.data if o.size else None for o in outs])
    caps = np.asarray([o.size for o in outs], np.int64)
    hs, ws, status = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(lib().ffp_jpeg_decode_batch(device, n, ptrs, sizes.ctypes.data_as(_p(C.c_int64)), int(bgr), optrs, caps.ctypes.data_as(_p(C.c_int64)),
                                       hs.ctypes.data_as(_p(C.c_int32)), ws.ctypes.data_as(_p(C.c_int32)), status.ctypes.data_as(_p(C.c_int32))))
    for i in range(n):
        if status[i] >= 0:
            res.append(outs[i])
        else:
            try:                                   # the file's own message: what the single-file call says about it
                jpeg_info(datas[i])
                res.append(FfpError(int(-status[i]), f"jpeg_decode_batch: file {i} was not decoded"))
            except FfpError as e:
                res.append(e)
    del keep
    return res


def jpeg_decode_batch_stats():
    """(batches since load, kernel launches of the latest batch, stream synchronisations of the latest batch)"""
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _check(lib().ffp_jpeg_decode_batch_stats(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def jpeg_decode_stats():
    """(files Huffman-decoded on the device, files that fell back to the host decoder, extra synchronisation rounds) since load"""
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _check(lib().ffp_jpeg_decode_stats(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


FFP_ERR_ARG = 1              # include/ffp.h
FFP_PNG_DEC_SERIAL = 1


def png_info(data: bytes):
    """(height, width, channels, bit depth) from the IHDR of a PNG file; FfpError(FFP_ERR_ARG) names the field of a file that is not decoded
    (palette, sub-byte depth, gray with alpha, interlace). No device."""
    buf = np.frombuffer(data, np.uint8)
    h, w, ch, bd = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(lib().ffp_png_info(buf.ctypes.data_as(_p(C.c_uint8)), len(buf), C.byref(h), C.byref(w), C.byref(ch), C.byref(bd)))
    return h.value, w.value, ch.value, bd.value


def png_decode(data: bytes, bgr: bool = False, flags: int = 0, device: int = 0) -> np.ndarray:
    """PNG file -> (h, w) or (h, w, channels) uint8 / uint16, what cv2.imread(path, IMREAD_UNCHANGED) gives (bgr=True). A file whose IDAT chunks
    inflate one by one (every file png_encode writes) is inflated on the GPU, one wavefront per chunk; others on the host (csrc/png_dec.hip).
    flags=FFP_PNG_DEC_SERIAL: the host inflate for every file."""
    h, w, ch, bd = png_info(data)
    buf = np.frombuffer(data, np.uint8)
    out = np.empty((h, w, ch), np.uint8 if bd == 8 else np.uint16)
    _check(lib().ffp_png_decode(device, buf.ctypes.data_as(_p(C.c_uint8)), len(buf), int(bgr), int(flags), C.c_void_p(out.ctypes.data), out.nbytes))
    return out[..., 0] if ch == 1 else out


def png_decode_dev(data: bytes, d_ptr: int, row_stride: int, cap: int, bgr: bool = True, flags: int = 0, device: int = 0):
    """Same into device memory (pointer, row pitch and capacity in bytes; pitch 0 = packed rows); returns (h, w, channels, bit depth)."""
    info = png_info(data)
    buf = np.frombuffer(data, np.uint8)
    _check(lib().ffp_png_decode_dev(device, buf.ctypes.data_as(_p(C.c_uint8)), len(buf), int(bgr), int(flags), C.c_void_p(d_ptr), row_stride, cap))
    return info


def png_decode_stats():
    """(files inflated on the device, files inflated on the host) since load"""
    a, b = C.c_int64(0), C.c_int64(0)
    _check(lib().ffp_png_decode_stats(C.byref(a), C.byref(b)))
    return a.value, b.value


def png_unfilter_geometry():
    """(rows one workgroup pass of the unfilter kernel covers, pixels of one of its steps): test hook"""
    r, c = C.c_int32(0), C.c_int32(0)
    _check(lib().ffp_png_unfilter_geometry(C.byref(r), C.byref(c)))
    return r.value, c.value


def _png_has_trns(data: bytes) -> bool:
    """a tRNS chunk among the chunks in front of the first IDAT (where the format puts it): a walk by chunk lengths, not a byte search"""
    pos = 8
    while pos + 12 <= len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        typ = data[pos + 4:pos + 8]
        if typ == b"tRNS":
            return True
        if typ in (b"IDAT", b"IEND"):
            return False
        pos += 12 + n
    return False


def png_read_rgb8(data: bytes, bgr: bool):
    """What np.asarray(Image.open(...).convert("RGB")) gives ([..., ::-1] of it when bgr) for an 8-bit gray, RGB or RGBA file, decoded by png_decode: gray
    replicated to three channels, alpha dropped. Both routes of the decoder beat Pillow on every measured frame (profiles/png_decode_mi355x.json), so every
    such file comes here. None when the file stays with Pillow: 16-bit, a geometry png_info refuses, a tRNS chunk, or any error of the decoder."""
    try:
        _, _, ch, depth = png_info(data)
        if depth != 8 or _png_has_trns(data):
            return None
        a = png_decode(data, bgr=bgr)
    except Exception:        # noqa: BLE001 — Pillow decides, and reports what is wrong with the file
        return None
    if ch == 1:
        return np.repeat(a[..., None], 3, axis=2)
    return np.ascontiguousarray(a[..., :3]) if ch == 4 else a


def _ragged(rows, width, dtype):
    """list of [n_i][width] arrays -> (contiguous [sum n][width], int64 offsets [len + 1])"""
    rows = [np.asarray(r, dtype).reshape(-1, width) for r in rows]
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    flat = np.ascontiguousarray(np.concatenate(rows + [np.zeros((0, width), dtype)], 0))
    return flat, off


def eval_wider_pr(preds, gts, evaluate, iou_thr: float = 0.5, thresh_num: int = 1000, device: int = 0) -> np.ndarray:
    """Official WIDER FACE protocol on the device (ffp_eval_wider_pr): per-image lists preds [N_i][5] (x, y, w, h, score), gts [G_i][4],
    evaluate [G_i] (1 = evaluated face). -> int64 [thresh_num][2] = {valid proposals, matched faces} per score threshold."""
    p, po = _ragged(preds, 5, np.float64)
    g, go = _ragged(gts, 4, np.float64)
    e, eo = _ragged([np.asarray(x, np.uint8).reshape(-1, 1) for x in evaluate], 1, np.uint8)
    if len(po) != len(go) or not np.array_equal(go, eo):
        raise ValueError("preds / gts / evaluate must describe the same images and faces")
    out = np.zeros((thresh_num, 2), np.int64)
    _check(lib().ffp_eval_wider_pr(device, p.ctypes.data_as(_p(C.c_double)), po.ctypes.data_as(_p(C.c_int64)), g.ctypes.data_as(_p(C.c_double)),
                                   go.ctypes.data_as(_p(C.c_int64)), e.ctypes.data_as(_p(C.c_uint8)), len(po) - 1, iou_thr, thresh_num,
                                   out.ctypes.data_as(_p(C.c_int64))))
    return out


def eval_dual_match(preds, faces, valid, iou_thr: float = 0.5, device: int = 0):
    """Dual-protocol matching on the device (ffp_eval_dual_match). -> list of int32 flag arrays per image (1 TP, 0 FP, 2 not counted)."""
    p, po = _ragged(preds, 5, np.float64)
    f, fo = _ragged(faces, 4, np.float64)
    v, vo = _ragged([np.asarray(x, np.uint8).reshape(-1, 1) for x in valid], 1, np.uint8)
    if len(po) != len(fo) or not np.array_equal(fo, vo):
        raise ValueError("preds / faces / valid must describe the same images and faces")
    flags = np.zeros(max(int(po[-1]), 1), np.int32)
    _check(lib().ffp_eval_dual_match(device, p.ctypes.data_as(_p(C.c_double)), po.ctypes.data_as(_p(C.c_int64)), f.ctypes.data_as(_p(C.c_double)),
                                     fo.ctypes.data_as(_p(C.c_int64)), v.ctypes.data_as(_p(C.c_uint8)), len(po) - 1, iou_thr, flags.ctypes.data_as(_p(C.c_int32))))
    return [flags[po[i]:po[i + 1]] for i in range(len(po) - 1)]


def eval_coco_bbox(dets, det_off, gts, gt_off, n_img: int, n_cat: int, iou_thrs, rec_thrs, area_rng, max_dets, matches: bool = False,
                   device: int = 0) -> dict:
    """pycocotools COCOeval (bbox) evaluate + accumulate on the device (ffp_eval_coco_bbox). dets [sum D][7] = x, y, w, h, score, area, id and
    gts [sum G][8] = x, y, w, h, area, iscrowd, ignore, id, ragged per unit by the int64 offsets det_off / gt_off [n_cat * n_img + 1]
    (category-major, images in sorted id order). -> dict of numpy arrays: precision / scores [T,R,K,A,M], recall [T,K,A,M] and, with
    matches=True, dt_matches / dt_ignore [A,T,ndc], gt_matches [A,T,ng], gt_ignore [A,ng] plus cut_off [U+1] (see include/ffp.h)."""
    d = np.ascontiguousarray(np.asarray(dets, np.float64).reshape(-1, 7))
    g = np.ascontiguousarray(np.asarray(gts, np.float64).reshape(-1, 8))
    do = np.ascontiguousarray(det_off, np.int64)
    go = np.ascontiguousarray(gt_off, np.int64)
    it = np.ascontiguousarray(iou_thrs, np.float64).reshape(-1)
    rt = np.ascontiguousarray(rec_thrs, np.float64).reshape(-1)
    ar = np.ascontiguousarray(area_rng, np.float64).reshape(-1, 2)
    md = np.ascontiguousarray(max_dets, np.int32).reshape(-1)
    U = int(n_img) * int(n_cat)
    if len(do) != U + 1 or len(go) != U + 1:
        raise ValueError(f"offsets must have n_cat * n_img + 1 = {U + 1} entries")
    T, R, K, A, M = len(it), len(rt), int(n_cat), len(ar), len(md)
    prec, sc = np.zeros((T, R, K, A, M)), np.zeros((T, R, K, A, M))
    rec = np.zeros((T, K, A, M))
    out = {"precision": prec, "recall": rec, "scores": sc}
    ptrs = [None] * 4
    if matches:
        cut = np.zeros(U + 1, np.int64)
        if U and len(md):
            np.cumsum(np.minimum(np.diff(do), int(md[-1])), out=cut[1:])
        ndc, ng = int(cut[-1]), int(go[-1]) if U else 0
        out.update(cut_off=cut, dt_matches=np.zeros((A, T, ndc)), dt_ignore=np.zeros((A, T, ndc), np.uint8), gt_matches=np.zeros((A, T, ng)),
                   gt_ignore=np.zeros((A, ng), np.uint8))
        ptrs = [out["dt_matches"].ctypes.data_as(_p(C.c_double)), out["dt_ignore"].ctypes.data_as(_p(C.c_uint8)),
                out["gt_matches"].ctypes.data_as(_p(C.c_double)), out["gt_ignore"].ctypes.data_as(_p(C.c_uint8))]
    dp = lambda a: a.ctypes.data_as(_p(C.c_double))
    _check(lib().ffp_eval_coco_bbox(device, int(n_img), int(n_cat), dp(d), do.ctypes.data_as(_p(C.c_int64)), dp(g), go.ctypes.data_as(_p(C.c_int64)),
                                    dp(it), T, dp(rt), R, dp(ar), A, md.ctypes.data_as(_p(C.c_int32)), M, dp(prec), dp(rec), dp(sc), *ptrs))
    return out


def op_conv1x1_up2(coarse: np.ndarray, fine: np.ndarray, w: np.ndarray, b: np.ndarray, act: int = 0, precision: int = PREC_F32X3, device: int = 0) -> np.ndarray:
    """1x1 conv over the virtual concat [nearest_x2(coarse) | fine]; coarse (n,h/2,w/2,c_up), fine (n,h,w,c_fine), w (cout, c_up+c_fine)."""
    coarse = np.ascontiguousarray(coarse, np.float32)
    fine = np.ascontiguousarray(fine, np.float32)
    w = np.ascontiguousarray(w, np.float32).reshape(w.shape[0], -1)
    b = np.ascontiguousarray(b, np.float32)
    n, h, wd, cf = fine.shape
    y = np.zeros((n, h, wd, w.shape[0]), np.float32)
    _check(lib().ffp_op_conv1x1_up2(device, precision, _fp(coarse), _fp(fine), n, h, wd, coarse.shape[3], cf, _fp(w), _fp(b), w.shape[0], act, _fp(y)))
    return y


def op_resize_lanczos4(img: np.ndarray, out_h: int, out_w: int, device: int = 0) -> np.ndarray:
    """cv2.resize(img, (out_w, out_h), interpolation=INTER_LANCZOS4) through the HIP kernel (ffp_op_resize_lanczos4).
    img: HxW, HxWx3 or HxWx4, uint8 or uint16; the result has the same type and channels."""
    a = np.ascontiguousarray(img)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3):
        raise ValueError(f"expected an HxW or HxWxC uint8 / uint16 array, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    out = np.zeros((int(out_h), int(out_w)) + a.shape[2:], a.dtype)
    _check(lib().ffp_op_resize_lanczos4(device, a.ctypes.data, h, w, 1 if a.ndim == 2 else a.shape[2], 8 * a.itemsize, int(out_h), int(out_w),
                                        out.ctypes.data))
    return out


SR_SEL_BGR, SR_SEL_GRAY, SR_SEL_ALPHA = 0, 1, 2      # channel selection of an image of the ffp_op_sr_* entries


def _sr_images(images) -> np.ndarray:
    """Images of the ffp_op_sr_* entries: rows (byte offset, bytes per row, h, w, channels, bits, range, selection) as int64."""
    a = np.ascontiguousarray(np.asarray(images, np.int64).reshape(-1, 8))
    return a


def op_sr_tiles(images, scale: int, tile: int = 0, tile_pad: int = 10, pre_pad: int = 0, precision: int = PREC_F32):
    """The padded tiles the enhancer cuts a batch into (ffp_op_sr_tiles, no device): ([(h, w), ...] in tile order, 16x16 body tiles,
    channels of the network's input record in `precision`)."""
    im = _sr_images(images)
    cap = 1 << 16
    hw = np.zeros((cap, 2), np.int32)
    n, t16, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(lib().ffp_op_sr_tiles(im.shape[0], _i64p(im), scale, tile, tile_pad, pre_pad, precision, cap, _ip(hw), C.byref(n), C.byref(t16), C.byref(ch)))
    return [(int(h), int(w)) for h, w in hw[:n.value]], t16.value, ch.value


def op_sr_pre(buf: np.ndarray, images, scale: int, tile: int = 0, tile_pad: int = 10, pre_pad: int = 0, precision: int = PREC_F32, fill=None,
              cap_t16: int = 0, first=None, device: int = 0):
    """The enhancer's input kernel alone (ffp_op_sr_pre) on the images described inside the uint8 buffer `buf`: (per-tile arrays
    (h/f, w/f, channels) float32, the level's whole flat buffer (records, channels), first record of every tile). fill: the flat buffer's
    contents going in (scalar or array); cap_t16 > 0: a capacity-mode level, with `first` (images of an earlier batch) run before."""
    b = np.ascontiguousarray(buf, np.uint8).reshape(-1)
    im = _sr_images(images)
    tiles, _, ch = op_sr_tiles(im, scale, tile, tile_pad, pre_pad, precision)
    f = 2 if scale == 2 else 1
    sizes = [(h // f, w // f) for h, w in tiles]
    npx = 256 * cap_t16 if cap_t16 > 0 else sum(h * w for h, w in sizes)
    flat = np.empty((npx, ch), np.float32)
    flat[...] = 0.0 if fill is None else fill
    offs = np.zeros(max(len(tiles), 1), np.int64)
    im1 = _sr_images(first) if first is not None else np.zeros((0, 8), np.int64)
    _check(lib().ffp_op_sr_pre(device, precision, b.ctypes.data, b.size, im.shape[0], _i64p(im), scale, tile, tile_pad, pre_pad, cap_t16, im1.shape[0],
                               _i64p(im1) if im1.shape[0] else None, flat.ctypes.data, npx, _i64p(offs)))
    out = [flat[o:o + h * w].reshape(h, w, ch).copy() for o, (h, w) in zip(offs.tolist(), sizes)]
    return out, flat, offs[:len(tiles)].copy()


def _sr_net_records(nets, cs: int) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([np.asarray(t, np.float32).reshape(-1, cs) for t in nets], axis=0))


def op_sr_post(canvas: np.ndarray, images, nets, scale: int, tile: int = 0, tile_pad: int = 10, pre_pad: int = 0, cap_t16: int = 0, first=None,
               only_tile: int = -1, device: int = 0) -> np.ndarray:
    """The enhancer's output kernel alone (ffp_op_sr_post): `canvas` (uint8 bytes, returned as a new array) holds the canvases `images`
    describe (h, w: the input size); nets: every tile's network output (scale * h, scale * w, cs >= 3) float32 in tile order. cap_t16 > 0:
    capacity-mode level and tables; first = (images, nets) of an earlier batch run before; only_tile >= 0: every other tile's core is emptied."""
    out = np.ascontiguousarray(canvas, np.uint8).reshape(-1).copy()
    im = _sr_images(images)
    cs = int(np.asarray(nets[0]).shape[-1])
    net = _sr_net_records(nets, cs)
    im1, net1 = (np.zeros((0, 8), np.int64), None) if first is None else (_sr_images(first[0]), _sr_net_records(first[1], cs))
    _check(lib().ffp_op_sr_post(device, im.shape[0], _i64p(im), scale, tile, tile_pad, pre_pad, net.ctypes.data, cs, cap_t16, im1.shape[0],
                                _i64p(im1) if im1.shape[0] else None, net1.ctypes.data if net1 is not None else None, int(only_tile), out.ctypes.data, out.size))
    return out


def op_alpha_linear(src: np.ndarray, dst: np.ndarray, max_range: int, device: int = 0) -> np.ndarray:
    """The 'cv2' alpha upsampler alone (ffp_op_alpha_linear): src HxWx4 uint8 / uint16, dst (out_h, out_w, 4) uint8 / uint16 going in;
    returns dst with channel 3 = rint(resize_linear(src[..., 3] / max_range) * max_range)."""
    s, d = np.ascontiguousarray(src), np.ascontiguousarray(dst).copy()
    if s.dtype not in (np.uint8, np.uint16) or d.dtype not in (np.uint8, np.uint16) or s.ndim != 3 or d.ndim != 3 or s.shape[2] != 4 or d.shape[2] != 4:
        raise ValueError("expected HxWx4 uint8 / uint16 arrays")
    _check(lib().ffp_op_alpha_linear(device, s.ctypes.data, s.shape[0], s.shape[1], 8 * s.itemsize, int(max_range), d.shape[0], d.shape[1],
                                     8 * d.itemsize, d.ctypes.data))
    return d


def op_crop_gather(frame: np.ndarray, boxes_xywh, offs, out: np.ndarray, device: int = 0) -> np.ndarray:
    """The crop gather alone (ffp_op_crop_gather): box i (x0, y0, w, h) of an HxWx3 uint8 frame -> w * h * 3 bytes at offs[i] of a copy of `out`."""
    f = _as_frame(frame)
    b = np.ascontiguousarray(np.asarray(boxes_xywh, np.int32).reshape(-1, 4))
    o = np.ascontiguousarray(np.asarray(offs, np.int64).reshape(-1))
    if o.size != b.shape[0]:
        raise ValueError("one offset per box")
    res = np.ascontiguousarray(out, np.uint8).reshape(-1).copy()
    _check(lib().ffp_op_crop_gather(device, f.ctypes.data, f.shape[0], f.shape[1], b.shape[0], _ip(b) if b.shape[0] else None,
                                    _i64p(o) if o.size else None, res.ctypes.data, res.size))
    return res


def op_conv2d_shape(shape: int = -1) -> None:
    """Pin the workgroup shape of the following op_conv2d calls (tests of one kernel variant); -1 restores the automatic choice."""
    _check(lib().ffp_op_conv2d_shape(int(shape)))


def op_conv2d_shape_name(shape: int) -> str:
    """'<family> <variant suffix>' of a shape number (the table in csrc/conv_route.cpp); FfpError code 1 for a number that is no shape. No device."""
    out = C.create_string_buffer(64)
    _check(lib().ffp_op_conv2d_shape_name(int(shape), out, len(out)))
    return out.value.decode()


def op_conv2d_last_variant() -> str:
    """Variant string of the op the last op_conv2d / op_conv1x1_up2 call of this thread launched ('' if it launched no dense conv)."""
    out = C.create_string_buffer(64)
    _check(lib().ffp_op_conv2d_last_variant(out, len(out)))
    return out.value.decode()


def op_conv2d_act_post(act: int = 0) -> None:
    """Activation the following op_conv2d calls apply after the residual term (epilogue contract tests); 0 restores none."""
    _check(lib().ffp_op_conv2d_act_post(int(act)))


def op_conv2d_time(n, h, w, cin, cout, k=3, stride=1, up=False, precision=PREC_F16, iters=50, dbg=0, shape=-1, device=0) -> float:
    """Tuning hook: mean microseconds per launch of one dense conv on synthetic data (see ffp_op_conv2d_time)."""
    us = C.c_float(0)
    _check(lib().ffp_op_conv2d_time(device, precision, n, h, w, cin, cout, k, stride, int(up), iters, dbg, shape, C.byref(us)))
    return us.value


def niqe_blocks(h: int, w: int) -> int:
    """96x96 blocks of an h x w image (host)."""
    n = C.c_int64(0)
    _check(lib().ffp_iqa_niqe_blocks(int(h), int(w), C.byref(n)))
    return n.value


def niqe_score(feat: np.ndarray, block_off: np.ndarray, mu: np.ndarray, cov: np.ndarray) -> np.ndarray:
    """ffp_iqa_niqe_score (host, float64): one score per image from [blocks, 36] features and the pristine model."""
    f = np.ascontiguousarray(feat, np.float64).reshape(-1, NIQE_FEATURES)
    off = np.ascontiguousarray(block_off, np.int64)
    m = np.ascontiguousarray(np.asarray(mu, np.float64).reshape(-1))
    c = np.ascontiguousarray(cov, np.float64)
    if m.shape != (NIQE_FEATURES,) or c.shape != (NIQE_FEATURES, NIQE_FEATURES):
        raise ValueError(f"the NIQE model is a 36-vector and a 36x36 matrix, got {m.shape} and {c.shape}")
    if off.ndim != 1 or off.size < 1 or off[-1] != f.shape[0]:
        raise ValueError("block offsets do not match the feature rows")
    out = np.zeros(off.size - 1, np.float64)
    dp = _p(C.c_double)
    _check(lib().ffp_iqa_niqe_score(f.ctypes.data_as(dp), off.ctypes.data_as(_p(C.c_int64)), off.size - 1, m.ctypes.data_as(dp), c.ctypes.data_as(dp),
                                    out.ctypes.data_as(dp)))
    return out


class IQA(_Handle):
    """No-reference image quality on one GPU (ffp_iqa_*): NIQE block features on the device, the score in float64 on the host."""

    _DESTROY = "ffp_iqa_destroy"

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        self.device = device
        _check(lib().ffp_iqa_create(device, C.byref(self._h)))

    def niqe_features(self, images: Sequence[np.ndarray], chan_order: int = CHAN_AS_RGB) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """A ragged batch, all images in one form: float32 planar (C, H, W) or (H, W) in [0,1] (RGB), or uint8 (H, W, C) or (H, W) in
        `chan_order`; C is 1 or 3. Returns features [blocks, 36] float64, per-block sharpness [blocks] and block offsets [n + 1]."""
        ims = [np.ascontiguousarray(i) for i in images]
        if not ims:
            raise ValueError("no images")
        kinds = {i.dtype == np.uint8 for i in ims}
        if len(kinds) != 1 or any(i.dtype not in (np.uint8, np.float32) for i in ims):
            raise ValueError("images must be all uint8 (H, W, C) or all float32 (C, H, W)")
        u8 = ims[0].dtype == np.uint8
        shp = []
        for i in ims:
            if i.ndim == 2:
                shp.append((i.shape[0], i.shape[1], 1))
            elif i.ndim == 3:
                shp.append((i.shape[0], i.shape[1], i.shape[2]) if u8 else (i.shape[1], i.shape[2], i.shape[0]))
            else:
                raise ValueError(f"expected a 2-d or 3-d image, got shape {i.shape}")
        return self._features([i.ctypes.data for i in ims], shp, IQA_U8_HWC if u8 else IQA_F32_CHW, chan_order, False)

    def luma(self, image: np.ndarray, chan_order: int = CHAN_AS_RGB) -> np.ndarray:
        """The rounded luma of one image's crop (ffp_iqa_niqe_luma): float32 holding integers 0..255."""
        a = np.ascontiguousarray(image)
        u8 = a.dtype == np.uint8
        if a.dtype not in (np.uint8, np.float32) or a.ndim not in (2, 3):
            raise ValueError(f"expected a uint8 (H, W, C) or float32 (C, H, W) image, got {a.dtype} {a.shape}")
        h, w, c = (a.shape[0], a.shape[1], 1) if a.ndim == 2 else ((a.shape[0], a.shape[1], a.shape[2]) if u8 else (a.shape[1], a.shape[2], a.shape[0]))
        out = np.zeros((max(h // 96 * 96, 1), max(w // 96 * 96, 1)), np.float32)
        _check(lib().ffp_iqa_niqe_luma(self._h, a.ctypes.data, h, w, c, IQA_U8_HWC if u8 else IQA_F32_CHW, int(chan_order), _fp(out)))
        return out

    def niqe_features_dev(self, ptrs: Sequence[int], shapes: Sequence[Tuple[int, int, int]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The same for float32 planar images already in device memory: pointers and (C, H, W) per image; the caller has synchronised."""
        return self._features(list(ptrs), [(h, w, c) for c, h, w in shapes], IQA_F32_CHW, CHAN_AS_RGB, True)

    def _features(self, ptrs, shp, layout, chan_order, on_device):
        n = len(ptrs)
        hs = np.asarray([s[0] for s in shp], np.int32)
        ws = np.asarray([s[1] for s in shp], np.int32)
        cs = np.asarray([s[2] for s in shp], np.int32)
        nb = max(1, sum((int(h) // 96) * (int(w) // 96) for h, w in zip(hs, ws)))
        feat = np.zeros((nb, NIQE_FEATURES), np.float64)
        sharp = np.zeros(nb, np.float64)
        off = np.zeros(n + 1, np.int64)
        ip = (C.c_void_p * n)(*ptrs)
        _check(lib().ffp_iqa_niqe_features(self._h, n, ip, _ip(hs), _ip(ws), _ip(cs), layout, int(chan_order), int(on_device),
                                           feat.ctypes.data_as(_p(C.c_double)), sharp.ctypes.data_as(_p(C.c_double)), nb, off.ctypes.data_as(_p(C.c_int64))))
        return feat[:off[-1]], sharp[:off[-1]], off

    def niqe(self, images: Sequence[np.ndarray], mu: np.ndarray, cov: np.ndarray, chan_order: int = CHAN_AS_RGB) -> np.ndarray:
        """One NIQE score (float64, lower is better) per image against the pristine model (mu [36], cov [36, 36])."""
        feat, _, off = self.niqe_features(images, chan_order)
        return niqe_score(feat, off, mu, cov)

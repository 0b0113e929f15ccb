"""insightface.app.FaceAnalysis (app/face_analysis.py) on the GPU: the first .onnx of <root>/models/<name> (sorted order) that lowers
as an SCRFD detector runs through ffp_scrfd_*; Face objects carry bbox, kps and det_score only."""
from __future__ import annotations

import glob
import os
from typing import List

import numpy as np


_MAX_DETECTOR_BYTES = 100 << 20


class Face(dict):
    """insightface.app.common.Face: a dict with attribute access."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            return None

    def __setattr__(self, name, value):
        self[name] = value


def _lib():
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib as L
    return L


class FaceAnalysis:
    def __init__(self, name: str = "buffalo_l", root: str = "~/.insightface", allowed_modules=None, providers=None, **kwargs):
        self.model_dir = os.path.join(os.path.expanduser(root), "models", name)
        if not os.path.isdir(self.model_dir):
            raise FileNotFoundError(f"model pack directory {self.model_dir} not found: put the pack's .onnx files there "
                                    "(nothing is downloaded)")
        L = _lib()
        self.det_file = None
        for path in sorted(glob.glob(os.path.join(self.model_dir, "*.onnx"))):
            # the size decides without reading: the 3-stride SCRFD detectors are tens of MB, while the pack's 3D landmark and
            # recognition models (1k3d68, w600k_r50) are well over 100 MB and are skipped unread
            if os.path.getsize(path) > _MAX_DETECTOR_BYTES:
                continue
            with open(path, "rb") as f:
                data = f.read()
            try:
                L.scrfd_describe(data)
            except L.FfpError:
                continue                      # landmark / attribute / recognition models: not run
            self.det_file, self._det_bytes = path, data
            break
        if self.det_file is None:
            raise FileNotFoundError(f"no SCRFD detector (.onnx) in {self.model_dir}")
        self.det = None
        self.det_thresh, self.nms_thresh, self.det_size = 0.5, 0.4, (640, 640)

    def prepare(self, ctx_id: int = 0, det_thresh: float = 0.5, det_size=(640, 640), **kwargs):
        """ctx_id is accepted and ignored: the GPU is always used."""
        self.det_thresh = float(det_thresh)
        self.nms_thresh = float(kwargs.get("nms_thresh", self.nms_thresh))
        self.det_size = (int(det_size[0]), int(det_size[1]))
        if self.det is None:
            L = _lib()
            self.det = L.FaceDetector(self._det_bytes, precision=L.PREC_F32)

    def _rows_to_faces(self, rows: np.ndarray) -> List[Face]:
        faces = []
        for r in rows:
            faces.append(Face(bbox=r[:4].astype(np.float32).copy(), kps=r[6:].reshape(5, 3)[:, :2].astype(np.float32).copy(),
                              det_score=np.float32(r[4])))
        return faces

    def detect_tiles(self, img: np.ndarray, tiles) -> List[List[Face]]:
        """One batched detector call over crops [x0, y0, x1, y1] of img (RGB as SAHI hands it) -> faces per crop."""
        if self.det is None:
            self.prepare()
        L = _lib()
        try:
            rows = self.det.infer_tiles(np.ascontiguousarray(img), tiles, self.det_size, self.det_thresh, self.nms_thresh, L.CHAN_AS_BGR)
        except L.FfpError as e:
            if e.code == 1 and "resizes to" in str(e):
                raise ValueError(str(e)) from None
            raise
        return [self._rows_to_faces(r) for r in rows]

    def get(self, img: np.ndarray, max_num: int = 0) -> List[Face]:
        if max_num != 0:
            raise NotImplementedError("FaceAnalysis.get(max_num != 0) is not supported (no reference caller passes it)")
        h, w = img.shape[:2]
        return self.detect_tiles(img, [[0, 0, w, h]])[0]

"""sahi.models.rtdetr.RTDetrDetectionModel (sahi 0.11.x: an UltralyticsDetectionModel whose load_model builds ultralytics.RTDETR) over this
build's `ultralytics` shim, i.e. RT-DETR-l on the GPU through libffp (ffp_rtdetr_*).

Upstream sahi was not available to run against. The conversion below restates UltralyticsDetectionModel.
_create_object_prediction_list_from_original_predictions from its source: float boxes (no int truncation), x1 / y1 raised to 0, x2 / y2
lowered to the full shape, a box dropped unless x1 < x2 and y1 < y2, category names from category_mapping. The same rules run on the device
in FFP_RT_TILES_SAHI (csrc/rtdetr_ops.hip rt_post_tiles) for RTDETRDetector.sliced_predict.

The engine runs in FFP_PREC_F32 on purpose: there an item's result does not depend on its batch mates, so the batched hook
(perform_inference_batch, all tiles of a frame in one infer_tiles call) and the per-slice path (perform_inference) give identical objects.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from sahi.models.base import DetectionModel
from sahi.prediction import ObjectPrediction


def _first(value, default):
    """sahi passes flat [x, y] / [h, w]; lists of them (one per image) are accepted too."""
    if value is None:
        return default
    value = list(value)
    if len(value) > 0 and isinstance(value[0], (list, tuple)):
        return list(value[0])
    return value if len(value) == 2 else default


class RTDetrDetectionModel(DetectionModel):
    def __init__(self, model_path: Optional[str] = None, confidence_threshold: float = 0.3, device: Optional[str] = None,
                 image_size: Optional[int] = None, **kwargs):
        super().__init__(model_path=model_path, confidence_threshold=confidence_threshold, device=device,
                         image_size=640 if image_size is None else image_size, **kwargs)

    def check_dependencies(self, packages: Optional[List[str]] = None) -> None:
        import ultralytics  # noqa: F401  (this build's shim, or the real package when it is installed)

    def load_model(self):
        from ultralytics import RTDETR
        self.set_model(RTDETR(self.model_path or "rtdetr-l.pt"))       # a .pt raises the shim's conversion message

    def set_model(self, model, **kwargs):
        self.model = model
        if not self.category_mapping:
            self.category_mapping = {str(i): name for i, name in enumerate(self.category_names)}

    def perform_inference(self, image: np.ndarray):
        """image: RGB, as sahi hands it; the model takes BGR (UltralyticsDetectionModel.perform_inference: self.model(image[:, :, ::-1], ...))."""
        if self.model is None:
            raise ValueError("Model is not loaded, load it by calling .load_model()")
        self._original_predictions = self.model(image[:, :, ::-1], imgsz=self.image_size, conf=self.confidence_threshold, verbose=False)
        self._original_shape = image.shape

    def perform_inference_batch(self, frame: np.ndarray, tiles) -> list:
        """All tiles [x0, y0, x1, y1] of one RGB frame in one infer_tiles call (tile-local rows, frame uploaded once); entry k is what
        perform_inference(frame[y0:y1, x0:x1]) would have stored."""
        if self.model is None:
            raise ValueError("Model is not loaded, load it by calling .load_model()")
        if not hasattr(self.model, "predict_tiles"):         # a real Ultralytics model: its own per-image call
            return [self.model(frame[y0:y1, x0:x1, ::-1], imgsz=self.image_size, conf=self.confidence_threshold, verbose=False)
                    for x0, y0, x1, y1 in tiles]
        return self.model.predict_tiles(np.ascontiguousarray(frame), tiles, conf=self.confidence_threshold, imgsz=self.image_size, rgb=True)

    def _create_object_prediction_list_from_original_predictions(self, shift_amount_list: Optional[List[List[int]]] = [[0, 0]],
                                                                 full_shape_list: Optional[List[List[int]]] = None):
        shift = _first(shift_amount_list, [0, 0])
        full_shape = _first(full_shape_list, None)
        original = self._original_predictions
        out: List[ObjectPrediction] = []
        if original is not None and len(original) > 0:
            res = original[0]
            data = res.boxes.data if hasattr(res, "boxes") else res
            data = data.cpu().numpy() if hasattr(data, "cpu") else np.asarray(data)
            for row in np.asarray(data, np.float32).reshape(-1, 6).tolist():
                x1, y1, x2, y2, score, cid = row
                x1, y1 = max(x1, 0), max(y1, 0)
                if full_shape is not None:
                    x2, y2 = min(x2, full_shape[1]), min(y2, full_shape[0])
                if not (x1 < x2 and y1 < y2):               # sahi logs "ignoring invalid prediction" and goes on
                    continue
                cid = int(cid)
                # The box is clipped already, so the prediction carries no full_shape. This build's GreedyNMM conversion
                # (sahi/postprocess/combine.py) hands a merged prediction the full_shape of its first source, which would clip a union
                # again whenever that source came from the full-frame pass (sahi's merge_object_prediction_pair, as read, passes None when there are
                # no masks; not run here).
                out.append(ObjectPrediction(bbox=[x1, y1, x2, y2], category_id=cid, category_name=self.category_mapping[str(cid)], score=score,
                                            segmentation=None, shift_amount=shift, full_shape=None))
        self._object_prediction_list_per_image = [out]

    @property
    def category_names(self) -> List[str]:
        if self.model is not None and getattr(self.model, "names", None):
            return list(self.model.names.values())
        mapping: Dict = self.category_mapping or {}
        return [mapping[k] for k in sorted(mapping, key=int)]

    @property
    def num_categories(self) -> int:
        return len(self.category_names)

    @property
    def has_mask(self) -> bool:
        return False

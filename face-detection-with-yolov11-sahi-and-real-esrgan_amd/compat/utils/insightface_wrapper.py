"""InsightFaceDetectionModel (utils/insightface_wrapper.py of the reference): SAHI's DetectionModel around insightface.app.FaceAnalysis,
here the GPU SCRFD detector (compat/insightface). Same constructor, load_model, perform_inference, conversion (face.bbox.astype(int),
score < confidence_threshold skipped), properties and category_mapping."""
from typing import List, Optional

import numpy as np

from sahi.models.base import DetectionModel
from sahi.prediction import ObjectPrediction


class InsightFaceDetectionModel(DetectionModel):
    def __init__(self, confidence_threshold: float = 0.3, providers: Optional[List[str]] = None, **kwargs):
        self.providers = providers
        kwargs.pop("device", None)
        super().__init__(confidence_threshold=confidence_threshold, device=None, **kwargs)

    def load_model(self):
        from insightface.app import FaceAnalysis
        providers = self.providers or ["CPUExecutionProvider"]
        ctx_id = 0 if "CUDAExecutionProvider" in providers else -1
        self.model = FaceAnalysis(providers=providers)
        self.model.prepare(ctx_id=ctx_id, det_size=(640, 640), det_thresh=self.confidence_threshold)
        self.category_mapping = {"0": "face"}

    def unload_model(self):
        self.model = None

    def perform_inference(self, image: np.ndarray):
        if image.dtype != np.uint8:
            image = (image * 255).astype(np.uint8)
        self._original_predictions = self.model.get(image)

    def perform_inference_batch(self, frame: np.ndarray, tiles) -> List[list]:
        """All crops [x0, y0, x1, y1] of one frame in one GPU call -> the faces of each crop (what perform_inference would hold)."""
        if frame.dtype != np.uint8:
            frame = (frame * 255).astype(np.uint8)
        return self.model.detect_tiles(frame, tiles)

    def _create_object_prediction_list_from_original_predictions(self, shift_amount_list: Optional[List[List[int]]] = [[0, 0]],
                                                                 full_shape_list: Optional[List[List[int]]] = None):
        original_predictions = self._original_predictions
        if not original_predictions:
            self._object_prediction_list_per_image = [[]]
            return
        object_prediction_list = []
        for face in original_predictions:
            score = float(face.det_score)
            if score < self.confidence_threshold:
                continue
            x1, y1, x2, y2 = face.bbox.astype(int)
            object_prediction_list.append(ObjectPrediction(bbox=[x1, y1, x2, y2], category_id=0, category_name="face", score=score,
                                                           shift_amount=shift_amount_list, full_shape=full_shape_list))
        self._object_prediction_list_per_image = [object_prediction_list]

    @property
    def num_categories(self):
        return len(self.category_names)

    @property
    def has_mask(self):
        return False

    @property
    def category_names(self):
        return ["face"]

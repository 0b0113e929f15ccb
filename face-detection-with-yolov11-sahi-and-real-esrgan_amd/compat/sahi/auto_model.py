"""sahi.AutoDetectionModel for the model types the reference loads (utils/tuning_sahi.py: model_type='yolov8').

sahi's own Ultralytics wrapper is not in the reference tree, so 'yolov8' / 'ultralytics' map to this build's
YOLOv11PoseDetectionModel: the semantics of the reference's utils/yolo_wrapper.py (boxes truncated to int), not sahi's
float boxes. 'rtdetr' maps to sahi's RTDetrDetectionModel (sahi/models/rtdetr.py) over the `ultralytics` shim, with sahi's float boxes.
Any other model type raises as sahi does for a type it does not know."""
from typing import Any, Dict, Optional

MODEL_TYPE_TO_MODEL_CLASS_NAME = {"yolov8": "YOLOv11PoseDetectionModel", "ultralytics": "YOLOv11PoseDetectionModel",
                                  "rtdetr": "RTDetrDetectionModel"}


class AutoDetectionModel:
    @staticmethod
    def from_pretrained(model_type: str, model_path: Optional[str] = None, model: Optional[Any] = None, config_path: Optional[str] = None,
                        device: Optional[str] = None, mask_threshold: float = 0.5, confidence_threshold: float = 0.3,
                        category_mapping: Optional[Dict] = None, category_remapping: Optional[Dict] = None, load_at_init: bool = True,
                        image_size: Optional[int] = None, **kwargs):
        if model_type not in MODEL_TYPE_TO_MODEL_CLASS_NAME:
            raise ValueError(f"Model type {model_type} not supported. Supported model types: {list(MODEL_TYPE_TO_MODEL_CLASS_NAME)}")
        if MODEL_TYPE_TO_MODEL_CLASS_NAME[model_type] == "RTDetrDetectionModel":
            from sahi.models.rtdetr import RTDetrDetectionModel
            return RTDetrDetectionModel(model_path=model_path, model=model, config_path=config_path, device=device, mask_threshold=mask_threshold,
                                        confidence_threshold=confidence_threshold, category_mapping=category_mapping,
                                        category_remapping=category_remapping, load_at_init=load_at_init, image_size=image_size, **kwargs)
        from utils.yolo_wrapper import YOLOv11PoseDetectionModel
        kw = dict(model_path=model_path, confidence_threshold=confidence_threshold, device=device if device is not None else "cuda:0",
                  mask_threshold=mask_threshold, category_mapping=category_mapping, category_remapping=category_remapping,
                  load_at_init=load_at_init, model=model, config_path=config_path, **kwargs)
        if image_size is not None:
            kw["image_size"] = image_size
        return YOLOv11PoseDetectionModel(**kw)

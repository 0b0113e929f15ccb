"""utils.tuning_sahi: the reference's SAHI grid search (slice size x overlap x postprocess type / metric / threshold, scored by COCO
bbox mAP on WIDER FACE val) with its names and behaviour: the three `param_grid_*` dicts, `param_grid`, `evaluate_sahi(model,
params)` and `main()`, which writes sahi_tuning_complete_results.json and best_sahi_config.json. The path constants are module
globals and may be overridden before a call.

Addition: `evaluate_grid(model, combinations)` returns exactly `[evaluate_sahi(model, p) for p in combinations]`, but decodes each
image once and runs slicing + the batched detector + the shift once per (image, slice size, overlap); only the postprocess runs per
configuration. `main()` uses it. COCOeval runs on the device (compat/pycocotools, csrc/coco_eval.hip)."""
import io
import itertools
import json
import os
from contextlib import redirect_stdout

from tqdm import tqdm

from pycocotools.coco import COCO
from pycocotools.cocoeval import COCOeval
from sahi import AutoDetectionModel
from sahi.predict import get_sliced_object_predictions, get_sliced_prediction, make_postprocess, postprocess_object_predictions
from sahi.slicing import slice_image
from sahi.utils.cv import read_image_as_array

BASE_DIR = os.path.join("data", "dataset", "widerface")
VAL_IMAGES_DIR = os.path.join(BASE_DIR, "WIDER_val", "images")
VAL_JSON_PATH = os.path.join(BASE_DIR, "val_ground_truth_coco.json")
MODEL_PATH = "models/yolo11s-pose-default/yolo11s_pose/weights/best.pt"
RESULTS_FILE = "sahi_tuning_complete_results.json"
BEST_CONFIG_FILE = "best_sahi_config.json"

param_grid_quick = {
    "slice_size": [512, 640],
    "overlap_ratio": [0.2, 0.3],
    "postprocess_type": ["NMS"],
    "postprocess_match_metric": ["IOS"],
    "postprocess_match_threshold": [0.5],
}
param_grid_balanced = {
    "slice_size": [320, 512, 640],
    "overlap_ratio": [0.2, 0.25, 0.3],
    "postprocess_type": ["NMS", "GREEDYNMM"],
    "postprocess_match_metric": ["IOS", "IOU"],
    "postprocess_match_threshold": [0.5],
}
param_grid_comprehensive = {
    "slice_size": [320, 512, 640, 800],
    "overlap_ratio": [0.1, 0.2, 0.25, 0.3, 0.4],
    "postprocess_type": ["NMS"],
    "postprocess_match_metric": ["IOS", "IOU"],
    "postprocess_match_threshold": [0.3, 0.5, 0.7],
}
param_grid = param_grid_comprehensive


def _desc(params):
    return (f"S{params['slice_size']}|O{params['overlap_ratio']:.2f}|{params['postprocess_type'][:3]}|"
            f"{params['postprocess_match_metric']}")


def _append_results(results, img_id, object_prediction_list):
    for object_prediction in object_prediction_list:
        results.append({"image_id": img_id, "category_id": 0, "bbox": object_prediction.bbox.to_xywh(), "score": object_prediction.score.value})


def _coco_metrics(coco_gt, results, params, skipped_count):
    """The end of evaluate_sahi: temporary result file, loadRes, COCOeval (bbox) -> dict of stats[0..2], or 0.0."""
    if skipped_count > 0:
        tqdm.write(f"Skipped {skipped_count} images")
    if not results:
        tqdm.write("No detections")
        return 0.0
    res_file = f"temp_results_{params['slice_size']}_{params['overlap_ratio']}_{params['postprocess_type']}.json"
    with open(res_file, "w") as f:
        json.dump(results, f)
    try:
        coco_dt = coco_gt.loadRes(res_file)
        coco_eval = COCOeval(coco_gt, coco_dt, "bbox")
        with redirect_stdout(io.StringIO()):
            coco_eval.evaluate()
            coco_eval.accumulate()
            coco_eval.summarize()
        if os.path.exists(res_file):
            os.remove(res_file)
        map_50_95, map_50, map_75 = coco_eval.stats[0], coco_eval.stats[1], coco_eval.stats[2]
        tqdm.write(f"mAP@50-95: {map_50_95:.4f} | mAP@50: {map_50:.4f} | mAP@75: {map_75:.4f}")
        return {"map_50_95": map_50_95, "map_50": map_50, "map_75": map_75}
    except Exception as e:
        tqdm.write(f"Error: {e}")
        return 0.0


def _load_gt():
    try:
        return COCO(VAL_JSON_PATH)
    except Exception as e:
        tqdm.write(f"ERROR: cannot read {VAL_JSON_PATH}: {e}")
        return None


def evaluate_sahi(model, params):
    """mAP of one configuration over every image of VAL_JSON_PATH: {'map_50_95', 'map_50', 'map_75'}, or 0.0 when the GT file cannot
    be read, nothing was detected or the evaluation failed. An image that is missing or raises is skipped."""
    coco_gt = _load_gt()
    if coco_gt is None:
        return 0.0
    results, skipped_count = [], 0
    for img_id in tqdm(coco_gt.getImgIds(), desc=_desc(params), ncols=100):
        img_info = coco_gt.loadImgs(img_id)[0]
        img_path = os.path.join(VAL_IMAGES_DIR, img_info["file_name"])
        if not os.path.exists(img_path):
            skipped_count += 1
            continue
        try:
            result = get_sliced_prediction(img_path, model, slice_height=params["slice_size"], slice_width=params["slice_size"],
                                           overlap_height_ratio=params["overlap_ratio"], overlap_width_ratio=params["overlap_ratio"],
                                           postprocess_type=params["postprocess_type"], postprocess_match_metric=params["postprocess_match_metric"],
                                           postprocess_match_threshold=params["postprocess_match_threshold"], postprocess_class_agnostic=True,
                                           verbose=0)
            _append_results(results, img_id, result.object_prediction_list)
        except Exception:
            skipped_count += 1
            continue
    return _coco_metrics(coco_gt, results, params, skipped_count)


def evaluate_grid(model, combinations, progress: bool = True):
    """[evaluate_sahi(model, p) for p in combinations], with the detector run once per (image, slice size, overlap) instead of once per
    configuration, and each image decoded once (read_image_as_array, the reader slice_image uses for a path)."""
    combinations = list(combinations)
    coco_gt = _load_gt()
    if coco_gt is None:
        return [0.0] * len(combinations)
    groups = {}
    for n, p in enumerate(combinations):
        groups.setdefault((p["slice_size"], p["overlap_ratio"]), []).append(n)
    results = [[] for _ in combinations]
    skipped = [0] * len(combinations)
    img_ids = coco_gt.getImgIds()
    for img_id in tqdm(img_ids, desc=f"{len(groups)} slicings x {len(combinations)} configs", ncols=100, disable=not progress):
        img_info = coco_gt.loadImgs(img_id)[0]
        img_path = os.path.join(VAL_IMAGES_DIR, img_info["file_name"])
        if not os.path.exists(img_path):
            for n in range(len(combinations)):
                skipped[n] += 1
            continue
        try:
            image = read_image_as_array(img_path)
        except Exception:
            image = None
        for (size, overlap), members in groups.items():
            try:
                if image is None:
                    raise ValueError(f"cannot read {img_path}")
                sl = slice_image(image=image, slice_height=size, slice_width=size, overlap_height_ratio=overlap, overlap_width_ratio=overlap)
                preds, _ = get_sliced_object_predictions(sl, image, model)
            except Exception:
                for n in members:
                    skipped[n] += 1
                continue
            for n in members:
                p = combinations[n]
                try:
                    pp = make_postprocess(p["postprocess_type"], p["postprocess_match_metric"], p["postprocess_match_threshold"], True)
                    _append_results(results[n], img_id, postprocess_object_predictions(list(preds), pp))
                except Exception:
                    skipped[n] += 1
    return [_coco_metrics(coco_gt, results[n], p, skipped[n]) for n, p in enumerate(combinations)]


def main():
    print("=" * 70)
    print("SAHI TUNING - WIDER FACE (COCO bbox mAP)")
    print("=" * 70)
    if not os.path.exists(VAL_JSON_PATH):
        print(f"\nERROR: {VAL_JSON_PATH} not found")
        return
    if not os.path.exists(MODEL_PATH):
        print(f"\nERROR: model not found: {MODEL_PATH}")
        return
    print(f"\nLoading model: {MODEL_PATH}")
    try:
        detection_model = AutoDetectionModel.from_pretrained(model_type="yolov8", model_path=MODEL_PATH, confidence_threshold=0.25, device="cuda:0")
    except Exception as e:
        print(f"Error: {e}")
        return
    keys, values = zip(*param_grid.items())
    combinations = [dict(zip(keys, v)) for v in itertools.product(*values)]
    n_det = len({(p["slice_size"], p["overlap_ratio"]) for p in combinations})
    print(f"\nConfigurations: {len(combinations)} ({n_det} detector passes per image)")
    print("=" * 70)

    best_map, best_params, history = 0, {}, []
    for idx, (params, metrics) in enumerate(zip(combinations, evaluate_grid(detection_model, combinations)), 1):
        tqdm.write(f"[{idx}/{len(combinations)}] Slice:{params['slice_size']} Over:{params['overlap_ratio']} Post:{params['postprocess_type']} "
                   f"Metric:{params['postprocess_match_metric']} Thresh:{params['postprocess_match_threshold']}")
        if isinstance(metrics, dict):
            current_map = metrics["map_50_95"]
        else:
            current_map = 0.0
            metrics = {"map_50_95": 0.0, "map_50": 0.0, "map_75": 0.0}
        history.append({"params": params, "metrics": metrics})
        if current_map > best_map:
            best_map, best_params = current_map, params
            tqdm.write(f"NEW BEST mAP@50-95: {best_map:.4f}")

    history_sorted = sorted(history, key=lambda x: x["metrics"]["map_50_95"], reverse=True)
    print("\n" + "=" * 70)
    print("TOP 10 CONFIGURATIONS")
    print(f"{'Rank':<5} {'Slice':<7} {'Over':<6} {'Post':<10} {'Metric':<6} {'Thresh':<7} {'mAP@50-95':<10}")
    print("-" * 70)
    for rank, h in enumerate(history_sorted[:10], 1):
        p, m = h["params"], h["metrics"]
        print(f"{rank:<5} {p['slice_size']:<7} {p['overlap_ratio']:<6.2f} {p['postprocess_type']:<10} {p['postprocess_match_metric']:<6} "
              f"{p['postprocess_match_threshold']:<7.2f} {m['map_50_95']:<10.4f}")
    if best_params:
        print(f"\nBest configuration: {best_params}  mAP@50-95 {best_map:.4f}")
    with open(RESULTS_FILE, "w") as f:
        json.dump({"best_params": best_params, "best_metrics": history_sorted[0]["metrics"] if history_sorted else {}, "all_results": history},
                  f, indent=2)
    print(f"\nAll results: {RESULTS_FILE}")
    with open(BEST_CONFIG_FILE, "w") as f:
        json.dump(best_params, f, indent=2)
    print(f"Best config : {BEST_CONFIG_FILE}")


if __name__ == "__main__":
    main()

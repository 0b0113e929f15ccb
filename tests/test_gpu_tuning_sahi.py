"""GPU: compat/utils/tuning_sahi.py on a small dataset built in tmp_path (the tests/golden/real/det_*.png frames, a synthetic COCO GT
and synthetic YOLO11n-pose weights): evaluate_grid returns exactly what per-configuration evaluate_sahi returns while running the detector
once per (image, slice size, overlap); evaluate_sahi equals get_sliced_prediction + the numpy COCOeval restatement; main() writes its
two JSON files."""
import copy
import itertools
import json
import os
import shutil

import numpy as np
import pytest

import coco_eval_ref as R

pytestmark = pytest.mark.gpu
REAL = os.path.join(os.path.dirname(__file__), "golden", "real")
FRAMES = ["det_test1.png", "det_parade.png", "det_family.png", "det_photo4k.png"]
GRID = {"slice_size": [128, 192], "overlap_ratio": [0.2, 0.3], "postprocess_type": ["NMS", "GREEDYNMM"], "postprocess_match_metric": ["IOU", "IOS"],
        "postprocess_match_threshold": [0.5]}


def combos(grid):
    keys, values = zip(*grid.items())
    return [dict(zip(keys, v)) for v in itertools.product(*values)]


@pytest.fixture(scope="module")
def env(gpu_lib, tmp_path_factory):
    from ffp_amd import compat, synth, weights_io
    compat.install()
    from sahi import AutoDetectionModel
    from sahi.predict import get_sliced_prediction
    from utils import tuning_sahi as T
    root = tmp_path_factory.mktemp("sweep")
    (root / "images").mkdir()
    for f in FRAMES:
        shutil.copy(os.path.join(REAL, f), root / "images" / f)
    model_path = str(root / "yolo11n_pose_synth.ffpw")
    weights_io.save(model_path, synth.yolo11_pose_weights("n"))
    model = AutoDetectionModel.from_pretrained(model_type="yolov8", model_path=model_path, confidence_threshold=0.05, device="cuda:0", image_size=256)
    # GT: boxes of one configuration's detections, jittered, plus a few misses, so that the mAPs are neither 0 nor 1
    rng = np.random.default_rng(0)
    images, anns = [], []
    for n, f in enumerate(FRAMES, 1):
        from PIL import Image
        w, h = Image.open(root / "images" / f).size
        images.append({"id": n, "file_name": f, "width": w, "height": h})
        res = get_sliced_prediction(str(root / "images" / f), model, slice_height=160, slice_width=160, overlap_height_ratio=0.2,
                                    overlap_width_ratio=0.2, postprocess_type="NMS", postprocess_match_metric="IOS", verbose=0)
        boxes = [p.bbox.to_xywh() for p in res.object_prediction_list][::2]
        boxes += [[int(rng.integers(0, w - 40)), int(rng.integers(0, h - 40)), 30, 30] for _ in range(2)]
        for b in boxes:
            b = [b[0] + int(rng.integers(-2, 3)), b[1] + int(rng.integers(-2, 3)), max(2, b[2]), max(2, b[3])]
            anns.append({"id": len(anns) + 1, "image_id": n, "category_id": 0, "bbox": b, "area": float(b[2] * b[3]), "iscrowd": 0})
    gt = {"images": images, "annotations": anns, "categories": [{"id": 0, "name": "face", "supercategory": "face"}]}
    (root / "gt.json").write_text(json.dumps(gt))
    old = (T.VAL_JSON_PATH, T.VAL_IMAGES_DIR, T.MODEL_PATH)
    T.VAL_JSON_PATH, T.VAL_IMAGES_DIR, T.MODEL_PATH = str(root / "gt.json"), str(root / "images"), model_path
    cwd = os.getcwd()
    os.chdir(root)
    yield dict(T=T, model=model, root=root, gt=gt, get_sliced_prediction=get_sliced_prediction)
    os.chdir(cwd)
    T.VAL_JSON_PATH, T.VAL_IMAGES_DIR, T.MODEL_PATH = old


def test_grid_equals_per_config(env):
    T, model = env["T"], env["model"]
    cs = combos(GRID)
    per = [T.evaluate_sahi(model, p) for p in cs]
    grid = T.evaluate_grid(model, cs)
    assert grid == per
    assert all(isinstance(m, dict) for m in per) and len({m["map_50_95"] for m in per}) > 1
    assert 0 < max(m["map_50_95"] for m in per) < 1


def test_evaluate_sahi_equals_restatement(env):
    T, model = env["T"], env["model"]
    p = {"slice_size": 128, "overlap_ratio": 0.25, "postprocess_type": "GREEDYNMM", "postprocess_match_metric": "IOS", "postprocess_match_threshold": 0.5}
    results = []
    for img in env["gt"]["images"]:
        r = env["get_sliced_prediction"](os.path.join(T.VAL_IMAGES_DIR, img["file_name"]), model, slice_height=128, slice_width=128,
                                         overlap_height_ratio=0.25, overlap_width_ratio=0.25, postprocess_type="GREEDYNMM",
                                         postprocess_match_metric="IOS", postprocess_match_threshold=0.5, postprocess_class_agnostic=True, verbose=0)
        results += [{"image_id": img["id"], "category_id": 0, "bbox": o.bbox.to_xywh(), "score": o.score.value} for o in r.object_prediction_list]
    ref = R.evaluate(env["gt"], json.loads(json.dumps(results)))
    assert T.evaluate_sahi(model, p) == {"map_50_95": ref.stats[0], "map_50": ref.stats[1], "map_75": ref.stats[2]}


def test_detector_runs_once_per_slicing(env, monkeypatch):
    T, model = env["T"], env["model"]
    calls = []
    orig = model.perform_inference_batch
    monkeypatch.setattr(model, "perform_inference_batch", lambda frame, tiles: calls.append(len(tiles)) or orig(frame, tiles))
    cs = combos(GRID)
    T.evaluate_grid(model, cs)
    assert len(calls) == len(FRAMES) * 4                   # 4 images x (2 slice sizes x 2 overlaps), not x 16 configurations


def test_main_writes_both_json_files(env, monkeypatch):
    T = env["T"]
    monkeypatch.setattr(T, "param_grid", {"slice_size": [128], "overlap_ratio": [0.2], "postprocess_type": ["NMS", "GREEDYNMM"],
                                          "postprocess_match_metric": ["IOS"], "postprocess_match_threshold": [0.5]})
    for f in (T.RESULTS_FILE, T.BEST_CONFIG_FILE):
        if os.path.exists(f):
            os.remove(f)
    T.main()
    full = json.load(open(T.RESULTS_FILE))
    best = json.load(open(T.BEST_CONFIG_FILE))
    assert len(full["all_results"]) == 2 and set(full) == {"best_params", "best_metrics", "all_results"}
    assert best == full["best_params"] or best == {}

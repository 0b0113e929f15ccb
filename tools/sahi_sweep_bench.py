"""Per-configuration wall time of utils.tuning_sahi.evaluate_grid against looping evaluate_sahi over the reference's balanced grid (36
configurations: 3 slice sizes x 3 overlaps x 2 postprocess types x 2 metrics) on N synthetic frames with a synthetic COCO GT and
synthetic YOLO11s-pose weights (model settings of tuning_sahi.main: confidence 0.25, image size 1024). Both paths must return the
same metrics; the script checks it.

    python tools/sahi_sweep_bench.py [--frames 8] [--json OUT]
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    a.json = os.path.abspath(a.json) if a.json else ""
    import ffp_amd  # noqa: F401
    from ffp_amd import compat, synth, weights_io
    compat.install()
    from PIL import Image
    from sahi import AutoDetectionModel
    from utils import tuning_sahi as T
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "images"))
    rng = np.random.default_rng(0)
    images, anns = [], []
    for n in range(1, a.frames + 1):
        f = f"frame_{n}.png"
        Image.fromarray(synth.synthetic_frame(a.height, a.width, seed=n)).save(os.path.join(tmp, "images", f))
        images.append({"id": n, "file_name": f, "width": a.width, "height": a.height})
        for _ in range(20):
            w, h = (int(v) for v in rng.integers(8, 120, 2))
            b = [int(rng.integers(0, a.width - w)), int(rng.integers(0, a.height - h)), w, h]
            anns.append({"id": len(anns) + 1, "image_id": n, "category_id": 0, "bbox": b, "area": float(w * h), "iscrowd": 0})
    with open(os.path.join(tmp, "gt.json"), "w") as fh:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": 0, "name": "face"}]}, fh)
    model_path = os.path.join(tmp, "yolo11s_pose_synth.ffpw")
    weights_io.save(model_path, synth.yolo11_pose_weights("s"))
    T.VAL_JSON_PATH, T.VAL_IMAGES_DIR, T.MODEL_PATH = os.path.join(tmp, "gt.json"), os.path.join(tmp, "images"), model_path
    os.chdir(tmp)
    model = AutoDetectionModel.from_pretrained(model_type="yolov8", model_path=model_path, confidence_threshold=0.25, device="cuda:0")
    keys, values = zip(*T.param_grid_balanced.items())
    cs = [dict(zip(keys, v)) for v in itertools.product(*values)]
    T.evaluate_sahi(model, cs[0])                  # warm-up: detector plans for every slice size, module loads
    for p in cs[:: len(cs) // 3]:
        T.evaluate_sahi(model, p)
    t0 = time.perf_counter()
    per = [T.evaluate_sahi(model, p) for p in cs]
    t_loop = time.perf_counter() - t0
    t0 = time.perf_counter()
    grid = T.evaluate_grid(model, cs, progress=False)
    t_grid = time.perf_counter() - t0
    out = {"what": "balanced grid (36 configs), synthetic frames + GT, yolo11s-pose synthetic weights, imgsz 1024, conf 0.25",
           "frames": a.frames, "frame_hw": [a.height, a.width], "configs": len(cs), "device": "MI355X (gfx950)",
           "loop_evaluate_sahi_s": t_loop, "evaluate_grid_s": t_grid, "per_config_ms": {"loop": 1e3 * t_loop / len(cs), "grid": 1e3 * t_grid / len(cs)},
           "speedup": t_loop / t_grid, "identical_metrics": grid == per}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

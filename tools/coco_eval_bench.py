"""Time COCOeval (bbox) on a synthetic dataset of WIDER FACE val's size (3,226 images, one category): the device path
(compat/pycocotools -> ffp_eval_coco_bbox, warm calls; the call returns after a device sync) against the numpy restatement of
pycocotools (tests/coco_eval_ref.py, one Python process — pycocotools' own loop is single-threaded too; pycocotools itself is not
installed, so nothing here is a claim about it).

    python tools/coco_eval_bench.py [--iters 10] [--device-only] [--json OUT]
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import coco_eval_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--images", type=int, default=3226)
    ap.add_argument("--max-gt", type=int, default=12)
    ap.add_argument("--max-dt", type=int, default=30)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import ffp_amd  # noqa: F401
    from ffp_amd import compat
    compat.install()
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    d, r = R.random_dataset(seed=2026, n_img=a.images, cats=(0,), max_gt=a.max_gt, max_dt=a.max_dt)
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "gt.json")
        with open(p, "w") as f:
            json.dump(d, f)
        gt = COCO(p)
        dt = gt.loadRes(copy.deepcopy(r))
    E = COCOeval(gt, dt, "bbox")
    E.evaluate()                                  # warm-up: module load, first allocations
    t_prep, t_call = [], []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        E._prepare()
        t1 = time.perf_counter()
        E._out = E._run(False)
        t2 = time.perf_counter()
        t_prep.append(t1 - t0)
        t_call.append(t2 - t1)
    E.accumulate()
    E.summarize()
    out = {"what": "COCOeval bbox evaluate+accumulate, synthetic dataset of WIDER val size", "images": a.images, "gts": len(d["annotations"]),
           "dets": len(r), "device": "MI355X (gfx950)",
           "device_call_ms": {"median": 1e3 * float(np.median(t_call)), "min": 1e3 * float(np.min(t_call)), "iters": a.iters},
           "host_unit_packing_ms_median": 1e3 * float(np.median(t_prep)), "stats": [float(x) for x in E.stats]}
    if not a.device_only:
        t0 = time.perf_counter()
        ref = R.evaluate(d, r)
        out["numpy_restatement_s"] = time.perf_counter() - t0
        out["numpy_restatement_note"] = "one Python process on the GPU machine's host CPU (the loop is single-threaded), not pycocotools"
        out["bit_identical"] = all(np.array_equal(E.eval[k], ref.eval[k]) for k in ("precision", "recall", "scores")) and \
            np.array_equal(np.asarray(E.stats), np.asarray(ref.stats))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

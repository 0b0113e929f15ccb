"""Write tests/golden/coco_eval_expected.npz: seeded COCO datasets (tests/coco_eval_ref.random_dataset) and what the numpy restatement
of pycocotools' COCOeval (tests/coco_eval_ref.py) returns for them — precision / recall / scores / stats. tests/test_gpu_coco_eval.py
regenerates the datasets from the stored seeds and checks the device against these arrays bit for bit.

    python tests/golden/make_coco_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import coco_eval_ref as R  # noqa: E402

CASES = {"small": dict(seed=11, n_img=12), "ties": dict(seed=12, n_img=30, max_dt=40), "big": dict(seed=13, n_img=4, big_units=True)}


def main():
    out = {}
    for name, kw in CASES.items():
        d, r = R.random_dataset(**kw)
        E = R.evaluate(d, r)
        for k in ("precision", "recall", "scores"):
            out[f"{name}_{k}"] = E.eval[k]
        out[f"{name}_stats"] = np.asarray(E.stats)
    np.savez_compressed(os.path.join(HERE, "coco_eval_expected.npz"), **out)


if __name__ == "__main__":
    main()

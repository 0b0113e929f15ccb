"""Add the YOLO11m-pose / YOLO11l-pose entries to <pkg>/synth_calib.json, by the method of make_synth_calibration.py (each
convolution's pre-activation output rescaled to the target standard deviation on the same synthetic frame) with the tests-side
reference of the larger scales (tests/yolo11_scales_ref.py). Every other key of the file is kept byte for byte: the n/s synthetic
weights, and every golden file made from them, depend on it.

    python tests/golden/make_synth_calibration_scales.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import ffp_amd  # noqa: E402
from ffp_amd import synth  # noqa: E402
from oracle import ultra_post  # noqa: E402
from yolo11_scales_ref import Yolo11ScalesRef  # noqa: E402

TARGET = {".cv2.{l}.2": 2.5, ".cv3.{l}.2": 2.0, ".cv4.{l}.2": 1.0}    # as make_synth_calibration.py


def calib_yolo(scale):
    W = synth.yolo11_pose_weights(scale, seed=0, calibrated=False)
    m = Yolo11ScalesRef(W, scale)
    factors = {}

    def hook(name, y):
        tgt = 1.0
        for l in range(3):
            for k, v in TARGET.items():
                if name.endswith(k.format(l=l)):
                    tgt = v
        b = m.w[name + ".bias"].view(1, -1, 1, 1)
        s = tgt / float((y - b).std())
        factors[name] = s
        return (y - b) * s + b          # only the weight is rescaled, the bias is kept

    m.pre_hook = hook
    img = synth.synthetic_frame(384, 384, seed=123)
    m.forward(ultra_post.preprocess(img, 384))
    return factors


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(ffp_amd.__file__), "synth_calib.json")
    with open(path) as f:
        out = json.load(f)           # insertion order kept: existing keys are written back exactly as they were
    for sc in ("m", "l"):
        out[f"yolo11{sc}-pose"] = calib_yolo(sc)
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, {k: len(v) for k, v in out.items()})

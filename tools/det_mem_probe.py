"""Device memory of one detector plan per buffer-reuse mode (ffp_det_set_buffer_reuse): the three ffp_det_mem_detail figures and
ffp_det_mem_bytes, for the batch shape a pipeline with these settings lays out.

    python tools/det_mem_probe.py --arch s --imgsz 512 --frames 5 [--height 2160 --width 3840 --slice 512 --overlap 0.2]
                                  [--precision f32x3] [--modes 0,1]

The batch is what pipeline.frame_items gives: per frame its slices, then the full frame. One call lays the plan out; the figures do not
depend on the pixels, so the frame is a synthetic one."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (its HIP runtime comes up before libffp.so's)
import ffp_amd  # noqa: F401,E402
from ffp_amd import _lib, pipeline, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="s", choices=["n", "s", "m", "l"])
    ap.add_argument("--imgsz", type=int, default=512)
    ap.add_argument("--frames", type=int, default=5, help="frames per detection group (one ragged batch)")
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--slice", type=int, default=512)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--precision", default="f32x3", choices=["f32", "f32x3", "f16"])
    ap.add_argument("--modes", default="0,1,2")
    ap.add_argument("--lanes", type=int, default=0)
    a = ap.parse_args()
    cfg = pipeline.PipeConfig(slice_h=a.slice, slice_w=a.slice, overlap=a.overlap, imgsz=a.imgsz)
    items = pipeline.frame_items(a.height, a.width, cfg, a.frames)
    one = synth.synthetic_frame(a.height, a.width, seed=1)
    frame = np.ascontiguousarray(np.concatenate([one] * a.frames, 0))
    prec = {"f32": _lib.PREC_F32, "f32x3": _lib.PREC_F32X3, "f16": _lib.PREC_F16}[a.precision]
    det = _lib.Detector(synth.yolo11_pose_weights(a.arch), arch=a.arch, precision=prec)
    det.set_lanes(a.lanes)
    print(f"# yolo11{a.arch} {a.precision}, {a.height}x{a.width} frame, {a.slice} slices at overlap {a.overlap} + full frame, imgsz {a.imgsz}, "
          f"{a.frames} frame(s) per group: {len(items)} items per batch, lanes {a.lanes}")
    for mode in [int(m) for m in a.modes.split(",")]:
        det.set_buffer_reuse(mode)
        det.infer_tiles(frame, items, a.imgsz, 0.5)
        d, m = det.mem_detail(), det.mem_bytes()
        row = {"mode": mode, **d, "plan_bytes": m["plans"], "weight_bytes": m["weights"],
               "activation_GB": round(d["activation_bytes"] / 1e9, 3), "no_reuse_GB": round(d["no_reuse_bytes"] / 1e9, 3),
               "peak_live_GB": round(d["peak_live_bytes"] / 1e9, 3),
               "activation_over_peak_live": round(d["activation_bytes"] / d["peak_live_bytes"], 4)}
        print(json.dumps(row), flush=True)
        det.drop_plans()
    det.close()


if __name__ == "__main__":
    main()

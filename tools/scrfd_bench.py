"""Throughput of the SCRFD face detector (ffp_scrfd_*) at the two workloads of the reference pipelines, on a synthetic
SCRFD-10G-KPS-shaped graph (synth.scrfd_onnx):
  * app_v1: a 3840x2160 frame, 512x512 slices at 0.2 overlap plus the full frame (61 crops), det_size 640;
  * app_v2: a x4-enhanced 1024x768 frame (4096x3072), app_v2.py's 4x4 grid (1024x768 slices, 0.2 overlap) plus the full frame.
For each: ms per frame of one batched call, next to the per-slice path (one call per crop, as FaceAnalysis.get per slice does),
the plan's conv FLOPs and the resulting TFLOP/s. Host clock around synchronous calls, after warm-up.

    python tools/scrfd_bench.py [--iters 10] [--precision f32|f32x3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ffp_amd  # noqa: E402,F401
from ffp_amd import _lib, synth  # noqa: E402


def workload(name, H, W, sh, sw):
    tiles = [list(map(int, t)) for t in _lib.slice_bboxes(H, W, sh, sw, 0.2, 0.2)] + [[0, 0, W, H]]
    return name, H, W, tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f32", choices=["f32", "f32x3"])
    a = ap.parse_args()
    data, _ = synth.scrfd_onnx(0)
    det = _lib.FaceDetector(data, precision=_lib.PREC_F32 if a.precision == "f32" else _lib.PREC_F32X3)
    for name, H, W, tiles in (workload("app_v1_4k", 2160, 3840, 512, 512), workload("app_v2_4x4", 3072, 4096, 768, 1024)):
        frame = synth.synthetic_frame(H, W, seed=5)
        for _ in range(a.warmup):
            det.infer_tiles(frame, tiles)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            out = det.infer_tiles(frame, tiles)
        ms_batched = (time.perf_counter() - t0) * 1e3 / a.iters
        flops = det.last_conv_flops()
        for t in tiles:                                   # warm the batch-1 plan
            det.infer_tiles(frame, [t])
        t0 = time.perf_counter()
        for _ in range(max(1, a.iters // 2)):
            for t in tiles:
                det.infer_tiles(frame, [t])
        ms_slice = (time.perf_counter() - t0) * 1e3 / max(1, a.iters // 2)
        print(json.dumps({"workload": name, "precision": a.precision, "frame": [W, H], "crops": len(tiles), "det_size": [640, 640],
                          "ms_per_frame_batched": round(ms_batched, 3), "ms_per_frame_per_slice": round(ms_slice, 3),
                          "conv_gflop_per_frame": round(flops / 1e9, 2), "tflops_batched": round(flops / ms_batched / 1e9, 2),
                          "faces_per_frame": int(sum(len(o) for o in out))}))


if __name__ == "__main__":
    main()

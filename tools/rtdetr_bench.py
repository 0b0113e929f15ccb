"""Throughput of RT-DETR-l (ffp_rtdetr_*) on synthetic weights (synth.rtdetr_l_weights): images/s of predict() at batch 1 and 8,
imgsz 640, FFP_PREC_F32 and FFP_PREC_F32X3, with the plan's conv FLOPs and hipGraph state. Host clock around synchronous calls
after warm-up (the first call builds and tunes the plan, the second captures it). Then, per precision and batch, one eager call with HIP
events around every launch (ffp_rtdetr_set_profile): milliseconds per kernel kind (the conv kernels by variant, every rtdetr_ops.hip
kernel by name), summed over the plan's launches. Event pairs around ~400 launches add their own gaps: the per-kind sums are for
ranking kernels, the images/s lines are the throughput.

    python tools/rtdetr_bench.py [--iters 20] [--imgsz 640] [--no-profile]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ffp_amd  # noqa: E402,F401
from ffp_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    w = synth.rtdetr_l_weights(1)
    frames = [synth.synthetic_frame(720, 1280, seed=i) for i in range(8)]
    for prec_name, prec in (("f32", _lib.PREC_F32), ("f32x3", _lib.PREC_F32X3)):
        det = _lib.RTDETRDetector(w, precision=prec)
        for bs in (1, 8):
            ims = frames[:bs]
            for _ in range(3):
                det.predict(ims, a.imgsz, 0.25)
            t = time.perf_counter()
            for _ in range(a.iters):
                det.predict(ims, a.imgsz, 0.25)
            dt = (time.perf_counter() - t) / a.iters
            inf = det.info()
            print(json.dumps({"precision": prec_name, "batch": bs, "imgsz": a.imgsz, "ms_per_call": round(dt * 1e3, 3),
                              "images_per_s": round(bs / dt, 1), "conv_gflop_per_image": round(inf["conv_flops"] / bs / 1e9, 2),
                              "graph_state": inf["graph_state"]}))
            if not a.no_profile:
                kinds = {}
                for name, ms in det.profile(ims, a.imgsz, 0.25):
                    parts = name.split(" ")
                    k = " ".join(parts[:2]) if parts[0] == "conv" else parts[0]
                    t_, c_ = kinds.get(k, (0.0, 0))
                    kinds[k] = (t_ + ms, c_ + 1)
                tot = sum(v[0] for v in kinds.values())
                for k, (ms, cnt) in sorted(kinds.items(), key=lambda kv: -kv[1][0]):
                    print(json.dumps({"precision": prec_name, "batch": bs, "kernel": k, "launches": cnt, "ms": round(ms, 4),
                                      "share": round(ms / tot, 4)}))
        det.close()


if __name__ == "__main__":
    main()

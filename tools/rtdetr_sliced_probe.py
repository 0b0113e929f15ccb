"""Sliced RT-DETR-l prediction on one MI355X: which max_batch, and is the tile path no slower than cropping on the host?

Input: a 2160 x 3840 synthetic frame, 512-pixel slices at overlap 0.2 plus the full frame (61 tiles), imgsz 640, synthetic weights,
FFP_PREC_F32 and FFP_PREC_F32X3. For max_batch in 4, 8, 16, 32, per precision:
  (a) RTDETRDetector.infer_tiles (ffp_rtdetr_infer_tiles, tile-local rows): the frame goes up once, the tiles are cut on the device;
  (b) the same tiles cropped on the host and passed to RTDETRDetector.predict (ffp_rtdetr_predict) in the same chunk sizes: the path
      that existed before the tile entry points.
Both use the same plans. Host clock around synchronous calls, after warm-up of every plan (build, then hipGraph capture); (a) and (b)
alternate within one process, `--repeats` times each, and the file keeps every sample, the median and the min..max spread, so a difference
can be judged against the run-to-run spread. Device bytes held by the plans' activations are read after (a).

The default max_batch rule: the fastest (a) in FFP_PREC_F32 (the precision the sahi model class runs) among the sizes whose plans stay
under 8 GB in both precisions.

    python tools/rtdetr_sliced_probe.py [--repeats 10] [--out profiles/rtdetr_sliced_mi355x.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ffp_amd  # noqa: E402,F401
from ffp_amd import _lib, synth  # noqa: E402

H, W, SLICE, OVERLAP, IMGSZ, CONF = 2160, 3840, 512, 0.2, 640, 0.25
LIMIT = 8 * 1000 ** 3


def by_crops(det, crops, max_batch):
    out, o = [], 0
    for m in _lib.tile_chunks(len(crops), max_batch):
        out += det.predict(crops[o:o + m], IMGSZ, CONF)
        o += m
    return out


def summary(samples):
    return {"median_ms": round(statistics.median(samples), 3), "min_ms": round(min(samples), 3), "max_ms": round(max(samples), 3),
            "samples_ms": [round(s, 3) for s in samples]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtdetr_sliced_mi355x.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("rtdetr_sliced_probe needs a GPU: nothing was measured")
    w = synth.rtdetr_l_weights(1)
    frame = synth.synthetic_frame(H, W, seed=11)
    tiles = [[int(v) for v in t] for t in _lib.slice_bboxes(H, W, SLICE, SLICE, OVERLAP, OVERLAP)] + [[0, 0, W, H]]
    crops = [np.ascontiguousarray(frame[y0:y1, x0:x1]) for x0, y0, x1, y1 in tiles]
    res = {"device": "MI355X", "frame": [H, W], "slice": SLICE, "overlap": OVERLAP, "imgsz": IMGSZ, "tiles": len(tiles), "weights": "synthetic",
           "repeats": a.repeats, "clock": "host perf_counter around synchronous calls, (a) and (b) alternating", "runs": []}
    for prec_name, prec in (("f32", _lib.PREC_F32), ("f32x3", _lib.PREC_F32X3)):
        det = _lib.RTDETRDetector(w, precision=prec)
        for mb in (4, 8, 16, 32):
            det.drop_plans()
            for _ in range(3):                                  # build, capture, replay
                ra = det.infer_tiles(frame, tiles, IMGSZ, CONF, "local", max_batch=mb)
            mem = det.mem_bytes()
            for _ in range(2):
                rb = by_crops(det, crops, mb)
            same = all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(ra, rb))
            ta, tb = [], []
            for _ in range(a.repeats):
                t = time.perf_counter()
                det.infer_tiles(frame, tiles, IMGSZ, CONF, "local", max_batch=mb)
                ta.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                by_crops(det, crops, mb)
                tb.append((time.perf_counter() - t) * 1e3)
            run = {"precision": prec_name, "max_batch": mb, "chunks": _lib.tile_chunks(len(tiles), mb), "plan_bytes": mem["plans"],
                   "plans_resident": mem["plans_resident"], "graph_state": det.info()["graph_state"], "detections": int(sum(len(r) for r in ra)),
                   "tiles_equal_host_crops": bool(same), "infer_tiles": summary(ta), "host_crops_predict": summary(tb)}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:                          # kept current: a later step that fails loses nothing measured so far
                json.dump(res, f, indent=1)
        det.close()
    fits = [mb for mb in (4, 8, 16, 32) if all(r["plan_bytes"] < LIMIT for r in res["runs"] if r["max_batch"] == mb)]
    f32 = {r["max_batch"]: r["infer_tiles"]["median_ms"] for r in res["runs"] if r["precision"] == "f32"}
    best = min(fits, key=lambda mb: f32[mb]) if fits else None
    res["default_max_batch"] = {"rule": "fastest infer_tiles median in f32 among sizes whose plans stay under 8e9 bytes in both precisions",
                                "under_limit": fits, "choice": best}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["default_max_batch"]))


if __name__ == "__main__":
    main()

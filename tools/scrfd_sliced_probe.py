"""Sliced SCRFD prediction on one MI355X: which max_batch, and is the fused call faster than the Python path on the same commit?

Input: a 2160 x 3840 synthetic frame, 512-pixel slices at overlap 0.2 plus the full frame (61 items), det size 640, the full-size synthetic
model synth.scrfd_onnx(0), FFP_PREC_F32 and FFP_PREC_F32X3. For max_batch in 8, 16, 32 and 0 (all 61 items in one batch), per precision:
  (a) FaceDetector.sliced_predict (ffp_scrfd_sliced_predict): frame up once, chunks, the wrapper's conversion and the merge on the device;
  (b) FFP_PREC_F32 only: sahi's get_sliced_prediction with InsightFaceDetectionModel through compat, the path that existed before: one
      61-item batch (ffp_scrfd_infer_tiles), then per face in Python the conversion, the shift and the merge.
Host clock around synchronous calls, after warm-up of every plan (build, then hipGraph capture); (a) and (b) alternate within one process,
`--repeats` times each, and the file keeps every sample, the median and the min..max spread, so a difference can be judged against the
run-to-run spread. Device bytes held by the plans are read after (a)'s warm-up from a detector holding only that size's plans.

A frame on which a box's far corner is negative after the clip fails in (a) and in (b) alike (sahi's BoundingBox raises), so the probe
takes the first (threshold, seed) of a short list on which the fused call succeeds, and records which.

Every GPU step runs under a time limit of its own (a watchdog thread ends the process: a call stuck in the driver never returns to Python).

The default max_batch rule: the fastest (a) in FFP_PREC_F32 (the precision FaceAnalysis runs) among the sizes whose plans stay under 8 GB in
both precisions.

    python tools/scrfd_sliced_probe.py [--repeats 10] [--out profiles/scrfd_sliced_mi355x.json]
"""
import argparse
import contextlib
import faulthandler
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ffp_amd  # noqa: E402,F401
from ffp_amd import _lib, synth  # noqa: E402

H, W, SLICE, OVERLAP, DET, NMS = 2160, 3840, 512, 0.2, (640, 640), 0.4
LIMIT = 8 * 1000 ** 3
BATCHES = (8, 16, 32, 0)


@contextlib.contextmanager
def step(name, seconds):
    """One GPU step under its own time limit: past it the traceback is printed and the process exits."""
    print(f"[step] {name} (limit {seconds} s)", flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def summary(samples):
    return {"median_ms": round(statistics.median(samples), 3), "min_ms": round(min(samples), 3), "max_ms": round(max(samples), 3),
            "samples_ms": [round(s, 3) for s in samples]}


def fused(det, frame, thr, mb):
    return det.sliced_predict(frame, SLICE, SLICE, OVERLAP, OVERLAP, True, DET, thr, NMS, thr, max_batch=mb, tile_cap=4096, cap=1 << 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrfd_sliced_mi355x.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("scrfd_sliced_probe needs a GPU: nothing was measured")
    onnx, _ = synth.scrfd_onnx(0)
    n_items = len(_lib.slice_bboxes(H, W, SLICE, SLICE, OVERLAP, OVERLAP)) + 1
    res = {"device": "MI355X", "frame": [H, W], "slice": SLICE, "overlap": OVERLAP, "det_size": list(DET), "items": n_items,
           "model": "synth.scrfd_onnx(0)", "repeats": a.repeats,
           "clock": "host perf_counter around synchronous calls, (a) and (b) alternating", "runs": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                              # kept current: a later step that fails loses nothing measured so far
            json.dump(res, f, indent=1)

    det = _lib.FaceDetector(onnx, precision=_lib.PREC_F32)
    frame = thr = None
    refused = []
    with step("find a frame the reference does not raise on", 420):
        for t, seed in [(t, s) for t in (0.5, 0.7, 0.9) for s in (11, 12, 13)]:
            cand = synth.synthetic_frame(H, W, seed=seed)
            try:
                fused(det, cand, t, 16)
            except _lib.FfpError as e:
                if "cannot be negative" not in str(e):
                    raise
                refused.append({"thresh": t, "seed": seed, "error": str(e)[:160]})
                continue
            frame, thr = cand, t
            res["frame_seed"], res["thresh"] = seed, t
            break
    res["frames_the_reference_raises_on"] = refused
    save()
    if frame is None:
        raise SystemExit("every candidate frame has a box with a negative far corner: nothing was measured")

    # (b) the Python path: the synthetic file installed as buffalo_l's detector under a temporary HOME
    home = tempfile.mkdtemp(prefix="scrfd_probe_home_")
    pack = os.path.join(home, ".insightface", "models", "buffalo_l")
    os.makedirs(pack)
    with open(os.path.join(pack, "det_10g.onnx"), "wb") as f:
        f.write(onnx)
    os.environ["HOME"] = home
    import ffp_amd.compat as compat
    compat.install()
    from sahi.predict import get_sliced_prediction
    from utils.insightface_wrapper import InsightFaceDetectionModel
    py_model = InsightFaceDetectionModel(confidence_threshold=thr)

    def python_path():
        return get_sliced_prediction(image=frame, detection_model=py_model, slice_height=SLICE, slice_width=SLICE, overlap_height_ratio=OVERLAP,
                                     overlap_width_ratio=OVERLAP, verbose=0).object_prediction_list

    with step("warm the Python path", 300):
        for _ in range(2):
            py = python_path()
    res["python_path_detections"] = len(py)

    for prec_name, prec in (("f32", _lib.PREC_F32), ("f32x3", _lib.PREC_F32X3)):
        if prec != _lib.PREC_F32:
            det.close()
            det = _lib.FaceDetector(onnx, precision=prec)
        for mb in BATCHES:
            with step(f"{prec_name} max_batch {mb}: warm", 300):
                det.drop_plans()
                for _ in range(3):                               # build, capture, replay
                    ra = fused(det, frame, thr, mb)
                mem = det.mem_bytes()
            ta, tb = [], []
            with step(f"{prec_name} max_batch {mb}: {a.repeats} alternating repeats", 600):
                for _ in range(a.repeats):
                    t = time.perf_counter()
                    fused(det, frame, thr, mb)
                    ta.append((time.perf_counter() - t) * 1e3)
                    if prec == _lib.PREC_F32:
                        t = time.perf_counter()
                        python_path()
                        tb.append((time.perf_counter() - t) * 1e3)
            run = {"precision": prec_name, "max_batch": mb, "chunks": _lib.tile_chunks(n_items, mb or n_items), "plan_bytes": mem["plans"],
                   "plans_resident": mem["plans_resident"], "detections": int(len(ra)), "sliced_predict": summary(ta)}
            if tb:
                same = len(py) == len(ra) and all([float(v) for v in p.bbox.to_xyxy()] == [float(v) for v in r[:4]] for p, r in zip(py, ra))
                run["python_path"] = summary(tb)
                run["equals_python_path"] = bool(same)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            save()
    det.close()
    shutil.rmtree(home, ignore_errors=True)
    fits = [mb for mb in BATCHES if all(r["plan_bytes"] < LIMIT for r in res["runs"] if r["max_batch"] == mb)]
    f32 = {r["max_batch"]: r["sliced_predict"]["median_ms"] for r in res["runs"] if r["precision"] == "f32"}
    best = min(fits, key=lambda mb: f32[mb]) if fits else None
    res["default_max_batch"] = {"rule": "fastest sliced_predict median in f32 among sizes whose plans stay under 8e9 bytes in both precisions",
                                "under_limit": fits, "choice": best}
    save()
    print(json.dumps(res["default_max_batch"]))


if __name__ == "__main__":
    main()

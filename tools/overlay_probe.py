"""The tail of a frame after the detector, measured (the figures README quotes and the route switches of compat/utils/visualization.py rest on):
utils.visualization.draw_detections and save_face_crops on a 3840 x 2160 JPEG tiled from a photograph fixture, file on disk to file(s) on disk,
on both routes in one process, alternating:
    device   the frame is decoded into device memory and stays there: csrc/overlay.hip draws on it / the crops are views of it, and only files come back
    host     the code path of before this route existed, forced with the module's switch (DRAW_DEVICE_ROUTE = False /
             CROPS_DEVICE_ROUTE_MIN_CROPS = None): cv2.imread brings the frame down, Pillow draws, cv2.imwrite sends it up again, once per file
draw_detections with 0, 32 and 512 detections that carry keypoints (show_keypoints=True), save_face_crops with 1, 32 and 512 crops of 24-96 px.
Median of 10 after one warm-up of each route, with min..max. The files of the two routes are compared byte for byte before a time counts.

    python tools/overlay_probe.py [--out profiles/overlay_mi355x.json]

One visit: every step is a child process under its own time limit, and the first one that fails or runs out of time ends the visit. The routing rule
is the codecs': a device route is taken by default only where its slowest sample beats the host route's fastest."""
import argparse
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from png_encode_probe import _stats, _tiled  # noqa: E402

STEPS = [("draw_0", 300), ("draw_32", 300), ("draw_512", 400), ("crops_1", 300), ("crops_32", 300), ("crops_512", 400)]
N = 10


def _detections(n, h, w, lo, hi, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    dets = []
    for _ in range(n):
        s = float(rng.uniform(lo, hi))
        x, y = float(rng.uniform(0, w - s - 1)), float(rng.uniform(30, h - s - 1))
        k = [[x + s * fx, y + s * fy, float(rng.uniform(0.35, 1.0))] for fx, fy in ((0.3, 0.35), (0.7, 0.35), (0.5, 0.55), (0.35, 0.75), (0.65, 0.75))]
        dets.append(SimpleNamespace(bbox=SimpleNamespace(to_xyxy=lambda b=(x, y, x + s, y + s): list(b)), score=SimpleNamespace(value=float(rng.uniform(0.3, 0.99))),
                                    keypoints=k))
    return SimpleNamespace(object_prediction_list=dets)


def _step(name):
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (its HIP runtime first, as the tests do)
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib, compat
    compat.install()
    from utils import visualization as V
    kind, n = name.split("_")
    n = int(n)
    h, w = 2160, 3840
    work = tempfile.mkdtemp(prefix="overlay_probe_")
    src = os.path.join(work, "frame.jpg")
    with open(src, "wb") as fh:
        fh.write(_lib.jpeg_encode(_tiled(h, w, 0), 92, bgr=True))
    res = _detections(n, h, w, 24, 96, 5) if kind == "crops" else _detections(n, h, w, 40, 280, 6)
    switch = "DRAW_DEVICE_ROUTE" if kind == "draw" else "CROPS_DEVICE_ROUTE_MIN_CROPS"
    on, off = (True, False) if kind == "draw" else (1, None)

    def files(tag):
        d = os.path.join(work, tag)
        return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}

    def run(route):
        setattr(V, switch, on if route == "device" else off)
        before = dict(V.ROUTE_CALLS)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            if kind == "draw":
                V.draw_detections(src, res, os.path.join(work, route, "overlay.jpg"), show_keypoints=True)
            else:
                V.save_face_crops(src, res, os.path.join(work, route))
        ms = (time.perf_counter() - t0) * 1e3
        took = [k for k in before if V.ROUTE_CALLS[k] != before[k]]
        assert took == [f"{kind}_{route}"], f"asked for the {route} route, took {took}"
        return ms

    for route in ("host", "device"):                                   # warm-up: code objects, workspaces, the font, the stamp cache
        run(route)
    a, b = files("host"), files("device")
    assert list(a) == list(b) and len(a) == (1 if kind == "draw" else n) and all(a[f] == b[f] for f in a), "the two routes wrote different files"
    ms = {"host": [], "device": []}
    for _ in range(N):
        for route in ("host", "device"):
            ms[route].append(run(route))
    assert files("host") == files("device")
    out = {"height": h, "width": w, "source_bytes": os.path.getsize(src), "files_written": len(a), "bytes_written": sum(len(v) for v in a.values()),
           "host": _stats(ms["host"]), "device": _stats(ms["device"])}
    if kind == "draw":
        prims, masks, _ = V.build_overlay_prims(res, w, h)
        out["primitives"], out["mask_bytes"] = int(len(prims)), int(masks.size)
        t = []
        for _ in range(N):                                              # the share of the device route that is the list being built on the host
            t0 = time.perf_counter()
            V.build_overlay_prims(res, w, h)
            t.append((time.perf_counter() - t0) * 1e3)
        out["builder_alone"] = _stats(t)
    out["device_slowest_beats_host_fastest"] = out["device"]["max_ms"] < out["host"]["min_ms"]
    shutil.rmtree(work, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_mi355x.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(_step(a.step)))
        return 0
    res = {"what": "utils.visualization.draw_detections (n detections with keypoints, show_keypoints=True, .jpg out) and save_face_crops (n crops of 24-96 px) on a "
                   "3840 x 2160 JPEG, file on disk to file(s) on disk, wall clock around the call, both routes alternating in one process, median of 10 after one "
                   "warm-up each; tools/overlay_probe.py",
           "host_route": "the code path of before the device routes (cv2.imread -> Pillow -> cv2.imwrite per file), forced with the module switch "
                         "DRAW_DEVICE_ROUTE = False / CROPS_DEVICE_ROUTE_MIN_CROPS = None",
           "steps": {}}
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result inside {limit} s; the visit ends here", file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{name}: exit {r.returncode}; the visit ends here\n{r.stdout[-2000:]}", file=sys.stderr)
            return 1
        res["steps"][name] = json.loads(line[-1][7:])
        print(name, json.dumps(res["steps"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    draw = [v for k, v in res["steps"].items() if k.startswith("draw_")]
    res["draw_device_route_by_default"] = all(v["device_slowest_beats_host_fastest"] for v in draw)
    wins = [int(k.split("_")[1]) for k, v in res["steps"].items() if k.startswith("crops_") and v["device_slowest_beats_host_fastest"]]
    loses = [int(k.split("_")[1]) for k, v in res["steps"].items() if k.startswith("crops_") and not v["device_slowest_beats_host_fastest"]]
    # the smallest measured count from which the device route wins at every measured count; None: it loses at the largest
    res["crops_device_route_min_crops"] = min((c for c in wins if all(c > l for l in loses)), default=None)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("draw device route by default:", res["draw_device_route_by_default"], "| crops device route from", res["crops_device_route_min_crops"], "crops")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Files that carry an EXIF orientation, measured (the figures README and DESIGN.md quote and the ORIENT_DEVICE_ROUTE switches of
compat/cv2, compat/sahi/utils/cv.py and compat/utils/visualization.py rest on): a 3840 x 2160 JPEG tiled from a photograph fixture, saved with the
tags 6 (a quarter turn: the transposing kind) and 3 (a half turn: mirrors only), through the four calls that read such a file, on both routes in
one process, alternating:
    device   the tag is read from the file's bytes (csrc/exif.hpp) and the frame is turned where it was decoded (csrc/orient.hip)
    host     the code path of before, forced with the three module switches (ORIENT_DEVICE_ROUTE = False): cv2.imread decodes on the device, brings
             the frame down and turns it with numpy; read_image_as_array leaves the file to Pillow; draw_detections and save_face_crops take their
             host routes (cv2.imread, Pillow drawing, one cv2.imwrite per file)
cv2.imread, read_image_as_array, draw_detections with 32 detections, save_face_crops with 32 crops: wall clock around the call, median of 10 after
one warm-up of each route, with min..max; the results of the two routes are compared bit for bit before a time counts. And the orient launch alone,
between two events, beside a device-to-device copy of the same bytes (what the memory system allows), for both tags.

    python tools/orient_probe.py [--out profiles/orient_mi355x.json]

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from overlay_probe import _detections  # noqa: E402
from png_encode_probe import _stats, _tiled  # noqa: E402

TAGS = (6, 3)
STEPS = [("imread", 300), ("read_array", 300), ("draw_32", 300), ("crops_32", 300), ("kernel", 200)]
N = 10
H, W = 2160, 3840


def _exif_app1(tag):
    tiff = b"II*\x00\x08\x00\x00\x00\x01\x00\x12\x01\x03\x00\x01\x00\x00\x00" + bytes([tag, 0, 0, 0]) + b"\x00\x00\x00\x00"
    body = b"Exif\x00\x00" + tiff
    return b"\xff\xe1" + (len(body) + 2).to_bytes(2, "big") + body


def _step(name):
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch  # (its HIP runtime first, as the tests do)
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib, compat
    compat.install()
    import cv2
    from sahi.utils import cv as sahi_cv
    from utils import visualization as V
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    out = {"height": H, "width": W}
    if name == "kernel":
        frame = torch.from_numpy(_tiled(H, W, 0).reshape(-1)).cuda()
        dst = torch.empty_like(frame)
        torch.cuda.synchronize()
        for tag in TAGS:
            k, c = [], []
            for _ in range(N):
                a, b = _lib.image_orient_time_dev(frame.data_ptr(), H, W, 3, tag, dst.data_ptr(), dst.numel(), iters=400)
                k.append(a)
                c.append(b)
            us = lambda v: {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "n": len(v)}
            ks, cs = us(k), us(c)
            out[f"tag_{tag}"] = {"orient_launch": ks, "device_to_device_copy": cs, "bytes": int(frame.numel()),
                                 "launch_over_copy": round(ks["median_us"] / cs["median_us"], 2),
                                 "launch_gb_per_s_read_plus_written": round(2 * frame.numel() / ks["median_us"] / 1e3, 1),
                                 "copy_gb_per_s_read_plus_written": round(2 * frame.numel() / cs["median_us"] / 1e3, 1)}
        return out
    work = tempfile.mkdtemp(prefix="orient_probe_")
    plain = _lib.jpeg_encode(_tiled(H, W, 0), 92, bgr=True)
    assert plain[:2] == b"\xff\xd8"
    mods = (cv2, sahi_cv, V)

    def switches(route):
        for m in mods:
            m.ORIENT_DEVICE_ROUTE = route == "device"

    for tag in TAGS:
        src = os.path.join(work, f"frame_{tag}.jpg")
        with open(src, "wb") as fh:
            fh.write(plain[:2] + _exif_app1(tag) + plain[2:])
        ow, oh = (H, W) if tag >= 5 else (W, H)
        res = _detections(32, oh, ow, 24, 96, 5) if name.startswith("crops") else _detections(32, oh, ow, 40, 280, 6)
        kept = {}

        def run(route):
            switches(route)
            before = dict(V.ROUTE_CALLS)
            turned = _lib.image_orient_stats()[0]
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                if name == "imread":
                    kept[route] = cv2.imread(src)
                elif name == "read_array":
                    kept[route] = sahi_cv.read_image_as_array(src)
                elif name == "draw_32":
                    V.draw_detections(src, res, os.path.join(work, f"{route}_{tag}", "overlay.jpg"), show_keypoints=True)
                else:
                    V.save_face_crops(src, res, os.path.join(work, f"{route}_{tag}"))
            ms = (time.perf_counter() - t0) * 1e3
            if name in ("draw_32", "crops_32"):
                took = [k for k in before if V.ROUTE_CALLS[k] != before[k]]
                assert took == [f"{name.split('_')[0]}_{route}"], f"asked for the {route} route, took {took}"
            assert (_lib.image_orient_stats()[0] != turned) == (route == "device"), f"the {route} route and the orient kernel"
            return ms

        def same():
            if name in ("imread", "read_array"):
                assert kept["host"].shape == (oh, ow, 3) and np.array_equal(kept["host"], kept["device"]), "the two routes read different frames"
                return
            a, b = ({f: open(os.path.join(work, f"{r}_{tag}", f), "rb").read() for f in sorted(os.listdir(os.path.join(work, f"{r}_{tag}")))} for r in ("host", "device"))
            assert list(a) == list(b) and len(a) == (1 if name == "draw_32" else 32) and all(a[f] == b[f] for f in a), "the two routes wrote different files"

        for route in ("host", "device"):                               # warm-up: code objects, workspaces, the font, the stamp cache
            run(route)
        same()
        ms = {"host": [], "device": []}
        for _ in range(N):
            for route in ("host", "device"):
                ms[route].append(run(route))
        same()
        r = {"source_bytes": os.path.getsize(src), "host": _stats(ms["host"]), "device": _stats(ms["device"])}
        r["device_slowest_beats_host_fastest"] = r["device"]["max_ms"] < r["host"]["min_ms"]
        out[f"tag_{tag}"] = r
    shutil.rmtree(work, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_mi355x.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(_step(a.step)))
        return 0
    res = {"what": "a 3840 x 2160 JPEG with EXIF orientation 6 and 3 through cv2.imread, read_image_as_array, draw_detections (32 detections with keypoints, .jpg "
                   "out) and save_face_crops (32 crops of 24-96 px), wall clock around the call, both routes alternating in one process, median of 10 after one "
                   "warm-up each; and the orient launch alone between two events (400 launches per sample, about 10 ms) beside a device-to-device copy of the same bytes; "
                   "tools/orient_probe.py",
           "host_route": "the code path of before the device orientation, forced with ORIENT_DEVICE_ROUTE = False in compat/cv2, compat/sahi/utils/cv.py and "
                         "compat/utils/visualization.py",
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
    wins = lambda step: all(res["steps"][step][f"tag_{t}"]["device_slowest_beats_host_fastest"] for t in TAGS)
    res["orient_device_route_by_default"] = {"compat/cv2": wins("imread"), "compat/sahi/utils/cv.py": wins("read_array"),
                                             "compat/utils/visualization.py": wins("draw_32") and wins("crops_32")}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("device orientation by default:", res["orient_device_route_by_default"])
    return 0


if __name__ == "__main__":
    sys.exit(main())

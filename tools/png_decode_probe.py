"""Reading PNG, measured (the figures README quotes and the routing of the cv2 / sahi shims rests on): from the file in host memory to the finished
array in host memory, for the frames of tools/png_encode_probe.py (three 3840 x 2160 contents, one 15360 x 8640 frame), each as two files: the one
the device encoder writes (segmented: ffp_png_decode inflates it on the device, one wave per IDAT) and the same pixels re-saved by Pillow at
compress_level=1 (one zlib stream: ffp_png_decode inflates it on the host). Decoders:
    device_parallel          ffp_png_decode on the device's file
    device_serial_flag       the same file with FFP_PNG_DEC_SERIAL (the A/B partner)
    library_serial           ffp_png_decode on Pillow's file (the serial route)
    pillow_on_device_file    np.asarray(Image.open(...).convert("RGB")) on the device's file
    pillow_on_pillow_file    the same on Pillow's file
Median of 10 after one warm-up with min..max. Every result is compared with the frame before
its time counts.

    python tools/png_decode_probe.py [--out profiles/png_decode_mi355x.json]

One visit: every step is a child process under its own time limit, and the first one that fails or runs out of time ends the visit. The routing
rule is the encoder's: a route is taken by the shims with no switch only where its slowest sample beats Pillow's fastest on all four frames."""
import argparse
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from png_encode_probe import _overlay, _stats, _tiled  # noqa: E402

STEPS = [("4k_photo_tiled", 300), ("4k_photo_tiled_noise3", 300), ("4k_overlay_on_flat", 300), ("16k_photo_tiled_noise3", 1000)]


def _timed(fn, n, check):
    out = fn()                                                        # warm-up: code objects, workspaces, page cache of the allocator
    assert check(out), "a decoder returned other pixels than the frame"
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert check(out)
    return _stats(ms)


def _frame_step(name):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (its HIP runtime first, as the tests do)
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib
    Image.MAX_IMAGE_PIXELS = None
    big = name.startswith("16k")
    h, w = (8640, 15360) if big else (2160, 3840)
    bgr = _overlay(h, w) if "overlay" in name else _tiled(h, w, 3 if "noise" in name else 0)
    rgb = np.ascontiguousarray(bgr[..., ::-1])
    dev_file = _lib.png_encode(bgr, bgr=True)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "PNG", compress_level=1)
    pil_file = b.getvalue()
    n_host = 10

    def same(a):
        return a.shape == rgb.shape and np.array_equal(a, rgb)

    def pillow(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    res = {"height": h, "width": w, "device_file_bytes": len(dev_file), "pillow_file_bytes": len(pil_file)}
    s0 = _lib.png_decode_stats()
    res["device_parallel"] = _timed(lambda: _lib.png_decode(dev_file), 10, same)
    s1 = _lib.png_decode_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (11, 0), "the device's file did not take the parallel route"
    print(name, "device_parallel", res["device_parallel"], file=sys.stderr, flush=True)
    res["device_serial_flag"] = _timed(lambda: _lib.png_decode(dev_file, flags=_lib.FFP_PNG_DEC_SERIAL), n_host, same)
    print(name, "device_serial_flag", res["device_serial_flag"], file=sys.stderr, flush=True)
    res["library_serial"] = _timed(lambda: _lib.png_decode(pil_file), n_host, same)
    s2 = _lib.png_decode_stats()
    assert s2[0] == s1[0], "Pillow's file took the parallel route"
    print(name, "library_serial", res["library_serial"], file=sys.stderr, flush=True)
    res["pillow_on_device_file"] = _timed(lambda: pillow(dev_file), n_host, same)
    print(name, "pillow_on_device_file", res["pillow_on_device_file"], file=sys.stderr, flush=True)
    res["pillow_on_pillow_file"] = _timed(lambda: pillow(pil_file), n_host, same)
    res["parallel_slowest_beats_pillow_fastest"] = res["device_parallel"]["max_ms"] < res["pillow_on_device_file"]["min_ms"]
    res["serial_slowest_beats_pillow_fastest"] = res["library_serial"]["max_ms"] < res["pillow_on_pillow_file"]["min_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_mi355x.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(_frame_step(a.step)))
        return 0
    res = {"what": "ffp_png_decode (file in host memory -> array in host memory, wall clock around the call, median of n after one warm-up) against "
                   "Pillow's PNG reader on the same machine and files; tools/png_decode_probe.py", "frames": {}}
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
        res["frames"][name] = json.loads(line[-1][7:])
        print(name, json.dumps(res["frames"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    res["parallel_route_by_default"] = all(v["parallel_slowest_beats_pillow_fastest"] for v in res["frames"].values())
    res["serial_route_by_default"] = all(v["serial_slowest_beats_pillow_fastest"] for v in res["frames"].values())
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("parallel route by default:", res["parallel_route_by_default"], "| serial route by default:", res["serial_route_by_default"])
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""PNG at the file boundaries, measured (the figures README quotes and the cv2 shim's default rests on): ffp_png_encode_dev on a frame
resident on the device, from the call to the finished file on the host, against Pillow (libpng + zlib, one core) at compress_level=1
(OpenCV's default for PNG) and at Pillow's default, on the same machine and the same pixels.

    python tools/png_encode_probe.py [--out profiles/png_encode_mi355x.json]

One visit: every step is a child process under its own time limit, and the first one that fails or runs out of time ends the visit.
Steps: three 3840 x 2160 BGR contents (a photograph fixture tiled; the same with +-3 noise; a drawn overlay on a flat background), one
15360 x 8640 frame, and the compression ratios of the photograph fixtures against zlib level 1 (tests/test_gpu_png.py asserts their
worst, rounded up to the next 0.05). Each device file is decoded by Pillow and compared with the pixels before its time counts."""
import argparse
import io
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = [("4k_photo_tiled", 240), ("4k_photo_tiled_noise3", 240), ("4k_overlay_on_flat", 240), ("16k_photo_tiled_noise3", 420), ("fixture_ratios", 120)]


def _photo():
    import numpy as np
    from PIL import Image
    return np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "real", "det_family.png")).convert("RGB"))


def _tiled(h, w, noise):
    import numpy as np
    p = _photo()
    a = np.tile(p, (-(-h // p.shape[0]), -(-w // p.shape[1]), 1))[:h, :w]
    if noise:
        rng = np.random.default_rng(0)
        a = np.clip(a.astype(np.int16) + rng.integers(-noise, noise + 1, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(a[..., ::-1])                    # BGR, as the frame lies on the device


def _overlay(h, w):
    import numpy as np
    from PIL import Image, ImageDraw
    im = Image.new("RGB", (w, h), (38, 42, 48))
    d = ImageDraw.Draw(im)
    rng = np.random.default_rng(1)
    for k in range(120):                                          # what draw_detections leaves: boxes, label plates, text, landmarks
        x, y = int(rng.integers(0, w - 300)), int(rng.integers(40, h - 300))
        s = int(rng.integers(40, 280))
        d.rectangle([x, y, x + s, y + s], outline=(0, 255, 0), width=2)
        d.rectangle([x, y - 18, x + 70, y], fill=(0, 255, 0))
        d.text((x + 2, y - 16), f"Face: 0.{int(rng.integers(50, 99))}", fill=(0, 0, 0))
        for _ in range(5):
            cx, cy = x + int(rng.integers(5, s - 5)), y + int(rng.integers(5, s - 5))
            d.ellipse([cx - 3, cy - 3, cx + 3, cy + 3], fill=(255, 0, 0), outline=(255, 255, 255))
    return np.ascontiguousarray(np.asarray(im)[..., ::-1])


def _stats(ms):
    ms = sorted(ms)
    n = len(ms)
    return {"median_ms": round((ms[(n - 1) // 2] + ms[n // 2]) / 2, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "n": n}


def _frame_step(name):
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib
    Image.MAX_IMAGE_PIXELS = None
    big = name.startswith("16k")
    h, w = (8640, 15360) if big else (2160, 3840)
    bgr = _overlay(h, w) if "overlay" in name else _tiled(h, w, 3 if "noise" in name else 0)
    d = torch.from_numpy(bgr).cuda()
    torch.cuda.synchronize()
    data = _lib.png_encode_dev(d.data_ptr(), h, w, 3, 8, w * 3, bgr=True)              # warm-up: code objects, workspace
    back = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(back, bgr[..., ::-1]), "the device's file does not decode to the frame"
    dev = []
    for _ in range(10):
        t0 = time.perf_counter()
        out = _lib.png_encode_dev(d.data_ptr(), h, w, 3, 8, w * 3, bgr=True)
        dev.append((time.perf_counter() - t0) * 1e3)
        assert out == data
    stored = len(_lib.png_encode_dev(d.data_ptr(), h, w, 3, 8, w * 3, level=0, bgr=True))
    rgb = Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]))
    res = {"height": h, "width": w, "device": dict(_stats(dev), file_bytes=len(data)), "device_level0_file_bytes": stored, "raw_bytes": int(bgr.nbytes)}
    for key, kw in (("pillow_level1", {"compress_level": 1}), ("pillow_default", {})):
        ms, size = [], 0
        for _ in range(1 if big else 3):
            b = io.BytesIO()
            t0 = time.perf_counter()
            rgb.save(b, "PNG", **kw)
            ms.append((time.perf_counter() - t0) * 1e3)
            size = b.tell()
        res[key] = dict(_stats(ms), file_bytes=size)
    res["device_slowest_beats_pillow_level1_fastest"] = res["device"]["max_ms"] < res["pillow_level1"]["min_ms"]
    return res


def _ratio_step():
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib
    import png_ref
    real = os.path.join(ROOT, "tests", "golden", "real")
    out = {}
    for f in sorted(os.listdir(real)):
        if f.endswith(".png"):
            p = png_ref.parse(_lib.png_encode(np.asarray(Image.open(os.path.join(real, f)).convert("RGB"))))
            out[f] = round(len(p["idat"]) / len(zlib.compress(p["filtered"], 1)), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_mi355x.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(_ratio_step() if a.step == "fixture_ratios" else _frame_step(a.step)))
        return 0
    res = {"what": "ffp_png_encode_dev (frame resident on the device -> file on the host, wall clock around the call, median of 10 after one warm-up) "
                   "against Pillow's PNG writer on the same machine and pixels; tools/png_encode_probe.py", "frames": {}}
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result inside {limit} s; the visit ends here", file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{name}: exit {r.returncode}; the visit ends here\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 1
        val = json.loads(line[-1][7:])
        if name == "fixture_ratios":
            res["fixture_ratios"] = val
            res["fixture_ratio_worst"] = max(val.values())
        else:
            res["frames"][name] = val
        print(name, json.dumps(val), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    four_k = [v for k, v in res["frames"].items() if k.startswith("4k")]
    res["device_by_default"] = all(v["device_slowest_beats_pillow_level1_fastest"] for v in four_k)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("device by default:", res["device_by_default"])
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Batched JPEG decode against the per-file loop, on one MI355X, in one process -> profiles/jpeg_decode_batch_mi355x.json.

    python tools/jpeg_batch_probe.py [--baseline-lib PATH] [--out profiles/jpeg_decode_batch_mi355x.json] [--no-crops-dir]

"decode": n in {1, 4, 16, 64, 256, 1024} crop files (quality 95, sizes from pipeline.sr_crop_sizes) from host memory to BGR pixels in device
memory, (a) a loop of ffp_jpeg_decode_dev, (b) one ffp_jpeg_decode_batch_dev. Host clock around calls that end in a stream synchronisation;
10 samples per route, the two routes alternating, after one warm-up pass of each; a sample repeats its pass until it has decoded at least
256 files and reports the time of one pass. Median, min and max in milliseconds. The two routes' pixels are compared once per n.

"crops_dir": compat/utils/enhancer.py::enhance_face_crops_batch over a directory of 4, 16, 64 and 256 such files (x4 model, synthetic weights,
tile 400, fp16), the batch route against the route that reads file by file, in the same form.

--single (with --baseline-lib) -> profiles/jpeg_decode_single_mi355x.json: only "single" — one file through ffp_jpeg_decode_dev of the parent
commit's build and of the library under test, a quality-95 crop and a 3840 x 2160 quality-95 4:2:0 frame, in the same form.

--codec-pool (with --baseline-lib) -> profiles/codec_pool_mi355x.json: one call each of ffp_jpeg_encode_dev, ffp_png_encode_dev, ffp_png_decode_dev and
ffp_jpeg_decode_dev (the four entries behind the workspace pool, csrc/ws_pool.hpp) of the parent commit's build and of the library under test, at a
crop size and at 3840 x 2160, in the same form; the files and pixels of the two libraries are compared once per case.

--baseline-lib: a libffp.so built from the PARENT commit. Route (a) and the old crops-directory route then run on it (this change shares
code with the single-file decoder, so the old routes are timed on the code as it was); without it they run on the library under test, and
the file says so."""
import argparse
import ctypes as C
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffp_amd  # noqa: E402,F401
from ffp_amd import _lib, pipeline, synth  # noqa: E402

NS = (1, 4, 16, 64, 256, 1024)
SAMPLES = 10


def load_library(path):
    """a second libffp.so beside the one _lib loaded, with the signatures of the entries it has"""
    _lib.lib()
    l = C.CDLL(path)
    for name, (res, args) in _lib._SIGS.items():
        if hasattr(l, name):
            f = getattr(l, name)
            f.restype, f.argtypes = res, args
    return l


def crop_files(n, seed):
    from PIL import Image
    frame = synth.synthetic_frame(540, 960, seed=seed)
    rng = np.random.default_rng(seed)
    files = []
    for s in pipeline.sr_crop_sizes(n, seed=seed):
        s = int(s)
        y, x = int(rng.integers(0, 540 - s + 1)), int(rng.integers(0, 960 - s + 1))
        b = io.BytesIO()
        Image.fromarray(frame[y:y + s, x:x + s]).save(b, "JPEG", quality=95)
        files.append(b.getvalue())
    return files


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4), "max_ms": round(float(max(ms)), 4), "n": len(ms)}


def alternate(routes, reps):
    """routes: {name: callable}; one warm-up each, then SAMPLES rounds in which every route runs once (reps passes per sample)"""
    for fn in routes.values():
        fn()
    ms = {k: [] for k in routes}
    for _ in range(SAMPLES):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ms[k].append((time.perf_counter() - t0) * 1e3 / reps)
    return {k: summary(v) for k, v in ms.items()}


def decode_probe(base):
    import torch
    out = {}
    for n in NS:
        files = crop_files(n, seed=100 + n)
        sizes = [_lib.jpeg_info(f)[:2] for f in files]
        offs = np.concatenate([[0], np.cumsum([(h * w * 3 + 255) // 256 * 256 for h, w in sizes])])
        cap = int(offs[-1])
        d_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bufs = [np.frombuffer(f, np.uint8) for f in files]
        ptrs = [b.ctypes.data_as(C.POINTER(C.c_uint8)) for b in bufs]

        def single_loop():
            for i in range(n):
                rc = base.ffp_jpeg_decode_dev(0, ptrs[i], len(bufs[i]), 1, C.c_void_p(d_a.data_ptr() + int(offs[i])), 0, cap - int(offs[i]))
                assert rc == 0, rc

        def batch():
            _, _, status = _lib.jpeg_decode_batch_dev(files, d_b.data_ptr(), offs[:-1], None, cap, bgr=True)
            assert not status.any(), status

        r = alternate({"single_file_loop": single_loop, "batch": batch}, reps=max(1, 256 // n))
        assert torch.equal(d_a, d_b), f"the two routes' pixels differ at n = {n}"
        r["file_bytes"] = int(sum(len(f) for f in files))
        r["batch_slowest_beats_loop_fastest"] = bool(r["batch"]["max_ms"] < r["single_file_loop"]["min_ms"])
        out[str(n)] = r
        print(n, json.dumps(r), flush=True)
    return out


def single_probe(base):
    """One file through ffp_jpeg_decode_dev of the parent library and of the library under test (where one file is a batch of one): a quality-95
    crop and a 3840 x 2160 quality-95 4:2:0 frame. Same form as above; "inside" says whether the new median lies in the parent's min-max range."""
    import torch
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(synth.synthetic_frame(2160, 3840, seed=11)).save(b, "JPEG", quality=95, subsampling=2)
    out = {}
    for name, data in (("crop", crop_files(1, seed=101)[0]), ("frame_3840x2160", b.getvalue())):
        h, w, _ = _lib.jpeg_info(data)
        cap = h * w * 3
        bufs = {k: torch.zeros(cap, dtype=torch.uint8, device="cuda") for k in ("parent", "new")}
        torch.cuda.synchronize()
        buf = np.frombuffer(data, np.uint8)
        ptr = buf.ctypes.data_as(C.POINTER(C.c_uint8))

        def route(l, d):
            def go():
                rc = l.ffp_jpeg_decode_dev(0, ptr, len(buf), 1, C.c_void_p(d.data_ptr()), 0, cap)
                assert rc == 0, rc
            return go

        r = alternate({"parent": route(base, bufs["parent"]), "new": route(_lib.lib(), bufs["new"])}, reps=256 if name == "crop" else 16)
        assert torch.equal(bufs["parent"], bufs["new"]), f"the two libraries' pixels differ ({name})"
        r["file_bytes"], r["height"], r["width"] = len(data), h, w
        r["new_median_inside_parent_range"] = bool(r["parent"]["min_ms"] <= r["new"]["median_ms"] <= r["parent"]["max_ms"])
        r["new_median_above_parent_max"] = bool(r["new"]["median_ms"] > r["parent"]["max_ms"])
        out[name] = r
        print("single", name, json.dumps(r), flush=True)
    return out


def codec_pool_probe(base):
    """One call of each of the four codec entries of the parent library and of the library under test, a crop (the size pipeline.sr_crop_sizes draws first)
    and a 3840 x 2160 frame. Same form as single_probe; the two libraries' bytes and pixels are compared."""
    import torch
    from PIL import Image
    cur = _lib.lib()
    s = int(pipeline.sr_crop_sizes(1, seed=101)[0])
    frame = synth.synthetic_frame(2160, 3840, seed=11)
    out = {}
    for name, img in (("crop", np.ascontiguousarray(frame[:s, :s])), ("frame_3840x2160", frame)):
        h, w = img.shape[:2]
        d_img = torch.from_numpy(img).cuda()
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=95)
        jpg = np.frombuffer(b.getvalue(), np.uint8)
        png = np.frombuffer(_lib.png_encode(img), np.uint8)
        cap = max(1024 + h * w * 3, _lib.png_bound(h, w))
        reps = 64 if name == "crop" else 4
        u8 = C.POINTER(C.c_uint8)
        for entry in ("jpeg_encode_dev", "png_encode_dev", "png_decode_dev", "jpeg_decode_dev"):
            host = {k: np.zeros(cap, np.uint8) for k in ("parent", "new")}
            dev = {k: torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda") for k in ("parent", "new")}
            size = {k: C.c_int64(0) for k in ("parent", "new")}
            torch.cuda.synchronize()

            def route(l, k):
                def go():
                    if entry == "jpeg_encode_dev":
                        rc = l.ffp_jpeg_encode_dev(0, C.c_void_p(d_img.data_ptr()), h, w, w * 3, 0, 95, host[k].ctypes.data_as(u8), cap, C.byref(size[k]))
                    elif entry == "png_encode_dev":
                        rc = l.ffp_png_encode_dev(0, C.c_void_p(d_img.data_ptr()), h, w, 3, 8, w * 3, 0, 1, host[k].ctypes.data_as(u8), cap, C.byref(size[k]))
                    elif entry == "png_decode_dev":
                        rc = l.ffp_png_decode_dev(0, png.ctypes.data_as(u8), len(png), 0, 0, C.c_void_p(dev[k].data_ptr()), 0, h * w * 3)
                    else:
                        rc = l.ffp_jpeg_decode_dev(0, jpg.ctypes.data_as(u8), len(jpg), 0, C.c_void_p(dev[k].data_ptr()), 0, h * w * 3)
                    assert rc == 0, (entry, rc)
                return go

            r = alternate({"parent": route(base, "parent"), "new": route(cur, "new")}, reps=reps)
            if entry.endswith("encode_dev"):
                assert size["parent"].value == size["new"].value > 0 and np.array_equal(host["parent"], host["new"]), f"the two libraries' files differ ({entry}, {name})"
                r["file_bytes"] = int(size["new"].value)
            else:
                assert torch.equal(dev["parent"], dev["new"]) and bool(dev["new"].any()), f"the two libraries' pixels differ ({entry}, {name})"
                r["file_bytes"] = int(len(png) if entry == "png_decode_dev" else len(jpg))
            r["height"], r["width"] = h, w
            r["new_median_inside_parent_range"] = bool(r["parent"]["min_ms"] <= r["new"]["median_ms"] <= r["parent"]["max_ms"])
            r["new_median_above_parent_max"] = bool(r["new"]["median_ms"] > r["parent"]["max_ms"])
            out[f"{entry}/{name}"] = r
            print("codec_pool", entry, name, json.dumps(r), flush=True)
    return out


def crops_dir_probe(base):
    from ffp_amd import compat
    compat.install()
    import utils.enhancer as ue
    out = {}
    work = tempfile.mkdtemp(prefix="ffp_jpeg_batch_probe_")
    cur, enh = _lib.lib(), {}
    try:
        for name, l in (("batch_route", cur), ("per_file_read_route", base)):
            _lib._lib = l                                            # an enhancer belongs to the library that made it
            enh[name] = ue.FaceEnhancer(model_path="synthetic:RealESRGAN_x4plus", tile=400, half=True)
        for n in (4, 16, 64, 256):
            d = os.path.join(work, f"n{n}", "crops")
            os.makedirs(d)
            for k, f in enumerate(crop_files(n, seed=200 + n)):
                with open(os.path.join(d, f"img_face_{k}_conf_0.90.jpg"), "wb") as fh:
                    fh.write(f)

            def run(name, min_files, l):
                def go():
                    _lib._lib = l
                    ue.BATCH_ROUTE_MIN_FILES = min_files
                    res = ue.enhance_face_crops_batch(d, enh[name], prefix=name)
                    assert res["statistics"]["successful"] == n, res["statistics"]
                return go

            r = alternate({"batch_route": run("batch_route", 1, cur), "per_file_read_route": run("per_file_read_route", None, base)}, reps=1)
            a, b = os.path.join(work, f"n{n}", "batch_route_enhanced"), os.path.join(work, f"n{n}", "per_file_read_route_enhanced")
            for f in sorted(os.listdir(a)):
                g = f.replace("batch_route_", "per_file_read_route_", 1)
                assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, g), "rb").read(), f
            r["batch_slowest_beats_per_file_fastest"] = bool(r["batch_route"]["max_ms"] < r["per_file_read_route"]["min_ms"])
            out[str(n)] = r
            print("crops_dir", n, json.dumps(r), flush=True)
    finally:
        for name, l in (("per_file_read_route", base), ("batch_route", cur)):          # every enhancer is destroyed by the library that made it
            if name in enh:
                _lib._lib = l
                enh[name].upsampler._sr.close()
        _lib._lib = cur
        shutil.rmtree(work, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_batch_mi355x.json"))
    ap.add_argument("--no-crops-dir", action="store_true")
    ap.add_argument("--single", action="store_true", help="only the single-file section (needs --baseline-lib) -> profiles/jpeg_decode_single_mi355x.json")
    ap.add_argument("--codec-pool", action="store_true", help="only the four codec entries (needs --baseline-lib) -> profiles/codec_pool_mi355x.json")
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing is measured here")
    base = load_library(a.baseline_lib) if a.baseline_lib else _lib.lib()
    if a.codec_pool:
        if not a.baseline_lib:
            raise SystemExit("--codec-pool compares against a build of the parent commit: give --baseline-lib")
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "codec_pool_mi355x.json")
        doc = {"what": "one call of each codec entry, host clock in ms around the call (it ends in a stream synchronisation); median / min / max of 10 samples per "
               "library, the parent commit's build and the library under test alternating in one process on one MI355X after one warm-up pass each; a sample is "
               "the mean of 64 (crop) or 4 (frame) calls; tools/jpeg_batch_probe.py --codec-pool",
               "codec_pool": codec_pool_probe(base)}
        doc["medians_above_parent_max"] = [k for k, r in doc["codec_pool"].items() if r["new_median_above_parent_max"]]
        with open(out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        print("wrote", out)
        return
    if a.single:
        if not a.baseline_lib:
            raise SystemExit("--single compares against a build of the parent commit: give --baseline-lib")
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "jpeg_decode_single_mi355x.json")
        doc = {"what": "one file through ffp_jpeg_decode_dev, host clock in ms around the call (it ends in a stream synchronisation); median / min / max of 10 samples per "
               "library, the parent commit's build and the library under test alternating in one process on one MI355X after one warm-up pass each; a sample is "
               "the mean of 256 (crop) or 16 (frame) calls; tools/jpeg_batch_probe.py --single",
               "single": single_probe(base)}
        with open(out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        print("wrote", out)
        return
    doc = {"what": "host clock in ms around calls that end in a stream synchronisation; median / min / max of 10 samples per route, the two routes alternating in one process "
           "on one MI355X after one warm-up pass each; tools/jpeg_batch_probe.py",
           "old_routes_run_on": "a build of the parent commit" if a.baseline_lib else "the library under test",
           "decode": decode_probe(base)}
    if not a.no_crops_dir:
        doc["crops_dir"] = crops_dir_probe(base)
        wins = [int(n) for n, r in doc["crops_dir"].items() if r["batch_slowest_beats_per_file_fastest"]]
        doc["crops_dir_min_files"] = min(wins) if wins else None
    wins = [n for n in NS if doc["decode"][str(n)]["batch_slowest_beats_loop_fastest"]]
    doc["decode_min_files"] = min(wins) if wins else None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

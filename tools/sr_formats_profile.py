"""Per-call time and kernel times of RealESRGANer.enhance's layouts on one GPU (x4, 23 blocks, synthetic weights, fp16).

    python tools/sr_formats_profile.py --out profiles/sr_formats.json            # timing, then one rocprofv3 run per case

Cases: 3-channel, gray, BGRA with each alpha upsampler and 16-bit BGR, all 200x200 with tile 400; and a 400x400 BGR call with
outscale 3.5 (1600x1600 -> 1400x1400 Lanczos4). Call time is a host clock around the synchronous call (median of --iters after
two warm-ups, with the profiler off); kernel times come from `rocprofv3 --kernel-trace --stats` on child processes that make
the same calls, as the difference of a 12-call and a 2-call run over 10 (steady state: plan set-up cancels out).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "bgr_u8": dict(kind="bgr", size=200),
    "gray_u8": dict(kind="gray", size=200),
    "bgra_u8_realesrgan": dict(kind="bgra", size=200, alpha="realesrgan"),
    "bgra_u8_cv2": dict(kind="bgra", size=200, alpha="cv2"),
    "bgr_u16": dict(kind="bgr16", size=200),
    "bgr_u8_400_outscale3.5": dict(kind="bgr", size=400, outscale=3.5),
}


def _image(kind, n):
    import numpy as np
    from ffp_amd import synth
    im = synth.synthetic_frame(n, n, seed=1, n_blobs=6)[..., ::-1]
    yy, xx = np.mgrid[0:n, 0:n]
    alpha = np.clip(128 + 120 * np.sin(xx / 7.0) * np.cos(yy / 9.0), 0, 255).astype(np.uint8)
    if kind == "gray":
        return np.ascontiguousarray(im[..., 1])
    if kind == "bgra":
        return np.ascontiguousarray(np.dstack([im, alpha]))
    if kind == "bgr16":
        return im.astype(np.uint16) * 257
    return np.ascontiguousarray(im)


def run_calls(names, iters):
    """Make the calls; returns {case: [seconds per call]}."""
    from ffp_amd import synth
    from ffp_amd.compat.utils.enhancer import RealESRGANer, RRDBNet
    up = RealESRGANer(scale=4, model_path=synth.rrdbnet_weights(4, 23), model=RRDBNet(scale=4, num_block=23), tile=400, tile_pad=10,
                      half=True, gpu_id=0)
    res = {}
    for name in names:
        c = CASES[name]
        img = _image(c["kind"], c["size"])
        kw = dict(outscale=c.get("outscale"), alpha_upsampler=c.get("alpha", "realesrgan"))
        for _ in range(2):
            up.enhance(img, **kw)
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            out, _ = up.enhance(img, **kw)
            ts.append(time.perf_counter() - t0)
        res[name] = ts
        print(f"{name:26s} out {out.shape} {out.dtype}  median {statistics.median(ts) * 1e3:8.2f} ms", flush=True)
    return res


def _profiled(name, iters, timeout):
    """rocprofv3 --kernel-trace --stats over a child making 2 + iters calls of one case -> {kernel: total ns}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__),
               "--child", name, "--iters", str(iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under the rocprofv3 output: {os.listdir(d)}")
        out = {}
        for row in csv.DictReader(open(files[0])):
            n = row["Name"].replace("ffp::", "").replace("(anonymous namespace)::", "")
            n = n.split("(")[0] if not n.startswith("void ") else n[5:].split("(")[0]
            out[n] = out.get(n, 0.0) + float(row["TotalDurationNs"])
        return out


def kernel_stats(name, timeout, short=2, long=12):
    """Steady-state kernel ns per call: (run with `long` timed calls - run with `short`) / (long - short), so that the first
    call's plan set-up (allocation, tuning, graph capture) cancels out."""
    a, b = _profiled(name, short, timeout), _profiled(name, long, timeout)
    return {k: (b.get(k, 0.0) - a.get(k, 0.0)) / (long - short) for k in set(a) | set(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) make the calls of one case, for the profiler")
    ap.add_argument("--no-rocprof", action="store_true")
    a = ap.parse_args()
    if a.child:
        run_calls([a.child], a.iters)
        return
    res = {"cases": {}}
    times = run_calls(list(CASES), a.iters)
    for name, ts in times.items():
        res["cases"][name] = {"call_ms_median": statistics.median(ts) * 1e3, "call_ms_min": min(ts) * 1e3, "iters": len(ts)}
    if not a.no_rocprof:
        for name in CASES:
            ks = kernel_stats(name, 600)
            e = res["cases"][name]
            e["kernel_ms_per_call"] = sum(ks.values()) / 1e6
            e["kernels_ms_per_call"] = {k: v / 1e6 for k, v in sorted(ks.items(), key=lambda kv: -kv[1])[:12] if v > 0}
            for key, pat in (("resize_ms", "resize_lanczos4"), ("alpha_linear_ms", "alpha_linear"), ("pre_ms", "sr_pre"), ("post_ms", "sr_post")):
                e[key] = sum(v for k, v in ks.items() if pat in k) / 1e6
    c = res["cases"]
    res["summary"] = {
        "rgba_realesrgan_over_bgr_call": c["bgra_u8_realesrgan"]["call_ms_median"] / c["bgr_u8"]["call_ms_median"],
    }
    big = c["bgr_u8_400_outscale3.5"]
    if "resize_ms" in big:
        res["summary"]["resize_share_of_outscale_call"] = big["resize_ms"] / big["call_ms_median"]
        res["summary"]["rgba_realesrgan_over_bgr_kernels"] = c["bgra_u8_realesrgan"]["kernel_ms_per_call"] / c["bgr_u8"]["kernel_ms_per_call"]
    print(json.dumps(res["summary"], indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

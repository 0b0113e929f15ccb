"""A/B of the stem-fused first conv on one 4K frame's SAHI items (60 slices of 512 + the full frame, f32x3): model.0 computed inside
model.1's loader (the default where the plan offers it: n and s) against model.0 + model.1 as two kernels (FFP_NO_STEM_FUSE=1), each
setting in a fresh child process, both in the same call. Reports the detector's front stage (letterbox / stem launch) and network stage in ms (median of the timed
runs) and the profiled model.0 / model.1 launches.

    python tools/stem_ab.py [--arch m] [--imgsz 512,1024] [--runs 20]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(arch, imgsz, runs):
    import numpy as np
    sys.path.insert(0, ROOT)
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib, synth
    H, W = 2160, 3840
    frame = synth.synthetic_frame(H, W, seed=0)
    tiles = [tuple(t) for t in _lib.slice_bboxes(H, W, 512, 512, 0.2, 0.2)] + [(0, 0, W, H)]
    det = _lib.Detector(synth.yolo11_pose_weights(arch), arch=arch, precision=_lib.PREC_F32X3)
    for _ in range(5):
        det.infer_tiles(frame, tiles, imgsz, 0.25, 0.7, 300)
    ms = {"total": [], "preprocess": [], "network": []}
    for _ in range(runs):
        det.infer_tiles(frame, tiles, imgsz, 0.25, 0.7, 300)
        lm = det.last_ms()
        for k in ms:
            ms[k].append(lm[k])
    det.set_profile(True)
    det.infer_tiles(frame, tiles, imgsz, 0.25, 0.7, 300)
    prof = [e for e in det.profile_detail() if "model.0.conv" in e["name"] or e["name"].endswith(" model.1.conv")]
    det.set_profile(False)
    return {k: float(np.median(v)) for k, v in ms.items()} | {"launches": [(e["name"], round(e["ms"], 4)) for e in prof]}


def main():
    arch = sys.argv[sys.argv.index("--arch") + 1] if "--arch" in sys.argv else "m"
    sizes = [int(x) for x in (sys.argv[sys.argv.index("--imgsz") + 1] if "--imgsz" in sys.argv else "512,1024").split(",")]
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 20
    rows = []
    for imgsz in sizes:
        for fused in (True, False):
            env = dict(os.environ)
            env.pop("FFP_NO_STEM_FUSE", None)
            if not fused:
                env["FFP_NO_STEM_FUSE"] = "1"
            r = subprocess.run([sys.executable, __file__, "--child", arch, str(imgsz), str(runs)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                sys.exit(r.returncode)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            res.update({"arch": arch, "imgsz": imgsz, "stem": "fused into model.1" if fused else "model.0 + model.1 (FFP_NO_STEM_FUSE=1)"})
            rows.append(res)
            print(json.dumps(res), flush=True)
    for imgsz in sizes:
        f, u = [r for r in rows if r["imgsz"] == imgsz]
        print(f"YOLO11{arch} imgsz {imgsz}, 61 items: front+network {f['preprocess'] + f['network']:.3f} ms fused vs "
              f"{u['preprocess'] + u['network']:.3f} ms two kernels ({(u['preprocess'] + u['network']) / (f['preprocess'] + f['network']):.3f}x); "
              f"detector total {f['total']:.3f} vs {u['total']:.3f} ms")


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        print(json.dumps(child(sys.argv[i + 1], int(sys.argv[i + 2]), int(sys.argv[i + 3]))))
    else:
        main()

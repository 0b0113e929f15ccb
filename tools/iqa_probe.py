"""Times NIQE's feature call (ffp_iqa_niqe_features, upload and read-back included) on one 3840x2160 frame and on a ragged batch of 32
face-crop-sized images, and the host-side score. Prints milliseconds; no pass / fail.

    python tools/iqa_probe.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib, synth
    q = _lib.IQA(0)
    frame = np.ascontiguousarray(synth.synthetic_frame(2160, 3840, seed=1)[:, :, ::-1])
    rng = np.random.default_rng(0)
    crops = []
    for _ in range(32):
        h, w = int(rng.integers(192, 640)), int(rng.integers(192, 640))
        y, x = int(rng.integers(0, 2160 - h)), int(rng.integers(0, 3840 - w))
        crops.append(np.ascontiguousarray(frame[y:y + h, x:x + w]))
    out = {}
    for name, ims in (("frame_3840x2160_u8", [frame]), ("ragged_32_crops_u8", crops)):
        med, best = _median_ms(lambda: q.niqe_features(ims), a.reps)
        feat, _, off = q.niqe_features(ims)
        mu, cov = np.nanmean(feat, 0), np.cov(feat[~np.isnan(feat).any(1)], rowvar=False) + 1e-6 * np.eye(36)
        smed, _ = _median_ms(lambda: _lib.niqe_score(feat, off, mu, cov), a.reps)
        out[name] = {"blocks": int(off[-1]), "pixels": int(sum(i.shape[0] * i.shape[1] for i in ims)), "features_ms_median": med, "features_ms_min": best,
                     "score_host_ms_median": smed}
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(frame.astype(np.float32) / 255, 2, 0))).cuda()
    torch.cuda.synchronize()
    med, best = _median_ms(lambda: q.niqe_features_dev([t.data_ptr()], [tuple(t.shape)]), a.reps)
    out["frame_3840x2160_f32_resident"] = {"blocks": (2160 // 96) * (3840 // 96), "features_ms_median": med, "features_ms_min": best}
    for k, v in out.items():
        print(k, json.dumps(v))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    q.close()


if __name__ == "__main__":
    main()

"""Write tests/golden/rows16_pins.json: the sha256 of what conv_rows16_kernel (force_shape 9, fp16) stores for seeded inputs, one
record per case — the smallest shapes that reach each path of the kernel. A GPU test regenerates the inputs from the stored seeds
(case_inputs / case_sha256 below) and compares the hashes for equality: a refactor of the kernel (or of the parts it shares with
conv_rows16pc_kernel and conv_trunk_kernel, which other tests tie to force_shape 9 bit for bit) must not move a single bit. Needs
the GPU; run it on the tree whose results are to be pinned — for a refactor, the commit BEFORE it.

    python tests/golden/make_rows16_pins.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED0 = 20261017
CASES = [
    # (n, h, w, cin, cout, act, up, res)
    (1, 1, 1, 64, 32, 2, 0, False),         # one pixel, everything else padding
    (2, 17, 16, 64, 64, 2, 1, False),       # upsample, two channel blocks
    (1, 20, 20, 64, 128, 1, 0, False),      # SiLU, four channel blocks
    (2, 41, 42, 64, 32, 2, 0, False),       # ragged in both directions
    (1, 70, 33, 96, 32, 2, 0, True),        # residual, 3 chunks
    (2, 52, 33, 160, 32, 2, 0, True),       # 5 chunks
    (1, 33, 17, 192, 64, 0, 0, True),       # 6 chunks, no activation
    (40, 24, 24, 128, 32, 2, 0, False),     # several items per workgroup
]


def case_inputs(case, seed):
    """(x, weights, bias, residual or None) of a case: the draws, in this order, are part of the pin."""
    n, h, w, cin, cout, act, up, has_res = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, cin), dtype=np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3), dtype=np.float32) / np.sqrt(cin * 9)).astype(np.float32)
    b = rng.standard_normal(cout, dtype=np.float32) * 0.1
    ho, wo = (h * 2, w * 2) if up else (h, w)
    res = rng.standard_normal((n, ho, wo, cout), dtype=np.float32) if has_res else None
    return x, wt, b, res


def case_sha256(lib, case, seed):
    """sha256 of the fp16 output of the case at force_shape 9 (the kernel stores fp16: the cast back is lossless)."""
    x, wt, b, res = case_inputs(case, seed)
    lib.op_conv2d_shape(9)
    try:
        y = lib.op_conv2d(x, wt, b, stride=1, act=case[5], up=bool(case[6]), res=res, res_scale=0.2 if res is not None else 1.0,
                          precision=lib.PREC_F16)
    finally:
        lib.op_conv2d_shape(-1)
    return hashlib.sha256(np.ascontiguousarray(y.astype(np.float16)).tobytes()).hexdigest()


def main():
    import torch  # noqa: F401  (one HIP runtime per process: see ffp_amd._lib.lib)
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib
    assert _lib.device_count() > 0, "the pins are computed on the GPU"
    out = [{"case": list(c), "seed": SEED0 + i, "sha256": case_sha256(_lib, c, SEED0 + i)} for i, c in enumerate(CASES)]
    path = os.path.join(HERE, "rows16_pins.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, len(out), "records")


if __name__ == "__main__":
    main()

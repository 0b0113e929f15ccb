"""Record the fused class tower's output bits (tests/golden/cls_tower_parent_bits.npz) for tests/test_gpu_cls_tower_bits.py.

Run it on a GPU with the build whose bits are to be the yardstick, i.e. BEFORE a change to csrc/conv_dwpw.hip that has to keep every bit:

    python tests/golden/make_cls_tower_bits.py

It needs only op_cls_tower. Inputs and weights are seeded the way tests/test_gpu_cls_tower_op.py seeds them (default_rng(1000 * cin + nc), N(0, 1)
images, depthwise weights N(0, 1) * 2, its "zero" / "small" / "large" / "outlier" value classes), on image sizes that hold every case of a 16-row
and of an 8-row tile: a single row, one row short of a half tile, an exact half tile and full tile, one row past each, right edges of 1 and 17
columns, images of 1, 2 and 6 tiles.

Stored per configuration cin -> 128 -> nc: every logit; e1 in full for the images (1, 5) and (9, 33); a SHA-256 of e1's bytes for the others."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cls_tower_parent_bits.npz")

C3 = 128
SIZES = [(1, 5), (7, 16), (8, 17), (9, 33), (16, 16), (17, 33), (24, 20)]
KINDS = ["plain", "small", "plain", "outlier", "zero", "plain", "large"]
CONFIGS = [(128, 1), (256, 3), (512, 1)]
E1_FULL = (0, 3)           # images whose e1 is stored in full


def batch(rng, cin):
    xs = []
    for (h, w), kind in zip(SIZES, KINDS):
        if kind == "zero":
            x = np.zeros((h, w, cin), np.float32)
        elif kind == "outlier":
            x = (rng.standard_normal((h, w, cin)) * 2.0 ** -16).astype(np.float32)
            idx = rng.integers(0, x.size, 6)
            x.reshape(-1)[idx] = np.float32(16.0) * rng.choice([-1.0, 1.0], 6).astype(np.float32)
        else:
            x = rng.standard_normal((h, w, cin)).astype(np.float32)
            if kind == "small":
                x = x * np.float32(2.0 ** -20)
        xs.append(x)
    return xs


def weights(rng, cin, nc):
    dw = lambda c: ((rng.standard_normal((c, 3, 3)) * 2.0).astype(np.float32), (rng.standard_normal(c) * 0.1).astype(np.float32))
    pw = lambda co, ci: ((rng.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32), (rng.standard_normal(co) * 0.1).astype(np.float32))
    return {"dw0": dw(cin), "pw0": pw(C3, cin), "dw1": dw(C3), "pw1": pw(C3, C3), "fin": pw(nc, C3)}


def case(cin, nc):
    """-> (images, weights, head records going in) of one configuration."""
    rng = np.random.default_rng(1000 * cin + nc)
    xs = batch(rng, cin)
    W = weights(rng, cin, nc)
    heads = [rng.integers(-1000, 1000, (x.shape[0], x.shape[1], 64 + nc + 3)).astype(np.float32) for x in xs]
    return xs, W, heads


def run(lib, cin, nc):
    """-> (e1 per image, logits per image) of the loaded build."""
    xs, W, heads = case(cin, nc)
    e1, out, stray = lib.op_cls_tower(xs, W["dw0"], W["pw0"], W["dw1"], W["pw1"], W["fin"], heads, 64, px_align=32)
    assert stray == 0, stray
    return e1, [np.ascontiguousarray(h[..., 64:64 + nc]) for h in out]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def main():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib
    rec = {}
    for cin, nc in CONFIGS:
        e1, lg = run(_lib, cin, nc)
        for i in range(len(SIZES)):
            rec[f"c{cin}_n{nc}_logits_{i}"] = lg[i]
            if i in E1_FULL:
                rec[f"c{cin}_n{nc}_e1_{i}"] = e1[i]
            else:
                rec[f"c{cin}_n{nc}_e1sha_{i}"] = np.asarray(digest(e1[i]))
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()

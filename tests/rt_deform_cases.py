"""The designed inputs of the rt_deform tests, shared by the GPU comparison (test_gpu_rtdetr_ops.py) and the CPU check that they
cover every kind of sample point (test_ops_ref.py)."""
import numpy as np

import ops_ref

NQ = 300
DEFORM_SHAPES = [(5, 7), (3, 4), (2, 2)]
DEFORM_SHAPES_T = [(7, 5), (4, 3), (2, 2)]


def deform_inputs(seed, weights):
    """n = 2 images of 300 queries; sample point (q, head, level, point) is of kind (q + head + 5 * level + point) % 10, so every head
    meets every kind at every level; queries with q % 25 == 7 / 8 have a box of width / height 0."""
    rng = np.random.default_rng(seed)
    n, shapes = 2, DEFORM_SHAPES
    nt = sum(h * w for h, w in shapes)
    val = rng.standard_normal((n, nt, 256)).astype(np.float32)
    ref = np.concatenate([0.2 + 0.6 * rng.random((n, NQ, 2)), 0.2 + 0.4 * rng.random((n, NQ, 2))], -1).astype(np.float32)
    qn = np.arange(NQ)
    ref[:, qn % 25 == 7, 2] = 0
    ref[:, qn % 25 == 8, 3] = 0
    q, hd, lv, pt = np.meshgrid(qn, np.arange(8), np.arange(3), np.arange(4), indexing="ij")
    kind = (q + hd + 5 * lv + pt) % 10
    W = np.asarray([s[1] for s in shapes], np.float64)[lv]
    H = np.asarray([s[0] for s in shapes], np.float64)[lv]
    off = np.empty((n, NQ, 8, 3, 4, 2), np.float32)
    for i in range(n):
        u = rng.random((4,) + kind.shape)
        xt, yt = u[0] * (W - 1), u[1] * (H - 1)
        xt = np.where(kind == 0, np.floor(u[0] * W), xt); yt = np.where(kind == 0, np.floor(u[1] * H), yt)
        xt = np.where(kind == 1, -1 + 0.999 * u[2], xt); yt = np.where(kind == 2, -1 + 0.999 * u[2], yt)
        xt = np.where(kind == 3, W - 1 + 0.999 * u[2], xt); yt = np.where(kind == 4, H - 1 + 0.999 * u[2], yt)
        xt = np.where(kind == 5, -1.0, xt); xt = np.where(kind == 6, W, xt)
        r = ref[i].astype(np.float64)[:, None, None, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            ox = ((xt + 0.5) / W - r[..., 0]) * 8 / r[..., 2]
            oy = ((yt + 0.5) / H - r[..., 1]) * 8 / r[..., 3]
        ox = np.where(np.isfinite(ox), ox, u[3] * 4 - 2); oy = np.where(np.isfinite(oy), oy, u[3] * 4 - 2)
        ox = np.where(kind == 7, 1e6, ox); oy = np.where(kind == 7, 1e6, oy)
        ox = np.where(kind == 8, -1e6, ox); oy = np.where(kind == 8, -1e6, oy)
        off[i, ..., 0], off[i, ..., 1] = ox, oy
    if weights == "unit":
        lg = rng.standard_normal((n, NQ, 8, 12))
    else:                                                # +-80 with one dominant point per (query, head)
        lg = rng.uniform(-80, 40, (n, NQ, 8, 12))
        np.put_along_axis(lg, ((qn[:, None] + np.arange(8)[None]) % 12)[None, :, :, None].repeat(n, 0), 80.0, 3)
    oa = np.concatenate([off.reshape(n, NQ, 192), lg.reshape(n, NQ, 96).astype(np.float32)], -1)
    # kinds "exactly -1" and "exactly W": walk the offset by single ulps until the float32 evaluation of the location formula hits the value
    target = np.where(kind == 5, -1.0, W).astype(np.float32)
    exact = (kind == 5) | (kind == 6)
    for i in range(n):
        offs = oa[i, :, :192].reshape(kind.shape + (2,)).copy()
        first = offs[..., 0].copy()
        done = np.zeros(kind.shape, bool)
        for step in range(33):
            for sgn in (1, -1):
                cand = first.copy()
                for _ in range(step):
                    cand = np.nextafter(cand, np.float32(sgn * np.inf), dtype=np.float32)
                trial = offs.copy()
                trial[..., 0] = cand
                X, _ = ops_ref.rt_deform_locations(np.concatenate([trial.reshape(NQ, 192), oa[i, :, 192:]], 1), ref[i], shapes, dtype=np.float32)
                hit = exact & ~done & (X == target)
                offs[..., 0] = np.where(hit, cand, offs[..., 0])
                done |= hit
        oa[i, :, :192] = offs.reshape(NQ, 192)
    return val, oa, ref, kind

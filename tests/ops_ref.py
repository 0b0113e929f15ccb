"""Plain float64 references of the detector's non-convolution operators, written from the definition of each operation
(not from the kernels): what tests/test_gpu_ops.py compares the HIP kernels with. tests/test_ops_ref.py checks these
against independent implementations (torch.nn.functional, oracle/ultra_post.py, torch.topk) on the CPU.

Images are (h, w, c) arrays, channels last, like the library's NHWC buffers."""
import numpy as np

MAX_WH = 7680.0          # ultralytics non_max_suppression: per-class box offset
RT_NQ = 300              # RT-DETR queries


def max_pool5(x):
    """MaxPool2d(kernel 5, stride 1, padding 2) of an (h, w, c) array; padding is -inf."""
    h, w, c = x.shape
    p = np.full((h + 4, w + 4, c), -np.inf, np.float64)
    p[2:2 + h, 2:2 + w] = x
    out = np.full((h, w, c), -np.inf, np.float64)
    for dy in range(5):
        for dx in range(5):
            out = np.maximum(out, p[dy:dy + h, dx:dx + w])
    return out


def sppf_pool(x):
    """SPPF: y1 = pool(x), y2 = pool(y1), y3 = pool(y2)."""
    y1 = max_pool5(np.asarray(x, np.float64))
    y2 = max_pool5(y1)
    return y1, y2, max_pool5(y2)


def upsample2x(x):
    """nn.Upsample(scale_factor=2, mode='nearest') of an (h, w, c) array."""
    return np.repeat(np.repeat(np.asarray(x), 2, axis=0), 2, axis=1)


def psa_attention(qkv, nh, kd=32, hd=64, dtype=np.float64):
    """C2PSA attention of an (h, w, nh*(2kd+hd)) array with per-head records [q(kd) | k(kd) | v(hd)]:
    out[i] = sum_j softmax_j(q_i . k_j * kd^-0.5) v_j over the N = h*w pixels -> (h, w, nh*hd).
    `dtype` float32 gives the plain single-precision evaluation of the same formula (the error yardstick of the tests)."""
    h, w, c = qkv.shape
    rec = 2 * kd + hd
    assert c == nh * rec
    t = np.asarray(qkv, dtype).reshape(h * w, nh, rec)
    out = np.empty((h * w, nh, hd), dtype)
    scale = dtype(kd) ** dtype(-0.5)
    for a in range(nh):
        q, k, v = t[:, a, :kd], t[:, a, kd:2 * kd], t[:, a, 2 * kd:]
        s = (q @ k.T) * scale
        s = s - s.max(axis=1, keepdims=True)
        e = np.exp(s)
        out[:, a] = (e / e.sum(axis=1, keepdims=True)) @ v
    return out.reshape(h, w, nh * hd)


def act_fn(v, act):
    """0 none, 1 SiLU, 2 LeakyReLU(0.2), 3 ReLU."""
    if act == 1:
        return v / (1.0 + np.exp(-v))
    if act == 2:
        return np.where(v >= 0, v, v * 0.2)
    if act == 3:
        return np.maximum(v, 0.0)
    return v


def grouped_gather(x, c, coff=0, grp=0, grp_stride=0, grp_off=0):
    """The c input channels of a depthwise conv reading grouped records: channel ch sits at
    coff + (ch // grp) * grp_stride + grp_off + ch % grp (grp = 0: at coff + ch)."""
    ch = np.arange(c)
    idx = coff + ch if grp <= 0 else coff + (ch // grp) * grp_stride + grp_off + ch % grp
    return np.asarray(x)[..., idx]


def dwconv3x3(x, w, b=None, act=0, res=None):
    """Depthwise 3x3 cross-correlation, stride 1, zero padding 1, of an (h, w, c) array; w (c, 3, 3); then bias,
    activation, and the residual added after the activation."""
    x = np.asarray(x, np.float64)
    h, wd, c = x.shape
    p = np.zeros((h + 2, wd + 2, c), np.float64)
    p[1:1 + h, 1:1 + wd] = x
    w = np.asarray(w, np.float64)
    out = np.zeros((h, wd, c), np.float64)
    for ky in range(3):
        for kx in range(3):
            out += p[ky:ky + h, kx:kx + wd] * w[:, ky, kx]
    if b is not None:
        out = out + np.asarray(b, np.float64)
    out = act_fn(out, act)
    if res is not None:
        out = out + np.asarray(res, np.float64)
    return out


# ---- Pose head ------------------------------------------------------------------------------------------------------------

def head_decode(levels, nc, nkpt, dtype=np.float64):
    """Ultralytics Detect._inference + Pose.kpts_decode on three (H/s, W/s, 64 + nc + 3*nkpt) head tensors, s = 8, 16, 32:
    DFL (softmax expectation over 16 bins per side), dist2bbox(xywh) on anchor centres x + 0.5, times the stride; class
    sigmoid; keypoints (raw * 2 + anchor - 0.5) * stride, visibility sigmoid. Returns (4 + nc + 3*nkpt, anchors), anchors
    level by level in row-major order."""
    cols = []
    bins = np.arange(16, dtype=dtype)
    for l, t in enumerate(levels):
        t = np.asarray(t, dtype)
        h, w, _ = t.shape
        stride = dtype(8 << l)
        r = t.reshape(h * w, -1)
        d = r[:, :64].reshape(-1, 4, 16)
        d = d - d.max(axis=2, keepdims=True)
        e = np.exp(d)
        dist = ((e / e.sum(axis=2, keepdims=True)) * bins).sum(axis=2)          # left, top, right, bottom
        ay, ax = np.divmod(np.arange(h * w), w)
        ax = ax.astype(dtype) + dtype(0.5)
        ay = ay.astype(dtype) + dtype(0.5)
        x1, y1, x2, y2 = ax - dist[:, 0], ay - dist[:, 1], ax + dist[:, 2], ay + dist[:, 3]
        rows = [(x1 + x2) / 2 * stride, (y1 + y2) / 2 * stride, (x2 - x1) * stride, (y2 - y1) * stride]
        for c in range(nc):
            rows.append(1 / (1 + np.exp(-r[:, 64 + c])))
        kp = r[:, 64 + nc:]
        for k in range(nkpt):
            rows.append((kp[:, 3 * k] * 2 + (ax - dtype(0.5))) * stride)
            rows.append((kp[:, 3 * k + 1] * 2 + (ay - dtype(0.5))) * stride)
            rows.append(1 / (1 + np.exp(-kp[:, 3 * k + 2])))
        cols.append(np.stack(rows, 0))
    return np.concatenate(cols, 1).astype(dtype)


def box_iou(a, b):
    """IoU of box a (4,) with boxes b (n, 4), xyxy."""
    iw = np.clip(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), 0, None)
    ih = np.clip(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), 0, None)
    inter = iw * ih
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union > 0, inter / union, 0.0)


def nms(raw, nc, conf, iou_thr, max_det):
    """ultralytics non_max_suppression on one image's (4 + nc + extra, A) decode: candidates = anchors whose best class
    score > conf; boxes xywh -> xyxy, offset by class * 7680; visited in (score descending, anchor ascending) order, a
    candidate is kept unless a kept one overlaps it with IoU > iou_thr; at most max_det.
    Returns (keep: anchor indices in kept order, cls: best class of every anchor, margins: {"iou": min |IoU - thr| over every
    pair the decision looked at, "conf": min |score - conf|}) — the tests require the margins to be wide before they demand
    exact agreement."""
    raw = np.asarray(raw, np.float64)
    sc_all = raw[4:4 + nc]
    cls = sc_all.argmax(0)                                   # first maximum: the lowest class index on ties
    score = sc_all.max(0)
    margins = {"iou": np.inf, "conf": float(np.abs(score - conf).min()) if score.size else np.inf}
    cand = np.flatnonzero(score > conf)
    cx, cy, w, h = raw[0], raw[1], raw[2], raw[3]
    xyxy = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    off = xyxy + (cls * MAX_WH)[:, None]
    order = cand[np.argsort(-score[cand], kind="stable")]    # stable: equal scores stay in anchor order
    alive = np.ones(order.size, bool)
    keep = []
    for i in range(order.size):
        if not alive[i]:
            continue
        if len(keep) == max_det:
            break
        keep.append(order[i])
        rest = np.flatnonzero(alive[i + 1:]) + i + 1
        if rest.size:
            ov = box_iou(off[order[i]], off[order[rest]])
            margins["iou"] = min(margins["iou"], float(np.abs(ov - iou_thr).min()))
            alive[rest[ov > iou_thr]] = False
    return np.asarray(keep, np.int64), cls, margins


def scale_boxes(xyxy, gain, pad_x, pad_y, sw, sh):
    """ultralytics scale_boxes: subtract the padding, divide by the gain, clip to the (sw x sh) source image."""
    b = np.array(xyxy, np.float64).reshape(-1, 4)
    b[:, [0, 2]] = np.clip((b[:, [0, 2]] - pad_x) / gain, 0, sw)
    b[:, [1, 3]] = np.clip((b[:, [1, 3]] - pad_y) / gain, 0, sh)
    return b


def scale_coords(kpts, gain, pad_x, pad_y, sw, sh):
    """ultralytics scale_coords on (n, K, 3) keypoints (x, y, visibility)."""
    k = np.array(kpts, np.float64)
    k[..., 0] = np.clip((k[..., 0] - pad_x) / gain, 0, sw)
    k[..., 1] = np.clip((k[..., 1] - pad_y) / gain, 0, sh)
    return k


def det_rows(raw, keep, cls, nc, nkpt, geom, round_boxes=False):
    """Rows [x1, y1, x2, y2, score, class, keypoints...] of the kept anchors in source-image pixels.
    geom = (gain, pad_x, pad_y, sw, sh, x0, y0)."""
    raw = np.asarray(raw, np.float64)
    gain, px, py, sw, sh = geom[:5]
    cx, cy, w, h = (raw[i][keep] for i in range(4))
    b = scale_boxes(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1), gain, px, py, sw, sh)
    if round_boxes:
        b = np.rint(b)
    k = scale_coords(raw[4 + nc:, keep].T.reshape(len(keep), nkpt, 3), gain, px, py, sw, sh)
    return np.concatenate([b, raw[4:4 + nc].max(0)[keep, None], cls[keep, None].astype(np.float64), k.reshape(len(keep), 3 * nkpt)], 1)


def truncate_shift(rows, nkpt, geom, full_h, full_w):
    """The wrapper's int() truncation of the box, the ObjectAnnotation clip (x2 <= full_w, y2 <= full_h on crop-local
    coordinates) and the shift of box and keypoints by the crop origin."""
    r = np.array(rows, np.float64)
    x0, y0 = geom[5], geom[6]
    b = np.trunc(r[:, :4])
    b[:, 0] = np.maximum(b[:, 0], 0); b[:, 1] = np.maximum(b[:, 1], 0)
    b[:, 2] = np.minimum(b[:, 2], full_w); b[:, 3] = np.minimum(b[:, 3], full_h)
    r[:, :4] = b + np.array([x0, y0, x0, y0])
    for q in range(nkpt):
        r[:, 6 + 3 * q] += x0
        r[:, 6 + 3 * q + 1] += y0
    return r


# ---- RT-DETR query selection --------------------------------------------------------------------------------------------

def total_order_key(v):
    """An integer key ordering float32 values as the IEEE total order does: -inf < ... < -0.0 < +0.0 < ... < +inf."""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)


def stable_topk(scores, k=RT_NQ, signed_zero=True):
    """Indices of the k largest entries of `scores` (NT,) ordered by (value descending, index ascending).
    signed_zero: order -0.0 below +0.0 (the bit-pattern order); False: plain float comparison."""
    key = total_order_key(scores) if signed_zero else np.asarray(scores, np.float64)
    return np.argsort(-key, kind="stable")[:k]

"""Plain float64 references of the detectors' non-convolution operators, written from the definition of each operation
(not from the kernels): what tests/test_gpu_ops.py, tests/test_gpu_rtdetr_ops.py and tests/test_gpu_scrfd_ops.py compare the HIP kernels with. tests/test_ops_ref.py checks these
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


# ---- RT-DETR operators (csrc/rtdetr_ops.hip) ------------------------------------------------------------------------------------
# `dtype=np.float32` evaluates the same formula in single precision: the error yardstick of tests/test_gpu_rtdetr_ops.py.

def _erf(x):
    import math
    return np.vectorize(math.erf, otypes=[np.float64])(np.asarray(x, np.float64))


def sigmoid(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    with np.errstate(over="ignore"):
        return dtype(1) / (dtype(1) + np.exp(-x))


def rt_dwconv(x, w, b, k, s, act=0, dtype=np.float64):
    """Depthwise k x k cross-correlation, stride s, zero padding k // 2, of an (h, w, c) array; w (c, k, k); bias, then act_fn."""
    x = np.asarray(x, dtype)
    h, wd, c = x.shape
    p = k // 2
    ho, wo = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
    xp = np.zeros((h + 2 * p, wd + 2 * p, c), dtype)
    xp[p:p + h, p:p + wd] = x
    w = np.asarray(w, dtype)
    out = np.zeros((ho, wo, c), dtype)
    for ky in range(k):
        for kx in range(k):
            out += xp[ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s] * w[:, ky, kx]
    return act_fn(out + np.asarray(b, dtype), act).astype(dtype)


def rt_maxpool2(x):
    """HGStem's pool: F.pad(x, [0, 1, 0, 1]) (zeros right and below) then MaxPool2d(2, 1): (h, w, c) -> (h, w, c)."""
    x = np.asarray(x)
    h, w, c = x.shape
    p = np.zeros((h + 1, w + 1, c), x.dtype)
    p[:h, :w] = x
    return np.maximum(np.maximum(p[:h, :w], p[:h, 1:]), np.maximum(p[1:, :w], p[1:, 1:]))


def layer_norm(x, gamma, beta, eps=1e-5, dtype=np.float64):
    """LayerNorm over the last axis: (x - mean) / sqrt(var + eps) * gamma + beta with the biased variance about the mean."""
    x = np.asarray(x, dtype)
    mean = x.mean(-1, keepdims=True, dtype=dtype)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True, dtype=dtype)
    return (d / np.sqrt(var + dtype(eps)) * np.asarray(gamma, dtype) + np.asarray(beta, dtype)).astype(dtype)


def gelu(x, dtype=np.float64):
    """Exact GELU 0.5 x (1 + erf(x / sqrt 2)). float32: the argument, a correctly rounded erf and the products in single precision."""
    x = np.asarray(x, dtype)
    e = _erf(x * dtype(0.7071067811865476)).astype(dtype)
    return (dtype(0.5) * x * (dtype(1) + e)).astype(dtype)


def rt_attention(qk, v, nh=8, dtype=np.float64):
    """Multi-head attention over L tokens: qk (L, 2 * nh * 32) = [q | k], v (L, nh * 32) -> (L, nh * 32);
    out_i = sum_j softmax_j(q_i . k_j / sqrt(32)) v_j per head."""
    qk, v = np.asarray(qk, dtype), np.asarray(v, dtype)
    L, hd = qk.shape[0], 32
    q, k = qk[:, :nh * hd].reshape(L, nh, hd), qk[:, nh * hd:].reshape(L, nh, hd)
    vv = v.reshape(L, nh, hd)
    out = np.empty((L, nh, hd), dtype)
    scale = dtype(hd) ** dtype(-0.5)
    for a in range(nh):
        s = (q[:, a] @ k[:, a].T) * scale
        s = s - s.max(axis=1, keepdims=True)
        e = np.exp(s)
        out[:, a] = (e / e.sum(axis=1, keepdims=True)) @ vv[:, a]
    return out.reshape(L, nh * hd)


def rt_enc_prep(levels, valid):
    """RTDETRDecoder._get_encoder_input + the valid mask: levels of (h, w, 256) -> (tokens, 256) t, and tm = t where valid else 0."""
    t = np.concatenate([np.asarray(a).reshape(-1, a.shape[-1]) for a in levels], 0)
    return t, np.where(np.asarray(valid).reshape(-1, 1) != 0, t, 0).astype(t.dtype)


def rt_gather(e, idx, anchors):
    """Rows of e (NT, c) and anchors (NT, 4) at idx clamped to [0, NT - 1]."""
    i = np.clip(np.asarray(idx, np.int64), 0, e.shape[0] - 1)
    return np.asarray(e)[i], np.asarray(anchors)[i]


def inverse_sigmoid(x, eps=1e-5, dtype=np.float64):
    """ultralytics inverse_sigmoid: log(max(x, eps) / max(1 - x, eps)) of x clamped to [0, 1]."""
    x = np.clip(np.asarray(x, dtype), dtype(0), dtype(1))
    return np.log(np.maximum(x, dtype(eps)) / np.maximum(dtype(1) - x, dtype(eps)))


def rt_ref(delta, ref=None, anc=None, dtype=np.float64):
    """Reference boxes: sigmoid(delta + anc) (query selection; an infinite anchor gives 1) or sigmoid(delta + inverse_sigmoid(ref))."""
    base = np.asarray(anc, dtype) if anc is not None else inverse_sigmoid(ref, dtype=dtype)
    return sigmoid(np.asarray(delta, dtype) + base, dtype)


def rt_deform_locations(oa, ref, shapes, dtype=np.float64):
    """MSDeformAttn sampling positions in pixels: loc = ref_xy + offset / 4 * ref_wh * 0.5, x = loc_x * W - 0.5 (align_corners=False).
    oa (Q, 288), ref (Q, 4) -> x, y of shape (Q, 8, 3, 4)."""
    oa, ref = np.asarray(oa, dtype), np.asarray(ref, dtype)
    off = oa[:, :192].reshape(-1, 8, 3, 4, 2)
    r = ref[:, None, None, None, :]
    lx = r[..., 0] + off[..., 0] / dtype(4) * r[..., 2] * dtype(0.5)
    ly = r[..., 1] + off[..., 1] / dtype(4) * r[..., 3] * dtype(0.5)
    W = np.asarray([s[1] for s in shapes], dtype)[None, None, :, None]
    H = np.asarray([s[0] for s in shapes], dtype)[None, None, :, None]
    return lx * W - dtype(0.5), ly * H - dtype(0.5)


def rt_deform(val, shapes, oa, ref, dtype=np.float64):
    """multi_scale_deformable_attn for one image: val (tokens, 256) = levels of (h, w) row-major, 8 heads of 32 channels; oa (Q, 288) =
    [offsets (head, level, point, xy) 192 | weight logits (head, level * point) 96]; ref (Q, 4) cxcywh -> (Q, 256). Bilinear sampling
    with zeros outside the map, softmax over the 12 weights of a head."""
    val, oa = np.asarray(val, dtype), np.asarray(oa, dtype)
    Q = oa.shape[0]
    lg = oa[:, 192:288].reshape(Q, 8, 12)
    lg = lg - lg.max(-1, keepdims=True)
    e = np.exp(lg)
    aw = (e / e.sum(-1, keepdims=True)).reshape(Q, 8, 3, 4)
    X, Y = rt_deform_locations(oa, ref, shapes, dtype)
    out = np.zeros((Q, 8, 32), dtype)
    start = 0
    heads = np.arange(8)[None, :, None]
    for l, (h, w) in enumerate(shapes):
        v = val[start:start + h * w].reshape(h, w, 8, 32)
        start += h * w
        x, y = X[:, :, l], Y[:, :, l]                        # (Q, 8, 4)
        x0, y0 = np.floor(x), np.floor(y)
        ax, ay = x - x0, y - y0
        s = np.zeros((Q, 8, 4, 32), dtype)
        for dy, wy in ((0, dtype(1) - ay), (1, ay)):
            for dx, wx in ((0, dtype(1) - ax), (1, ax)):
                xi, yi = x0 + dx, y0 + dy
                ok = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
                xc = np.where(ok, xi, 0).astype(np.int64)
                yc = np.where(ok, yi, 0).astype(np.int64)
                g = v[yc, xc, heads]                          # (Q, 8, 4, 32)
                s += np.where(ok, wx * wy, dtype(0))[..., None] * g
        out += (aw[:, :, l][..., None] * s).sum(2)
    return out.reshape(Q, 256).astype(dtype)


def rt_raw(ref, logits, dtype=np.float64):
    """[boxes cxcywh | sigmoid scores] per query."""
    return np.concatenate([np.asarray(ref, dtype), sigmoid(logits, dtype)], -1)


def rt_post(ref, logits, conf, orig_wh):
    """RTDETRPredictor.postprocess for one image: rows (x1, y1, x2, y2, score, class) of the queries whose best score > conf, in query
    order, boxes scaled by (width, height). Returns (rows, margin = min |best score - conf| over the scores that are not conf itself)."""
    ref = np.asarray(ref, np.float64)
    sc = sigmoid(logits)
    cls = sc.argmax(-1)                                      # the first maximum
    best = sc.max(-1)
    keep = best > conf
    ow, oh = orig_wh
    dw, dh = ref[:, 2] / 2, ref[:, 3] / 2
    rows = np.stack([(ref[:, 0] - dw) * ow, (ref[:, 1] - dh) * oh, (ref[:, 0] + dw) * ow, (ref[:, 1] + dh) * oh, best, cls.astype(np.float64)], 1)
    d = np.abs(best - conf)
    return rows[keep], float(d[d > 0].min()) if (d > 0).any() else np.inf


# ---- SCRFD operators (csrc/scrfd_ops.hip) -----------------------------------------------------------------------------------------

def scrfd_maxpool(x):
    """MaxPool 3x3 / stride 2 / pad 1 of an (h, w, c) array; the padding is -inf."""
    x = np.asarray(x)
    h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    p = np.full((2 * ho + 1, 2 * wo + 1, c), -np.inf, x.dtype)
    p[1:1 + h, 1:1 + w] = x
    out = np.full((ho, wo, c), -np.inf, x.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, p[dy:dy + 2 * ho:2, dx:dx + 2 * wo:2])
    return out


def scrfd_avgpool(x, k, dtype=np.float64):
    """AveragePool k x k / stride k, ceil_mode, count_include_pad = 0: windows are clipped to the map and divide by what is left."""
    x = np.asarray(x, dtype)
    h, w, c = x.shape
    ho, wo = -(-h // k), -(-w // k)
    out = np.empty((ho, wo, c), dtype)
    for oy in range(ho):
        for ox in range(wo):
            win = x[oy * k:min(oy * k + k, h), ox * k:min(ox * k + k, w)].reshape(-1, c)
            out[oy, ox] = win.sum(0, dtype=dtype) / dtype(win.shape[0])
    return out


def scrfd_post(score, bbox, kps, net_hw, det_scale, thresh, nms_thresh, A=2, strides=(8, 16, 32)):
    """RetinaFace.detect's decode + NMS in float64 from the definition. score / bbox / kps: per level (h, w, A) sigmoid scores,
    (h, w, 4A) distances, (h, w, 10A) keypoint offsets or None. Anchors are numbered level by level, pixel by pixel, anchor by anchor.
    Candidates score >= thresh, visited by (score descending, anchor ascending); a candidate is kept when its overlap (areas and
    intersections with the "+1" pixel convention) with every kept one is <= nms_thresh.
    Returns (kept anchor numbers, boxes (k, 4), keypoints (k, 5, 2), margins {"score", "ovr"})."""
    boxes, kpts, scs = [], [], []
    for l, s in enumerate(strides):
        h, w = net_hw[0] // s, net_hw[1] // s
        yy, xx = np.divmod(np.repeat(np.arange(h * w), A), w)
        cx, cy = xx * float(s), yy * float(s)
        d = np.asarray(bbox[l], np.float64).reshape(-1, 4) * s
        boxes.append(np.stack([cx - d[:, 0], cy - d[:, 1], cx + d[:, 2], cy + d[:, 3]], 1) / det_scale)
        scs.append(np.asarray(score[l], np.float64).reshape(-1))
        if kps is not None:
            kk = np.asarray(kps[l], np.float64).reshape(-1, 5, 2) * s
            kpts.append((np.stack([cx, cy], 1)[:, None, :] + kk) / det_scale)
    boxes, scs = np.concatenate(boxes), np.concatenate(scs)
    kpts = np.concatenate(kpts) if kps is not None else np.zeros((len(scs), 5, 2))
    margins = {"score": float(np.abs(scs - thresh)[scs != thresh].min()), "ovr": np.inf}
    cand = np.flatnonzero(scs >= thresh)
    order = cand[np.lexsort((cand, -scs[cand]))]
    area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    keep, alive = [], np.ones(order.size, bool)
    for i in range(order.size):
        if not alive[i]:
            continue
        a = order[i]
        keep.append(a)
        rest = np.flatnonzero(alive[i + 1:]) + i + 1
        if rest.size:
            b = order[rest]
            iw = np.maximum(0.0, np.minimum(boxes[a, 2], boxes[b, 2]) - np.maximum(boxes[a, 0], boxes[b, 0]) + 1)
            ih = np.maximum(0.0, np.minimum(boxes[a, 3], boxes[b, 3]) - np.maximum(boxes[a, 1], boxes[b, 1]) + 1)
            inter = iw * ih
            ovr = inter / (area[a] + area[b] - inter)
            margins["ovr"] = min(margins["ovr"], float(np.abs(ovr - nms_thresh).min()))
            alive[rest[~(ovr <= nms_thresh)]] = False
    keep = np.asarray(keep, np.int64)
    return keep, boxes[keep], kpts[keep], margins

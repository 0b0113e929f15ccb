"""Seeded random-init weights and synthetic frames.

No checkpoint of the reference exists offline (its `models/` is git-ignored: /root/reference/.gitignore:7-8),
so benchmarks and parity tests run the real architectures with deterministic random weights, as
BASELINE.md §3 / SURVEY.md §8(d) prescribe: variance-preserving conv init with BatchNorm folded, a classifier
prior so that ~1 % of anchors clear conf=0.5, and residual-scaled ESRGAN weights whose output stays inside [0,1].
"""
from __future__ import annotations

import json
import os
from typing import Dict

import numpy as np

from . import arch


_CALIB = None


def _calib(key: str) -> Dict[str, float]:
    """Per-conv scalar multipliers (tests/golden/make_synth_calibration.py) standing in for trained BatchNorm statistics."""
    global _CALIB
    if _CALIB is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "synth_calib.json")
        with open(path) as f:
            _CALIB = json.load(f)
    return _CALIB[key]


def yolo11_pose_weights(scale: str = "s", nc: int = 1, kpt_shape=(5, 3), seed: int = 0,
                        calibrated: bool = True) -> Dict[str, np.ndarray]:
    """Fused (conv.weight, conv.bias) tensors for every conv of YOLO11{n,s}-pose, He-style init, then (calibrated)
    each conv rescaled so its pre-activation output has unit std on a synthetic frame; class-logit bias -4.6
    (~1 % of anchors clear conf=0.5)."""
    rng = np.random.default_rng(seed)
    cal = _calib(f"yolo11{scale}-pose") if calibrated else None
    out: Dict[str, np.ndarray] = {}
    for s in arch.yolo11_pose_convs(scale, nc, kpt_shape):
        fan_in = (s.c1 // s.g) * s.k * s.k
        std = np.sqrt((2.0 if s.act else 1.0) / fan_in)
        w = rng.standard_normal(s.weight_shape, dtype=np.float32) * np.float32(std)
        b = rng.standard_normal((s.c2,), dtype=np.float32) * np.float32(0.1)
        if ".cv3." in s.name and s.name.endswith(".2"):
            b = b * 0 + np.float32(-4.6)
        if cal is not None:
            w = w * np.float32(cal[s.name])
        out[s.name + ".weight"] = w
        out[s.name + ".bias"] = b
    return out


def rrdbnet_weights(scale: int = 4, num_block: int = 23, seed: int = 0, calibrated: bool = True) -> Dict[str, np.ndarray]:
    """RRDBNet conv weights/biases; (calibrated) unit-std conv outputs, conv_last centred on 0.5 so the uint8 output
    is neither black nor saturated."""
    rng = np.random.default_rng(seed + 1000)
    cal = _calib(f"rrdbnet_x{scale}") if calibrated else None
    out: Dict[str, np.ndarray] = {}
    for s in arch.rrdbnet_convs(scale, num_block):
        fan_in = s.c1 * 9
        w = rng.standard_normal(s.weight_shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in))
        b = rng.standard_normal((s.c2,), dtype=np.float32) * np.float32(0.05)
        if s.name == "conv_last":
            b = b * 0 + np.float32(0.5)
        if cal is not None:
            key = s.name if s.name in cal else s.name.replace(f"body.{s.name.split('.')[1]}.", "body.0.") if s.name.startswith("body.") else s.name
            w = w * np.float32(cal[key])
        out[s.name + ".weight"] = w
        out[s.name + ".bias"] = b
    return out


def _octave_noise(rng: np.random.Generator, h: int, w: int, octaves=(64, 32, 16, 8)) -> np.ndarray:
    """Sum of bilinearly upsampled uniform noise grids -> float32 (h, w) in ~[0, 1]."""
    acc = np.zeros((h, w), np.float32)
    amp, tot = 1.0, 0.0
    for cell in octaves:
        gh, gw = h // cell + 2, w // cell + 2
        g = rng.random((gh, gw), dtype=np.float32)
        ys = (np.arange(h, dtype=np.float32) / cell)
        xs = (np.arange(w, dtype=np.float32) / cell)
        y0 = ys.astype(np.int32); x0 = xs.astype(np.int32)
        fy = (ys - y0)[:, None]; fx = (xs - x0)[None, :]
        a = g[y0][:, x0]; b = g[y0][:, x0 + 1]; c = g[y0 + 1][:, x0]; d = g[y0 + 1][:, x0 + 1]
        acc += amp * ((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy)
        tot += amp
        amp *= 0.5
    return acc / tot


def synthetic_frame(h: int, w: int, seed: int = 0, n_blobs: int = 48) -> np.ndarray:
    """uint8 (h, w, 3) frame: low-frequency background + face-like elliptical blobs."""
    rng = np.random.default_rng(seed)
    img = np.stack([_octave_noise(rng, h, w) for _ in range(3)], axis=-1)
    img = 0.15 + 0.7 * img
    for _ in range(n_blobs):
        s = int(np.exp(rng.uniform(np.log(16), np.log(min(160, h // 2, w // 2)))))
        cy = int(rng.integers(s, max(s + 1, h - s))); cx = int(rng.integers(s, max(s + 1, w - s)))
        y0, y1, x0, x1 = max(0, cy - s), min(h, cy + s), max(0, cx - s), min(w, cx + s)
        yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float32)
        r2 = ((yy - cy) / (0.5 * s)) ** 2 + ((xx - cx) / (0.38 * s)) ** 2
        m = np.clip(1.2 - r2, 0, 1)[..., None]
        tone = np.array([0.85, 0.65, 0.55], np.float32) * rng.uniform(0.6, 1.1)
        eyes = ((np.abs(yy - (cy - 0.12 * s)) < 0.05 * s) & (np.abs(np.abs(xx - cx) - 0.15 * s) < 0.06 * s))[..., None]
        patch = img[y0:y1, x0:x1]
        patch[:] = patch * (1 - m) + (tone * (1 - 0.7 * eyes)) * m
    return np.clip(img * 255.0 + 0.5, 0, 255).astype(np.uint8)


# ---- SCRFD (InsightFace det_*.onnx) ---------------------------------------------------------------------------------------------
# A small ONNX writer (protobuf wire format, no onnx package) and an SCRFD-10G-KPS-shaped random graph: ResNet-v1e backbone (deep stem,
# BasicBlock stages with avg_down shortcuts), PAFPN neck, per-stride head towers with a learned Scale on the bbox branch, InsightFace's
# 9 outputs. BatchNorm statistics are calibrated on a synthetic frame while the graph is built (each conv's output comes out roughly
# zero-mean, unit-variance), score biases so that ~1 % of anchors clear 0.5, bbox biases so that boxes are positive and overlap.

def _pb_varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _pb_key(field: int, wt: int) -> bytes:
    return _pb_varint((field << 3) | wt)


def _pb_bytes(field: int, data: bytes) -> bytes:
    return _pb_key(field, 2) + _pb_varint(len(data)) + data


def _pb_str(field: int, s: str) -> bytes:
    return _pb_bytes(field, s.encode())


def _pb_int(field: int, v: int) -> bytes:
    return _pb_key(field, 0) + _pb_varint(int(v))


def _pb_packed_ints(field: int, vals) -> bytes:
    return _pb_bytes(field, b"".join(_pb_varint(int(v)) for v in vals))


def onnx_tensor(name: str, a: np.ndarray, typed: bool = False) -> bytes:
    """TensorProto: float32 / int64, raw_data (typed=True: float_data / int64_data)."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        a = a.astype("<f4")
        dt = 1
    else:
        a = a.astype("<i8")
        dt = 7
    out = _pb_packed_ints(1, a.shape) + _pb_int(2, dt) + _pb_str(8, name)
    if typed:
        out += _pb_bytes(4, a.tobytes()) if dt == 1 else _pb_packed_ints(7, a.ravel())
    else:
        out += _pb_bytes(9, a.tobytes())
    return out


def _onnx_attr(name: str, v) -> bytes:
    out = _pb_str(1, name)
    if isinstance(v, float):
        return out + _pb_key(2, 5) + np.float32(v).tobytes() + _pb_int(20, 1)
    if isinstance(v, (bool, int, np.integer)):
        return out + _pb_int(3, int(v)) + _pb_int(20, 2)
    if isinstance(v, str):
        return out + _pb_bytes(4, v.encode()) + _pb_int(20, 3)
    if isinstance(v, np.ndarray):
        return out + _pb_bytes(5, onnx_tensor("", v)) + _pb_int(20, 4)
    if isinstance(v, (list, tuple)) and v and all(isinstance(x, float) for x in v):
        return out + _pb_bytes(7, np.asarray(v, "<f4").tobytes()) + _pb_int(20, 6)
    return out + _pb_packed_ints(8, v) + _pb_int(20, 7)


def _onnx_value_info(name: str, shape) -> bytes:
    dims = b"".join(_pb_bytes(1, _pb_int(1, d) if isinstance(d, int) and d > 0 else _pb_str(2, str(d))) for d in shape)
    ttype = _pb_int(1, 1) + _pb_bytes(2, dims)
    return _pb_str(1, name) + _pb_bytes(2, _pb_bytes(1, ttype))


def onnx_model(g: dict, opset: int = 11) -> bytes:
    """ModelProto bytes of a graph dict {nodes: [{op, name, inputs, outputs, attrs}], init: {name: array}, input: (name, shape),
    outputs: [(name, shape)]}."""
    body = b""
    for nd in g["nodes"]:
        n = b"".join(_pb_str(1, s) for s in nd["inputs"]) + b"".join(_pb_str(2, s) for s in nd["outputs"])
        n += _pb_str(3, nd["name"]) + _pb_str(4, nd["op"])
        n += b"".join(_pb_bytes(5, _onnx_attr(k, v)) for k, v in nd.get("attrs", {}).items())
        body += _pb_bytes(1, n)
    body += _pb_str(2, g.get("name", "scrfd"))
    for k, v in g["init"].items():
        body += _pb_bytes(5, onnx_tensor(k, v, typed=k in g.get("typed", ())))
    body += _pb_bytes(11, _onnx_value_info(*g["input"]))
    for name, shape in g["outputs"]:
        body += _pb_bytes(12, _onnx_value_info(name, shape))
    opset_b = _pb_str(1, "") + _pb_int(2, opset)
    return _pb_int(1, 7) + _pb_str(2, "ffp-synth") + _pb_bytes(8, opset_b) + _pb_bytes(7, body)


def scrfd_onnx(seed: int = 0, style: str = "unfolded", stem: int = 28, widths=(56, 88, 88, 224), depths=(3, 4, 2, 3), neck: int = 56,
               head: int = 80, stacked: int = 3, kps: bool = True, calib_size: int = 320, head_order: str = "batched"):
    """-> (onnx_bytes, graph dict). style 'unfolded': BatchNormalization nodes, Resize sizes from Shape; 'folded': BN folded into
    the convs, Resize with constant scales. head_order 'batched': Sigmoid -> Transpose(0,2,3,1) -> Reshape; 'export': the batch-1
    export's Transpose(2,3,0,1) -> Reshape -> Sigmoid. The graph dict is what tests/scrfd_ref.py interprets (no protobuf library needed)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    folded = style == "folded"
    g = {"nodes": [], "init": {}, "input": ("input.1", ["None", 3, "?", "?"]), "outputs": [], "typed": set()}
    cnt = [0]

    def uid(p):
        cnt[0] += 1
        return f"{p}_{cnt[0]}"

    def node(op, inputs, attrs=None, n_out=1):
        name = uid(op)
        outs = [f"{name}_out{i}" for i in range(n_out)]
        g["nodes"].append({"op": op, "name": name, "inputs": list(inputs), "outputs": outs, "attrs": attrs or {}})
        return outs[0] if n_out == 1 else outs

    def init(name, a):
        g["init"][name] = a
        return name

    # calibrated on picture-like input, as the tests feed: a frame and a x2-upscaled crop of it (slices are resized to the net size)
    img = synthetic_frame(calib_size, calib_size, seed=seed + 1)
    up = np.repeat(np.repeat(img[: calib_size // 2, : calib_size // 2], 2, 0), 2, 1)
    x0 = ((np.stack([img, up]).astype(np.float32) - 127.5) / 128.0).transpose(0, 3, 1, 2).copy()
    vals = {"input.1": torch.from_numpy(x0)}

    def conv(x, cout, k=3, s=1, bn=True, relu=True, gamma=(0.8, 1.2), wstd=None):
        t = vals[x]
        cin = t.shape[1]
        w = (rng.standard_normal((cout, cin, k, k)) * (wstd if wstd is not None else np.sqrt(2.0 / (cin * k * k)))).astype(np.float32)
        y = F.conv2d(t, torch.from_numpy(w), None, s, k // 2)
        b = np.zeros(cout, np.float32)
        if bn:
            m = y.mean(dim=(0, 2, 3)).numpy().astype(np.float32)
            v = y.var(dim=(0, 2, 3)).numpy().astype(np.float32) + 1e-3
            m = m + rng.normal(0, 0.05, cout).astype(np.float32) * np.sqrt(v)
            ga = rng.uniform(*gamma, cout).astype(np.float32)
            be = rng.normal(0, 0.1, cout).astype(np.float32)
            eps = 1e-5
            if folded:
                sc = ga / np.sqrt(v + eps)
                w = (w * sc[:, None, None, None]).astype(np.float32)
                b = (be - m * sc).astype(np.float32)
        else:
            b = rng.normal(0, 0.1, cout).astype(np.float32)
        ins = [x, init(uid("w"), w)]
        if not (bn and not folded):
            ins.append(init(uid("b"), b))
        out = node("Conv", ins, {"kernel_shape": [k, k], "strides": [s, s], "pads": [k // 2] * 4, "dilations": [1, 1], "group": 1})
        y = F.conv2d(t, torch.from_numpy(w), torch.from_numpy(b) if len(ins) == 3 else None, s, k // 2)
        if bn and not folded:
            out = node("BatchNormalization", [out, init(uid("g"), ga), init(uid("be"), be), init(uid("m"), m), init(uid("v"), v)], {"epsilon": eps})
            y = F.batch_norm(y, torch.from_numpy(m), torch.from_numpy(v), torch.from_numpy(ga), torch.from_numpy(be), False, 0.0, eps)
        vals[out] = y
        if relu:
            r = node("Relu", [out])
            vals[r] = F.relu(y)
            return r
        return out

    def add_relu(a, b):
        o = node("Add", [a, b])
        vals[o] = vals[a] + vals[b]
        r = node("Relu", [o])
        vals[r] = F.relu(vals[o])
        return r

    def basic_block(x, cout, s):
        cin = vals[x].shape[1]
        y = conv(x, cout, 3, s)
        y = conv(y, cout, 3, 1, relu=False, gamma=(0.2, 0.4))
        idt = x
        if s != 1 or cin != cout:
            if s != 1:
                idt = node("AveragePool", [x], {"kernel_shape": [s, s], "strides": [s, s], "ceil_mode": 1, "count_include_pad": 0})
                vals[idt] = F.avg_pool2d(vals[x], s, s, ceil_mode=True, count_include_pad=False)
            idt = conv(idt, cout, 1, 1, relu=False)
        return add_relu(y, idt)

    def up2(x, like):
        if folded:
            sc = init(uid("scales"), np.array([1.0, 1.0, 2.0, 2.0], np.float32))
            o = node("Resize", [x, "", sc], {"mode": "nearest", "coordinate_transformation_mode": "asymmetric", "nearest_mode": "floor"})
        else:
            sh = node("Shape", [like])
            st = init(uid("st"), np.array([2], np.int64))
            en = init(uid("en"), np.array([4], np.int64))
            hw = node("Slice", [sh, st, en])
            shx = node("Shape", [x])
            st0 = init(uid("st"), np.array([0], np.int64))
            en0 = init(uid("en"), np.array([2], np.int64))
            nc = node("Slice", [shx, st0, en0])
            sizes = node("Concat", [nc, hw], {"axis": 0})
            o = node("Resize", [x, "", "", sizes], {"mode": "nearest", "coordinate_transformation_mode": "asymmetric", "nearest_mode": "floor"})
        vals[o] = F.interpolate(vals[x], scale_factor=2, mode="nearest")
        return o

    # ---- backbone
    x = conv("input.1", stem, 3, 2)
    x = conv(x, stem, 3, 1)
    x = conv(x, 2 * stem, 3, 1)
    mp = node("MaxPool", [x], {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]})
    vals[mp] = F.max_pool2d(vals[x], 3, 2, 1)
    x = mp
    feats = []
    for si, (c, d) in enumerate(zip(widths, depths)):
        for bi in range(d):
            x = basic_block(x, c, 2 if (si > 0 and bi == 0) else 1)
        feats.append(x)
    c2, c3, c4 = feats[1], feats[2], feats[3]
    # ---- PAFPN
    lat = [conv(f, neck, 1, 1, bn=False, relu=False, wstd=1.0 / np.sqrt(vals[f].shape[1])) for f in (c2, c3, c4)]
    for i in (2, 1):
        u = up2(lat[i], lat[i - 1])
        o = node("Add", [lat[i - 1], u])
        vals[o] = vals[lat[i - 1]] + vals[u]
        lat[i - 1] = o
    outs = [conv(l, neck, 3, 1, bn=False, relu=False, wstd=1.0 / np.sqrt(9 * neck)) for l in lat]
    for i in (0, 1):
        dn = conv(outs[i], neck, 3, 2, bn=False, relu=False, wstd=1.0 / np.sqrt(9 * neck))
        o = node("Add", [outs[i + 1], dn])
        vals[o] = vals[outs[i + 1]] + vals[dn]
        outs[i + 1] = o
    outs = [outs[0]] + [conv(o, neck, 3, 1, bn=False, relu=False, wstd=1.0 / np.sqrt(9 * neck)) for o in outs[1:]]
    # ---- heads
    scores, bboxes, kpss = [], [], []
    A = 2
    for li, f in enumerate(outs):
        t = f
        for _ in range(stacked):
            t = conv(t, head, 3, 1)
        # score: calibrated so that ~1 % of the anchors clear 0.5
        # logits rescaled to std 0.3 (scores stay far from saturation on other inputs too: no exact ties at 1.0)
        cls = conv(t, A, 3, 1, bn=False, relu=False, wstd=1.0 / np.sqrt(9 * head))
        wname, bname = g["nodes"][-1]["inputs"][1], g["nodes"][-1]["inputs"][2]
        lg = vals[cls].numpy() - g["init"][bname][None, :, None, None]
        k = np.float32(0.3 / max(float(lg.std()), 1e-6))
        g["init"][wname] = (g["init"][wname] * k).astype(np.float32)
        lg = lg * k
        q = float(np.quantile(lg, 0.99))
        g["init"][bname] = np.full(A, -q, np.float32)
        vals[cls] = torch.from_numpy((lg - q).astype(np.float32))

        def layout(x, width, sigmoid=False):
            if head_order == "export":
                tr = node("Transpose", [x], {"perm": [2, 3, 0, 1]})
                r = node("Reshape", [tr, init(uid("shape"), np.array([-1, width], np.int64))])
                return node("Sigmoid", [r]) if sigmoid else r
            if sigmoid:
                x = node("Sigmoid", [x])
            tr = node("Transpose", [x], {"perm": [0, 2, 3, 1]})
            return node("Reshape", [tr, init(uid("shape"), np.array([-1, width], np.int64))])

        scores.append(layout(cls, 1, sigmoid=True))
        # bbox: positive distances of a few strides (overlapping boxes), then the learned Scale
        reg = conv(t, 4 * A, 3, 1, bn=False, relu=False, wstd=0.3 / np.sqrt(9 * head))
        wname, bname = g["nodes"][-1]["inputs"][1], g["nodes"][-1]["inputs"][2]
        dv = vals[reg].numpy() - g["init"][bname][None, :, None, None]
        g["init"][wname] = (g["init"][wname] * np.float32(0.05 / max(float(dv.std()), 1e-6))).astype(np.float32)    # distances stay positive
        g["init"][bname] = rng.uniform(2.0, 3.0, 4 * A).astype(np.float32)
        scale = np.array(rng.uniform(0.8, 1.2), np.float32).reshape(())
        ms = node("Mul", [reg, init(uid("scale"), scale)])
        bboxes.append(layout(ms, 4))
        if kps:
            kp = conv(t, 10 * A, 3, 1, bn=False, relu=False, wstd=0.3 / np.sqrt(9 * head))
            kpss.append(layout(kp, 10))
    for nm, w in [(s, 1) for s in scores] + [(b, 4) for b in bboxes] + [(k, 10) for k in kpss]:
        g["outputs"].append((nm, ["?", w]))
    return onnx_model(g), g


# ---- RT-DETR-l ----------------------------------------------------------------------------------------------------------------
def rtdetr_l_state_dict(nc: int = 1, seed: int = 0, calibrated: bool = True) -> Dict[str, np.ndarray]:
    """An unfused Ultralytics RT-DETR-l state dict (the key names and shapes of `RTDETR('rtdetr-l.pt').model.state_dict()`) with
    random tensors: He-style conv weights under near-identity BatchNorm statistics (eps 1e-3), unit LayerNorms, and heads
    calibrated so that a synthetic frame gives encoder / decoder logits spread around sigmoid^-1(0.25) (tens of detections per
    image at conf 0.25, a clear gap at the 300th encoder score) and boxes that stay near their anchors."""
    rng = np.random.default_rng(seed + 7000)
    sd: Dict[str, np.ndarray] = {}
    f32 = lambda a: np.asarray(a, np.float32)

    def conv(p, c1, c2, k, g=1, gain=np.sqrt(2.0)):
        sd[p + ".conv.weight"] = f32(rng.standard_normal((c2, c1 // g, k, k)) * gain / np.sqrt(c1 // g * k * k))
        sd[p + ".bn.weight"] = f32(rng.uniform(0.8, 1.2, c2))
        sd[p + ".bn.bias"] = f32(rng.normal(0, 0.05, c2))
        sd[p + ".bn.running_mean"] = f32(rng.normal(0, 0.05, c2))
        sd[p + ".bn.running_var"] = f32(rng.uniform(0.8, 1.2, c2))
        sd[p + ".bn.num_batches_tracked"] = np.zeros((), np.float32)

    def lin(p, c1, c2, gain=1.0, bias=0.02):
        sd[p + ".weight"] = f32(rng.standard_normal((c2, c1)) * gain / np.sqrt(c1))
        sd[p + ".bias"] = f32(rng.normal(0, bias, c2))

    def ln(p, c):
        sd[p + ".weight"] = f32(rng.uniform(0.9, 1.1, c))
        sd[p + ".bias"] = f32(rng.normal(0, 0.02, c))

    def mha(p, d):
        sd[p + ".in_proj_weight"] = f32(rng.standard_normal((3 * d, d)) / np.sqrt(d))
        sd[p + ".in_proj_bias"] = f32(rng.normal(0, 0.02, 3 * d))
        lin(p + ".out_proj", d, d)

    conv("model.0.stem1", 3, 32, 3)
    conv("model.0.stem2a", 32, 16, 2)
    conv("model.0.stem2b", 16, 32, 2)
    conv("model.0.stem3", 64, 32, 3)
    conv("model.0.stem4", 32, 48, 1)
    for (li, c1, cm, c2, k, light, _sc) in arch.RTDETR_L_HGBLOCKS:
        for i in range(6):
            ci = c1 if i == 0 else cm
            if light:
                conv(f"model.{li}.m.{i}.conv1", ci, cm, 1, gain=1.0)
                conv(f"model.{li}.m.{i}.conv2", cm, cm, k, g=cm)
            else:
                conv(f"model.{li}.m.{i}", ci, cm, k)
        conv(f"model.{li}.sc", c1 + 6 * cm, c2 // 2, 1)
        conv(f"model.{li}.ec", c2 // 2, c2, 1, gain=1.0)
    for (li, c) in arch.RTDETR_L_DWCONVS:
        conv(f"model.{li}", c, c, 3, g=c, gain=1.0)
    hd = arch.RTDETR_HD
    conv("model.10", 2048, hd, 1, gain=1.0)
    mha("model.11.ma", hd)
    lin("model.11.fc1", hd, 1024, gain=np.sqrt(2.0))
    lin("model.11.fc2", 1024, hd)
    ln("model.11.norm1", hd)
    ln("model.11.norm2", hd)
    conv("model.12", hd, hd, 1)
    conv("model.14", 1024, hd, 1, gain=1.0)
    conv("model.17", hd, hd, 1)
    conv("model.19", 512, hd, 1, gain=1.0)
    conv("model.22", hd, hd, 3)
    conv("model.25", hd, hd, 3)
    for li in arch.RTDETR_L_REPC3:
        conv(f"model.{li}.cv1", 2 * hd, hd, 1)
        conv(f"model.{li}.cv2", 2 * hd, hd, 1)
        for j in range(3):
            conv(f"model.{li}.m.{j}.conv1", hd, hd, 3, gain=1.0)
            conv(f"model.{li}.m.{j}.conv2", hd, hd, 1, gain=0.5)
    d = "model.28"
    for i in range(3):
        sd[f"{d}.input_proj.{i}.0.weight"] = f32(rng.standard_normal((hd, hd, 1, 1)) / np.sqrt(hd))
        sd[f"{d}.input_proj.{i}.1.weight"] = f32(rng.uniform(0.8, 1.2, hd))
        sd[f"{d}.input_proj.{i}.1.bias"] = f32(rng.normal(0, 0.05, hd))
        sd[f"{d}.input_proj.{i}.1.running_mean"] = f32(rng.normal(0, 0.05, hd))
        sd[f"{d}.input_proj.{i}.1.running_var"] = f32(rng.uniform(0.8, 1.2, hd))
        sd[f"{d}.input_proj.{i}.1.num_batches_tracked"] = np.zeros((), np.float32)
    sd[f"{d}.denoising_class_embed.weight"] = f32(rng.standard_normal((nc + 1, hd)))
    lin(f"{d}.enc_output.0", hd, hd, bias=0.0)          # an invalid anchor's feature is LayerNorm(bias): keep it far below the top 300
    sd[f"{d}.enc_output.0.bias"][:] = 0
    ln(f"{d}.enc_output.1", hd)
    sd[f"{d}.enc_output.1.bias"][:] = 0
    for j, (a, b) in enumerate([(hd, hd), (hd, hd), (hd, 4)]):
        lin(f"{d}.enc_bbox_head.layers.{j}", a, b, gain=np.sqrt(2.0) if j < 2 else 0.1)
    lin(f"{d}.query_pos_head.layers.0", 4, 2 * hd, gain=np.sqrt(2.0) * 2)
    lin(f"{d}.query_pos_head.layers.1", 2 * hd, hd)
    L, H, P = arch.RTDETR_LEVELS, arch.RTDETR_HEADS, arch.RTDETR_POINTS
    for i in range(arch.RTDETR_LAYERS):
        p = f"{d}.decoder.layers.{i}"
        mha(p + ".self_attn", hd)
        ln(p + ".norm1", hd)
        lin(p + ".cross_attn.sampling_offsets", hd, H * L * P * 2, gain=1.0, bias=0.5)
        lin(p + ".cross_attn.attention_weights", hd, H * L * P, gain=1.0)
        lin(p + ".cross_attn.value_proj", hd, hd)
        lin(p + ".cross_attn.output_proj", hd, hd)
        ln(p + ".norm2", hd)
        lin(p + ".linear1", hd, arch.RTDETR_FFN, gain=np.sqrt(2.0))
        lin(p + ".linear2", arch.RTDETR_FFN, hd)
        ln(p + ".norm3", hd)
        for j, (a, b) in enumerate([(hd, hd), (hd, hd), (hd, 4)]):
            lin(f"{d}.dec_bbox_head.{i}.layers.{j}", a, b, gain=np.sqrt(2.0) if j < 2 else 0.1)
    # class heads last, from their own stream: everything above does not depend on nc. The decoder's queries share a large common
    # component (random weights, no training): the score head is scaled up and centred on the mean final query embedding measured
    # on synthetic frames (synth_calib_rtdetr.json), so that logits spread about -1.1 with a std near 1.
    rng = np.random.default_rng(seed + 7001)
    cal = {}
    if calibrated:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "synth_calib_rtdetr.json")) as f:
            cal = json.load(f)
    mean = np.asarray(cal.get(f"dec_mean_nc{nc}", cal.get("dec_mean_nc1")), np.float64) if calibrated else np.zeros(hd)
    lin(f"{d}.enc_score_head", hd, nc, gain=1.0)
    sd[f"{d}.enc_score_head.bias"][:] = -1.1
    for i in range(arch.RTDETR_LAYERS):
        w = rng.standard_normal((nc, hd)) * (12.0 if calibrated else 1.0) / np.sqrt(hd)
        sd[f"{d}.dec_score_head.{i}.weight"] = f32(w)
        sd[f"{d}.dec_score_head.{i}.bias"] = f32(-1.1 - w @ mean)
    return sd


def rtdetr_l_weights(nc: int = 1, seed: int = 0, calibrated: bool = True) -> Dict[str, np.ndarray]:
    """rtdetr_l_state_dict through the checkpoint converter: the FFPW tensors ffp_rtdetr_create loads."""
    from .weights_io import from_ultralytics_rtdetr_state_dict
    return from_ultralytics_rtdetr_state_dict(rtdetr_l_state_dict(nc, seed, calibrated))

"""CPU oracle of realesrgan 0.3.0 RealESRGANer.enhance(img, outscale, alpha_upsampler) for every input layout it takes
(reference call utils/enhancer.py:214): gray ('L'), BGR ('RGB') and BGRA ('RGBA', both alpha upsamplers), 8- or 16-bit,
with the Lanczos4 outscale. The network is oracle.rrdbnet_ref.RRDBNetRef.forward; the tile loop of
oracle.rrdbnet_ref.enhance is restated here for float input. The three cv2 functions the path uses are restated in numpy:

* cvtColor(BGR2GRAY), float32: Y = B*0.114f + G*0.587f + R*0.299f, summed left to right;
* resize(INTER_LINEAR), float32: fx = (float)((dx + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx; horizontally a tap
  outside the image resets to the border pixel with weight 0, vertically only the rows are clamped;
* resize(INTER_LANCZOS4): OpenCV's interpolateLanczos4 weights (sin / cos in double: math.sin / math.cos, the libm the
  library's host code calls too), taps sx-3 .. sx+4 clamped; uint8 with int16 weights (x2048) and integer sums (checked to
  stay inside int32), uint16 with float32 weights and float32 sums left to right.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


# ---- cv2 pieces ----------------------------------------------------------------------------------------------------------
def bgr2gray(bgr: np.ndarray) -> np.ndarray:
    b, g, r = bgr[..., 0].astype(F32), bgr[..., 1].astype(F32), bgr[..., 2].astype(F32)
    return (b * F32(0.114) + g * F32(0.587)) + r * F32(0.299)


def _phase(d: int, scale: float):
    """(sx, fx) of output index d: fx = (float)((d + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx (float32)."""
    f = F32((d + 0.5) * scale - 0.5)
    s = int(math.floor(float(f)))
    return s, F32(f - F32(s))


def linear_phases(n_in: int, n_out: int, reset: bool):
    """Per output index: (first tap, weight of the second tap). reset = the horizontal border rule of cv::resize."""
    scale = 1.0 / (n_out / n_in)
    out = []
    for d in range(n_out):
        s, f = _phase(d, scale)
        if reset:
            if s < 0:
                s, f = 0, F32(0)
            if s >= n_in - 1:
                s, f = n_in - 1, F32(0)
        out.append((s, f))
    return out


def resize_linear_f32(src: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """cv2.resize(src, (out_w, out_h), interpolation=INTER_LINEAR) of a float32 HxW plane."""
    src = np.asarray(src, F32)
    h, w = src.shape
    px = linear_phases(w, out_w, True)
    py = linear_phases(h, out_h, False)
    sx = np.array([p[0] for p in px])
    fx = np.array([p[1] for p in px], F32)
    sx1 = np.minimum(sx + 1, w - 1)
    hor = src[:, sx] * (F32(1) - fx) + src[:, sx1] * fx                          # h x out_w, float32
    sy = np.array([p[0] for p in py])
    fy = np.array([p[1] for p in py], F32)[:, None]
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    return hor[y0] * (F32(1) - fy) + hor[y1] * fy


_S45 = 0.70710678118654752440084436210485
_CS = ((1, 0), (-_S45, -_S45), (0, 1), (_S45, -_S45), (-1, 0), (_S45, _S45), (0, -1), (-_S45, _S45))


def lanczos4_coefs(fx) -> np.ndarray:
    """OpenCV interpolateLanczos4(x) for a float32 x in [0, 1): 8 float32 weights summing to ~1."""
    x3 = F32(F32(fx) + F32(3))
    y0 = -float(x3) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c = np.zeros(8, F32)
    tot = F32(0)
    for i in range(8):
        t = F32(x3 - F32(i))
        if abs(float(t)) >= float(F32(1e-6)):
            y = -float(t) * math.pi * 0.25
            c[i] = F32((_CS[i][0] * s0 + _CS[i][1] * c0) / (y * y))
        else:
            c[i] = F32(1e30)
        tot = F32(tot + c[i])
    inv = F32(F32(1) / tot)
    return (c * inv).astype(F32)


def lanczos4_axis(n_in: int, n_out: int):
    """(sx per output index, float32 weights n_out x 8, int16 weights rint(w * 2048))."""
    scale = 1.0 / (n_out / n_in)
    ofs = np.zeros(n_out, np.int64)
    cf = np.zeros((n_out, 8), F32)
    for d in range(n_out):
        s, f = _phase(d, scale)
        ofs[d] = s
        cf[d] = lanczos4_coefs(f)
    ic = np.rint(cf * F32(2048)).astype(np.int64)
    return ofs, cf, ic


INT32_MAX = 2 ** 31 - 1


def resize_lanczos4(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """cv2.resize(img, (out_w, out_h), interpolation=INTER_LANCZOS4) for uint8 / uint16, HxW or HxWxC."""
    h, w = img.shape[:2]
    if (out_w, out_h) == (w, h):
        return img.copy()
    two_d = img.ndim == 2
    src = img[..., None] if two_d else img
    xo, xc, xi = lanczos4_axis(w, out_w)
    yo, yc, yi = lanczos4_axis(h, out_h)
    xs = np.clip(xo[:, None] - 3 + np.arange(8)[None, :], 0, w - 1)            # out_w x 8
    ys = np.clip(yo[:, None] - 3 + np.arange(8)[None, :], 0, h - 1)            # out_h x 8
    if img.dtype == np.uint8:
        s = src.astype(np.int64)
        hor = np.zeros((h, out_w, src.shape[2]), np.int64)
        for k in range(8):
            hor += s[:, xs[:, k]] * xi[:, k][None, :, None]
        v = np.zeros((out_h, out_w, src.shape[2]), np.int64)
        for r in range(8):
            v += hor[ys[:, r]] * yi[:, r][:, None, None]
        assert np.abs(hor).max() <= INT32_MAX and np.abs(v).max() <= INT32_MAX, "int32 accumulation would overflow"
        out = np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    elif img.dtype == np.uint16:
        s = src.astype(F32)
        hor = np.zeros((h, out_w, src.shape[2]), F32)
        for k in range(8):
            hor = hor + s[:, xs[:, k]] * xc[:, k][None, :, None]
        v = np.zeros((out_h, out_w, src.shape[2]), F32)
        for r in range(8):
            v = v + hor[ys[:, r]] * yc[:, r][:, None, None]
        out = np.clip(np.rint(v), 0, 65535).astype(np.uint16)
    else:
        raise TypeError(img.dtype)
    return out[..., 0] if two_d else out


# ---- the network on float input --------------------------------------------------------------------------------------------
def net_rgb(net, x_rgb: np.ndarray, tile: int = 0, tile_pad: int = 10, pre_pad: int = 0) -> np.ndarray:
    """RealESRGANer pre_process / tile_process / post_process on an HxWx3 float32 RGB image -> clamp(0, 1), (s*h) x (s*w) x 3 RGB."""
    s = net.scale
    x = torch.from_numpy(np.ascontiguousarray(x_rgb.transpose(2, 0, 1))).float().unsqueeze(0)
    if pre_pad:
        x = F.pad(x, (0, pre_pad, 0, pre_pad), "reflect")
    mod = 2 if s == 2 else 4 if s == 1 else None
    mph = mpw = 0
    if mod is not None:
        _, _, h, w = x.shape
        if h % mod:
            mph = mod - h % mod
        if w % mod:
            mpw = mod - w % mod
        x = F.pad(x, (0, mpw, 0, mph), "reflect")
    _, c, H, W = x.shape
    if tile > 0:
        out = x.new_zeros((1, c, H * s, W * s))
        for ty in range(math.ceil(H / tile)):
            for tx in range(math.ceil(W / tile)):
                sx, ex = tx * tile, min(tx * tile + tile, W)
                sy, ey = ty * tile, min(ty * tile + tile, H)
                sxp, exp_ = max(sx - tile_pad, 0), min(ex + tile_pad, W)
                syp, eyp = max(sy - tile_pad, 0), min(ey + tile_pad, H)
                o = net.forward(x[:, :, syp:eyp, sxp:exp_])
                oxs, oys = (sx - sxp) * s, (sy - syp) * s
                out[:, :, sy * s:ey * s, sx * s:ex * s] = o[:, :, oys:oys + (ey - sy) * s, oxs:oxs + (ex - sx) * s]
    else:
        out = net.forward(x)
    _, _, h, w = out.shape
    out = out[:, :, 0:h - mph * s, 0:w - mpw * s]
    _, _, h, w = out.shape
    out = out[:, :, 0:h - pre_pad * s, 0:w - pre_pad * s]
    return out.squeeze(0).float().clamp_(0, 1).numpy().transpose(1, 2, 0).astype(F32)


def _net_bgr(net, x_rgb, **kw):
    return net_rgb(net, x_rgb, **kw)[..., ::-1]


def enhance(net, img: np.ndarray, outscale=None, alpha_upsampler: str = "realesrgan", tile: int = 0, tile_pad: int = 10,
            pre_pad: int = 0, resize: bool = True):
    """RealESRGANer.enhance -> (output, mode). resize=False stops before the outscale step (the test compares the Lanczos4
    step on the library's own outscale=None output)."""
    s = net.scale
    kw = dict(tile=tile, tile_pad=tile_pad, pre_pad=pre_pad)
    h_in, w_in = img.shape[:2]
    x = img.astype(F32)
    max_range = 65535 if np.max(x) > 256 else 255
    x = x / F32(max_range)
    alpha = None
    if x.ndim == 2:
        mode = "L"
        x = np.repeat(x[..., None], 3, axis=2)
    elif x.shape[2] == 4:
        mode = "RGBA"
        alpha = x[..., 3]
        x = x[..., 2::-1]
    else:
        mode = "RGB"
        x = x[..., ::-1]
    out = _net_bgr(net, np.ascontiguousarray(x), **kw)
    if mode == "L":
        out = bgr2gray(out)
    elif mode == "RGBA":
        if alpha_upsampler == "realesrgan":
            a = bgr2gray(_net_bgr(net, np.ascontiguousarray(np.repeat(alpha[..., None], 3, axis=2)), **kw))
        else:
            a = resize_linear_f32(alpha, w_in * s, h_in * s)
        out = np.concatenate([out, a[..., None]], axis=2)
    if max_range == 65535:
        out = (out * F32(65535.0)).round().astype(np.uint16)
    else:
        out = (out * F32(255.0)).round().astype(np.uint8)
    if resize and outscale is not None and outscale != float(s):
        out = resize_lanczos4(out, int(w_in * outscale), int(h_in * outscale))
    return out, mode

"""What the operator-level tests of the Real-ESRGAN pre/post kernels share (tests/test_sr_ops_ref.py on the CPU, tests/test_gpu_sr_ops.py on the
GPU): a fake network for the oracle in tests/realesrgan_formats_ref.py, the test images and their layouts inside one byte buffer, and the
prescribed network outputs.

The fake network has `.scale` and `.forward` like oracle.rrdbnet_ref.RRDBNetRef. It records every tensor the oracle's tile loop hands it — for
scale 2 after F.pixel_unshuffle(x, 2), which RRDBNetRef.forward applies internally — and returns a prescribed (1, 3, s*h, s*w) tensor per
call. The recorded tensors are then what the input kernel has to write, and what `enhance` returns is the canvas the output kernel has to
write from the same prescribed tensors."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import realesrgan_formats_ref as R

F32 = np.float32
SEL_BGR, SEL_GRAY, SEL_ALPHA = 0, 1, 2


class FakeNet:
    """make_out(call index, recorded input (h, w, C), out_h, out_w) -> (out_h, out_w, 3) float32 RGB."""

    def __init__(self, scale: int, make_out):
        self.scale = scale
        self.make_out = make_out
        self.inputs, self.outputs = [], []

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.detach().clone()
        assert x.dtype == torch.float32 and x.shape[0] == 1 and x.shape[1] == 3, (x.dtype, x.shape)
        rec = F.pixel_unshuffle(x, 2) if self.scale == 2 else x
        self.inputs.append(rec[0].permute(1, 2, 0).contiguous().numpy().copy())
        h, w = x.shape[2] * self.scale, x.shape[3] * self.scale
        o = np.ascontiguousarray(self.make_out(len(self.outputs), self.inputs[-1], h, w), F32)
        assert o.shape == (h, w, 3), (o.shape, h, w)
        self.outputs.append(o)
        return torch.from_numpy(o.transpose(2, 0, 1)[None].copy())


def nearest_out(scale: int):
    """An identity-like network: every input pixel repeated scale x scale times."""
    def make(_k, rec, h, w):
        x = rec
        if scale == 2:      # undo the pixel_unshuffle: channel c*4 + dy*2 + dx of (h/2, w/2) -> pixel (2y + dy, 2x + dx) of channel c
            hh, ww, _ = rec.shape
            x = rec.reshape(hh, ww, 3, 2, 2).transpose(0, 3, 1, 4, 2).reshape(2 * hh, 2 * ww, 3)
        return np.repeat(np.repeat(x, scale, axis=0), scale, axis=1)
    return make


def tie_values(max_range: int, parity: int, count: int, rng) -> np.ndarray:
    """float32 v with v * max_range == k + 0.5 exactly in float32, k of the given parity: candidates (k + 0.5) / max_range, kept where the
    float32 product confirms the tie."""
    ks = np.arange(parity, max_range, 2, dtype=np.int64)
    v = (ks.astype(F32) + F32(0.5)) / F32(max_range)
    ok = (v * F32(max_range)) == (ks.astype(F32) + F32(0.5))
    assert ok.sum() >= 8, (max_range, parity, int(ok.sum()))
    return rng.choice(v[ok], count)


def prescribed_out(max_range: int, seed: int):
    """Seeded network outputs: per tile and in equal shares values below 0 and above 1, -0.0, +inf, -inf, k / range exactly, ties k + 0.5 under
    `* range` for even and for odd k, and ordinary values. No NaN: the oracle's cast of NaN to an integer is undefined."""
    def make(k, _rec, h, w):
        rng = np.random.default_rng([seed, k, h, w])
        n = h * w * 3
        v = rng.uniform(-0.25, 1.25, n).astype(F32)
        cat = rng.permutation(n) % 16
        v[cat == 0] = F32(-0.0)
        v[cat == 1] = F32(np.inf)
        v[cat == 2] = F32(-np.inf)
        m = cat == 3
        v[m] = rng.integers(0, max_range, m.sum(), endpoint=True).astype(F32) / F32(max_range)
        for c, parity in ((4, 0), (5, 1)):
            m = cat == c
            v[m] = tie_values(max_range, parity, int(m.sum()), rng)
        m = cat == 6
        v[m] = rng.uniform(-3.0, -1e-3, m.sum()).astype(F32)
        m = cat == 7
        v[m] = rng.uniform(1.0 + 1e-3, 3.0, m.sum()).astype(F32)
        assert all((cat == c).any() for c in range(16))
        return v.reshape(h, w, 3)
    return make


# ---- test images --------------------------------------------------------------------------------------------------------------------
# layout: (name, channels, storage dtype, max_range, selections one enhance() call sends through the network, in its order)
LAYOUTS = [
    ("gray8", 1, np.uint8, 255), ("gray16r255", 1, np.uint16, 255), ("gray16", 1, np.uint16, 65535),
    ("bgr8", 3, np.uint8, 255), ("bgr16r255", 3, np.uint16, 255), ("bgr16", 3, np.uint16, 65535),
    ("bgra8", 4, np.uint8, 255), ("bgra16r255", 4, np.uint16, 255), ("bgra16", 4, np.uint16, 65535),
]


def layout(name: str):
    return next(l for l in LAYOUTS if l[0] == name)


def selections(cn: int):
    return {1: [SEL_GRAY], 3: [SEL_BGR], 4: [SEL_BGR, SEL_ALPHA]}[cn]


def make_image(name: str, h: int, w: int, seed: int) -> np.ndarray:
    """Random image of a layout whose maximum makes the oracle pick the layout's max_range (> 256: 65535, else 255); 16-bit storage with
    range 255 holds values up to 256, as the oracle's `> 256` rule admits."""
    _, cn, dt, max_range = layout(name)
    rng = np.random.default_rng([seed, h, w, cn])
    top = 65535 if max_range == 65535 else 256 if dt == np.uint16 else 255
    a = rng.integers(0, top, (h, w, cn), endpoint=True).astype(dt)
    a[rng.integers(0, h), rng.integers(0, w), rng.integers(0, cn)] = top
    a[rng.integers(0, h), rng.integers(0, w), rng.integers(0, cn)] = 0
    if max_range == 65535:
        a[0, 0, 0] = max(int(a[0, 0, 0]), 257)
    assert (65535 if a.max() > 256 else 255) == max_range
    return a[..., 0] if cn == 1 else a


class Buffer:
    """Images inside one byte buffer: tight (offset 0, 16-byte rounded, rows of w * px bytes) or strided (a first offset of 6 bytes, gaps that are
    no multiple of 16, rows padded by three elements)."""

    def __init__(self, strided: bool, fill_seed: int = 0):
        self.strided = strided
        self.size = 6 if strided else 0
        self.items = []
        self.fill_seed = fill_seed

    def add(self, h: int, w: int, cn: int, dt) -> int:
        es = np.dtype(dt).itemsize
        stride = (w * cn + (3 if self.strided else 0)) * es
        off = self.size
        self.items.append((off, stride, h, w, cn, np.dtype(dt)))
        end = off + h * stride
        self.size = end + 10 if self.strided else (end + 15) // 16 * 16
        return len(self.items) - 1

    def alloc(self) -> np.ndarray:
        return np.random.default_rng([77, self.fill_seed, self.size]).integers(0, 256, self.size + 32, dtype=np.uint8)

    def view(self, buf: np.ndarray, i: int) -> np.ndarray:
        off, stride, h, w, cn, dt = self.items[i]
        return np.ndarray((h, w, cn), dt, buffer=buf, offset=off, strides=(stride, cn * dt.itemsize, dt.itemsize))

    def desc(self, i: int, max_range: int, sel: int, h: int = None, w: int = None):
        """The 8-field image description of the operator entries; h, w override the stored size (a canvas is described by its input size)."""
        off, stride, ih, iw, cn, dt = self.items[i]
        return (off, stride, ih if h is None else h, iw if w is None else w, cn, 8 * dt.itemsize, max_range, sel)


def enhance_with(fake: FakeNet, img: np.ndarray, tile: int, tile_pad: int, pre_pad: int):
    """One oracle enhance() call ('realesrgan' alpha): (output, recorded inputs of this call, prescribed outputs of this call)."""
    k = len(fake.inputs)
    out, _ = R.enhance(fake, img, None, "realesrgan", tile=tile, tile_pad=tile_pad, pre_pad=pre_pad)
    return out, fake.inputs[k:], fake.outputs[k:]

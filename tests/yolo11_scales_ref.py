"""CPU reference (test infrastructure) for every YOLO11-pose scale: n, s, m, l (and x).

`oracle.yolo11_ref.Yolo11PoseRef` restates the n/s graph. The larger scales differ in two Ultralytics `parse_model` rules:
  * scales m, l and x set c3k=True on every C3k2 (n/s: only model.6, model.8 and model.22);
  * repeats are max(round(2 * depth), 1): 2 for l, which applies to every C3k2 (m.0, m.1 chained; cv2 takes (2 + n) * c
    channels) and to C2PSA (PSABlocks m.0, m.1 applied one after the other on b).
This subclass generalises c3k2, c2psa and features for both rules and is bit-for-bit the parent on n/s (same torch ops in the same
order). `oracle.ultra_post.predict / preprocess` take it as they take the parent.
"""
from __future__ import annotations

import os
import sys
from typing import Dict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.yolo11_ref import Yolo11PoseRef  # noqa: E402

DEPTH = {"n": 0.50, "s": 0.50, "m": 0.50, "l": 1.00, "x": 1.00}


class Yolo11ScalesRef(Yolo11PoseRef):
    def __init__(self, weights: Dict[str, np.ndarray], scale: str = "s", nc: int = 1, kpt_shape=(5, 3)):
        super().__init__(weights, scale, nc, kpt_shape)
        self.n = max(round(2 * DEPTH[scale]), 1)
        self.force_c3k = scale in "mlx"

    def c3k2(self, x, p, c3k: bool):
        c3k = c3k or self.force_c3k
        y = list(self.conv(x, p + ".cv1.conv", 1).chunk(2, 1))
        for i in range(self.n):
            y.append(self.c3k(y[-1], f"{p}.m.{i}") if c3k else self.bottleneck(y[-1], f"{p}.m.{i}"))
        return self.conv(torch.cat(y, 1), p + ".cv2.conv", 1)

    def c2psa(self, x, p):
        y = self.conv(x, p + ".cv1.conv", 1)
        a, b = y.chunk(2, 1)
        for i in range(self.n):
            b = b + self.attention(b, f"{p}.m.{i}.attn")
            b = b + self.conv(self.conv(b, f"{p}.m.{i}.ffn.0.conv", 1), f"{p}.m.{i}.ffn.1.conv", 1, act=False)
        return self.conv(torch.cat((a, b), 1), p + ".cv2.conv", 1)

    # features(): the parent's layer sequence already routes every C3k2 / C2PSA through the two methods above


def conv_flops(weights: Dict[str, np.ndarray], scale: str, h: int, w: int, nc=1, kpt_shape=(5, 3)) -> int:
    """2*MAC over convolutions + attention matmuls of every PSABlock for one (h, w) pass (oracle.yolo11_ref.conv_flops for any scale)."""
    m = Yolo11ScalesRef(weights, scale, nc, kpt_shape)
    m.keep_taps = True
    m.forward(torch.zeros(1, 3, h, w))
    total = 0
    for name, y in m.taps.items():
        wt = m.w[name + ".weight"]
        total += 2 * wt[0].numel() * wt.shape[0] * y.shape[2] * y.shape[3]
    C = m.w["model.10.m.0.attn.proj.conv.weight"].shape[0]
    nh = C // 64; hd = C // nh; kd = hd // 2
    N = (h // 32) * (w // 32)
    total += m.n * 2 * nh * N * N * (kd + hd)
    return total


class ReadCounter(dict):
    """A weight dict that counts how often each tensor is read (every tensor of a forward pass must be read exactly once)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.reads: Dict[str, int] = {}

    def __getitem__(self, k):
        self.reads[k] = self.reads.get(k, 0) + 1
        return super().__getitem__(k)


def forward_counting_reads(weights: Dict[str, np.ndarray], scale: str, h: int = 64, w: int = 64) -> Dict[str, int]:
    """Run one forward pass with a read-counting weight table; returns {tensor name: number of reads}."""
    m = Yolo11ScalesRef(weights, scale)
    m.w = ReadCounter(m.w)
    m.forward(torch.zeros(1, 3, h, w))
    return dict(m.w.reads)


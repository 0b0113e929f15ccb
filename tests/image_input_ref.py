"""Reference of the image-input kernels (tests/test_gpu_image_input.py, tests/test_image_input_ref.py): "the network image of box b of this
frame" for the three pre-processings, composed from the oracles the repository already has and nothing else —

  YOLO     oracle/ultra_post.py  letterbox (LetterBox auto=True, pad 114) over resize_linear_u8, then / 255
  RT-DETR  tests/rtdetr_ref.py   preprocess: resize_linear_u8 to imgsz x imgsz (a stretch), then / 255
  SCRFD    tests/scrfd_ref.py    geometry + blob: the resized picture at the top-left of a zero canvas, then (v - 127.5) / 128

as uint8 H x W x 3 first (so pad areas and clamps can be named exactly), then as the float records the kernels store: the three channels, flipped
when the frame is handed over as BGR, followed by zero pad channels. tests/test_image_input_ref.py ties these compositions back to the oracles'
own end-to-end functions and to hand-checked geometry, so that a wrong reference cannot agree with a wrong kernel by construction."""
import numpy as np

from oracle import ultra_post

import rtdetr_ref
import scrfd_ref

YOLO, RTDETR, SCRFD = 0, 1, 2
YOLO_PAD, SCRFD_PAD = 114, 0


def crop(frame: np.ndarray, box) -> np.ndarray:
    x0, y0, x1, y1 = (int(v) for v in box)
    return np.ascontiguousarray(frame[y0:y1, x0:x1])


def geometry(kind: int, box, size):
    """(net_h, net_w, new_h, new_w, top, bottom, left, right) of one box; size = imgsz, or (det_w, det_h) for SCRFD."""
    x0, y0, x1, y1 = (int(v) for v in box)
    h, w = y1 - y0, x1 - x0
    if kind == YOLO:
        new_w, new_h, top, bottom, left, right = ultra_post.letterbox_geometry(h, w, int(size))
        return new_h + top + bottom, new_w + left + right, new_h, new_w, top, bottom, left, right
    if kind == RTDETR:
        return int(size), int(size), int(size), int(size), 0, 0, 0, 0
    det_w, det_h = size
    new_w, new_h, _ = scrfd_ref.geometry(h, w, det_w, det_h)
    return det_h, det_w, new_h, new_w, 0, det_h - new_h, 0, det_w - new_w


def scrfd_scale(box, size) -> np.float32:
    x0, y0, x1, y1 = (int(v) for v in box)
    return np.float32(scrfd_ref.geometry(y1 - y0, x1 - x0, size[0], size[1])[2])


def network_u8(kind: int, frame: np.ndarray, box, size) -> np.ndarray:
    """The network image as uint8 H x W x 3 in the frame's own channel order."""
    src = crop(frame, box)
    if kind == YOLO:
        return ultra_post.letterbox(src, int(size))
    if kind == RTDETR:
        return ultra_post.resize_linear_u8(src, int(size), int(size))
    det_w, det_h = size
    new_w, new_h, _ = scrfd_ref.geometry(src.shape[0], src.shape[1], det_w, det_h)
    if new_w == 0 or new_h == 0:
        raise ValueError("cv2.resize: zero-size destination")
    canvas = np.zeros((det_h, det_w, 3), np.uint8)
    canvas[:new_h, :new_w] = ultra_post.resize_linear_u8(src, new_w, new_h)
    return canvas


def normalise(kind: int, u8: np.ndarray, half: bool = False) -> np.ndarray:
    """uint8 -> the float32 value the kernel stores (through fp16 when half)."""
    if kind == SCRFD:
        return (u8.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 128)
    q = u8.astype(np.float32) / np.float32(255)
    return q.astype(np.float16).astype(np.float32) if half else q


def records(kind: int, frame: np.ndarray, box, size, flip: bool, half: bool = False) -> np.ndarray:
    """(net_h, net_w, cs) float32: the whole pixel records, cs = 8 for half (YOLO, RT-DETR) and 4 otherwise, pad channels zero."""
    u8 = network_u8(kind, frame, box, size)
    if flip:
        u8 = u8[..., ::-1]
    cs = 8 if half and kind != SCRFD else 4
    out = np.zeros(u8.shape[:2] + (cs,), np.float32)
    out[..., :3] = normalise(kind, u8, half)
    return out


def pad_mask(kind: int, box, size) -> np.ndarray:
    """(net_h, net_w) bool: True where the network image is padding."""
    net_h, net_w, new_h, new_w, top, _, left, _ = geometry(kind, box, size)
    m = np.ones((net_h, net_w), bool)
    m[top:top + new_h, left:left + new_w] = False
    return m


def pad_value(kind: int) -> np.float32:
    return normalise(kind, np.asarray([SCRFD_PAD if kind == SCRFD else YOLO_PAD], np.uint8))[0]


ACTS = {0: lambda v: v, 1: lambda v: v / (1.0 + np.exp(-v)), 2: lambda v: np.where(v >= 0, v, 0.2 * v), 3: lambda v: np.maximum(v, 0.0)}


def conv3x3(x: np.ndarray, w: np.ndarray, b: np.ndarray, stride: int, act: int) -> np.ndarray:
    """float64 3x3 conv, pad 1, of an (h, w, cin) image with (cout, cin, 3, 3) weights, then the activation: (ho, wo, cout) float64."""
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float64)).permute(2, 0, 1)[None]
    y = F.conv2d(xt, torch.from_numpy(np.ascontiguousarray(w, np.float64)), torch.from_numpy(np.ascontiguousarray(b, np.float64)), stride=stride, padding=1)
    return ACTS[act](y[0].permute(1, 2, 0).numpy())

"""Shared inputs of the RT-DETR tile tests (tests/test_gpu_rtdetr_tiles.py, tests/test_gpu_rtdetr_sahi_compat.py): the frame, its seven tiles
and the float32 numpy restatement of FFP_RT_TILES_SAHI."""
import numpy as np

H, W, IMGSZ = 200, 264, 320
# Frame seeds 0..4 were run through rtdetr_ref (float64) on the CPU, all seven crops each, for the gap between the 300th and the 301st
# encoder score (a gap <= 1e-5 could reorder every query between two implementations). Smallest gap over the crops per seed:
# 0: 1.5e-04, 1: 9.7e-05, 2: 1.1e-04, 3: 1.3e-05, 4: 9.2e-05. Seed 0 has the widest margin and is used; seed 3 would be too close.
SEED = 0


def frame_bgr():
    from ffp_amd import synth
    return synth.synthetic_frame(H, W, seed=SEED)


def tiles(lib):
    """Six slices of the 96 x 96 grid at overlap 0.25 and the full-frame tile."""
    g = lib.slice_bboxes(H, W, 96, 96, 0.25, 0.25)
    assert len(g) >= 6
    return [[int(v) for v in t] for t in g[:6]] + [[0, 0, W, H]]


def crops(frame, tl):
    return [np.ascontiguousarray(frame[y0:y1, x0:x1]) for x0, y0, x1, y1 in tl]


def median_conf(det, frame, tl):
    """The median over all tiles' queries of the max class score: every test keeps and drops detections, whatever the weights produce."""
    raw, _ = det.forward_raw(crops(frame, tl), IMGSZ)
    return float(np.float32(np.median(raw[..., 4:].max(-1))))


def sahi_rows(local, tile, full_h, full_w):
    """FFP_RT_TILES_SAHI from tile-local rows, every step one float32 operation: clip against the FULL shape, drop unless x1 < x2 and
    y1 < y2, shift by the tile origin."""
    d = np.asarray(local, np.float32).reshape(-1, 6)
    zero, fw, fh = np.float32(0), np.float32(full_w), np.float32(full_h)
    x1, y1 = np.maximum(d[:, 0], zero), np.maximum(d[:, 1], zero)
    x2, y2 = np.minimum(d[:, 2], fw), np.minimum(d[:, 3], fh)
    keep = (x1 < x2) & (y1 < y2)
    sx, sy = np.float32(tile[0]), np.float32(tile[1])
    out = np.stack([x1 + sx, y1 + sy, x2 + sx, y2 + sy, d[:, 4], d[:, 5]], 1).astype(np.float32)
    assert out.dtype == np.float32
    return out[keep]

"""The two overlay primitives of include/ffp.h (ffp_overlay_prim) restated in numpy: the oracle for csrc/overlay.hip and for the primitive
builder of utils.visualization. `apply(img, prims, masks)` paints the records in list order into a copy of an h x w x 3 uint8 image."""
import numpy as np

RECT, STAMP = 0, 1


def _fill(img, x0, y0, x1, y1, color):
    """inclusive corners, clipped to the image"""
    h, w = img.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if x0 <= x1 and y0 <= y1:
        img[y0:y1 + 1, x0:x1 + 1] = color


def apply(img, prims, masks=None):
    out = np.array(img, np.uint8, copy=True)
    h, w = out.shape[:2]
    masks = np.zeros(0, np.uint8) if masks is None else np.asarray(masks, np.uint8).reshape(-1)
    for p in prims:
        x0, y0, x1, y1, t = int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"]), int(p["width"])
        color = np.asarray(p["color"][:3], np.uint8)
        if int(p["kind"]) == RECT:
            if t == 0 or x1 - x0 + 1 <= 2 * t or y1 - y0 + 1 <= 2 * t:          # no pixel is further than t from an edge
                _fill(out, x0, y0, x1, y1, color)
            else:
                _fill(out, x0, y0, x1, y0 + t - 1, color)
                _fill(out, x0, y1 - t + 1, x1, y1, color)
                _fill(out, x0, y0, x0 + t - 1, y1, color)
                _fill(out, x1 - t + 1, y0, x1, y1, color)
        else:
            mw, mh, off = x1, y1, int(p["mask_off"])
            ax, ay, bx, by = max(x0, 0), max(y0, 0), min(x0 + mw, w), min(y0 + mh, h)      # [ax, bx) x [ay, by)
            if ax >= bx or ay >= by:
                continue
            rows = off + (np.arange(ay, by) - y0)[:, None] * t + (np.arange(ax, bx) - x0)[None, :]
            m = masks[rows].astype(np.uint32)[..., None]
            dst = out[ay:by, ax:bx].astype(np.uint32)
            v = dst * (255 - m) + color.astype(np.uint32) * m + 128
            out[ay:by, ax:bx] = (((v >> 8) + v) >> 8).astype(np.uint8)
    return out

"""The eight EXIF orientations as numpy indexing: what csrc/orient.hip computes, what ImageOps.exif_transpose does to an image that carries the
tag, and what the cv2 shim's _oriented does to a decoded frame. A permutation of pixels, so every comparison against it is bit for bit."""
import numpy as np


def orient(a: np.ndarray, o: int) -> np.ndarray:
    """a: h x w or h x w x c. 1 as stored, 2 mirror x, 3 mirror both, 4 mirror y, 5 transpose, 6 transpose then mirror x, 7 transpose then mirror
    both, 8 transpose then mirror y. For 5..8 the result is w x h."""
    if not 1 <= o <= 8:
        raise ValueError(f"orientation {o}")
    if o >= 5:
        a = a.swapaxes(0, 1)
    if o in (2, 3, 6, 7):
        a = a[:, ::-1]
    if o in (3, 4, 7, 8):
        a = a[::-1]
    return np.ascontiguousarray(a)


def out_shape(h: int, w: int, o: int):
    return (w, h) if o >= 5 else (h, w)

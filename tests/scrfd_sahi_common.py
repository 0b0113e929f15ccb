"""Shared by tests/test_scrfd_sahi_rule.py and tests/test_gpu_scrfd_sliced.py: a numpy restatement of what ffp_op_scrfd_sahi_rows documents
(include/ffp.h), the hand-made faces both tests use, and the product's own per-face Python path over the same rows."""
import numpy as np

STRIDE = 21
FULL = (200, 260)                   # (h, w) of the frame the hand-made tiles are cut from
CONF = 0.5
CAP = 8
SENTINEL = -7.0
TILES = np.array([[40, 8, 136, 104], [164, 104, 260, 200], [0, 0, 260, 200]], np.int32)      # 96 x 96, 96 x 96 at the corner, the full frame


def sahi_rows(rows, tile, full_h, full_w, conf):
    """The six rules on the rows of one tile -> (surviving rows (k, 21) float32 in their order, indices of the rows the reference raises on)."""
    x0, y0 = int(tile[0]), int(tile[1])
    out, bad = [], []
    for r, row in enumerate(np.asarray(rows, np.float32).reshape(-1, STRIDE)):
        if row[4] < np.float32(conf):                                   # 1. strict, float32
            continue
        x1, y1, x2, y2 = (int(v) for v in row[:4].astype(np.int64))     # 2. toward zero
        x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, full_w), min(y2, full_h)      # 3. against the FULL frame
        if x2 < 0 or y2 < 0:                                            # 4. BoundingBox raises
            bad.append(r)
            continue
        o = row.copy()
        o[:4] = np.float32([x1 + x0, y1 + y0, x2 + x0, y2 + y0])         # 5. integers, then floats for the keypoints
        o[6::3] += np.float32(x0)
        o[7::3] += np.float32(y0)
        out.append(o)                                                   # 6. order kept
    return np.asarray(out, np.float32).reshape(-1, STRIDE), bad


def _row(box, score, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(STRIDE, np.float32)
    r[:4] = box
    r[4] = score
    k = r[6:].reshape(5, 3)
    k[:, 0] = rng.uniform(box[0], box[2] + 1, 5)
    k[:, 1] = rng.uniform(box[1], box[3] + 1, 5)
    k[:, 2] = 1.0
    return r


BELOW = np.nextafter(np.float32(CONF), np.float32(0))               # the float32 just below conf

HAND = {                            # (tile, row): box, score
    "plain": (0, 0, [10.7, 20.2, 50.9, 60.1], 0.9),
    "neg_corner": (0, 1, [-5.5, -3.2, 30.6, 40.4], 0.8),             # x1, y1 < 0: clamped to 0
    "frac_neg": (0, 2, [-0.7, -0.2, 20.5, 22.5], 0.7),               # truncates to 0 (a floor would give -1)
    "frac_neg_far": (0, 3, [-8.0, -9.0, -0.5, 12.3], 0.65),          # x2 truncates to 0: not negative, kept although x1 >= x2
    "on_conf": (0, 4, [30.0, 30.0, 40.0, 44.0], np.float32(CONF)),   # score == conf: kept (strict <)
    "below_conf": (0, 5, [31.0, 31.0, 41.0, 45.0], BELOW),           # dropped
    "past_crop": (0, 6, [90.1, 90.2, 120.9, 130.5], 0.6),            # past the 96 x 96 crop, inside the frame: not clipped
    "past_frame": (2, 0, [250.3, 190.2, 300.7, 240.9], 0.95),        # x2 > full_w, y2 > full_h: clamped
    "ff_plain": (2, 1, [100.5, 50.5, 140.2, 99.9], 0.85),
    "ff_below": (2, 2, [-40.0, 5.0, -3.0, 30.0], BELOW),             # negative x2 but skipped first: nobody raises
    "ff_last": (2, 3, [5.9, 6.9, 7.1, 8.1], 0.55),
}
NEGATIVE = {                        # the error variant: these replace rows of HAND
    "neg_x2": (2, 1, [-30.5, 3.0, -2.5, 10.0], 0.6),
    "neg_y2": (2, 3, [4.0, -20.0, 9.0, -1.5], 0.58),
}


def hand_rows(negative=False):
    """-> (dets (3, CAP, 21) with sentinels behind each tile's count, counts (7, 0, 4))."""
    dets = np.full((3, CAP, STRIDE), SENTINEL, np.float32)
    counts = np.array([7, 0, 4], np.int32)
    items = dict(HAND)
    if negative:
        items.update(NEGATIVE)
    for seed, (t, r, box, score) in enumerate(items.values()):
        dets[t, r] = _row(np.float32(box), score, seed)
    return dets, counts


def python_path(rows, tile, full, conf):
    """The product's per-face Python on one tile's rows: InsightFaceDetectionModel's conversion, then get_shifted_object_prediction
    -> (k, 5) float64 [x1, y1, x2, y2, score]. Raises what the reference raises."""
    import ffp_amd.compat as compat
    compat.install()
    from insightface.app import Face
    from utils.insightface_wrapper import InsightFaceDetectionModel
    m = InsightFaceDetectionModel(confidence_threshold=conf, load_at_init=False)
    m._original_predictions = [Face(bbox=r[:4].copy(), kps=r[6:].reshape(5, 3)[:, :2].copy(), det_score=np.float32(r[4])) for r in rows]
    m.convert_original_predictions(shift_amount=[int(tile[0]), int(tile[1])], full_shape=[int(full[0]), int(full[1])])
    out = [p.get_shifted_object_prediction() for p in m.object_prediction_list]
    return np.asarray([p.bbox.to_xyxy() + [p.score.value] for p in out], np.float64).reshape(-1, 5)

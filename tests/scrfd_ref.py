"""Tests-side reference of InsightFace's SCRFD detector (insightface 0.7.3): a node-by-node torch-CPU fp32 NCHW interpreter of the
ONNX subset (BatchNormalization, Mul by the Scale and the Shape subgraphs evaluated literally, nothing folded) over the graph dict
synth.scrfd_onnx returns, and a NumPy restatement of RetinaFace.detect / nms, FaceAnalysis.get and InsightFaceDetectionModel's
conversion.

Behaviour restated (model_zoo/retinaface.py, app/face_analysis.py, utils/insightface_wrapper.py):
- Geometry per tile (h, w) at net size (W, H): im_ratio = h / w, model_ratio = H / W; if im_ratio > model_ratio: new_h = H,
  new_w = int(new_h / im_ratio); else new_w = W, new_h = int(new_w * im_ratio). det_scale = new_h / h, used for both axes
  (small slices are upscaled). new_w or new_h == 0: cv2.resize raises (the library returns FFP_ERR_ARG, the compat layer ValueError).
- The resized picture (cv2 INTER_LINEAR) goes to the top-left of a zero canvas; blobFromImage(1/128, mean 127.5, swapRB=True).
- Scores: pos = scores >= det_thresh; anchor centres (x * stride, y * stride) repeated for the 2 anchors; distance2bbox /
  distance2kps with the distances * stride; / det_scale (float32). All levels stacked, ordered by descending score, then NMS:
  areas (x2 - x1 + 1) * (y2 - y1 + 1), overlap with +1 widths / heights floored at 0, kept when ovr <= nms_thresh (0.4).
  Equal scores: ascending anchor order (numpy's argsort is unstable; the tests avoid exact ties).
- Wrapper: x1, y1, x2, y2 = face.bbox.astype(int) (truncation toward zero), score < confidence_threshold skipped; a non-uint8
  image becomes (img * 255).astype(np.uint8).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ultra_post import resize_linear_u8


# ---- interpreter ------------------------------------------------------------------------------------------------------------------
def run_graph(g: dict, x: np.ndarray) -> list:
    """x: N x 3 x H x W float32 -> the graph outputs (numpy float32) in file order."""
    env = {g["input"][0]: torch.from_numpy(np.ascontiguousarray(x, np.float32))}
    for k, v in g["init"].items():
        env[k] = torch.from_numpy(np.asarray(v))

    def get(n):
        return env[n] if n else None

    for nd in g["nodes"]:
        op, a, ins = nd["op"], nd.get("attrs", {}), nd["inputs"]
        if op == "Conv":
            s = a.get("strides", [1, 1])[0]
            p = a.get("pads", [0, 0, 0, 0])[0]
            y = F.conv2d(get(ins[0]), get(ins[1]), get(ins[2]) if len(ins) > 2 else None, s, p)
        elif op == "BatchNormalization":
            y = F.batch_norm(get(ins[0]), get(ins[3]), get(ins[4]), get(ins[1]), get(ins[2]), False, 0.0, a.get("epsilon", 1e-5))
        elif op == "Relu":
            y = F.relu(get(ins[0]))
        elif op == "Sigmoid":
            y = torch.sigmoid(get(ins[0]))
        elif op == "Add":
            y = get(ins[0]) + get(ins[1])
        elif op == "Mul":
            y = get(ins[0]) * get(ins[1])
        elif op == "MaxPool":
            y = F.max_pool2d(get(ins[0]), a["kernel_shape"][0], a["strides"][0], a["pads"][0])
        elif op == "AveragePool":
            k = a["kernel_shape"][0]
            y = F.avg_pool2d(get(ins[0]), k, a["strides"][0], 0, ceil_mode=bool(a.get("ceil_mode", 0)),
                             count_include_pad=bool(a.get("count_include_pad", 0)))
        elif op == "Resize":
            t = get(ins[0])
            sizes = get(ins[3]) if len(ins) > 3 and ins[3] else None
            if sizes is not None:
                y = F.interpolate(t, size=[int(v) for v in sizes[2:]], mode="nearest")
            else:
                sc = get(ins[2]).tolist()
                y = F.interpolate(t, scale_factor=(sc[2], sc[3]), mode="nearest")
        elif op == "Shape":
            y = torch.tensor(list(get(ins[0]).shape), dtype=torch.int64)
        elif op == "Slice":
            t = get(ins[0])
            y = t[int(get(ins[1])[0]):int(get(ins[2])[0])]
        elif op == "Concat":
            y = torch.cat([get(i) for i in ins], dim=a.get("axis", 0))
        elif op == "Transpose":
            y = get(ins[0]).permute(*a["perm"])
        elif op == "Reshape":
            y = get(ins[0]).reshape(*[int(v) for v in get(ins[1])])
        else:
            raise NotImplementedError(op)
        env[nd["outputs"][0]] = y
    return [env[name].numpy().astype(np.float32) for name, _ in g["outputs"]]


# ---- RetinaFace.detect ------------------------------------------------------------------------------------------------------------
def geometry(h: int, w: int, net_w: int, net_h: int):
    im_ratio = float(h) / w
    model_ratio = float(net_h) / net_w
    if im_ratio > model_ratio:
        new_h = net_h
        new_w = int(new_h / im_ratio)
    else:
        new_w = net_w
        new_h = int(new_w * im_ratio)
    return new_w, new_h, float(new_h) / h


def blob(img_rgb_or_bgr: np.ndarray, net_w: int, net_h: int, flip: bool = True):
    """The network input of one tile: resize, top-left on zeros, (v - 127.5) / 128, channel swap when flip."""
    h, w = img_rgb_or_bgr.shape[:2]
    new_w, new_h, det_scale = geometry(h, w, net_w, net_h)
    if new_w == 0 or new_h == 0:
        raise ValueError("cv2.resize: zero-size destination")
    canvas = np.zeros((net_h, net_w, 3), np.uint8)
    canvas[:new_h, :new_w] = resize_linear_u8(np.ascontiguousarray(img_rgb_or_bgr), new_w, new_h)
    if flip:
        canvas = canvas[..., ::-1]
    x = (canvas.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 128)
    return x.transpose(2, 0, 1)[None].copy(), det_scale


def nms(dets: np.ndarray, thresh: float = 0.4) -> list:
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = np.arange(dets.shape[0])          # dets arrive in descending score order (see detect)
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        xx1 = np.maximum(x1[i], x1[order[1:]])
        yy1 = np.maximum(y1[i], y1[order[1:]])
        xx2 = np.minimum(x2[i], x2[order[1:]])
        yy2 = np.minimum(y2[i], y2[order[1:]])
        w = np.maximum(np.float32(0.0), xx2 - xx1 + np.float32(1))
        h = np.maximum(np.float32(0.0), yy2 - yy1 + np.float32(1))
        inter = w * h
        ovr = inter / (areas[i] + areas[order[1:]] - inter)
        inds = np.where(ovr <= np.float32(thresh))[0]
        order = order[inds + 1]
    return keep


def post(outs: list, det_scale: float, net_w: int, net_h: int, det_thresh: float = 0.5, nms_thresh: float = 0.4):
    """RetinaFace.forward's decode + detect's sort / NMS over one image's graph outputs (scores already sigmoid'ed).
    -> (det (k, 5) float32, kpss (k, 5, 2) float32)."""
    fmc = 3
    use_kps = len(outs) == 9
    scores_list, bboxes_list, kpss_list, idx_list = [], [], [], []
    base = 0
    for idx, stride in enumerate((8, 16, 32)):
        scores = outs[idx].reshape(-1, 1)
        bbox_preds = outs[idx + fmc].reshape(-1, 4) * np.float32(stride)
        height, width = net_h // stride, net_w // stride
        ac = np.stack(np.mgrid[:height, :width][::-1], axis=-1).astype(np.float32)
        ac = (ac * np.float32(stride)).reshape((-1, 2))
        ac = np.stack([ac] * 2, axis=1).reshape((-1, 2))
        pos = np.where(scores >= np.float32(det_thresh))[0]
        x1 = ac[:, 0] - bbox_preds[:, 0]
        y1 = ac[:, 1] - bbox_preds[:, 1]
        x2 = ac[:, 0] + bbox_preds[:, 2]
        y2 = ac[:, 1] + bbox_preds[:, 3]
        bboxes = np.stack([x1, y1, x2, y2], axis=-1)
        scores_list.append(scores[pos])
        bboxes_list.append(bboxes[pos])
        idx_list.append(pos + base)
        base += scores.shape[0]
        if use_kps:
            kp = outs[idx + 2 * fmc].reshape(-1, 10) * np.float32(stride)
            preds = []
            for i in range(0, 10, 2):
                preds.append(ac[:, i % 2] + kp[:, i])
                preds.append(ac[:, i % 2 + 1] + kp[:, i + 1])
            kpss_list.append(np.stack(preds, axis=-1).reshape((-1, 5, 2))[pos])
    scores = np.vstack(scores_list).ravel()
    anchor = np.concatenate(idx_list)
    order = np.lexsort((anchor, -scores))          # descending score, ties in ascending anchor order
    ds = np.float32(det_scale)
    bboxes = np.vstack(bboxes_list) / ds
    pre_det = np.hstack((bboxes, scores[:, None])).astype(np.float32, copy=False)[order]
    keep = nms(pre_det, nms_thresh)
    det = pre_det[keep]
    kpss = (np.vstack(kpss_list) / ds)[order][keep] if use_kps else np.zeros((len(keep), 5, 2), np.float32)
    return det, kpss.astype(np.float32)


def detect(g: dict, img: np.ndarray, net_w: int, net_h: int, det_thresh: float = 0.5, nms_thresh: float = 0.4, flip: bool = True):
    x, det_scale = blob(img, net_w, net_h, flip)
    outs = run_graph(g, x)
    return post(outs, det_scale, net_w, net_h, det_thresh, nms_thresh), outs


def wrapper_convert(det: np.ndarray, confidence_threshold: float):
    """InsightFaceDetectionModel's conversion: face.bbox.astype(int), score < threshold skipped -> [(x1, y1, x2, y2, score)]."""
    res = []
    for d in det:
        if d[4] < confidence_threshold:
            continue
        x1, y1, x2, y2 = d[:4].astype(int)
        res.append((int(x1), int(y1), int(x2), int(y2), float(d[4])))
    return res

"""Drop-in for the part of Ultralytics (8.x) that pipeline_v3_RTDETR/inference.py uses: `ultralytics.RTDETR(weights)` and its
`.predict(source=..., conf=...)`, with RT-DETR-l running on the GPU through libffp (ffp_rtdetr_*). Results carry `.boxes` with
`.xyxy` / `.conf` / `.cls` as torch CPU tensors (`box.xyxy[0].cpu().numpy()`, `box.conf[0]`), `.orig_shape`, `.orig_img`, `.path` and
`.names`. A real Ultralytics further down sys.path always wins: this module then re-exports it untouched (as the cv2 shim does).

Weights are FFPW files converted from the checkpoint (weights_io.from_ultralytics_rtdetr_state_dict, run where Ultralytics can unpickle
it) or "synthetic:rtdetr-l" (random calibrated weights, nc = 1). Training, validation, video, webcam and stream=True are not provided.
"""
import importlib.machinery
import importlib.util
import os
import sys

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _real_ultralytics():
    for p in sys.path:
        if not p or os.path.abspath(p) == _here:
            continue
        spec = importlib.machinery.PathFinder.find_spec("ultralytics", [p])
        if spec is not None and spec.origin and os.path.dirname(os.path.dirname(os.path.abspath(spec.origin))) != _here:
            return spec
    return None


_spec = _real_ultralytics()
if _spec is not None:                                   # Ultralytics is installed: be it
    _mod = importlib.util.module_from_spec(_spec)
    sys.modules[__name__] = _mod
    _spec.loader.exec_module(_mod)
else:
    from pathlib import Path

    import numpy as np

    __version__ = "8.0-ffp-shim"
    _VIDEO = (".mp4", ".avi", ".mov", ".mkv", ".webm", ".m4v", ".mpg", ".mpeg", ".wmv", ".gif")

    class Boxes:
        """The detections of one image (or one of them when iterated): torch CPU tensors xyxy [k, 4], conf [k], cls [k]."""

        def __init__(self, data):
            import torch
            self.data = torch.as_tensor(np.asarray(data, np.float32).reshape(-1, 6))

        def __len__(self):
            return int(self.data.shape[0])

        def __iter__(self):
            return (Boxes(self.data[i:i + 1].numpy()) for i in range(len(self)))

        def __getitem__(self, i):
            return Boxes(self.data[i].reshape(-1, 6).numpy())

        @property
        def xyxy(self):
            return self.data[:, :4]

        @property
        def conf(self):
            return self.data[:, 4]

        @property
        def cls(self):
            return self.data[:, 5]

        def cpu(self):
            return self

        def numpy(self):
            return self.data.numpy()

    class Results:
        def __init__(self, orig_img, path, names, boxes):
            self.orig_img = orig_img
            self.orig_shape = tuple(orig_img.shape[:2])
            self.path = path
            self.names = names
            self.boxes = Boxes(boxes)

        def __len__(self):
            return len(self.boxes)

    def _conversion_error(weights):
        return ValueError(f"{weights}: Ultralytics .pt checkpoints are pickled module graphs; convert them once with "
                          "weights_io.from_ultralytics_rtdetr_state_dict where `ultralytics` is installed and pass the .ffpw file")

    class RTDETR:
        """ultralytics.RTDETR (models/rtdetr/model.py) for rtdetr-l weights: predict() only."""

        def __init__(self, model="synthetic:rtdetr-l", task=None, verbose=False):
            from ffp_amd import synth, weights_io
            m = str(model)
            if m.startswith("synthetic:"):
                if m != "synthetic:rtdetr-l":
                    raise ValueError(f"{m}: only synthetic:rtdetr-l is provided")
                w = synth.rtdetr_l_weights(1)
            elif m.endswith((".pt", ".pth")):
                raise _conversion_error(m)
            elif m.endswith(".ffpw") or m.endswith(".bin"):
                w = weights_io.load(m)
            else:
                raise ValueError(f"{m}: expected an .ffpw file or synthetic:rtdetr-l")
            self.ckpt_path = m
            self.names = {i: ("face" if i == 0 else str(i)) for i in range(int(w["model.28.enc_score_head.weight"].shape[0]))}
            self._weights = w
            self._dets = {}

        def _det(self, precision):
            from ffp_amd import _lib
            if precision not in self._dets:
                self._dets[precision] = _lib.RTDETRDetector(self._weights, precision=precision)
            return self._dets[precision]

        def __call__(self, source=None, stream=False, **kw):
            return self.predict(source, stream=stream, **kw)

        def predict(self, source=None, conf=0.25, imgsz=640, max_det=300, classes=None, save=False, show=False, verbose=True, stream=False,
                    **kw):
            from ffp_amd import _lib
            if stream:
                raise NotImplementedError("RTDETR.predict(stream=True) is not provided by this build: pass images or a list of them")
            if show:
                raise NotImplementedError("RTDETR.predict(show=True) is not provided by this build (no display window)")
            if source is None:
                raise NotImplementedError("RTDETR.predict() without a source (the default asset) is not provided by this build")
            if isinstance(imgsz, (list, tuple)):
                if len(set(imgsz)) != 1:
                    raise NotImplementedError("RTDETR.predict: only square imgsz is provided")
                imgsz = imgsz[0]
            items = list(source) if isinstance(source, (list, tuple)) else [source]
            ims, paths = [], []
            for i, s in enumerate(items):
                if isinstance(s, np.ndarray):
                    ims.append(np.ascontiguousarray(s))
                    paths.append(f"image{i}.jpg")
                    continue
                if isinstance(s, int) or (isinstance(s, str) and (s.isdigit() or "://" in s)):
                    raise NotImplementedError(f"RTDETR.predict: webcam / stream source {s!r} is not provided by this build")
                p = str(s)
                if p.lower().endswith(_VIDEO):
                    raise NotImplementedError(f"RTDETR.predict: video source {p!r} is not provided by this build")
                import cv2
                im = cv2.imread(p)
                if im is None:
                    raise FileNotFoundError(p)
                ims.append(im)
                paths.append(p)
            for im in ims:
                if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                    raise ValueError(f"RTDETR.predict: expected HxWx3 uint8 BGR images, got {im.dtype} {im.shape}")
            dets = self._det(_lib.PREC_F32).predict(ims, int(imgsz), float(conf)) if ims else []
            out = []
            for im, p, d in zip(ims, paths, dets):
                if classes is not None:
                    d = d[np.isin(d[:, 5].astype(np.int64), np.asarray(classes, np.int64).reshape(-1))]
                out.append(Results(im, p, self.names, d[:max_det]))
            if save and out:
                self._save(out)
            return out

        def predict_tiles(self, frame, tiles, conf=0.25, imgsz=640, rgb=False, max_batch=0):
            """Not part of Ultralytics: the crops [x0, y0, x1, y1] of one frame as network batches (ffp_rtdetr_infer_tiles, tile-local rows),
            per tile the list predict() returns for that crop. rgb: the frame is RGB (sahi's arrays), as if every crop were passed flipped."""
            from ffp_amd import _lib
            if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                raise ValueError(f"RTDETR.predict_tiles: expected an HxWx3 uint8 frame, got {frame.dtype} {frame.shape}")
            rows = self._det(_lib.PREC_F32).infer_tiles(frame, tiles, int(imgsz), float(conf), "local",
                                                        _lib.CHAN_AS_RGB if rgb else _lib.CHAN_AS_BGR, max_batch)
            out = []
            for k, ((x0, y0, x1, y1), d) in enumerate(zip(tiles, rows)):
                crop = frame[y0:y1, x0:x1, ::-1] if rgb else frame[y0:y1, x0:x1]
                out.append([Results(crop, f"image{k}.jpg", self.names, d)])
            return out

        def _save(self, results):
            """save=True: each image with its boxes and 'name score' labels written to runs/detect/predict, predict2, ... (a new directory
            per call, as Ultralytics' increment_path), named after the source file. Drawn with the cv2 shim, so the labels are not
            Ultralytics' Annotator glyphs."""
            import cv2
            base = os.path.join("runs", "detect", "predict")
            d, k = base, 2
            while os.path.exists(d):
                d, k = f"{base}{k}", k + 1
            os.makedirs(d)
            for r in results:
                img = r.orig_img.copy()
                for b in r.boxes.data.numpy():
                    x1, y1, x2, y2 = (int(v) for v in b[:4])
                    cv2.rectangle(img, (x1, y1), (x2, y2), (0, 255, 0), 2)
                    cv2.putText(img, f"{self.names.get(int(b[5]), int(b[5]))} {b[4]:.2f}", (x1, max(y1 - 4, 10)), cv2.FONT_HERSHEY_SIMPLEX, 0.5,
                                (0, 255, 0), 1)
                cv2.imwrite(os.path.join(d, os.path.basename(r.path)), img)
            self.save_dir = d

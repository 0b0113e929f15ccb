"""Drop-in for the part of pyiqa (0.1.x) that pipeline_v4_yolo/1_Inference.py uses: `pyiqa.create_metric('niqe', device=...)` and the
call of the metric on a (1, 3, H, W) tensor in [0,1] followed by `.item()` (1_Inference.py:124, :171-176), with NIQE's block features
computed on the GPU through libffp (ffp_iqa_*) and the 36-dimensional distance in float64 on the host. A real pyiqa further down
sys.path always wins: this module then re-exports it untouched (as the cv2 and ultralytics shims do).

Only NIQE is built. BRISQUE needs pyiqa's SVR model file and the 36 feature bounds of its source, which this build neither ships nor
restates; `create_metric('brisque')` raises NotImplementedError, which the reference's `load_iqa_metric` turns into "metric not
available" (1_Inference.py:122-150). The pristine model (pyiqa's niqe_modelparameters.mat) is never fetched: see ffp_amd.iqa.
Parity with pyiqa itself has not been run. `as_loss=True` and gradients are not provided.
"""
import importlib.machinery
import importlib.util
import os
import sys

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _real_pyiqa():
    for p in sys.path:
        if not p or os.path.abspath(p) == _here:
            continue
        spec = importlib.machinery.PathFinder.find_spec("pyiqa", [p])
        if spec is not None and spec.origin and os.path.dirname(os.path.dirname(os.path.abspath(spec.origin))) != _here:
            return spec
    return None


_spec = _real_pyiqa()
if _spec is not None:                                   # pyiqa is installed: be it
    _mod = importlib.util.module_from_spec(_spec)
    sys.modules[__name__] = _mod
    _spec.loader.exec_module(_mod)
else:
    import numpy as np

    __version__ = "0.1-ffp-shim"
    _BLOCK = 96

    def list_models(metric_mode=None, filter="", exclude_filters=""):
        return ["niqe"]

    def _device_index(device):
        s = str(device) if device is not None else ""
        return int(s.split(":", 1)[1]) if ":" in s and s.split(":", 1)[1].isdigit() else 0

    class NIQE:
        """The callable `create_metric('niqe')` returns: image(s) in, a float32 tensor of shape (B,) out, lower is better."""

        metric_name = "niqe"
        lower_better = True
        metric_mode = "NR"

        def __init__(self, device=None, pretrained_model_path=None, as_loss=False, **kwargs):
            if as_loss:
                raise NotImplementedError("as_loss=True needs gradients, which this build does not provide")
            from ffp_amd import iqa
            self.device = device
            self.model_path = iqa.find_niqe_model(pretrained_model_path)
            self.mu, self.cov = iqa.load_niqe_model(self.model_path)
            self._engine = None                          # the GPU is first touched by a call, not by create_metric

        def _iqa(self):
            if self._engine is None:
                from ffp_amd import _lib
                self._engine = _lib.IQA(_device_index(self.device))
            return self._engine

        @staticmethod
        def _check_size(h, w):
            if (h // _BLOCK) * (w // _BLOCK) < 2:
                raise ValueError(f"NIQE needs at least two 96x96 blocks, the image is {h} x {w}")

        def _from_path(self, path):
            from PIL import Image
            with Image.open(path) as im:
                a = np.asarray(im.convert("L" if im.mode in ("L", "1", "I;16", "I", "F") else "RGB"))
            return [np.ascontiguousarray(a)]

        def __call__(self, target, ref=None, **kwargs):
            import torch
            from ffp_amd import _lib
            out_device = "cpu"
            if isinstance(target, (str, os.PathLike)):
                ims = self._from_path(target)
                for a in ims:
                    self._check_size(a.shape[0], a.shape[1])
                feat, _, off = self._iqa().niqe_features(ims, _lib.CHAN_AS_RGB)
            elif isinstance(target, torch.Tensor):
                t = target.detach()
                if t.ndim == 3:
                    t = t[None]
                if t.ndim != 4 or t.shape[1] not in (1, 3):
                    raise ValueError(f"expected a (B, 1|3, H, W) or (1|3, H, W) tensor, got {tuple(target.shape)}")
                self._check_size(int(t.shape[2]), int(t.shape[3]))
                out_device = t.device
                t = t.to(torch.float32).contiguous()
                if t.is_cuda and t.device.index == self._iqa().device:
                    torch.cuda.synchronize(t.device)
                    step = t.stride(0) * 4
                    feat, _, off = self._iqa().niqe_features_dev([t.data_ptr() + i * step for i in range(t.shape[0])],
                                                                 [tuple(t.shape[1:])] * t.shape[0])
                else:
                    feat, _, off = self._iqa().niqe_features(list(t.cpu().numpy()))
            else:
                a = np.asarray(target)
                if a.ndim == 2:
                    a = a[None, None]
                elif a.ndim == 3:
                    a = (np.moveaxis(a, 2, 0) if a.shape[2] in (1, 3) else a)[None]
                if a.ndim != 4 or a.shape[1] not in (1, 3):
                    raise ValueError(f"expected an (H, W), (H, W, 1|3), (1|3, H, W) or (B, 1|3, H, W) array in [0,1], got {np.shape(target)}")
                self._check_size(a.shape[2], a.shape[3])
                feat, _, off = self._iqa().niqe_features(list(np.ascontiguousarray(a, np.float32)))
            scores = _lib.niqe_score(feat, off, self.mu, self.cov)
            return torch.as_tensor(scores.astype(np.float32)).to(out_device)

        forward = __call__

        def to(self, device):
            return self

        def eval(self):
            return self

    def create_metric(metric_name, as_loss=False, device=None, **kwargs):
        name = str(metric_name).lower()
        if name == "niqe":
            return NIQE(device=device, as_loss=as_loss, **kwargs)
        if name == "brisque":
            raise NotImplementedError(
                "BRISQUE is not built: it needs pyiqa's SVR model file and the 36 feature bounds of pyiqa's source, which this build "
                "neither ships nor restates. Only 'niqe' is available (pyiqa.list_models()).")
        raise NotImplementedError(f"metric '{metric_name}' is not built: only 'niqe' is available (pyiqa.list_models()); BRISQUE, "
                                  "TOPIQ and the others need model files and code this build does not ship.")

"""`pycocotools` stand-in (COCO + COCOeval for iouType 'bbox') with the evaluation on the device (csrc/coco_eval.hip). Like the `cv2`
shim, a real pycocotools further down sys.path always wins: this package then re-exports it untouched."""
import importlib.machinery
import importlib.util
import os
import sys

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _real_pycocotools():
    for p in sys.path:
        if not p or os.path.abspath(p) == _here:
            continue
        spec = importlib.machinery.PathFinder.find_spec("pycocotools", [p])
        if spec is not None and spec.origin and os.path.dirname(os.path.dirname(os.path.abspath(spec.origin))) != _here:
            return spec
    return None


_spec = _real_pycocotools()
if _spec is not None:                                   # pycocotools is installed: be it (its submodules resolve through its __path__)
    _mod = importlib.util.module_from_spec(_spec)
    sys.modules[__name__] = _mod
    _spec.loader.exec_module(_mod)
else:
    __version__ = "2.0+ffp"

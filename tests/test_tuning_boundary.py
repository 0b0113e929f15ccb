"""CPU: the literal import block of the reference's utils/tuning_sahi.py (lines 1-12) resolves against the compat shims, and
sahi.AutoDetectionModel maps the reference's model types the way sahi does (unknown types raise)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TUNING_SAHI_IMPORTS = """
import os
import json
import itertools
import io
from contextlib import redirect_stdout
from tqdm import tqdm

# Library SAHI & COCO
from sahi import AutoDetectionModel
from sahi.predict import get_sliced_prediction
from pycocotools.coco import COCO
from pycocotools.cocoeval import COCOeval
"""


def test_literal_import_block_resolves():
    code = ("import sys; sys.path.insert(0, %r)\nimport ffp_amd\nfrom ffp_amd import compat\ncompat.install()\n" % ROOT) + TUNING_SAHI_IMPORTS + (
        "\nimport pycocotools, sahi, utils.tuning_sahi as T\n"
        "assert pycocotools.__file__.startswith(compat.install()) and callable(AutoDetectionModel.from_pretrained)\n"
        "assert callable(T.evaluate_grid) and callable(T.evaluate_sahi) and callable(T.main)\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_auto_detection_model_unknown_type_raises():
    import pytest
    import ffp_amd  # noqa: F401
    from ffp_amd import compat
    compat.install()
    from sahi import AutoDetectionModel
    with pytest.raises(ValueError, match="not supported"):
        AutoDetectionModel.from_pretrained(model_type="mmdet", model_path="x")
    with pytest.raises(ValueError):             # a .pt checkpoint is refused by the loader, as for YOLOv11PoseDetectionModel
        AutoDetectionModel.from_pretrained(model_type="yolov8", model_path="best.pt", device="cuda:0")

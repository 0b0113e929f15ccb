"""sahi.AutoDetectionModel(model_type="rtdetr") on the GPU: get_sliced_prediction through the batched hook equals the generic per-slice
path object for object, and equals RTDETRDetector.sliced_predict (the fused call) after casting the Python boxes to float32."""
import numpy as np
import pytest

import rtdetr_tiles_common as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def compat(gpu_lib):
    from ffp_amd import compat as c
    c.install()
    return c


@pytest.fixture(scope="module")
def setup(gpu_lib, compat):
    from ffp_amd import synth
    from sahi import AutoDetectionModel
    frame = T.frame_bgr()
    direct = gpu_lib.RTDETRDetector(synth.rtdetr_l_weights(1), precision=gpu_lib.PREC_F32)
    conf = T.median_conf(direct, frame, T.tiles(gpu_lib))
    model = AutoDetectionModel.from_pretrained(model_type="rtdetr", model_path="synthetic:rtdetr-l", confidence_threshold=conf, image_size=T.IMGSZ)
    assert type(model).__name__ == "RTDetrDetectionModel" and model.num_categories == 1 and model.category_names == ["face"]
    assert model.has_mask is False and model.category_mapping == {"0": "face"}
    return frame, direct, conf, model


def _values(result):
    return [(p.bbox.to_xyxy(), p.score.value, p.category.id, p.category.name) for p in result.object_prediction_list]


@pytest.mark.parametrize("pp", [("NMS", "IOU"), ("GREEDYNMM", "IOS")])
def test_sliced_prediction_paths_agree(gpu_lib, setup, pp):
    from sahi.predict import get_sliced_prediction
    frame, direct, conf, model = setup
    rgb = np.ascontiguousarray(frame[:, :, ::-1])                   # sahi hands RGB arrays
    kw = dict(slice_height=96, slice_width=96, overlap_height_ratio=0.25, overlap_width_ratio=0.25, postprocess_type=pp[0],
              postprocess_match_metric=pp[1], postprocess_match_threshold=0.5, verbose=0)
    batched = _values(get_sliced_prediction(rgb, model, **kw))
    generic = _values(get_sliced_prediction(rgb, model, merge_buffer_length=10 ** 9, **kw))     # forces one perform_inference per slice
    assert len(batched) > 1 and batched == generic                  # boxes, scores and categories as Python values
    # The fused call. The Python boxes are float32 values held as doubles; the shift adds an integer below 2^9 to a value below 2^9, which
    # is exact in double, so rounding the sum to float32 is the device's single float32 addition.
    fused = direct.sliced_predict(frame, 96, 96, 0.25, 0.25, True, T.IMGSZ, conf, pp[0], pp[1], 0.5)
    py = np.array([list(b) + [s, c] for b, s, c, _ in batched], np.float64).astype(np.float32)
    assert py.shape == fused.shape
    bad = np.flatnonzero((py != fused).any(1))
    print(f"{pp}: {len(py)} merged rows, {len(bad)} differ", py[bad[:5]], fused[bad[:5]])
    assert np.array_equal(py, fused)

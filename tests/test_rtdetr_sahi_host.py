"""CPU tests of the sahi model type "rtdetr": the loader's refusal of pickled checkpoints, unknown types, and the conversion of a hand-built
ultralytics.Results into ObjectPredictions (clip against the full shape, invalid boxes dropped, category names, shift) with float boxes."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def compat():
    import ffp_amd.compat as c
    c.install()
    return c


def test_pt_and_unknown_types_raise(compat):
    from sahi import AutoDetectionModel
    with pytest.raises(ValueError, match="from_ultralytics_rtdetr_state_dict"):
        AutoDetectionModel.from_pretrained("rtdetr", model_path="best.pt", load_at_init=True)
    with pytest.raises(ValueError, match="not supported"):
        AutoDetectionModel.from_pretrained(model_type="mmdet", model_path="best.pt")


@pytest.mark.parametrize("nested", [False, True])
def test_conversion_of_hand_built_results(compat, nested):
    import ultralytics
    from sahi import AutoDetectionModel
    model = AutoDetectionModel.from_pretrained("rtdetr", model_path="best.pt", load_at_init=False, category_mapping={"0": "face", "1": "mask"})
    assert model.model is None and model.image_size == 640 and model.has_mask is False
    assert model.category_names == ["face", "mask"] and model.num_categories == 2
    f = lambda v: float(np.float32(v))
    rows = np.array([[10.25, 20.5, 50.75, 60.125, 0.9, 0],          # in range
                     [-3.5, -0.25, 30.1, 40.2, 0.8, 1],             # negative corners, class 1
                     [60.5, 70.5, 130.7, 140.9, 0.7, 0],            # beyond full_shape (h 100, w 120)
                     [-20.0, 10.0, -5.0, 30.0, 0.6, 0],             # x2 < 0: invalid, dropped
                     [40.0, 50.0, 40.0, 70.0, 0.5, 1]], np.float32)  # zero width: invalid, dropped
    model._original_predictions = [ultralytics.Results(np.zeros((96, 96, 3), np.uint8), "image0.jpg", {0: "face", 1: "mask"}, rows)]
    shift, full = [40, 8], [100, 120]
    model.convert_original_predictions(shift_amount=[shift] if nested else shift, full_shape=[full] if nested else full)
    preds = model.object_prediction_list
    assert [p.bbox.to_xyxy() for p in preds] == [[f(10.25), f(20.5), f(50.75), f(60.125)], [0, 0, f(30.1), f(40.2)], [f(60.5), f(70.5), 120, 100]]
    assert all(isinstance(v, float) for v in preds[0].bbox.to_xyxy())            # float boxes, no int truncation
    assert [p.score.value for p in preds] == [f(0.9), f(0.8), f(0.7)]
    assert [(p.category.id, p.category.name) for p in preds] == [(0, "face"), (1, "mask"), (0, "face")]
    assert all(p.bbox.shift_amount == shift for p in preds)
    shifted = [p.get_shifted_object_prediction().bbox.to_xyxy() for p in preds]
    assert shifted == [[f(10.25) + 40, f(20.5) + 8, f(50.75) + 40, f(60.125) + 8], [40, 8, f(30.1) + 40, f(40.2) + 8],
                       [f(60.5) + 40, f(70.5) + 8, 160, 108]]                     # no second clip: 160 > 120, 108 > 100
    model._original_predictions = [ultralytics.Results(np.zeros((96, 96, 3), np.uint8), "image0.jpg", {0: "face"}, np.zeros((0, 6), np.float32))]
    model.convert_original_predictions(shift_amount=shift, full_shape=full)
    assert model.object_prediction_list == []

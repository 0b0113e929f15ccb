"""CPU known answers for tests/coco_eval_ref.py (the numpy restatement of pycocotools' COCO.loadRes + COCOeval 'bbox' that the device
evaluation is checked against), worked by hand; plus the COCO index of compat/pycocotools and the control flow of
compat/utils/tuning_sahi.py with a stub model."""
import json
import os

import numpy as np
import pytest

import coco_eval_ref as R

EPS = np.spacing(1)
THRS = np.linspace(.5, 0.95, 10)


def ds(gts, cats=(1,), imgs=(1,)):
    anns = []
    for n, g in enumerate(gts, 1):
        a = {"id": g.get("id", n), "image_id": g.get("img", imgs[0]), "category_id": g.get("cat", cats[0]), "bbox": g["bbox"],
             "area": g.get("area", g["bbox"][2] * g["bbox"][3]), "iscrowd": g.get("crowd", 0)}
        anns.append(a)
    return {"images": [{"id": i, "file_name": f"{i}.jpg"} for i in imgs], "annotations": anns,
            "categories": [{"id": c, "name": str(c), "supercategory": "s"} for c in cats]}


def det(bbox, score, img=1, cat=1):
    return {"image_id": img, "category_id": cat, "bbox": list(bbox), "score": score}


def test_single_match_iou_between_070_and_075():
    # GT 0,0,10,10; det 0,0,10,13.9 -> IoU 100/139 = 0.719...: a TP at 0.50..0.70, not at 0.75..0.95
    E = R.evaluate(ds([{"bbox": [0, 0, 10, 10]}]), [det([0, 0, 10, 13.9], 0.9)])
    iou = 100 / 139
    assert 0.70 < iou < 0.75
    p = E.eval["precision"][:, :, 0, 0, 2]
    assert np.all(p[:5] == 1 / (1 + EPS)) and 1 / (1 + EPS) != 1.0
    assert np.all(p[5:] == 0)
    assert np.array_equal(E.eval["recall"][:, 0, 0, 2], np.array([1.0] * 5 + [0.0] * 5))
    assert E.stats[0] == np.mean(np.concatenate([np.full(5 * 101, 1 / (1 + EPS)), np.zeros(5 * 101)]))
    assert E.stats[1] == np.mean(np.full(101, 1 / (1 + EPS))) and E.stats[2] == 0.0


def test_crowd_absorbs_detections():
    # one normal GT far away (npig = 1) and a crowd region; three dets inside the crowd are ignored: neither TP nor FP
    d = ds([{"bbox": [500, 500, 10, 10]}, {"bbox": [0, 0, 100, 100], "crowd": 1}])
    res = [det([10, 10, 20, 20], 0.9), det([40, 40, 20, 20], 0.8), det([70, 10, 20, 20], 0.7), det([500, 500, 10, 10], 0.5)]
    E = R.evaluate(d, res)
    e = E.evalImgs[0]
    assert np.all(e["dtIgnore"][:, :3]) and not np.any(e["dtIgnore"][:, 3])
    assert np.all(e["dtMatches"][:, :3] == 2)                # all matched to the crowd (id 2)
    assert np.all(E.eval["precision"][:, :, 0, 0, 2] == 1 / (1 + EPS))


def test_area_range_ignores():
    # GT area 400 (small); det matches it. 'medium' range: GT ignored -> npig 0 -> -1; an unmatched det outside the range is ignored
    d = ds([{"bbox": [0, 0, 20, 20]}, {"bbox": [300, 300, 50, 50]}])
    E = R.evaluate(d, [det([0, 0, 20, 20], 0.9), det([600, 600, 5, 5], 0.8)])
    e_small = E.evalImgs[1]                                   # (cat, area=small, img)
    assert list(e_small["gtIgnore"]) == [0, 1]
    assert not e_small["dtIgnore"][0, 1]                      # 25 px^2 det is 'small': an FP there
    e_med = E.evalImgs[2]
    assert list(e_med["gtIds"]) == [2, 1]                     # ignored (small) GT sorted last
    assert e_med["dtIgnore"][0, 0] and e_med["dtIgnore"][0, 1]   # matched to an ignored GT / unmatched and outside the range
    assert np.all(E.eval["recall"][:, 0, 2, 2] == 0)         # medium: one GT, no TP
    assert np.all(E.eval["recall"][:, 0, 3, 2] == -1)        # large: no GT -> -1


def test_equal_iou_tie_goes_to_later_gt():
    d = ds([{"bbox": [0, 0, 10, 10]}, {"bbox": [0, 0, 10, 10]}])
    E = R.evaluate(d, [det([0, 0, 10, 10], 0.9)])
    assert np.all(E.evalImgs[0]["dtMatches"] == 2)
    assert np.all(E.evalImgs[0]["gtMatches"][:, 0] == 0) and np.all(E.evalImgs[0]["gtMatches"][:, 1] == 1)


def test_equal_scores_keep_input_order():
    d = ds([{"bbox": [0, 0, 10, 10]}])
    E = R.evaluate(d, [det([50, 50, 10, 10], 0.5), det([0, 0, 10, 10], 0.5)])
    e = E.evalImgs[0]
    assert e["dtIds"] == [1, 2]
    assert np.all(e["dtMatches"][:, 0] == 0) and np.all(e["dtMatches"][:, 1] == 1)
    # FP first then TP: precision at recall 1 is 1 / (2 + eps)
    assert np.all(E.eval["precision"][0, :, 0, 0, 2] == 1 / (2 + EPS))


def test_max_dets_cuts():
    d = ds([{"bbox": [0, 0, 10, 10]}, {"bbox": [100, 0, 10, 10]}])
    res = [det([0, 0, 10, 10], 0.9), det([100, 0, 10, 10], 0.8)] + [det([300 + 20 * i, 300, 10, 10], 0.5) for i in range(120)]
    E = R.evaluate(d, res)
    r = E.eval["recall"][0, 0, 0]
    assert list(r) == [0.5, 1.0, 1.0]
    assert len(E.evalImgs[0]["dtIds"]) == 100
    assert E.eval["precision"][0, 100, 0, 0, 0] == 0 and E.eval["precision"][0, 100, 0, 0, 1] == 2 / (2 + EPS)


def test_image_with_dets_and_no_gts_counts_fps():
    d = ds([{"bbox": [0, 0, 10, 10], "img": 1}], imgs=(1, 2))
    E = R.evaluate(d, [det([0, 0, 10, 10], 0.5, img=1), det([0, 0, 10, 10], 0.9, img=2)])
    assert E.evalImgs[1] is not None and len(E.evalImgs[1]["gtIds"]) == 0
    assert np.all(E.eval["precision"][0, :, 0, 0, 2] == 1 / (2 + EPS))


def test_category_without_gts_is_minus_one():
    d = ds([{"bbox": [0, 0, 10, 10], "cat": 1}], cats=(1, 2))
    E = R.evaluate(d, [det([0, 0, 10, 10], 0.9, cat=1), det([0, 0, 10, 10], 0.9, cat=2)])
    assert np.all(E.eval["precision"][:, :, 1] == -1) and np.all(E.eval["recall"][:, 1] == -1)
    assert np.all(E.eval["precision"][:, :, 0, 0, 2] >= 0)


def test_gt_with_id_zero_never_counts_as_tp():
    d = ds([{"bbox": [0, 0, 10, 10], "id": 0}])
    E = R.evaluate(d, [det([0, 0, 10, 10], 0.9)])
    e = E.evalImgs[0]
    assert np.all(e["dtMatches"] == 0) and np.all(e["gtMatches"] == 1)     # matched, but dtm stores the GT id 0
    assert np.all(E.eval["recall"][:, 0, 0, 2] == 0) and np.all(E.eval["precision"][:, :, 0, 0, 2] == 0)


def test_load_res_fields():
    gt = R.COCO(ds([{"bbox": [0, 0, 10, 10]}], imgs=(1, 2)))
    dt = gt.loadRes([det([1, 2, 3, 4], 0.5), det([0, 0, 2.5, 2], 0.7, img=2)])
    a = dt.loadAnns(dt.getAnnIds())
    assert [x["id"] for x in a] == [1, 2] and [x["area"] for x in a] == [12, 5.0] and all(x["iscrowd"] == 0 for x in a)
    assert dt.dataset["categories"] == gt.dataset["categories"] and dt.dataset["categories"] is not gt.dataset["categories"]
    with pytest.raises(AssertionError):
        gt.loadRes([det([0, 0, 1, 1], 0.5, img=9)])
    arr = np.array([[2, 0, 0, 4, 5, 0.25, 1]])
    assert gt.loadRes(arr).anns[1]["area"] == 20.0


def test_shim_coco_index_and_load_res(tmp_path):
    import ffp_amd  # noqa: F401
    from ffp_amd import compat
    compat.install()
    from pycocotools.coco import COCO
    d = ds([{"bbox": [0, 0, 10, 10], "img": 5}, {"bbox": [1, 1, 5, 5], "img": 3, "cat": 2}, {"bbox": [2, 2, 5, 5], "img": 5, "cat": 2, "crowd": 1}],
           cats=(1, 2), imgs=(5, 3))
    p = tmp_path / "gt.json"
    p.write_text(json.dumps(d))
    gt, ref = COCO(str(p)), R.COCO(json.loads(p.read_text()))
    assert gt.getImgIds() == ref.getImgIds() == [5, 3]
    assert gt.getCatIds() == [1, 2] and gt.getCatIds(catNms=["2"]) == [2]
    assert gt.getAnnIds(imgIds=[5]) == [1, 3] and gt.getAnnIds(catIds=2, iscrowd=0) == [2]
    assert gt.getImgIds(catIds=[2]) and sorted(gt.getImgIds(catIds=[2])) == [3, 5]
    assert gt.loadImgs(3)[0]["file_name"] == "3.jpg" and len(gt.imgToAnns[5]) == 2
    res = [det([0, 0, 10, 10], 0.9, img=5), det([1, 1, 5, 5], 0.3, img=3, cat=2)]
    a, b = gt.loadRes(json.loads(json.dumps(res))), ref.loadRes(json.loads(json.dumps(res)))
    assert a.dataset["annotations"] == b.dataset["annotations"]
    rf = tmp_path / "res.json"
    rf.write_text(json.dumps(res))
    assert gt.loadRes(str(rf)).dataset["annotations"] == b.dataset["annotations"]
    from pycocotools.cocoeval import COCOeval
    for t in ("segm", "keypoints"):
        with pytest.raises(NotImplementedError, match="pycocotools"):
            COCOeval(gt, a, t)
    E = COCOeval(gt, a, "bbox")
    E.params.useCats = 0
    with pytest.raises(NotImplementedError, match="pycocotools"):
        E.evaluate()


# ---- tuning_sahi control flow -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def tuning(monkeypatch, tmp_path):
    import ffp_amd  # noqa: F401
    from ffp_amd import compat
    compat.install()
    from utils import tuning_sahi as T
    d = ds([{"bbox": [0, 0, 10, 10], "img": 1}, {"bbox": [20, 20, 10, 10], "img": 2}], imgs=(1, 2, 3), cats=(0,))
    (tmp_path / "gt.json").write_text(json.dumps(d))
    (tmp_path / "imgs").mkdir()
    for i in (1, 2):                      # image 3 is missing on disk
        (tmp_path / "imgs" / f"{i}.jpg").write_bytes(b"x")
    monkeypatch.setattr(T, "VAL_JSON_PATH", str(tmp_path / "gt.json"))
    monkeypatch.setattr(T, "VAL_IMAGES_DIR", str(tmp_path / "imgs"))
    monkeypatch.setattr(T, "COCO", R.COCO)                 # the device COCOeval is tested on the GPU; here: the restatement
    monkeypatch.setattr(T, "COCOeval", R.COCOeval)
    monkeypatch.chdir(tmp_path)
    return T


class _P:
    def __init__(self, xyxy, s):
        from sahi.prediction import ObjectPrediction
        self.o = ObjectPrediction(bbox=xyxy, category_id=0, category_name="face", score=s)


def test_grids():
    import ffp_amd  # noqa: F401
    from ffp_amd import compat
    compat.install()
    from utils import tuning_sahi as T
    import itertools
    n = lambda g: len(list(itertools.product(*g.values())))
    assert (n(T.param_grid_quick), n(T.param_grid_balanced), n(T.param_grid_comprehensive)) == (4, 36, 120)
    assert T.param_grid is T.param_grid_comprehensive
    assert list(T.param_grid_balanced) == ["slice_size", "overlap_ratio", "postprocess_type", "postprocess_match_metric", "postprocess_match_threshold"]


def test_evaluate_sahi_control_flow(tuning, monkeypatch):
    T = tuning
    calls = []

    def fake(path, model, **kw):
        calls.append((os.path.basename(path), kw))
        if path.endswith("2.jpg"):
            raise RuntimeError("decoder failed")              # skipped, like the reference
        class Res:
            object_prediction_list = [_P([0, 0, 10, 10], 0.9).o]
        return Res()

    monkeypatch.setattr(T, "get_sliced_prediction", fake)
    params = {"slice_size": 320, "overlap_ratio": 0.25, "postprocess_type": "NMS", "postprocess_match_metric": "IOS", "postprocess_match_threshold": 0.5}
    out = T.evaluate_sahi(object(), params)
    assert [c[0] for c in calls] == ["1.jpg", "2.jpg"]
    kw = calls[0][1]
    assert kw["slice_height"] == kw["slice_width"] == 320 and kw["postprocess_class_agnostic"] is True and kw["verbose"] == 0
    ref = R.evaluate(json.load(open(T.VAL_JSON_PATH)), [det([0, 0, 10, 10], 0.9, img=1, cat=0)])
    assert out == {"map_50_95": ref.stats[0], "map_50": ref.stats[1], "map_75": ref.stats[2]}
    assert not any(f.startswith("temp_results_") for f in os.listdir("."))
    monkeypatch.setattr(T, "get_sliced_prediction", lambda *a, **k: (_ for _ in ()).throw(RuntimeError()))
    assert T.evaluate_sahi(object(), params) == 0.0           # no results
    monkeypatch.setattr(T, "VAL_JSON_PATH", "/nonexistent.json")
    assert T.evaluate_sahi(object(), params) == 0.0           # unreadable GT

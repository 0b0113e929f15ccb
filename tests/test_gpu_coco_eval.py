"""GPU: pycocotools' COCOeval (bbox) through compat/pycocotools on the device (csrc/coco_eval.hip, ffp_eval_coco_bbox) is bit-identical to
the numpy restatement tests/coco_eval_ref.py — precision / recall / scores, summarize()'s stats and every evalImgs match array — on
seeded datasets with score and IoU ties, crowds, empty images, big units, two categories and non-default params; on a dataset of
WIDER FACE val's size; and on tests/golden/coco_eval_expected.npz. Malformed input is FFP_ERR_ARG."""
import copy
import json
import os

import numpy as np
import pytest

import coco_eval_ref as R

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "coco_eval_expected.npz")


@pytest.fixture(scope="module")
def shim(gpu_lib):
    from ffp_amd import compat
    compat.install()
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    return COCO, COCOeval


def run_device(shim, tmp_path, dataset, results, params=None):
    COCO, COCOeval = shim
    p = tmp_path / "gt.json"
    p.write_text(json.dumps(dataset))
    gt = COCO(str(p))
    E = COCOeval(gt, gt.loadRes(copy.deepcopy(results)), "bbox")
    for k, v in (params or {}).items():
        setattr(E.params, k, v)
    E.evaluate()
    E.accumulate()
    E.summarize()
    return E


def assert_same(dev, ref, eval_imgs=True):
    for k in ("precision", "recall", "scores"):
        a, b = dev.eval[k], ref.eval[k]
        assert a.shape == b.shape and a.dtype == b.dtype == np.float64, k
        bad = np.flatnonzero(a.view(np.int64) != b.view(np.int64))
        assert bad.size == 0, (k, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    assert np.asarray(dev.stats).view(np.int64).tolist() == np.asarray(ref.stats).view(np.int64).tolist()
    if not eval_imgs:
        return
    assert len(dev.evalImgs) == len(ref.evalImgs)
    for n, (a, b) in enumerate(zip(dev.evalImgs, ref.evalImgs)):
        assert (a is None) == (b is None), n
        if a is None:
            continue
        assert a["dtIds"] == b["dtIds"] and a["gtIds"] == b["gtIds"] and a["dtScores"] == b["dtScores"], n
        for k in ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])) and np.asarray(a[k]).shape == np.asarray(b[k]).shape, (n, k)


CASES = {
    "two_cats": (dict(seed=1, n_img=25), None),
    "ties_crowds": (dict(seed=2, n_img=40, max_dt=45, crowd_p=0.2), None),
    "big_units": (dict(seed=3, n_img=5, big_units=True), None),
    "empty_heavy": (dict(seed=4, n_img=30, empty_p=0.6), None),
    "custom_params": (dict(seed=5, n_img=20, max_dt=60), dict(maxDets=[3, 20, 50], areaRng=[[0, 1e10], [0, 900], [900, 5000], [5000, 1e10]],
                                                             iouThrs=np.array([0.6]))),
    "unsorted_maxdets": (dict(seed=6, n_img=15), dict(maxDets=[100, 1, 10])),
}


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(shim, tmp_path, name):
    kw, params = CASES[name]
    d, r = R.random_dataset(**kw)
    ref = R.evaluate(d, r, params)
    dev = run_device(shim, tmp_path, d, r, params)
    if kw.get("big_units"):
        big = max(dev.evalImgs, key=lambda e: -1 if e is None else len(e["gtIds"]))
        assert len(big["gtIds"]) > 500 and len(dev._units["dets"]) > 100
    assert_same(dev, ref)


def test_wider_val_size(shim, tmp_path):
    d, r = R.random_dataset(seed=7, n_img=3226, cats=(0,), max_gt=8, max_dt=14)
    ref = R.evaluate(d, r)
    dev = run_device(shim, tmp_path, d, r)
    assert_same(dev, ref, eval_imgs=False)
    assert dev.stats[0] > 0


def test_golden_file(shim, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_coco_fixtures as M
    fx = np.load(FX)
    for name, kw in M.CASES.items():
        d, r = R.random_dataset(**kw)
        dev = run_device(shim, tmp_path, d, r)
        for k in ("precision", "recall", "scores"):
            assert np.array_equal(dev.eval[k], fx[f"{name}_{k}"]), (name, k)
        assert np.array_equal(np.asarray(dev.stats), fx[f"{name}_stats"]), name


def test_malformed_input_is_arg_error(gpu_lib):
    L = gpu_lib
    dets = np.array([[0, 0, 10, 10, 0.9, 100, 1]], np.float64)
    gts = np.array([[0, 0, 10, 10, 100, 0, 0, 1]], np.float64)
    P = R.Params()
    args = (P.iouThrs, P.recThrs, P.areaRng, P.maxDets)
    ok = L.eval_coco_bbox(dets, [0, 1], gts, [0, 1], 1, 1, *args)
    assert ok["precision"][0, 0, 0, 0, 2] == 1 / (1 + np.spacing(1))
    bad = [
        (dets, [1, 1], gts, [0, 1]),                 # offsets must start at 0
        (dets, [0, 1], gts, [0, -1]),                # decreasing
        (dets[:, [0, 1, 2, 3, 4, 5, 5]] * [1, 1, 1, 1, 1, 1, 0], [0, 1], gts, [0, 1]),   # det id 0
        (np.where(np.arange(7) == 4, np.nan, dets), [0, 1], gts, [0, 1]),              # NaN score
        (dets, [0, 1], gts * [1, 1, 1, 1, 1, 0, 0, 1] + [0, 0, 0, 0, 0, 1, 0, 0], [0, 1]),  # crowd not ignored
    ]
    for d, do, g, go in bad:
        with pytest.raises(L.FfpError) as e:
            L.eval_coco_bbox(d, do, g, go, 1, 1, *args)
        assert e.value.code == 1
    with pytest.raises(L.FfpError):
        L.eval_coco_bbox(dets, [0, 1], gts, [0, 1], 1, 1, P.iouThrs, P.recThrs, P.areaRng, [10, 1, 100])    # maxDets not ascending

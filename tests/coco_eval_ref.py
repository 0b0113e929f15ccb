"""numpy restatement of pycocotools 2.0.x `COCO` (index + loadRes) and `COCOeval` for iouType 'bbox' — the reference the device
evaluation (csrc/coco_eval.hip) is tested against. pycocotools itself is not a dependency, so this follows its loops literally:
cocoeval.py `_prepare` / `computeIoU` / `evaluateImg` / `accumulate` / `summarize`, and maskApi.c `bbIou` for the IoU.
Slow by design (triple Python loop, as the original); it is a checker, not a product path."""
from __future__ import annotations

import copy
import itertools
import json
from collections import defaultdict

import numpy as np


def _is_array_like(obj):
    return hasattr(obj, "__iter__") and hasattr(obj, "__len__")


class COCO:
    def __init__(self, annotation_file=None):
        self.dataset, self.anns, self.cats, self.imgs = dict(), dict(), dict(), dict()
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        if annotation_file is not None:
            if isinstance(annotation_file, dict):
                dataset = annotation_file
            else:
                with open(annotation_file, "r") as f:
                    dataset = json.load(f)
            assert type(dataset) == dict
            self.dataset = dataset
            self.createIndex()

    def createIndex(self):
        anns, cats, imgs = {}, {}, {}
        imgToAnns, catToImgs = defaultdict(list), defaultdict(list)
        for ann in self.dataset.get("annotations", []):
            imgToAnns[ann["image_id"]].append(ann)
            anns[ann["id"]] = ann
        for img in self.dataset.get("images", []):
            imgs[img["id"]] = img
        for cat in self.dataset.get("categories", []):
            cats[cat["id"]] = cat
        if "annotations" in self.dataset and "categories" in self.dataset:
            for ann in self.dataset["annotations"]:
                catToImgs[ann["category_id"]].append(ann["image_id"])
        self.anns, self.imgToAnns, self.catToImgs, self.imgs, self.cats = anns, imgToAnns, catToImgs, imgs, cats

    def getAnnIds(self, imgIds=[], catIds=[], areaRng=[], iscrowd=None):
        imgIds = imgIds if _is_array_like(imgIds) else [imgIds]
        catIds = catIds if _is_array_like(catIds) else [catIds]
        if len(imgIds) == len(catIds) == len(areaRng) == 0:
            anns = self.dataset["annotations"]
        else:
            if len(imgIds) != 0:
                anns = list(itertools.chain.from_iterable(self.imgToAnns[i] for i in imgIds if i in self.imgToAnns))
            else:
                anns = self.dataset["annotations"]
            anns = anns if len(catIds) == 0 else [a for a in anns if a["category_id"] in catIds]
            anns = anns if len(areaRng) == 0 else [a for a in anns if a["area"] > areaRng[0] and a["area"] < areaRng[1]]
        if iscrowd is not None:
            return [a["id"] for a in anns if a["iscrowd"] == iscrowd]
        return [a["id"] for a in anns]

    def getCatIds(self, catNms=[], supNms=[], catIds=[]):
        catNms = catNms if _is_array_like(catNms) else [catNms]
        supNms = supNms if _is_array_like(supNms) else [supNms]
        catIds = catIds if _is_array_like(catIds) else [catIds]
        cats = self.dataset["categories"]
        if not len(catNms) == len(supNms) == len(catIds) == 0:
            cats = cats if len(catNms) == 0 else [c for c in cats if c["name"] in catNms]
            cats = cats if len(supNms) == 0 else [c for c in cats if c["supercategory"] in supNms]
            cats = cats if len(catIds) == 0 else [c for c in cats if c["id"] in catIds]
        return [c["id"] for c in cats]

    def getImgIds(self, imgIds=[], catIds=[]):
        imgIds = imgIds if _is_array_like(imgIds) else [imgIds]
        catIds = catIds if _is_array_like(catIds) else [catIds]
        if len(imgIds) == len(catIds) == 0:
            ids = self.imgs.keys()
        else:
            ids = set(imgIds)
            for i, catId in enumerate(catIds):
                if i == 0 and len(ids) == 0:
                    ids = set(self.catToImgs[catId])
                else:
                    ids &= set(self.catToImgs[catId])
        return list(ids)

    def _load(self, table, ids):
        if _is_array_like(ids):
            return [table[i] for i in ids]
        elif type(ids) == int:
            return [table[ids]]

    def loadAnns(self, ids=[]):
        return self._load(self.anns, ids)

    def loadCats(self, ids=[]):
        return self._load(self.cats, ids)

    def loadImgs(self, ids=[]):
        return self._load(self.imgs, ids)

    def loadRes(self, resFile):
        res = COCO()
        res.dataset["images"] = [img for img in self.dataset["images"]]
        if type(resFile) == str:
            with open(resFile) as f:
                anns = json.load(f)
        elif type(resFile) == np.ndarray:
            assert resFile.shape[1] == 7
            anns = [{"image_id": int(r[0]), "bbox": [r[1], r[2], r[3], r[4]], "score": r[5], "category_id": int(r[6])} for r in resFile]
        else:
            anns = resFile
        assert type(anns) == list, "results in not an array of objects"
        annsImgIds = [a["image_id"] for a in anns]
        assert set(annsImgIds) == (set(annsImgIds) & set(self.getImgIds())), "Results do not correspond to current coco set"
        assert "bbox" in anns[0] and not anns[0]["bbox"] == [], "only bbox results are restated"
        res.dataset["categories"] = copy.deepcopy(self.dataset["categories"])
        for i, ann in enumerate(anns):
            bb = ann["bbox"]
            x1, x2, y1, y2 = [bb[0], bb[0] + bb[2], bb[1], bb[1] + bb[3]]
            if "segmentation" not in ann:
                ann["segmentation"] = [[x1, y1, x1, y2, x2, y2, x2, y1]]
            ann["area"] = bb[2] * bb[3]
            ann["id"] = i + 1
            ann["iscrowd"] = 0
        res.dataset["annotations"] = anns
        res.createIndex()
        return res


class Params:
    def __init__(self, iouType="bbox"):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "small", "medium", "large"]
        self.useCats = 1
        self.iouType = iouType


def bb_iou(d, g, iscrowd):
    """maskApi.c bbIou: d [m][4], g [n][4] xywh -> [m][n]"""
    o = np.zeros((len(d), len(g)))
    for gi, G in enumerate(g):
        ga = G[2] * G[3]
        crowd = bool(iscrowd[gi])
        for di, D in enumerate(d):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[di, gi] = i / u
    return o


class COCOeval:
    def __init__(self, cocoGt=None, cocoDt=None, iouType="bbox"):
        assert iouType == "bbox"
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.evalImgs = defaultdict(list)
        self.eval = {}
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        self.params = Params(iouType)
        self._paramsEval = {}
        self.stats = []
        self.ious = {}
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    def _prepare(self):
        p = self.params
        gts = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        dts = self.cocoDt.loadAnns(self.cocoDt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        for gt in gts:
            gt["ignore"] = gt["ignore"] if "ignore" in gt else 0
            gt["ignore"] = "iscrowd" in gt and gt["iscrowd"]
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for gt in gts:
            self._gts[gt["image_id"], gt["category_id"]].append(gt)
        for dt in dts:
            self._dts[dt["image_id"], dt["category_id"]].append(dt)
        self.evalImgs = defaultdict(list)
        self.eval = {}

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self.params = p
        self._prepare()
        self.ious = {(i, c): self.computeIoU(i, c) for i in p.imgIds for c in p.catIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(i, c, a, maxDet) for c in p.catIds for a in p.areaRng for i in p.imgIds]
        self._paramsEval = copy.deepcopy(self.params)

    def computeIoU(self, imgId, catId):
        p = self.params
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds]
        if len(dt) > p.maxDets[-1]:
            dt = dt[0:p.maxDets[-1]]
        if len(dt) == 0 or len(gt) == 0:
            return []
        return bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], [int(o["iscrowd"]) for o in gt])

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g["_ignore"] = 1 if (g["ignore"] or (g["area"] < aRng[0] or g["area"] > aRng[1])) else 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T, G, D = len(p.iouThrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gtIg = np.array([g["_ignore"] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["area"] < aRng[0] or d["area"] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"image_id": imgId, "category_id": catId, "aRng": aRng, "maxDet": maxDet, "dtIds": [d["id"] for d in dt],
                "gtIds": [g["id"] for g in gt], "dtMatches": dtm, "gtMatches": gtm, "dtScores": [d["score"] for d in dt],
                "gtIgnore": gtIg, "dtIgnore": dtIg}

    def accumulate(self, p=None):
        if p is None:
            p = self.params
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        _pe = self._paramsEval
        setK, setA, setM, setI = set(_pe.catIds), set(map(tuple, _pe.areaRng)), set(_pe.maxDets), set(_pe.imgIds)
        k_list = [n for n, k in enumerate(p.catIds) if k in setK]
        m_list = [m for n, m in enumerate(p.maxDets) if m in setM]
        a_list = [n for n, a in enumerate(map(lambda x: tuple(x), p.areaRng)) if a in setA]
        i_list = [n for n, i in enumerate(p.imgIds) if i in setI]
        I0, A0 = len(_pe.imgIds), len(_pe.areaRng)
        for k, k0 in enumerate(k_list):
            Nk = k0 * A0 * I0
            for a, a0 in enumerate(a_list):
                Na = a0 * I0
                for m, maxDet in enumerate(m_list):
                    E = [self.evalImgs[Nk + Na + i] for i in i_list]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind="mergesort")
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp, fp = np.array(tp), np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q, ss = np.zeros((R,)), np.zeros((R,))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr, q = pr.tolist(), q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, p.recThrs, side="left")
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dtScoresSorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = {"params": p, "counts": [T, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
            p = self.params
            aind = [i for i, a in enumerate(p.areaRngLbl) if a == areaRng]
            mind = [i for i, m in enumerate(p.maxDets) if m == maxDets]
            if ap == 1:
                s = self.eval["precision"]
                if iouThr is not None:
                    s = s[np.where(iouThr == p.iouThrs)[0]]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval["recall"]
                if iouThr is not None:
                    s = s[np.where(iouThr == p.iouThrs)[0]]
                s = s[:, :, aind, mind]
            return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

        if not self.eval:
            raise Exception("Please run accumulate() first")
        md = self.params.maxDets
        stats = np.zeros((12,))
        stats[0] = _summarize(1)
        stats[1] = _summarize(1, iouThr=.5, maxDets=md[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=md[2])
        stats[3] = _summarize(1, areaRng="small", maxDets=md[2])
        stats[4] = _summarize(1, areaRng="medium", maxDets=md[2])
        stats[5] = _summarize(1, areaRng="large", maxDets=md[2])
        stats[6] = _summarize(0, maxDets=md[0])
        stats[7] = _summarize(0, maxDets=md[1])
        stats[8] = _summarize(0, maxDets=md[2])
        stats[9] = _summarize(0, areaRng="small", maxDets=md[2])
        stats[10] = _summarize(0, areaRng="medium", maxDets=md[2])
        stats[11] = _summarize(0, areaRng="large", maxDets=md[2])
        self.stats = stats


def evaluate(gt_dataset, results, params=None):
    """COCO(gt) + loadRes(results) + evaluate / accumulate / summarize; params: dict of Params attributes to override. -> COCOeval"""
    gt = COCO(copy.deepcopy(gt_dataset))
    dt = gt.loadRes(copy.deepcopy(results))
    E = COCOeval(gt, dt, "bbox")
    for k, v in (params or {}).items():
        setattr(E.params, k, v)
    E.evaluate()
    E.accumulate()
    E.summarize()
    return E


def random_dataset(seed, n_img=20, cats=(1, 2), max_gt=12, max_dt=30, big_units=False, crowd_p=0.05, empty_p=0.15):
    """Seeded COCO-style GT dataset + bbox results with what makes COCOeval subtle: integer boxes (IoU ties), scores on a 0.05 grid
    (score ties), crowds, empty images, GT areas that disagree with the box, unsorted image ids. big_units: one image whose
    category-1 unit holds > 500 GTs and > 100 dets."""
    rng = np.random.default_rng(seed)
    img_ids = [int(x) for x in rng.permutation(np.arange(1, 4 * n_img + 1))[:n_img]]
    images = [{"id": i, "file_name": f"{i}.jpg", "width": 1000, "height": 1000} for i in img_ids]
    anns, res = [], []
    aid = 1
    for n, img in enumerate(img_ids):
        big = big_units and n == 0
        for c in cats:
            if rng.random() < empty_p and not big:
                continue
            ng = 520 if big and c == cats[0] else int(rng.integers(0, max_gt + 1))
            nd = 140 if big and c == cats[0] else int(rng.integers(0, max_dt + 1))
            gts = []
            for _ in range(ng):
                w, h = (int(v) for v in rng.integers(4, 160, 2))
                x, y = (int(v) for v in rng.integers(0, 900, 2))
                area = float(w * h) if rng.random() < 0.85 else float(rng.uniform(10, 20000))
                crowd = int(rng.random() < crowd_p)
                gts.append([x, y, w, h])
                anns.append({"id": aid, "image_id": img, "category_id": c, "bbox": [x, y, w, h], "area": area, "iscrowd": crowd})
                aid += 1
            for _ in range(nd):
                if gts and rng.random() < 0.7:
                    x, y, w, h = gts[int(rng.integers(len(gts)))]
                    j = rng.integers(-6, 7, 4) * (rng.random() < 0.7)
                    x, y, w, h = x + int(j[0]), y + int(j[1]), max(1, w + int(j[2])), max(1, h + int(j[3]))
                else:
                    w, h = (int(v) for v in rng.integers(4, 160, 2))
                    x, y = (int(v) for v in rng.integers(0, 900, 2))
                score = float(np.round(rng.integers(1, 21) * 0.05, 2)) if rng.random() < 0.5 else float(rng.uniform(0.01, 1))
                res.append({"image_id": img, "category_id": c, "bbox": [x, y, w, h], "score": score})
    rng.shuffle(res)
    dataset = {"images": images, "annotations": anns, "categories": [{"id": c, "name": f"c{c}", "supercategory": "x"} for c in cats]}
    return dataset, res

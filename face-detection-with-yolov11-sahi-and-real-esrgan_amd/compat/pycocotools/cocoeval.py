"""pycocotools.cocoeval.COCOeval for iouType 'bbox'. `evaluate()` packs the (image, category) units and runs pycocotools' evaluate +
accumulate on the device in one call (ffp_eval_coco_bbox, bit-identical to pycocotools 2.0.x); `accumulate()` publishes the arrays;
`summarize()` is pycocotools' own numpy code. `evalImgs` is materialised from the device's match arrays on first access. There is no
CPU path: without a device, `evaluate()` raises."""
import copy
import datetime

import numpy as np

import ffp_amd  # noqa: F401
from ffp_amd import _lib

_MISSING = "pycocotools is not installed; this build evaluates iouType='bbox' with useCats=1 only ({} needs `pip install pycocotools`)"


class Params:
    def setDetParams(self):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "small", "medium", "large"]
        self.useCats = 1

    def __init__(self, iouType="segm"):
        if iouType in ("segm", "keypoints"):
            raise NotImplementedError(_MISSING.format(f"iouType={iouType!r}"))
        if iouType != "bbox":
            raise Exception("iouType not supported")
        self.setDetParams()
        self.iouType = iouType
        self.useSegm = None


class COCOeval:
    def __init__(self, cocoGt=None, cocoDt=None, iouType="segm"):
        if not iouType:
            print("iouType not specified. use default iouType segm")
        self.cocoGt = cocoGt
        self.cocoDt = cocoDt
        self._evalImgs = None
        self.eval = {}
        self.params = Params(iouType=iouType)
        self._paramsEval = {}
        self.stats = []
        self._units = None
        self._out = None
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    # ---- evaluate ---------------------------------------------------------------------------------------------------------------
    def _prepare(self):
        """_prepare + the unit layout of ffp_eval_coco_bbox: units (category-major, images sorted), dets in loadRes order and GTs in
        annotation order per unit."""
        p = self.params
        gts = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        dts = self.cocoDt.loadAnns(self.cocoDt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        for gt in gts:
            gt["ignore"] = gt["ignore"] if "ignore" in gt else 0
            gt["ignore"] = "iscrowd" in gt and gt["iscrowd"]
        ui = {i: n for n, i in enumerate(p.imgIds)}
        uc = {c: n for n, c in enumerate(p.catIds)}
        I, K = len(p.imgIds), len(p.catIds)
        g_unit = np.array([uc[g["category_id"]] * I + ui[g["image_id"]] for g in gts], np.int64)
        d_unit = np.array([uc[d["category_id"]] * I + ui[d["image_id"]] for d in dts], np.int64)
        g_rows = np.array([[*g["bbox"], g["area"], int(g["iscrowd"]), 1 if g["ignore"] else 0, g["id"]] for g in gts], np.float64).reshape(-1, 8)
        d_rows = np.array([[*d["bbox"], d["score"], d["area"], d["id"]] for d in dts], np.float64).reshape(-1, 7)
        go, do = np.argsort(g_unit, kind="stable"), np.argsort(d_unit, kind="stable")
        g_off, d_off = np.zeros(I * K + 1, np.int64), np.zeros(I * K + 1, np.int64)
        np.cumsum(np.bincount(g_unit, minlength=I * K), out=g_off[1:])
        np.cumsum(np.bincount(d_unit, minlength=I * K), out=d_off[1:])
        self._units = dict(I=I, K=K, gts=g_rows[go], dets=d_rows[do], g_off=g_off, d_off=d_off)

    def _run(self, matches):
        p, u = self.params, self._units
        return _lib.eval_coco_bbox(u["dets"], u["d_off"], u["gts"], u["g_off"], u["I"], u["K"], p.iouThrs, p.recThrs, p.areaRng,
                                   p.maxDets, matches=matches)

    def evaluate(self):
        p = self.params
        if not p.useCats:
            raise NotImplementedError(_MISSING.format("useCats=0"))
        if p.iouType != "bbox":
            raise NotImplementedError(_MISSING.format(f"iouType={p.iouType!r}"))
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self.params = p
        self._prepare()
        self._evalImgs = None
        self.eval = {}
        self._out = self._run(False)
        self._paramsEval = copy.deepcopy(self.params)

    @property
    def evalImgs(self):
        """pycocotools' per (category, area range, image) list of dicts (None for a unit without GTs and dets), built on first access."""
        if self._evalImgs is None and self._units is not None:
            self._evalImgs = self._materialize()
        return self._evalImgs

    @evalImgs.setter
    def evalImgs(self, value):
        self._evalImgs = value

    def _materialize(self):
        p, u = self._paramsEval, self._units
        o = self._run(True)
        I, K, d_off, g_off, cut = u["I"], u["K"], u["d_off"], u["g_off"], o["cut_off"]
        maxDet = p.maxDets[-1]
        out = []
        for k, catId in enumerate(p.catIds):
            for a, aRng in enumerate(p.areaRng):
                for i, imgId in enumerate(p.imgIds):
                    n = k * I + i
                    D, G = d_off[n + 1] - d_off[n], g_off[n + 1] - g_off[n]
                    if D == 0 and G == 0:
                        out.append(None)
                        continue
                    dets, gts = u["dets"][d_off[n]:d_off[n + 1]], u["gts"][g_off[n]:g_off[n + 1]]
                    dt = np.argsort(-dets[:, 4], kind="mergesort")[0:maxDet]
                    ig = (gts[:, 6] != 0) | (gts[:, 4] < aRng[0]) | (gts[:, 4] > aRng[1])
                    gt = np.argsort(ig.astype(np.int64), kind="mergesort")
                    c0, c1 = cut[n], cut[n + 1]
                    out.append({"image_id": imgId, "category_id": catId, "aRng": aRng, "maxDet": maxDet,
                                "dtIds": [int(x) for x in dets[dt, 6]], "gtIds": [int(x) for x in gts[gt, 7]],
                                "dtMatches": o["dt_matches"][a, :, c0:c1].copy(), "gtMatches": o["gt_matches"][a, :, g_off[n]:g_off[n + 1]].copy(),
                                "dtScores": [float(x) for x in dets[dt, 4]], "gtIgnore": o["gt_ignore"][a, g_off[n]:g_off[n + 1]].astype(np.int64),
                                "dtIgnore": o["dt_ignore"][a, :, c0:c1].astype(bool)})
        return out

    # ---- accumulate / summarize -------------------------------------------------------------------------------------------------
    def accumulate(self, p=None):
        print("Accumulating evaluation results...")
        if self._out is None:
            print("Please run evaluate() first")
        p = self.params if p is None else p
        T, R, K, A, M = (len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets))
        self.eval = {"params": p, "counts": [T, R, K, A, M], "date": datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S"),
                     "precision": self._out["precision"], "recall": self._out["recall"], "scores": self._out["scores"]}

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
            p = self.params
            iStr = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
            titleStr = "Average Precision" if ap == 1 else "Average Recall"
            typeStr = "(AP)" if ap == 1 else "(AR)"
            iouStr = "{:0.2f}:{:0.2f}".format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval["precision"]
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval["recall"]
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            print(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
            return mean_s

        def _summarizeDets():
            stats = np.zeros((12,))
            stats[0] = _summarize(1)
            stats[1] = _summarize(1, iouThr=.5, maxDets=self.params.maxDets[2])
            stats[2] = _summarize(1, iouThr=.75, maxDets=self.params.maxDets[2])
            stats[3] = _summarize(1, areaRng="small", maxDets=self.params.maxDets[2])
            stats[4] = _summarize(1, areaRng="medium", maxDets=self.params.maxDets[2])
            stats[5] = _summarize(1, areaRng="large", maxDets=self.params.maxDets[2])
            stats[6] = _summarize(0, maxDets=self.params.maxDets[0])
            stats[7] = _summarize(0, maxDets=self.params.maxDets[1])
            stats[8] = _summarize(0, maxDets=self.params.maxDets[2])
            stats[9] = _summarize(0, areaRng="small", maxDets=self.params.maxDets[2])
            stats[10] = _summarize(0, areaRng="medium", maxDets=self.params.maxDets[2])
            stats[11] = _summarize(0, areaRng="large", maxDets=self.params.maxDets[2])
            return stats

        if not self.eval:
            raise Exception("Please run accumulate() first")
        self.stats = _summarizeDets()

    def __str__(self):
        self.summarize()

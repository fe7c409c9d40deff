"""The score families of inference.evaluate, one scorer each.  A scorer is built from its keyword's value (which it checks),
`update(batch)` scores one batch, and `result(images)` gives its keys in order once the run is over.  Surface, instances, curves and
detection sum on the device and copy once, in result(); only the confusion matrices are copied per batch."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import consistency, metrics


class Batch(NamedTuple):
    """What one forward of evaluate hands every scorer.  scored: fp32 [B,C,H,W], the main head's logits on the plain path
    (from_logits), probabilities under tta and tiled; masked: what the mask-level scores look at -- the one-hot maps of the cleaned
    arg-max where a clean-up chain is given, else `scored`; labels [B,H,W]; heads: the raw heads of the plain forward, else None."""
    scored: torch.Tensor
    from_logits: bool
    masked: torch.Tensor
    labels: torch.Tensor
    heads: Optional[Tuple[torch.Tensor, ...]]


def _keywords(value, allowed, what: str, listed: Optional[str] = None) -> dict:
    """The keywords of a family's argument (True: the defaults)."""
    if value is True:
        return {}
    if not isinstance(value, dict) or set(value) - set(allowed):
        raise TypeError(f"evaluate: {what} is True or a dict with the keywords " + (listed or ", ".join(allowed)))
    return dict(value)


def _label_keywords(kw) -> dict:
    return {k: kw[k] for k in ("min_area", "connectivity", "max_instances") if k in kw}


def _split(pred, maps, lab: Dict, split):
    """The prediction's defects, cut by split.split_instances where evaluate(split=) asks for it (the pieces keep the labelling's
    connectivity, min_area and rows); `pred` itself without."""
    if split is None:
        return pred
    from .split import split_instances
    return split_instances(pred, maps=maps, connectivity=lab.get("connectivity", 8), min_area=lab.get("min_area", 1), **split).instances


class ConfusionScorer:
    """The score table of notebook cell 25: mIoU, mDice and pixel accuracy of the scored maps' arg-max computed image by image
    (utilities/metrics.py conventions) and averaged over the images, in percent, and "images", their number."""

    def __init__(self):
        self.miou, self.mdice, self.acc = [], [], []

    def _add(self, maps, labels):
        for cm in metrics.seg_confusion_per_image(maps, labels).cpu().numpy():
            m = metrics.metrics_from_confusion(cm)
            self.miou.append(m["miou"]); self.mdice.append(m["mdice"]); self.acc.append(m["acc"])

    def update(self, batch: Batch) -> None:
        self._add(batch.scored, batch.labels)

    @property
    def images(self) -> int:
        return len(self.acc)

    def result(self, images: int) -> Dict:
        return {"mIoU(%)": float(np.mean(self.miou) * 100), "mDice(%)": float(np.mean(self.mdice) * 100),
                "Accuracy(%)": float(np.mean(self.acc) * 100), "images": images}


class CleanScorer(ConfusionScorer):
    """With a clean-up chain (cleanup=, components= or both): "mIoU_clean(%)" and "mDice_clean(%)", the same per-image rule on the
    cleaned mask."""

    def update(self, batch: Batch) -> None:
        self._add(batch.masked, batch.labels)

    def result(self, images: int) -> Dict:
        return {"mIoU_clean(%)": float(np.mean(self.miou) * 100), "mDice_clean(%)": float(np.mean(self.mdice) * 100)}


class SurfaceScorer:
    """surface=True, or a dict with the keywords percentile, tolerance and classes: the boundary metrics of
    surface.surface_distances on the masked maps -- "HD95(px)" and "ASSD(px)" (and "NSD(%)" with a tolerance), the means over the valid
    (image, class) pairs of the whole run (classes: default 1 .. C-1), and "surface_pairs", their number."""

    def __init__(self, surface):
        self.kw = _keywords(surface, ("percentile", "tolerance", "classes"), "surface", "percentile, tolerance and classes")
        self.sums = []                                       # per batch float64 [4] on the device: the sums of hd95, assd, nsd; the pairs

    def update(self, batch: Batch) -> None:
        from .surface import surface_distances
        kw, Cn = self.kw, batch.masked.shape[1]
        r = surface_distances(batch.masked.float(), batch.labels, Cn, percentile=kw.get("percentile", 95.0), tolerance=kw.get("tolerance"))
        classes = list(range(1, Cn)) if kw.get("classes") is None else [int(c) for c in kw["classes"]]
        ok = r.valid[:, classes]
        total = lambda v: torch.where(ok, v[:, classes], torch.zeros_like(v[:, classes])).sum()
        nsd = total(r.nsd) if r.tolerance is not None else torch.zeros((), dtype=torch.float64, device=ok.device)
        self.sums.append(torch.stack([total(r.hd95), total(r.assd), nsd, ok.sum().to(torch.float64)]))

    def result(self, images: int) -> Dict:
        tot = torch.stack(self.sums).sum(dim=0).cpu().tolist() if self.sums else [0.0] * 4
        pairs = int(tot[3])
        mean = lambda v: v / pairs if pairs else float("nan")
        out = {"HD95(px)": mean(tot[0]), "ASSD(px)": mean(tot[1])}
        if self.kw.get("tolerance") is not None:
            out["NSD(%)"] = mean(tot[2]) * 100
        out["surface_pairs"] = pairs
        return out


class InstanceScorer:
    """instances=True, or a dict with the keywords iou_threshold, min_area, connectivity, max_instances and classes: the defects of
    the masked maps' arg-max are matched against the defects of the labels (instances.label_instances on both,
    matching.match_instances) and the per-defect scores are added -- "PQ(%)", "SQ(%)", "RQ(%)", "DefectPrecision(%)",
    "DefectRecall(%)", "PRO(%)" (the overall values of matching.summarize over the chosen classes, default 1 .. C-1), "defects_gt",
    "defects_pred" and "instance_images_skipped" (images with more defects than max_instances on either side are left out)."""
    KEYS = ("classes", "connectivity", "iou_threshold", "max_instances", "min_area")

    def __init__(self, instances, split=None):
        self.kw = _keywords(instances, self.KEYS, "instances")
        self.split = split                                   # split.split_instances keywords: the prediction's defects are cut first
        self.sums = []                                       # per batch matching.MatchResult.sums: float64 [K,7] on the device

    def update(self, batch: Batch) -> None:
        from .instances import label_instances
        from .matching import match_instances
        lab = _label_keywords(self.kw)
        pred = _split(label_instances(torch.argmax(batch.masked, dim=1), **lab), (), lab, self.split)
        target = label_instances(batch.labels.to(torch.int64), **lab)
        match = match_instances(pred, target, batch.masked.shape[1], iou_threshold=self.kw.get("iou_threshold", 0.5))
        self.sums.append(match.sums(self.kw.get("classes")))

    def result(self, images: int) -> Dict:
        from .matching import SUM_COLUMNS, summarize
        classes = self.kw.get("classes")
        classes = list(range(1, (self.sums[0].shape[0] if self.sums else 0) + 1)) if classes is None else [int(c) for c in classes]
        tot = torch.stack(self.sums).sum(dim=0).cpu().numpy() if self.sums else np.zeros((len(classes), len(SUM_COLUMNS)))
        s = summarize(tot, classes, images)
        out = {key: s[name] * 100 for key, name in (("PQ(%)", "PQ"), ("SQ(%)", "SQ"), ("RQ(%)", "RQ"), ("DefectPrecision(%)", "precision"),
                                                    ("DefectRecall(%)", "recall"), ("PRO(%)", "PRO"))}
        out["defects_gt"], out["defects_pred"], out["instance_images_skipped"] = s["n_gt"], s["n_pred"], s["images_skipped"]
        return out


class DetectionScorer:
    """detection=True, or a dict with the keywords iou_thresholds, min_area, connectivity, max_instances, classes and max_dets: the
    defects of the masked maps' arg-max, each scored by its mean confidence (the largest class probability of the scored maps, after a
    softmax where they are logits; label_instances(mask, maps=(confidence,))), are assigned to the defects of the labels at every IoU
    threshold (detection.detection_match; default COCO's 0.50 .. 0.95) -- "mAP(%)" (the mean AP over thresholds and classes, default
    1 .. C-1), "AP50(%)" and "AP75(%)" (NaN where that threshold is not in the sweep), "DefectAR(%)" (the recall left at the end of the
    list) and "detection_images_skipped" (images with more defects than max_instances on either side are left out)."""
    KEYS = ("classes", "connectivity", "iou_thresholds", "max_dets", "max_instances", "min_area")

    def __init__(self, detection, split=None):
        from .detection import COCO_THRESHOLDS, per_mille
        self.kw = _keywords(detection, self.KEYS, "detection")
        self.split = split
        self.thresholds = tuple(k / 1000.0 for k in per_mille(self.kw.get("iou_thresholds", COCO_THRESHOLDS)))
        self.parts, self.num_classes = [], 0                 # per batch detection.DetectionSums on the device

    def update(self, batch: Batch) -> None:
        from .detection import detection_match
        from .instances import label_instances
        lab = _label_keywords(self.kw)
        probs = torch.softmax(batch.scored.float(), dim=1) if batch.from_logits else batch.scored.float()
        conf = probs.amax(dim=1).contiguous()
        pred = _split(label_instances(torch.argmax(batch.masked, dim=1), maps=(conf,), **lab), (conf,), lab, self.split)
        target = label_instances(batch.labels.to(torch.int64), **lab)
        self.num_classes = batch.masked.shape[1]
        res = detection_match(pred, target, self.num_classes, iou_thresholds=self.thresholds, max_dets=self.kw.get("max_dets"))
        self.parts.append(res.sums(self.kw.get("classes")))

    def result(self, images: int) -> Dict:
        from .detection import summarize
        classes = self.kw.get("classes")
        classes = list(range(1, self.num_classes)) if classes is None else [int(c) for c in classes]
        s = summarize(self.parts, classes, self.thresholds, images)
        nan = float("nan")
        return {"mAP(%)": s["mAP"] * 100, "AP50(%)": s.get("AP50", nan) * 100, "AP75(%)": s.get("AP75", nan) * 100,
                "DefectAR(%)": s["AR"] * 100, "detection_images_skipped": s["images_skipped"]}


class CurveScorer:
    """curves=True, or a dict (an empty one: the defaults) with the keywords bins, fpr_limit, ece_bins, classes, max_instances,
    connectivity, min_area, uncertainty, lo and hi: the threshold-sweep scores of curves.score_curves on the scored maps (they score
    maps, not masks: a clean-up chain does not change them; the logits of the plain path go through the kernel's softmax, under tta
    and tiled the maps are probabilities already) -- "AUROC(%)", "AP(%)", "AUPRO(%)" (up to fpr_limit, default 0.3, over the defects
    of the labels), "ECE(%)" (ece_bins groups, default 16) and "curve_images_skipped" (images with more real defects than
    max_instances are left out).  uncertainty=True (plain path only, a model with an auxiliary head) adds "UncAUROC(%)" and "AURC":
    how well consistency.uncertainty_map(main, aux1), binned over [lo, hi] (default 0, 1), marks the wrong pixels of the main head."""
    KEYS = ("bins", "classes", "connectivity", "ece_bins", "fpr_limit", "hi", "lo", "max_instances", "min_area", "uncertainty")

    def __init__(self, curves, plain_path: bool):
        self.kw = _keywords(curves, self.KEYS, "curves")
        if self.kw.get("uncertainty") and not plain_path:
            raise ValueError("evaluate: curves with uncertainty=True scores the plain forward's uncertainty map: not built under tta or tiled")
        self.sums = self.unc_sums = None                     # curves.CurveSums on the device, added up batch by batch

    def update(self, batch: Batch) -> None:
        from .curves import plane_curves, score_curves
        from .instances import label_instances
        kw, y = self.kw, batch.labels
        if kw.get("uncertainty"):
            if len(batch.heads) < 2:
                raise ValueError("evaluate: curves with uncertainty=True needs a model with an auxiliary head")
            unc = consistency.uncertainty_map(batch.heads[0], batch.heads[1])
            part = plane_curves(unc.float(), torch.argmax(batch.heads[0], dim=1), y, bins=kw.get("bins", 1024), lo=kw.get("lo", 0.0),
                                hi=kw.get("hi", 1.0)).sums()
            self.unc_sums = part if self.unc_sums is None else self.unc_sums + part
        regions = label_instances(y.to(torch.int64), **_label_keywords(kw))
        part = score_curves(batch.scored.float(), y, classes=kw.get("classes"), bins=kw.get("bins", 1024), top=True,
                            from_logits=batch.from_logits, regions=regions, want_sums=True).sums()
        self.sums = part if self.sums is None else self.sums + part

    def result(self, images: int) -> Dict:
        from .curves import summarize
        kw, nan = self.kw, float("nan")
        s = {"AUROC": nan, "AP": nan, "AUPRO": nan, "ECE": nan, "images_skipped": 0}
        if self.sums is not None:
            classes = kw.get("classes")                      # (the sums hold the class rows and the top row)
            classes = list(range(1, self.sums.hist.shape[0])) if classes is None else [int(c) for c in classes]
            s = summarize(self.sums, classes, fpr_limit=kw.get("fpr_limit", 0.3), ece_bins=kw.get("ece_bins", 16))
        out = {key + "(%)": s[key] * 100 for key in ("AUROC", "AP", "AUPRO", "ECE")}
        out["curve_images_skipped"] = s["images_skipped"]
        if kw.get("uncertainty"):
            u = {"AUROC": nan, "AURC": nan}
            if self.unc_sums is not None:
                u = summarize(self.unc_sums, (), lo=kw.get("lo", 0.0), hi=kw.get("hi", 1.0), plane=True)
            out["UncAUROC(%)"], out["AURC"] = u["AUROC"] * 100, u["AURC"]
        return out

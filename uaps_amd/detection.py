"""Defect detection scores on the kernels of csrc/detect.hip: average precision of the defect list over a sweep of IoU thresholds.

`detection_match` takes two results of `label_instances` -- the prediction's, whose per-defect confidence sum is the detection score,
and the ground truth's -- and runs COCO's assignment: per image, class and threshold the detections are visited in score order and
each takes the free ground-truth defect of largest IoU among those with IoU >= threshold.  Thresholds are integers per mille from 0.1
to 1.0 and every IoU comparison is made in 64-bit integers, so every table is exact and the same bits from run to run.  Nothing
synchronises with the host; `DetectionResult.sums()` gives what a run accumulates, `summarize` makes the one copy and forms AP50, AP75,
AP@[.50:.95], AR and whatever other thresholds were asked for in float64 on the host.

Against pycocotools: score ties go to the lower label (pycocotools: a stable sort of its input order), the precision's denominator
carries no np.spacing(1), and there are no crowd or ignore regions and no area ranges.

CPU tensors take the numpy restatement below, as in the other modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import check_instance_pair, pair_matrix_np, pair_operands
from .instances import FIXED_ONE, InstanceResult

COCO_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))
MAX_CLASSES = _lib.MATCH_MAX_CLASSES
MAX_THRESHOLDS, MAX_CANDIDATES, MAX_ROWS = _lib.DETECT_MAX_THRESHOLDS, _lib.DETECT_MAX_CANDIDATES, _lib.DETECT_MAX_ROWS
_ws = _lib.Workspace()


def per_mille(iou_thresholds: Sequence[float]) -> Tuple[int, ...]:
    """The thresholds as integers per mille: strictly ascending, 1 <= T <= 32, each within 1e-9 of a step and in [0.1, 1]."""
    try:
        values = [float(t) for t in iou_thresholds]
    except TypeError:
        raise ValueError("detection_match: iou_thresholds is a sequence of numbers") from None
    if not 1 <= len(values) <= MAX_THRESHOLDS:
        raise ValueError(f"detection_match: 1 <= len(iou_thresholds) <= {MAX_THRESHOLDS}")
    out = []
    for t in values:
        if not t == t or abs(t) > 2.0:
            raise ValueError(f"detection_match: IoU threshold {t} lies outside [0.1, 1]")
        k = int(round(1000.0 * t))
        if abs(t - k / 1000.0) > 1e-9:
            raise ValueError(f"detection_match: IoU threshold {t} is not a multiple of 0.001")
        if not 100 <= k <= 1000:
            raise ValueError(f"detection_match: IoU threshold {t} lies outside [0.1, 1]")
        if out and k <= out[-1]:
            raise ValueError("detection_match: iou_thresholds is strictly ascending")
        out.append(k)
    return tuple(out)


class DetectionSums(NamedTuple):
    """What a run accumulates, on the device: rows float64 [N,3] (class or -1, score, the matched bit mask over the thresholds), n_gt
    float64 [K] per chosen class and images float64 [] (the valid ones)."""
    rows: torch.Tensor
    n_gt: torch.Tensor
    images: torch.Tensor


def _average_precision(tp: np.ndarray, n_gt: int) -> Tuple[float, float]:
    """(AP, final recall) of one class and threshold; tp: 0 / 1 per detection in score order."""
    if n_gt <= 0:
        return float("nan"), float("nan")
    if len(tp) == 0:
        return 0.0, 0.0
    ctp = np.cumsum(tp, dtype=np.float64)
    cfp = np.cumsum(1 - tp, dtype=np.float64)
    recall = ctp / float(n_gt)
    precision = np.maximum.accumulate((ctp / (ctp + cfp))[::-1])[::-1]
    at = np.searchsorted(recall, np.linspace(0.0, 1.0, 101), side="left")
    q = np.where(at < len(tp), precision[np.minimum(at, len(tp) - 1)], 0.0)
    return float(q.mean()), float(recall[-1])


def _nanmean(values) -> float:
    vals = [v for v in values if v == v]
    return float(np.mean(vals)) if vals else float("nan")


def summarize(parts: Sequence[DetectionSums], classes: Sequence[int], thresholds: Sequence[float], images_total: int) -> Dict:
    """The score table of the `DetectionResult.sums(classes)` of any number of batches (one device-to-host copy).  Per class and
    threshold the participating detections of all valid images are sorted by score descending (stable: ties keep the order of the
    parts, then image, then label), recall = cumulative tp / n_gt, precision = tp / (tp + fp) made non-increasing from the right, and
    AP is the mean over r in linspace(0, 1, 101) of the precision at the first index with recall >= r (0 where there is none); AR is
    the final recall.  Per class "AP" (the mean over the thresholds), "AP_at" and "AR" (likewise the mean), NaN for a class without a
    ground-truth defect, which is left out of the overall means "mAP", "AP50", "AP75" (where 0.5, 0.75 are among the thresholds) and
    "AR"; "n_gt", "n_pred", "images", "images_skipped"."""
    classes = [int(c) for c in classes]
    t1000 = per_mille(thresholds)
    K, T = len(classes), len(t1000)
    if parts:
        flat = torch.cat([torch.cat([p.rows for p in parts]).reshape(-1), torch.stack([p.n_gt for p in parts]).sum(dim=0).reshape(-1),
                          torch.stack([p.images for p in parts]).sum().reshape(1)]).cpu().numpy()
    else:
        flat = np.zeros(K + 1, dtype=np.float64)
    rows, n_gt, used = flat[:len(flat) - K - 1].reshape(-1, 3), flat[len(flat) - K - 1:-1], int(flat[-1])
    per, n_pred = {}, 0
    for c, gt in zip(classes, n_gt.tolist()):
        sel = rows[:, 0] == c
        order = np.argsort(-rows[sel, 1], kind="stable")
        mask = rows[sel, 2].astype(np.int64)[order]
        n_pred += int(sel.sum())
        both = [_average_precision((mask >> t) & 1, int(gt)) for t in range(T)]
        per[c] = {"AP": _nanmean(v[0] for v in both), "AP_at": [v[0] for v in both], "AR": _nanmean(v[1] for v in both),
                  "n_gt": int(gt), "n_pred": int(sel.sum())}
    out = {"classes": classes, "thresholds": [k / 1000.0 for k in t1000], "per_class": per,
           "mAP": _nanmean(v["AP"] for v in per.values()), "AR": _nanmean(v["AR"] for v in per.values())}
    for name, k in (("AP50", 500), ("AP75", 750)):
        if k in t1000:
            out[name] = _nanmean(v["AP_at"][t1000.index(k)] for v in per.values())
    out["n_gt"], out["n_pred"] = int(n_gt.sum()), n_pred
    out["images"], out["images_skipped"] = used, int(images_total) - used
    return out


class DetectionResult(NamedTuple):
    """score: float64 [B,Mp], the key detections are ordered by (sum0 / area of map 0 -- times 2^-24 it is the mean -- or the caller's
    score; NaN and rows without a defect: -inf); rank: int64 [B,Mp], the position within its (image, class), -1 for rows without a
    defect, of a class outside [0, num_classes) or cut by max_dets; pred_match: int64 [B,Mp,T], the ground-truth number taken at every
    threshold, 0: none (a false positive there); pred_inter: int64 [B,Mp,T], the intersection with it; target_match: int64 [B,Mg,T],
    the detection number, 0: none; counts: int64 [B,num_classes,T+2], tp per threshold, then n_pred taking part, then n_gt; valid:
    bool [B], false where either side has more components than table rows; the thresholds per mille, the flags and the two inputs."""
    score: torch.Tensor
    rank: torch.Tensor
    pred_match: torch.Tensor
    pred_inter: torch.Tensor
    target_match: torch.Tensor
    counts: torch.Tensor
    valid: torch.Tensor
    t1000: Tuple[int, ...]
    class_agnostic: bool
    from_map: bool
    pred_instances: InstanceResult
    target_instances: InstanceResult

    @property
    def iou_thresholds(self) -> Tuple[float, ...]:
        return tuple(k / 1000.0 for k in self.t1000)

    @property
    def num_classes(self) -> int:
        return self.counts.shape[1]

    def iou(self) -> torch.Tensor:
        """float64 [B,Mp,T]: the IoU of every detection with the ground-truth defect it took, 0 where it took none."""
        B, Mp, T = self.pred_match.shape
        area_g = torch.gather(self.target_instances.table[..., 1], 1, (self.pred_match - 1).clamp(min=0).reshape(B, Mp * T)).reshape(B, Mp, T)
        union = (self.pred_instances.table[..., 1][..., None] + area_g - self.pred_inter).clamp(min=1).to(torch.float64)
        return torch.where(self.pred_match > 0, self.pred_inter.to(torch.float64) / union, torch.zeros_like(union))

    def _classes(self, classes) -> List[int]:
        Cn = self.num_classes
        if classes is None:
            return [0] if self.class_agnostic else list(range(1, Cn))
        classes = [int(c) for c in classes]
        if any(c < 0 or c >= Cn for c in classes):
            raise ValueError(f"DetectionResult: classes lie in [0, {Cn})")
        return classes

    def sums(self, classes: Optional[Sequence[int]] = None) -> DetectionSums:
        """What a run accumulates (`summarize` takes a list of these); does not synchronise.  rows: float64 [B * Mp, 3], per table row
        its class -- -1 where it takes no part, is of another class or its image is invalid --, score, and the bit mask of the
        thresholds at which it is a true positive (below 2^32: exact in float64).  classes: default 1 .. num_classes-1 (class_agnostic:
        0, the one class everything is counted as)."""
        classes = self._classes(classes)
        dev, T = self.counts.device, len(self.t1000)
        cl = torch.tensor(classes, dtype=torch.int64, device=dev)
        cls = torch.zeros_like(self.rank) if self.class_agnostic else self.pred_instances.table[..., 0]
        keep = (self.rank >= 0) & self.valid[:, None] & (cls[..., None] == cl).any(dim=-1)
        cls = torch.where(keep, cls, torch.full_like(cls, -1))
        mask = ((self.pred_match > 0).to(torch.int64) << torch.arange(T, device=dev)).sum(dim=-1)
        rows = torch.stack([cls.to(torch.float64), self.score, mask.to(torch.float64)], dim=-1).reshape(-1, 3)
        n_gt = torch.where(self.valid[:, None], self.counts[:, classes, T + 1], torch.zeros_like(self.counts[:, classes, T + 1]))
        return DetectionSums(rows, n_gt.sum(dim=0).to(torch.float64), self.valid.sum().to(torch.float64))

    def summary(self, classes: Optional[Sequence[int]] = None) -> Dict:
        """One device-to-host copy: `summarize` of this result alone."""
        classes = self._classes(classes)
        return summarize([self.sums(classes)], classes, self.iou_thresholds, self.valid.shape[0])

    def records(self) -> List[List[dict]]:
        """One device-to-host copy; per image a dict per in-table detection: label, cls, area, score (the mean of map 0 where the
        score came from it), rank, and per threshold matched (the ground-truth number or 0) and iou."""
        B, Mp, T = self.pred_match.shape
        tab = self.pred_instances.table
        packed = torch.cat([tab[..., :2].reshape(B, -1).to(torch.float64), self.score, self.rank.to(torch.float64),
                            self.pred_match.reshape(B, -1).to(torch.float64), self.iou().reshape(B, -1),
                            self.pred_instances.count.to(torch.float64).reshape(B, 1)], dim=1).cpu().numpy()
        scale = 1.0 / FIXED_ONE if self.from_map else 1.0
        out = []
        for row in packed:
            tb, sc, rk = row[:2 * Mp].reshape(Mp, 2), row[2 * Mp:3 * Mp], row[3 * Mp:4 * Mp]
            pm, iou, n = row[4 * Mp:(4 + T) * Mp].reshape(Mp, T), row[(4 + T) * Mp:(4 + 2 * T) * Mp].reshape(Mp, T), int(row[-1])
            out.append([{"label": k + 1, "cls": int(tb[k, 0]), "area": int(tb[k, 1]), "score": float(sc[k]) * scale, "rank": int(rk[k]),
                         "matched": [int(v) for v in pm[k]], "iou": [float(v) for v in iou[k]]} for k in range(min(n, Mp))])
        return out


# ------------------------------------------------------------------------------------------------ numpy restatement
def _by_iou(a, b) -> int:
    """(g, inter, union) tuples of Python ints: the larger IoU first (cross-multiplied), the lower number on ties."""
    l, r = a[1] * b[2], b[1] * a[2]
    return -1 if l > r else (1 if l < r else a[0] - b[0])


def _detect_cpu(pred: InstanceResult, target: InstanceResult, Cn: int, t1000, agnostic: bool, max_dets, scores):
    tp_, tg_ = pred.table.numpy(), target.table.numpy()
    B, Mp, Mg, T = tp_.shape[0], tp_.shape[1], tg_.shape[1], len(t1000)
    score = np.full((B, Mp), -np.inf, dtype=np.float64)
    rank = np.full((B, Mp), -1, dtype=np.int64)
    pm, pi = np.zeros((B, Mp, T), dtype=np.int64), np.zeros((B, Mp, T), dtype=np.int64)
    tm = np.zeros((B, Mg, T), dtype=np.int64)
    counts = np.zeros((B, Cn, T + 2), dtype=np.int64)
    for b in range(B):
        inter, np_, ng = pair_matrix_np(pred, target, b, agnostic)
        area_p, area_g = tp_[b, :np_, 1], tg_[b, :ng, 1]
        if scores is None:
            with np.errstate(divide="ignore", invalid="ignore"):
                s = tp_[b, :np_, 7].astype(np.float64) / area_p.astype(np.float64)
        else:
            s = scores[b, :np_].astype(np.float64)
        nan = np.isnan(s)
        s = np.where(nan, -np.inf, s + 0.0)
        score[b, :np_] = s
        cls_p = np.zeros(np_, dtype=np.int64) if agnostic else tp_[b, :np_, 0]
        cls_g = np.zeros(ng, dtype=np.int64) if agnostic else tg_[b, :ng, 0]
        for c in range(Cn):
            dets = np.nonzero(cls_p == c)[0]
            order = dets[np.lexsort((dets, -s[dets], nan[dets]))]              # NaN last, score descending, label ascending
            if max_dets is not None:
                order = order[:max_dets]
            counts[b, c, T], counts[b, c, T + 1] = len(order), int((cls_g == c).sum())
            taken = np.zeros((T, ng), dtype=bool)
            for r, d in enumerate(order.tolist()):
                rank[b, d] = r
                gs = np.nonzero(inter[d] > 0)[0]
                i = inter[d, gs]
                u = area_p[d] + area_g[gs] - i
                ok = 1000 * i >= t1000[0] * u
                cand = sorted(zip(gs[ok].tolist(), i[ok].tolist(), u[ok].tolist()), key=functools.cmp_to_key(_by_iou))
                for t, thr in enumerate(t1000):
                    for gg, ii, uu in cand:
                        if 1000 * ii < thr * uu:
                            break
                        if not taken[t, gg]:
                            taken[t, gg] = True
                            pm[b, d, t], pi[b, d, t], tm[b, gg, t] = gg + 1, ii, d + 1
                            counts[b, c, t] += 1
                            break
    return tuple(torch.from_numpy(v) for v in (score, rank, pm, pi, tm, counts))


# ------------------------------------------------------------------------------------------------ public function
def detection_match(pred: InstanceResult, target: InstanceResult, num_classes: int, *, scores: Optional[torch.Tensor] = None,
                    iou_thresholds: Sequence[float] = COCO_THRESHOLDS, class_agnostic: bool = False,
                    max_dets: Optional[int] = None) -> DetectionResult:
    """Assign the defects of `pred` to those of `target`, two results of `label_instances` over the same B, H, W on one device (their
    max_instances, at most 4096, may differ), at every threshold of `iou_thresholds` (per_mille's rules).

    The pair matrix is match_instances': a pixel with prediction number p and ground-truth number g, both with a table row and of one
    class (class_agnostic: of any classes), adds 1 to inter[b, p, g].  IoU(p, g) >= t is 1000 inter >= t1000 (area_p + area_g - inter)
    in integers.  A detection's score is float64(sum0) / float64(area) of map 0 of `pred` (pred.n_maps == 0 is an error), or
    scores[b, p] (float32 or float64 [B, Mp], read as float64); -0 counts as 0, a NaN orders after every number and is reported as
    -inf.  Within an (image, class) -- classes in [0, num_classes); class_agnostic: every defect as class 0 -- detections are ordered
    by score descending, the lower label first on ties, and with max_dets = n only the first n take part.  Per image, class and
    threshold, in that order, a detection takes the free ground-truth defect of largest IoU among those that pass (the lowest number on
    ties) or is a false positive there; a ground-truth defect is taken at most once per threshold.  Does not synchronise."""
    B, H, W, Mp, Mg, Cn, valid = check_instance_pair("detection_match", pred, target, num_classes, MAX_CLASSES)
    t1000 = per_mille(iou_thresholds)
    if max_dets is not None:
        max_dets = int(max_dets)
        if max_dets < 1:
            raise ValueError("detection_match: max_dets is None or at least 1")
        max_dets = min(max_dets, 2 ** 31 - 1)
    T, dev = len(t1000), pred.labels.device
    if scores is None:
        if pred.n_maps < 1:
            raise ValueError("detection_match: pred carries no map (label_instances(mask, maps=(confidence,))) and no scores are given")
    else:
        if not isinstance(scores, torch.Tensor) or scores.dtype not in (torch.float32, torch.float64):
            raise TypeError("detection_match: scores is a float32 or float64 tensor")
        if scores.device != dev or tuple(scores.shape) != (B, Mp):
            raise ValueError(f"detection_match: scores is [{B}, {Mp}] on {dev}")
        scores = scores.to(torch.float64).contiguous()
    if Mp > MAX_ROWS or Mg > MAX_ROWS:
        raise ValueError(f"detection_match: max_instances <= {MAX_ROWS} on both sides")
    agnostic, from_map = bool(class_agnostic), scores is None
    if not pred.labels.is_cuda:
        out = _detect_cpu(pred, target, Cn, t1000, agnostic, max_dets, None if scores is None else scores.numpy())
        return DetectionResult(*out, valid, t1000, agnostic, from_map, pred, target)
    held = pair_operands(pred, target)
    score = torch.empty((B, Mp), dtype=torch.float64, device=dev)
    rank = torch.empty((B, Mp), dtype=torch.int64, device=dev)
    pm = torch.empty((B, Mp, T), dtype=torch.int64, device=dev)
    pi = torch.empty((B, Mp, T), dtype=torch.int64, device=dev)
    tm = torch.empty((B, Mg, T), dtype=torch.int64, device=dev)
    counts = torch.empty((B, Cn, T + 2), dtype=torch.int64, device=dev)
    _lib.call("uaps_detect_match", _lib.DetectCall, dev, _ws, _lib.workspace_bytes("uaps_detect_workspace_bytes", B, Mp, Mg, T),
              B=B, H=H, W=W, num_classes=Cn, class_agnostic=1 if agnostic else 0, T=T, max_dets=max_dets or 0, t1000=list(t1000),
              max_pred=Mp, max_gt=Mg, scores=None if scores is None else scores.data_ptr(), score=score.data_ptr(),
              rank=rank.data_ptr(), pred_match=pm.data_ptr(), pred_inter=pi.data_ptr(), target_match=tm.data_ptr(),
              counts=counts.data_ptr(), **{name: t.data_ptr() for name, t in held.items()})
    return DetectionResult(score, rank, pm, pi, tm, counts, valid, t1000, agnostic, from_map, pred, target)

"""Defect matching against ground truth on the kernels of csrc/match.hip: how many of the real defects were found, and how many of the
reported ones are false alarms.

`match_instances` takes two results of `label_instances` -- the prediction's and the ground truth's -- and gives, per defect of either
side, its partner (the component of the other side it shares the most pixels with), that intersection, the pixels covered by the other
side and whether the pair is matched under the panoptic-quality rule IoU > iou_threshold (strict, 0.5 <= iou_threshold < 1: a match is
then unique on both sides, no assignment step), and per image and class tp, n_pred, n_gt.  Every entry of the three tables is an
integer: exact, and the same bits from run to run.  Nothing synchronises with the host; `MatchResult` forms IoU, PQ / SQ / RQ, defect
precision / recall / F1, per-region overlap (PRO) and purity from the tables in float64 on the device, `summary()` and `records()` are
the device-to-host copies.

CPU tensors take the numpy restatement below, as in the other modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._checks import check_instance_pair, pair_matrix_np, pair_operands
from .instances import InstanceResult

MATCH_COLUMNS = ("partner", "inter", "covered", "matched")
COUNT_COLUMNS = ("tp", "n_pred", "n_gt")
SUM_COLUMNS = ("tp", "fp", "fn", "sum_iou", "sum_pro", "sum_purity", "images")
MAX_CLASSES = _lib.MATCH_MAX_CLASSES
_ws = _lib.Workspace()


def _ratio(num: float, den: float) -> float:
    return num / den if den else float("nan")


def summarize(sums, classes: Sequence[int], images_total: int) -> Dict:
    """The score table of accumulated `MatchResult.sums()` rows (host values [len(classes), 7], columns SUM_COLUMNS; rows of several
    batches simply added) over `images_total` images.  Per class and overall PQ = sum_iou / (tp + fp/2 + fn/2), SQ = sum_iou / tp,
    RQ = tp / (tp + fp/2 + fn/2), precision = tp / n_pred, recall = tp / n_gt, F1 = 2 tp / (n_pred + n_gt), PRO = sum_pro / n_gt,
    purity = sum_purity / n_pred; a ratio with a zero denominator is NaN.  An overall value is the mean of the per-class values over
    the classes with at least one defect on either side (PQ and RQ are defined for every one of them; a class whose ratio is NaN --
    SQ without a match, precision and purity without a predicted defect, recall and PRO without a real one -- is left out of that
    ratio's mean); NaN when no class is left."""
    rows = np.asarray(sums, dtype=np.float64).reshape(len(classes), len(SUM_COLUMNS))
    per = {}
    for c, (tp, fp, fn, s_iou, s_pro, s_pur, _) in zip(classes, rows.tolist()):
        n_pred, n_gt, den = tp + fp, tp + fn, tp + 0.5 * fp + 0.5 * fn
        per[int(c)] = {"tp": int(tp), "fp": int(fp), "fn": int(fn), "n_pred": int(n_pred), "n_gt": int(n_gt),
                       "PQ": _ratio(s_iou, den), "SQ": _ratio(s_iou, tp), "RQ": _ratio(tp, den), "precision": _ratio(tp, n_pred),
                       "recall": _ratio(tp, n_gt), "F1": _ratio(2.0 * tp, n_pred + n_gt), "PRO": _ratio(s_pro, n_gt),
                       "purity": _ratio(s_pur, n_pred)}
    out = {"classes": [int(c) for c in classes], "per_class": per}
    present = [v for v in per.values() if v["n_pred"] + v["n_gt"] > 0]
    for name in ("PQ", "SQ", "RQ", "precision", "recall", "F1", "PRO", "purity"):
        vals = [v[name] for v in present if v[name] == v[name]]
        out[name] = float(np.mean(vals)) if vals else float("nan")
    for name in ("tp", "fp", "fn", "n_pred", "n_gt"):
        out[name] = sum(v[name] for v in per.values())
    used = int(rows[0, 6]) if len(classes) else 0
    out["images"], out["images_skipped"] = used, int(images_total) - used
    return out


class MatchResult(NamedTuple):
    """pred: int64 [B,Mp,4] and target: int64 [B,Mg,4], columns MATCH_COLUMNS, rows from min(count, max_instances) on zero; counts:
    int64 [B,num_classes,3], columns COUNT_COLUMNS (fp = n_pred - tp, fn = n_gt - tp); valid: bool [B], false where either side has
    more components than table rows; the threshold and the two InstanceResults the tables refer to."""
    pred: torch.Tensor
    target: torch.Tensor
    counts: torch.Tensor
    valid: torch.Tensor
    iou_threshold: float
    pred_instances: InstanceResult
    target_instances: InstanceResult

    @property
    def num_classes(self) -> int:
        return self.counts.shape[1]

    def _side_iou(self, mine: torch.Tensor, own: InstanceResult, other: InstanceResult) -> torch.Tensor:
        partner, inter = mine[..., 0], mine[..., 1]
        area_other = torch.gather(other.table[..., 1], 1, (partner - 1).clamp(min=0))
        union = (own.table[..., 1] + area_other - inter).clamp(min=1).to(torch.float64)
        return torch.where(partner > 0, inter.to(torch.float64) / union, torch.zeros_like(union))

    def iou(self) -> torch.Tensor:
        """float64 [B,Mg]: the IoU of every ground-truth defect with its partner, 0 where it has none."""
        return self._side_iou(self.target, self.target_instances, self.pred_instances)

    def pred_iou(self) -> torch.Tensor:
        """float64 [B,Mp]: the same from the prediction's side."""
        return self._side_iou(self.pred, self.pred_instances, self.target_instances)

    def _classes(self, classes) -> List[int]:
        Cn = self.num_classes
        classes = list(range(1, Cn)) if classes is None else [int(c) for c in classes]
        if any(c < 0 or c >= Cn for c in classes):
            raise ValueError(f"MatchResult: classes lie in [0, {Cn})")
        return classes

    def sums(self, classes: Optional[Sequence[int]] = None) -> torch.Tensor:
        """float64 [len(classes), 7] on the device, columns SUM_COLUMNS, over the valid images: tp, fp, fn, the sum of the IoU of the
        matched pairs (by the ground-truth defect's class), the sum of covered / area over the ground-truth defects and over the
        predicted defects of the class, and the number of images used.  Rows of several batches add up.  classes: default
        1 .. num_classes-1.  Does not synchronise."""
        classes = self._classes(classes)
        dev = self.counts.device
        cl = torch.tensor(classes, dtype=torch.int64, device=dev)
        ok = self.valid
        cnt = torch.where(ok[:, None, None], self.counts, torch.zeros_like(self.counts))[:, classes].sum(dim=0).to(torch.float64)   # [K,3]

        def side(mine, inst):
            M = mine.shape[1]
            rows = torch.arange(M, device=dev)[None] < inst.count.clamp(max=M)[:, None].to(torch.int64)
            sel = (inst.table[..., 0][None] == cl[:, None, None]) & (rows & ok[:, None])[None]                                    # [K,B,M]
            frac = mine[..., 2].to(torch.float64) / inst.table[..., 1].clamp(min=1).to(torch.float64)
            return sel, frac
        sel_g, frac_g = side(self.target, self.target_instances)
        sel_p, frac_p = side(self.pred, self.pred_instances)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        s_iou = torch.where(sel_g & (self.target[..., 3] > 0)[None], self.iou()[None], zero).sum(dim=(1, 2))
        s_pro = torch.where(sel_g, frac_g[None], zero).sum(dim=(1, 2))
        s_pur = torch.where(sel_p, frac_p[None], zero).sum(dim=(1, 2))
        used = ok.sum().to(torch.float64).expand(len(classes))
        return torch.stack([cnt[:, 0], cnt[:, 1] - cnt[:, 0], cnt[:, 2] - cnt[:, 0], s_iou, s_pro, s_pur, used], dim=1)

    def summary(self, classes: Optional[Sequence[int]] = None) -> Dict:
        """One device-to-host copy: `summarize` of this result's sums (per class and overall PQ, SQ, RQ, precision, recall, F1, PRO,
        purity, the counts, "images" and "images_skipped")."""
        classes = self._classes(classes)
        return summarize(self.sums(classes).cpu().numpy(), classes, self.valid.shape[0])

    def records(self) -> List[Dict[str, List[dict]]]:
        """One device-to-host copy; per image {"target": [...], "pred": [...]}: a dict per in-table defect with label, cls, area,
        partner, iou, covered (the fraction of its pixels on in-table components of its class on the other side) and matched."""
        out = []
        sides = []
        for name, mine, inst, iou in (("target", self.target, self.target_instances, self.iou()),
                                      ("pred", self.pred, self.pred_instances, self.pred_iou())):
            B, M = mine.shape[:2]
            packed = torch.cat([mine.reshape(B, -1).to(torch.float64), inst.table[..., :2].reshape(B, -1).to(torch.float64), iou,
                                inst.count.to(torch.float64).reshape(B, 1)], dim=1).cpu().numpy()
            sides.append((name, M, packed))
        for b in range(self.valid.shape[0]):
            rec = {}
            for name, M, packed in sides:
                row = packed[b]
                mine, tab, iou, n = row[:4 * M].reshape(M, 4), row[4 * M:6 * M].reshape(M, 2), row[6 * M:7 * M], int(row[-1])
                rec[name] = [{"label": k + 1, "cls": int(tab[k, 0]), "area": int(tab[k, 1]), "partner": int(mine[k, 0]), "iou": float(iou[k]),
                              "covered": float(mine[k, 2]) / float(tab[k, 1]), "matched": bool(mine[k, 3])} for k in range(min(n, M))]
            out.append(rec)
        return out


# ------------------------------------------------------------------------------------------------ numpy restatement
def _reduce_np(inter: np.ndarray, axis: int, area_mine: np.ndarray, area_other: np.ndarray, thr: float) -> np.ndarray:
    """int64 [n,4] for the components along the axis that is kept: np.argmax returns the first, i.e. the lowest number on ties."""
    other = inter.shape[axis]
    n = inter.shape[1 - axis]
    out = np.zeros((n, 4), dtype=np.int64)
    if n == 0 or other == 0:
        return out
    best = inter.argmax(axis=axis)
    top = inter.max(axis=axis)
    has = top > 0
    out[:, 0] = np.where(has, best + 1, 0)
    out[:, 1] = top
    out[:, 2] = inter.sum(axis=axis)
    union = area_mine + area_other[best] - top
    out[:, 3] = has & (top.astype(np.float64) > thr * union.astype(np.float64))
    return out


def _match_cpu(pred: InstanceResult, target: InstanceResult, Cn: int, thr: float, agnostic: bool):
    tp_, tg_ = pred.table.numpy(), target.table.numpy()
    B, Mp, Mg = tp_.shape[0], tp_.shape[1], tg_.shape[1]
    out_p = np.zeros((B, Mp, 4), dtype=np.int64)
    out_g = np.zeros((B, Mg, 4), dtype=np.int64)
    counts = np.zeros((B, Cn, 3), dtype=np.int64)
    for b in range(B):
        inter, np_, ng = pair_matrix_np(pred, target, b, agnostic)
        out_p[b, :np_] = _reduce_np(inter, 1, tp_[b, :np_, 1], tg_[b, :ng, 1], thr)
        out_g[b, :ng] = _reduce_np(inter, 0, tg_[b, :ng, 1], tp_[b, :np_, 1], thr)
        for c in range(Cn):
            of_c = tg_[b, :ng, 0] == c
            counts[b, c] = (int((of_c & (out_g[b, :ng, 3] > 0)).sum()), int((tp_[b, :np_, 0] == c).sum()), int(of_c.sum()))
    return torch.from_numpy(out_p), torch.from_numpy(out_g), torch.from_numpy(counts)


# ------------------------------------------------------------------------------------------------ public function
def match_instances(pred: InstanceResult, target: InstanceResult, num_classes: int, *, iou_threshold: float = 0.5,
                    class_agnostic: bool = False) -> MatchResult:
    """Match the defects of `pred` against those of `target`, two results of `label_instances` over the same B, H, W on one device
    (their max_instances may differ).  A pixel with prediction number p and ground-truth number g, both with a table row and of one
    class (class_agnostic: of any classes), adds 1 to inter[b, p, g]; p and g are matched iff
    float64(inter) > float64(iou_threshold) * float64(area_p + area_g - inter).  Only 0.5 <= iou_threshold < 1 is accepted (below
    0.5 a match is not unique and needs an assignment step).  Does not synchronise with the host."""
    B, H, W, Mp, Mg, Cn, valid = check_instance_pair("match_instances", pred, target, num_classes, MAX_CLASSES)
    thr = float(iou_threshold)
    if not 0.5 <= thr < 1.0:
        raise ValueError("match_instances: 0.5 <= iou_threshold < 1 (a lower threshold needs an assignment step, which is not built)")
    if not pred.labels.is_cuda:
        out_p, out_g, counts = _match_cpu(pred, target, Cn, thr, bool(class_agnostic))
        return MatchResult(out_p, out_g, counts, valid, thr, pred, target)
    dev = pred.labels.device
    held = pair_operands(pred, target)
    out_p = torch.empty((B, Mp, 4), dtype=torch.int64, device=dev)
    out_g = torch.empty((B, Mg, 4), dtype=torch.int64, device=dev)
    counts = torch.empty((B, Cn, 3), dtype=torch.int64, device=dev)
    _lib.call("uaps_match_instances", _lib.MatchCall, dev, _ws, _lib.workspace_bytes("uaps_match_workspace_bytes", B, Mp, Mg),
              B=B, H=H, W=W, num_classes=Cn, class_agnostic=1 if class_agnostic else 0, iou_threshold=thr, max_pred=Mp, max_gt=Mg,
              pred_out=out_p.data_ptr(), target_out=out_g.data_ptr(), counts=counts.data_ptr(),
              **{name: t.data_ptr() for name, t in held.items()})
    return MatchResult(out_p, out_g, counts, valid, thr, pred, target)

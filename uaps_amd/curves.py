"""Threshold-sweep metrics on the kernels of csrc/curves.hip: how good the scores themselves are, not only their arg-max.

`score_curves` histograms the quantised class scores of a [B,C,H,W] map split by "is this pixel of the class" (one row per class), the
top score split by "is the arg-max right" (the top row) and, with the ground truth's `label_instances` result, the scores inside every
real defect; `plane_curves` does the same for any per-pixel score -- the uncertainty map -- split by "is the prediction right".  From
those integer histograms the host forms, in float64: pixel AUROC (the Mann-Whitney statistic of the quantised scores, ties at one
half), average precision, the best F1 and its threshold, AUPRO (the area under per-region overlap against the false-positive rate up
to fpr_limit), ECE / MCE with the reliability table, and for a plane the AUROC of error detection and the area under the risk-coverage
curve (AURC).  The histograms are exact and the same bits from run to run; nothing synchronises with the host before `summary()`.

Bin rule (the contract, include/uaps_hip.h): inv = float32(bins) / (float32(hi) - float32(lo));
bin(s) = clamp(floor((s - lo) * inv), 0, bins - 1), every step rounded in fp32, a NaN enters no bin and is counted.

CPU tensors take the numpy restatement below, as in the other modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._checks import LABEL_DTYPE_CODE as _DTYPE_CODE, TOO_BIG as _TOO_BIG, as_labels
from .instances import FIXED_ONE, InstanceResult, fixed_point

MAX_BINS = _lib.CURVES_MAX_BINS
MAX_CLASSES = 8                          # UAPS_MAX_CLASSES
_ws = _lib.Workspace()


def bin_factor(bins: int, lo: float, hi: float) -> np.float32:
    """inv of the bin rule: formed once, in fp32."""
    return np.float32(bins) / (np.float32(hi) - np.float32(lo))


def bin_index(s, bins: int, lo: float = 0.0, hi: float = 1.0) -> np.ndarray:
    """The bin rule on the host: int64 bins of float32 scores, -1 for a NaN."""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((s - np.float32(lo)).astype(np.float32) * bin_factor(bins, lo, hi)).astype(np.float32)
        t = np.minimum(np.maximum(t, np.float32(0)), np.float32(bins - 1))
    nan = np.isnan(s)
    return np.where(nan, -1, np.where(nan, 0, t).astype(np.int64))


def _ratio(num, den) -> float:
    return float(num) / float(den) if den else float("nan")


# ------------------------------------------------------------------------------------------------ scores from pooled histograms
def auroc(pos: Sequence[int], neg: Sequence[int]) -> float:
    """sum_i pos[i] (2 neg_below[i] + neg[i]) / (2 P N) in Python integers: the Mann-Whitney statistic of the bin indices, ties at 1/2."""
    pos, neg = [int(v) for v in pos], [int(v) for v in neg]
    below = num = 0
    for p, n in zip(pos, neg):
        num += p * (2 * below + n)
        below += n
    return _ratio(num, 2 * sum(pos) * sum(neg))


def average_precision(pos: Sequence[int], neg: Sequence[int]) -> float:
    """sum over the non-empty bins, descending, of (recall_n - recall_{n-1}) precision_n."""
    P = sum(int(v) for v in pos)
    if not P:
        return float("nan")
    tp = fp = 0
    ap, last = 0.0, 0.0
    for p, n in zip(reversed(list(pos)), reversed(list(neg))):
        p, n = int(p), int(n)
        if p + n == 0:
            continue
        tp, fp = tp + p, fp + n
        recall = tp / P
        ap += (recall - last) * (tp / (tp + fp))
        last = recall
    return ap


def best_f1(pos: Sequence[int], neg: Sequence[int], lo: float, hi: float):
    """(F1, threshold): the largest 2 tp / (2 tp + fp + fn) over "predicted = bin >= i" and the lower edge of that bin (the highest
    such bin on ties)."""
    bins, P = len(pos), sum(int(v) for v in pos)
    best, at, tp, fp = float("nan"), float("nan"), 0, 0
    for i in range(bins - 1, -1, -1):
        tp, fp = tp + int(pos[i]), fp + int(neg[i])
        den = tp + fp + P
        if den and not (tp * 2 / den <= best):
            best, at = tp * 2 / den, lo + i * (hi - lo) / bins
    return best, at


def aupro(neg: Sequence[int], pro_sum: Sequence[float], n_regions: int, fpr_limit: float = 0.3) -> float:
    """The area under (FPR_i, PRO_i), i = bins .. 0 ("predicted" = bin >= i; both 0 at i = bins), by the trapezoid rule over ascending
    FPR up to fpr_limit with the crossing segment interpolated linearly, divided by fpr_limit."""
    N = sum(int(v) for v in neg)
    if not N or not n_regions:
        return float("nan")
    bins = len(neg)
    x0 = y0 = area = 0.0
    above = 0
    for i in range(bins - 1, -1, -1):
        above += int(neg[i])
        x1, y1 = above / N, float(pro_sum[i]) / n_regions
        if x1 >= fpr_limit:
            if x1 > x0:
                yl = y0 + (y1 - y0) * (fpr_limit - x0) / (x1 - x0)
                area += (fpr_limit - x0) * (y0 + yl) / 2
            return area / fpr_limit
        area += (x1 - x0) * (y0 + y1) / 2
        x0, y0 = x1, y1
    return area / fpr_limit                                   # fpr_limit > 1: the whole curve


def calibration(false: Sequence[int], true: Sequence[int], q_false: Sequence[int], q_true: Sequence[int], lo: float, hi: float,
                ece_bins: int = 16) -> Dict:
    """ECE = sum_g (n_g / n) |acc_g - conf_g| and MCE = max_g |acc_g - conf_g| over groups of bins / ece_bins fine bins, with
    conf_g = sum qsum / 2^24 / n_g, and the reliability table."""
    bins = len(true)
    if ece_bins < 1 or bins % ece_bins:
        raise ValueError(f"ece_bins divides bins: {bins} % {ece_bins} != 0")
    w = bins // ece_bins
    total = sum(int(v) for v in false) + sum(int(v) for v in true)
    ece, mce, table = 0.0, float("nan"), []
    for g in range(ece_bins):
        sl = slice(g * w, (g + 1) * w)
        t = sum(int(v) for v in true[sl])
        n = t + sum(int(v) for v in false[sl])
        qs = sum(int(v) for v in q_true[sl]) + sum(int(v) for v in q_false[sl])
        row = {"lo": lo + g * (hi - lo) / ece_bins, "hi": lo + (g + 1) * (hi - lo) / ece_bins, "n": n, "accuracy": _ratio(t, n),
               "confidence": _ratio(qs / FIXED_ONE, n)}
        table.append(row)
        if n:
            gap = abs(row["accuracy"] - row["confidence"])
            ece += n / total * gap
            mce = gap if not (gap <= mce) else mce
    return {"ECE": ece if total else float("nan"), "MCE": mce, "reliability": table}


def aurc(false: Sequence[int], true: Sequence[int]) -> float:
    """Risk-coverage over ascending score: the pixels of one bin enter together; sum over the non-empty bins of
    (cov_i - cov_{i-1}) risk_i, both cumulative (risk = errors so far / pixels so far)."""
    n = sum(int(v) for v in false) + sum(int(v) for v in true)
    if not n:
        return float("nan")
    seen = wrong = 0
    out, last = 0.0, 0.0
    for f, t in zip(false, true):
        f, t = int(f), int(t)
        if f + t == 0:
            continue
        seen, wrong = seen + f + t, wrong + f
        cov = seen / n
        out += (cov - last) * (wrong / seen)
        last = cov
    return out


class CurveSums(NamedTuple):
    """Pooled over the valid images of one or more batches; `a + b` adds two of them field by field.  hist int64 [R,2,bins], qsum the
    same or None, nan int64 [R], pro_sum float64 [K,bins] and n_regions int64 [K] (None without regions), images int64 [2]: used, seen."""
    hist: torch.Tensor
    qsum: Optional[torch.Tensor]
    nan: torch.Tensor
    pro_sum: Optional[torch.Tensor]
    n_regions: Optional[torch.Tensor]
    images: torch.Tensor

    def __add__(self, other):
        if not isinstance(other, CurveSums):
            return NotImplemented
        if any((a is None) != (b is None) for a, b in zip(self, other)) or self.hist.shape != other.hist.shape:
            raise ValueError("CurveSums: the two sums come from different settings")
        return CurveSums(*(None if a is None else a + b for a, b in zip(self, other)))

    def host(self) -> "CurveSums":
        """One device-to-host copy: every field packed into one int64 vector."""
        parts = [(i, t) for i, t in enumerate(self) if t is not None]
        flat = torch.cat([(t.view(torch.int64) if t.dtype == torch.float64 else t).reshape(-1) for _, t in parts]).cpu()
        out, at = [None] * len(self), 0
        for i, t in parts:
            v = flat[at:at + t.numel()].reshape(t.shape)
            out[i] = v.view(torch.float64) if t.dtype == torch.float64 else v
            at += t.numel()
        return CurveSums(*out)


def summarize(sums: CurveSums, classes: Sequence[int], *, lo: float = 0.0, hi: float = 1.0, has_top: bool = True, plane: bool = False,
              fpr_limit: float = 0.3, ece_bins: int = 16) -> Dict:
    """The score table of accumulated `CurveResult.sums()` (several batches: added with +).

    Rows of `score_curves`: per class AUROC, AP, F1 (the best over the thresholds) and F1_threshold, AUPRO (NaN without regions), the
    pixel counts; the overall values are the means over the classes with at least one positive and one negative pixel (a NaN value is
    left out of its mean; NaN when none is left).  With the top row: top_accuracy and, where the sums carry qsum, ECE, MCE and the
    reliability table.  plane=True (the one row of `plane_curves`): AUROC of error detection -- "error" (event false) is the positive
    class, a high score should mark a wrong pixel -- AURC and error_rate.  A ratio with a zero denominator is NaN."""
    s = sums.host() if sums.hist.is_cuda else sums
    hist = s.hist.numpy()
    bins = hist.shape[-1]
    used, seen = (int(v) for v in s.images.tolist())
    out: Dict = {"bins": bins, "images": used, "images_skipped": seen - used, "nan": [int(v) for v in s.nan.tolist()]}
    if plane:
        false, true = hist[0, 0].tolist(), hist[0, 1].tolist()
        out["AUROC"], out["AURC"] = auroc(false, true), aurc(false, true)
        out["error_rate"] = _ratio(sum(false), sum(false) + sum(true))
        return out
    classes = [int(c) for c in classes]
    K = len(classes)
    if hist.shape[0] != K + (1 if has_top else 0):
        raise ValueError(f"summarize: {hist.shape[0]} rows for {K} classes" + (" and the top row" if has_top else ""))
    per = {}
    for k, c in enumerate(classes):
        neg, pos = hist[k, 0].tolist(), hist[k, 1].tolist()
        f1, at = best_f1(pos, neg, lo, hi)
        row = {"positives": sum(pos), "negatives": sum(neg), "AUROC": auroc(pos, neg), "AP": average_precision(pos, neg), "F1": f1,
               "F1_threshold": at, "AUPRO": float("nan"), "regions": 0}
        if s.pro_sum is not None:
            row["regions"] = int(s.n_regions[k])
            row["AUPRO"] = aupro(neg, s.pro_sum[k].tolist(), row["regions"], fpr_limit)
        per[c] = row
    out["classes"], out["per_class"] = classes, per
    present = [v for v in per.values() if v["positives"] > 0 and v["negatives"] > 0]
    for name in ("AUROC", "AP", "F1", "AUPRO"):
        vals = [v[name] for v in present if v[name] == v[name]]
        out[name] = float(np.mean(vals)) if vals else float("nan")
    if has_top:
        false, true = hist[K, 0].tolist(), hist[K, 1].tolist()
        out["top_accuracy"] = _ratio(sum(true), sum(true) + sum(false))
        if s.qsum is not None:
            q = s.qsum.numpy()
            out.update(calibration(false, true, q[K, 0].tolist(), q[K, 1].tolist(), lo, hi, ece_bins))
    return out


class CurveResult(NamedTuple):
    """hist: int64 [B,R,2,bins] (index 0 = event false, 1 = true; the class rows in the order of `classes`, then the top row); qsum: the
    same with the sums of q(s) = rint(s 2^24), or None; nan: int64 [B,R]; pro_sum: float64 [B,K,bins] and n_regions: int64 [B,K], None
    without regions; valid: bool [B], false where the image has more regions than table rows."""
    hist: torch.Tensor
    qsum: Optional[torch.Tensor]
    nan: torch.Tensor
    pro_sum: Optional[torch.Tensor]
    n_regions: Optional[torch.Tensor]
    valid: torch.Tensor
    classes: tuple
    bins: int
    lo: float
    hi: float
    has_top: bool
    plane: bool = False

    def sums(self) -> CurveSums:
        """Pooled over the valid images (without regions every image is valid); sums of several batches add up.  Does not synchronise."""
        ok = self.valid

        def pool(t):
            if t is None:
                return None
            m = ok.reshape((-1,) + (1,) * (t.dim() - 1))
            return torch.where(m, t, torch.zeros_like(t)).sum(dim=0)
        images = torch.stack([ok.sum(), torch.ones_like(ok, dtype=torch.int64).sum()])
        return CurveSums(pool(self.hist), pool(self.qsum), pool(self.nan), pool(self.pro_sum), pool(self.n_regions), images)

    def summary(self, fpr_limit: float = 0.3, ece_bins: int = 16) -> Dict:
        """The one copy to the host: `summarize` of this result's sums."""
        return summarize(self.sums(), self.classes, lo=self.lo, hi=self.hi, has_top=self.has_top, plane=self.plane, fpr_limit=fpr_limit,
                         ece_bins=ece_bins)


# ------------------------------------------------------------------------------------------------ numpy restatement
def _softmax32(z: np.ndarray) -> np.ndarray:
    """softmax over axis 1 as the kernel forms it: fp32, the maximum by fmax, the sum in class order."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = z[:, 0]
        for c in range(1, z.shape[1]):
            m = np.fmax(m, z[:, c])
        e = np.exp((z - m[:, None]).astype(np.float32)).astype(np.float32)
        s = np.zeros_like(m)
        for c in range(z.shape[1]):
            s = (s + e[:, c]).astype(np.float32)
        return (e / s[:, None]).astype(np.float32)


def _rows_np(S: np.ndarray, t: np.ndarray, classes, top: bool, from_logits: bool):
    """([(score [B,H,W] fp32, event bool, ok bool, nan bool)] per row, the probabilities [B,C,H,W] the regions are scored on)."""
    Cn = S.shape[1]
    rows = []
    with np.errstate(invalid="ignore", over="ignore"):
        if Cn == 1:
            z = S[:, 0]
            p = (np.float32(1) / (np.float32(1) + np.exp(-z).astype(np.float32))).astype(np.float32) if from_logits else z
            ok = (t == 0) | (t == 1)
            bad = np.isnan(p)
            for _ in classes:
                rows.append((p, t == 1, ok, bad))
            if top:
                pred = (z > 0) if from_logits else (p > np.float32(0.5))
                rows.append((np.fmax(p, (np.float32(1) - p).astype(np.float32)), pred.astype(np.int64) == t, ok, bad))
            return rows, p[:, None]
        am = np.argmax(np.where(np.isnan(S), -np.inf, S), axis=1)             # the lowest index among equal values
        P = _softmax32(S) if from_logits else S
        ok = (t >= 0) & (t < Cn)
        for c in classes:
            rows.append((P[:, c], t == c, ok, np.isnan(P[:, c])))
        if top:
            bad = np.isnan(P).any(axis=1)
            rows.append((np.where(bad, np.float32(np.nan), np.max(np.where(np.isnan(P), -np.inf, P), axis=1)).astype(np.float32),
                         am == t, ok, bad))
        return rows, P


def _hist_np(rows, bins, lo, hi, want_sums):
    B, R = rows[0][0].shape[0], len(rows)
    hist = np.zeros((B, R, 2, bins), dtype=np.int64)
    qsum = np.zeros((B, R, 2, bins), dtype=np.int64) if want_sums else None
    nan = np.zeros((B, R), dtype=np.int64)
    for r, (s, ev, ok, bad) in enumerate(rows):
        idx = bin_index(s, bins, lo, hi)
        for b in range(B):
            use = ok[b] & ~bad[b]
            key = ev[b][use].astype(np.int64) * bins + idx[b][use]
            hist[b, r] = np.bincount(key, minlength=2 * bins).reshape(2, bins)
            nan[b, r] = int((ok[b] & bad[b]).sum())
            if want_sums:
                q = fixed_point(s[b][use])
                np.add.at(qsum[b, r].reshape(-1), key, q)
    return hist, qsum, nan


def _regions_np(P: np.ndarray, regions: InstanceResult, classes, bins, lo, hi):
    labels, count, table = regions.labels.numpy(), regions.count.numpy(), regions.table.numpy()
    B, Cn = P.shape[:2]
    Mg, K = table.shape[1], len(classes)
    pro = np.zeros((B, K, bins), dtype=np.float64)
    n_reg = np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        nr = min(max(int(count[b]), 0), Mg)
        g = labels[b].reshape(-1).astype(np.int64)
        sel = np.nonzero((g >= 1) & (g <= Mg))[0]
        rc = table[b, g[sel] - 1, 0]
        good = (rc == 1) if Cn == 1 else ((rc >= 0) & (rc < Cn))
        sel, rc = sel[good], (np.zeros_like(rc[good]) if Cn == 1 else rc[good])
        s = P[b].reshape(Cn, -1)[rc, sel]
        idx = bin_index(s, bins, lo, hi)
        keep = idx >= 0
        rh = np.bincount((g[sel][keep] - 1) * bins + idx[keep], minlength=Mg * bins).reshape(Mg, bins)
        for k, c in enumerate(classes):
            for r in range(nr):
                if table[b, r, 0] != c or table[b, r, 1] <= 0:
                    continue
                n_reg[b, k] += 1
                pro[b, k] += np.cumsum(rh[r][::-1])[::-1].astype(np.float64) / np.float64(table[b, r, 1])
    return pro, n_reg


# ------------------------------------------------------------------------------------------------ public functions
def _check_bins(what: str, bins, lo, hi):
    bins, lo, hi = int(bins), float(lo), float(hi)
    if not 2 <= bins <= MAX_BINS:
        raise ValueError(f"{what}: 2 <= bins <= {MAX_BINS}")
    if not (np.isfinite(lo) and np.isfinite(hi) and np.float32(lo) < np.float32(hi)):
        raise ValueError(f"{what}: finite lo < hi (in fp32)")
    with np.errstate(over="ignore"):
        if not np.isfinite(bin_factor(bins, lo, hi)):
            raise ValueError(f"{what}: the range hi - lo is too narrow for {bins} bins in fp32")
    return bins, lo, hi


def score_curves(scores: torch.Tensor, target: torch.Tensor, *, classes: Optional[Sequence[int]] = None, bins: int = 1024,
                 top: bool = True, from_logits: bool = False, regions: Optional[InstanceResult] = None,
                 want_sums: bool = False) -> CurveResult:
    """The histograms of the class scores of `scores` fp32 [B,C,H,W] (probabilities; from_logits: logits, the softmax -- C == 1: the
    sigmoid -- is formed in the kernel) against `target` [B,H,W] over [0, 1] in `bins` bins: one row per class of `classes` (default
    1 .. C-1; [1] at C == 1), event "target is the class", and with top=True the top row, the largest score against "the arg-max is
    right".  A pixel whose target lies outside [0, C) (C == 1: outside {0, 1}) enters nothing.  regions: `label_instances(target)`,
    for AUPRO.  want_sums: also the fixed-point sums of the scores per cell (ECE needs them).  Does not synchronise with the host."""
    if scores.dim() != 4 or scores.dtype != torch.float32:
        raise ValueError("score_curves: scores is a float32 tensor [B,C,H,W]")
    B, Cn, H, W = scores.shape
    if target.dim() != 3 or tuple(target.shape) != (B, H, W):
        raise ValueError(f"score_curves: scores {tuple(scores.shape)}, target {tuple(target.shape)}")
    if target.device != scores.device:
        raise ValueError(f"score_curves: scores are on {scores.device}, target on {target.device}")
    target = as_labels(target)
    if not 1 <= Cn <= MAX_CLASSES:
        raise ValueError(f"score_curves: 1 <= C <= {MAX_CLASSES}")
    if min(B, H, W) < 1:
        raise ValueError("score_curves: an empty tensor")
    bins, lo, hi = _check_bins("score_curves", bins, 0.0, 1.0)
    classes = ([1] if Cn == 1 else list(range(1, Cn))) if classes is None else [int(c) for c in classes]
    if len(classes) > MAX_CLASSES or any((c != 1) if Cn == 1 else not 0 <= c < Cn for c in classes):
        raise ValueError(f"score_curves: at most {MAX_CLASSES} classes in [0, {Cn})" + (" (the sigmoid head scores class 1)" if Cn == 1 else ""))
    top = bool(top)
    K = len(classes)
    R = K + (1 if top else 0)
    if R == 0:
        raise ValueError("score_curves: no class row and no top row")
    if H * W >= _TOO_BIG or B * Cn * H * W * 4 >= _TOO_BIG or B * H * W * target.element_size() >= _TOO_BIG or B * R * 2 * bins * 8 >= _TOO_BIG:
        raise ValueError("score_curves: H*W < 2^31 and every tensor below 2 GiB")
    Mg = 0
    if regions is not None:
        if not isinstance(regions, InstanceResult):
            raise TypeError("score_curves: regions is a result of label_instances")
        if tuple(regions.labels.shape) != (B, H, W) or regions.labels.device != scores.device:
            raise ValueError(f"score_curves: regions labels {tuple(regions.labels.shape)} on {regions.labels.device}")
        Mg = regions.max_instances
        if B * Mg * bins * 4 >= _TOO_BIG:
            raise ValueError(f"score_curves: the region histograms of B * {Mg} * {bins} * 4 bytes reach 2 GiB: lower max_instances or bins")
    dev = scores.device
    valid = ~regions.overflow if regions is not None else torch.ones(B, dtype=torch.bool, device=dev)
    meta = (tuple(classes), bins, lo, hi, top)
    if not scores.is_cuda:
        S, t = scores.detach().numpy(), target.numpy().astype(np.int64)
        rows, P = _rows_np(S, t, classes, top, bool(from_logits))
        hist, qsum, nan = _hist_np(rows, bins, lo, hi, want_sums)
        pro = n_reg = None
        if regions is not None:
            pro, n_reg = _regions_np(P, regions, classes, bins, lo, hi)
            pro, n_reg = torch.from_numpy(pro), torch.from_numpy(n_reg)
        return CurveResult(torch.from_numpy(hist), None if qsum is None else torch.from_numpy(qsum), torch.from_numpy(nan), pro, n_reg,
                           valid, *meta)
    scores, target = scores.detach().contiguous(), target.contiguous()
    hist = torch.empty((B, R, 2, bins), dtype=torch.int64, device=dev)
    qsum = torch.empty((B, R, 2, bins), dtype=torch.int64, device=dev) if want_sums else None
    nan = torch.empty((B, R), dtype=torch.int64, device=dev)
    pro = n_reg = None
    fields, ws, need = {}, None, 0                         # (the workspace holds the region histograms: none without regions)
    if regions is not None:
        held = [t.contiguous() for t in (regions.labels, regions.count, regions.table)]
        pro = torch.empty((B, K, bins), dtype=torch.float64, device=dev)
        n_reg = torch.empty((B, K), dtype=torch.int64, device=dev)
        fields = dict(region_labels=held[0].data_ptr(), region_count=held[1].data_ptr(), region_table=held[2].data_ptr(), max_regions=Mg,
                      pro_sum=pro.data_ptr(), n_regions=n_reg.data_ptr())
        ws, need = _ws, _lib.workspace_bytes("uaps_curves_workspace_bytes", B, Mg, bins)
    _lib.call("uaps_score_curves", _lib.CurvesCall, dev, ws, need, B=B, C=Cn, H=H, W=W, bins=bins, from_logits=1 if from_logits else 0,
              top_row=1 if top else 0, n_classes=K, classes=classes, target_dtype=_DTYPE_CODE[target.dtype], lo=lo, hi=hi,
              scores=scores.data_ptr(), target=target.data_ptr(), hist=hist.data_ptr(), qsum=qsum.data_ptr() if want_sums else None,
              nan=nan.data_ptr(), **fields)
    return CurveResult(hist, qsum, nan, pro, n_reg, valid, *meta)


def plane_curves(score: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, *, bins: int = 1024, lo: float = 0.0, hi: float = 1.0,
                 want_sums: bool = False) -> CurveResult:
    """The histogram of a per-pixel score fp32 [B,H,W] that is no class probability -- the uncertainty map -- over [lo, hi] in `bins`
    bins, split by "pred == target" (two label maps [B,H,W]); pixels with target < 0 are ignored.  One row.  Does not synchronise."""
    if score.dim() != 3 or score.dtype != torch.float32:
        raise ValueError("plane_curves: score is a float32 tensor [B,H,W]")
    B, H, W = score.shape
    for t, what in ((pred, "pred"), (target, "target")):
        if t.dim() != 3 or tuple(t.shape) != (B, H, W):
            raise ValueError(f"plane_curves: score {tuple(score.shape)}, {what} {tuple(t.shape)}")
        if t.device != score.device:
            raise ValueError(f"plane_curves: score is on {score.device}, {what} on {t.device}")
    pred, target = as_labels(pred), as_labels(target)
    if min(B, H, W) < 1:
        raise ValueError("plane_curves: an empty tensor")
    bins, lo, hi = _check_bins("plane_curves", bins, lo, hi)
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG or B * 2 * bins * 8 >= _TOO_BIG:
        raise ValueError("plane_curves: H*W < 2^31 and every tensor below 2 GiB")
    dev = score.device
    valid = torch.ones(B, dtype=torch.bool, device=dev)
    meta = ((), bins, lo, hi, False, True)
    if not score.is_cuda:
        s, p, t = score.detach().numpy(), pred.numpy().astype(np.int64), target.numpy().astype(np.int64)
        hist, qsum, nan = _hist_np([(s, p == t, t >= 0, np.isnan(s))], bins, lo, hi, want_sums)
        return CurveResult(torch.from_numpy(hist), None if qsum is None else torch.from_numpy(qsum), torch.from_numpy(nan), None, None,
                           valid, *meta)
    score, pred, target = score.detach().contiguous(), pred.contiguous(), target.contiguous()
    hist = torch.empty((B, 1, 2, bins), dtype=torch.int64, device=dev)
    qsum = torch.empty((B, 1, 2, bins), dtype=torch.int64, device=dev) if want_sums else None
    nan = torch.empty((B, 1), dtype=torch.int64, device=dev)
    _lib.call("uaps_plane_curves", _lib.PlaneCurvesCall, dev, B=B, H=H, W=W, bins=bins, from_logits=0, pred_dtype=_DTYPE_CODE[pred.dtype],
              target_dtype=_DTYPE_CODE[target.dtype], lo=lo, hi=hi, score=score.data_ptr(), pred=pred.data_ptr(), target=target.data_ptr(),
              hist=hist.data_ptr(), qsum=qsum.data_ptr() if want_sums else None, nan=nan.data_ptr())
    return CurveResult(hist, qsum, nan, None, None, valid, *meta)

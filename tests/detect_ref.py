"""The reference of the detection tests (tests/test_detect_host.py, tests/test_gpu_detect.py): a literal statement of the definitions of
uaps_amd/detection.py, with which it shares no code.  Labels and tables come from instances_ref.label_batch (scipy); the pair counts are
np.logical_and sums; an IoU is a fractions.Fraction; detections are ordered by a Python sort on (-score, label); the assignment is the
triple loop over thresholds, detections and ground-truth defects with the greedy rule verbatim; AP is formed with plain loops.  Every
comparison of tables built on it is exact, `score` bit for bit."""
import functools
import math
from fractions import Fraction

import numpy as np

import instances_ref as R
import match_ref as M

SHAPES = M.SHAPES
MP, MG = M.MP, M.MG
COCO = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))
LOW = (0.1, 0.2, 0.3, 0.5, 0.75, 1.0)                                  # the crack benchmarks' thresholds, the ends of the range
T32 = tuple((100 + 29 * i) / 1000 for i in range(31)) + (1.0,)          # 32 thresholds from 0.100 to 1.000
NAN, INF = float("nan"), float("inf")


def t1000_of(thresholds):
    return [int(round(1000 * t)) for t in thresholds]


def detect_image(lp, lg, np_all, ng_all, tp, tg, num_classes, thresholds, agnostic=False, max_dets=None, scores=None):
    """One image.  lp, lg: label maps; np_all, ng_all: the true component counts; tp [Mp,9], tg [Mg,9]: the tables; scores: None (the
    mean of map 0, as float64(sum0) / float64(area)) or [Mp] floats.
    -> score float64 [Mp], rank [Mp], pred_match [Mp,T], pred_inter [Mp,T], target_match [Mg,T], counts [C,T+2], valid."""
    Mp, Mg, T = tp.shape[0], tg.shape[0], len(thresholds)
    n_p, n_g = max(0, min(int(np_all), Mp)), max(0, min(int(ng_all), Mg))
    cls_p = lambda p: 0 if agnostic else int(tp[p - 1, 0])
    cls_g = lambda g: 0 if agnostic else int(tg[g - 1, 0])
    inter = [dict() for _ in range(n_p + 1)]
    for p in range(1, n_p + 1):
        y0, x0, y1, x1 = (int(v) for v in tp[p - 1, 2:6])       # the component's box: no pixel of p lies outside it
        mp, box_g = lp[y0:y1, x0:x1] == p, lg[y0:y1, x0:x1]
        for g in np.unique(box_g[mp]):
            if 1 <= g <= n_g and (agnostic or tp[p - 1, 0] == tg[g - 1, 0]):
                inter[p][int(g)] = int(np.logical_and(mp, box_g == g).sum())
    score = np.full(Mp, -INF, dtype=np.float64)
    shown = {}
    for p in range(1, n_p + 1):
        s = np.float64(tp[p - 1, 7]) / np.float64(tp[p - 1, 1]) if scores is None else np.float64(scores[p - 1])
        shown[p] = (1, 0.0) if math.isnan(s) else (0, -float(s))               # a NaN after every number
        score[p - 1] = -INF if math.isnan(s) else s + 0.0
    rank = np.full(Mp, -1, dtype=np.int64)
    pm, pi = np.zeros((Mp, T), dtype=np.int64), np.zeros((Mp, T), dtype=np.int64)
    tm = np.zeros((Mg, T), dtype=np.int64)
    counts = np.zeros((num_classes, T + 2), dtype=np.int64)
    for c in range(num_classes):
        dets = sorted((p for p in range(1, n_p + 1) if cls_p(p) == c), key=lambda p: (shown[p], p))
        if max_dets is not None:
            dets = dets[:max_dets]
        gts = [g for g in range(1, n_g + 1) if cls_g(g) == c]
        counts[c, T], counts[c, T + 1] = len(dets), len(gts)
        for r, p in enumerate(dets):
            rank[p - 1] = r
        for t, k in enumerate(t1000_of(thresholds)):
            thr, taken = Fraction(k, 1000), set()
            for p in dets:
                best, best_iou = 0, None
                for g in gts:                                                  # ascending: the lowest number wins ties
                    i = inter[p].get(g, 0)
                    if i == 0 or g in taken:
                        continue
                    iou = Fraction(i, int(tp[p - 1, 1]) + int(tg[g - 1, 1]) - i)
                    if iou >= thr and (best_iou is None or iou > best_iou):
                        best, best_iou = g, iou
                if best:
                    taken.add(best)
                    pm[p - 1, t], pi[p - 1, t], tm[best - 1, t] = best, inter[p][best], p
                    counts[c, t] += 1
    return score, rank, pm, pi, tm, counts, (np_all <= Mp and ng_all <= Mg)


def detect_batch(ref_p, ref_g, num_classes, thresholds=COCO, agnostic=False, max_dets=None, scores=None):
    """ref_p, ref_g: (labels, count, table) of instances_ref.label_batch -> the seven arrays of detect_image, stacked."""
    out = [detect_image(ref_p[0][b], ref_g[0][b], ref_p[1][b], ref_g[1][b], ref_p[2][b], ref_g[2][b], num_classes, thresholds, agnostic,
                        max_dets, None if scores is None else scores[b]) for b in range(ref_p[0].shape[0])]
    return tuple(np.stack([o[k] for o in out]) for k in range(6)) + (np.array([o[6] for o in out]),)


NAMES = ("score", "rank", "pred_match", "pred_inter", "target_match", "counts")


def assert_tables(res, ref, what=""):
    """Exact equality of a DetectionResult with detect_batch's tuple; `score` by its bits."""
    for name, want in zip(NAMES, ref):
        got = getattr(res, name).cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, got.shape, want.shape)
        if name == "score":
            got, want = got.view(np.int64), want.view(np.int64)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(res.valid.cpu().numpy(), ref[6]), (what, "valid")


def average_precision(flags, n_gt):
    """(AP, final recall) of one class and threshold; flags: 1 (true positive) or 0 per detection in score order."""
    if n_gt == 0:
        return NAN, NAN
    tp = fp = 0
    rec, prec = [], []
    for f in flags:
        tp, fp = tp + f, fp + 1 - f
        rec.append(tp / n_gt)
        prec.append(tp / (tp + fp))
    for i in range(len(prec) - 2, -1, -1):
        if prec[i] < prec[i + 1]:
            prec[i] = prec[i + 1]
    total = 0.0
    for r in np.linspace(0.0, 1.0, 101):
        for i in range(len(rec)):
            if rec[i] >= r:
                total += prec[i]
                break
    return total / 101, (rec[-1] if rec else 0.0)


def _mean(values):
    vals = [v for v in values if not math.isnan(v)]
    return sum(vals) / len(vals) if vals else NAN


def summary(parts, classes, thresholds, agnostic=False):
    """parts: a list of (detect_batch's tuple, ref_p) -> the figures of detection.summarize."""
    T = len(thresholds)
    k1000 = t1000_of(thresholds)
    per = {}
    skipped = sum(int((~ref[6]).sum()) for ref, _ in parts)
    for c in classes:
        dets, n_gt = [], 0
        for ref, ref_p in parts:
            for b in np.nonzero(ref[6])[0]:
                n_gt += int(ref[5][b, c, T + 1])
                for p in range(ref[1].shape[1]):
                    if ref[1][b, p] >= 0 and (0 if agnostic else int(ref_p[2][b, p, 0])) == c:
                        dets.append((float(ref[0][b, p]), [int(ref[2][b, p, t] > 0) for t in range(T)]))
        dets.sort(key=lambda d: -d[0])                                         # stable: parts, then image, then label
        both = [average_precision([d[1][t] for d in dets], n_gt) for t in range(T)]
        per[c] = {"AP": _mean(v[0] for v in both), "AP_at": [v[0] for v in both], "AR": _mean(v[1] for v in both), "n_gt": n_gt,
                  "n_pred": len(dets)}
    out = {"per_class": per, "mAP": _mean(v["AP"] for v in per.values()), "AR": _mean(v["AR"] for v in per.values()),
           "n_gt": sum(v["n_gt"] for v in per.values()), "n_pred": sum(v["n_pred"] for v in per.values()), "images_skipped": skipped}
    for name, k in (("AP50", 500), ("AP75", 750)):
        if k in k1000:
            out[name] = _mean(v["AP_at"][k1000.index(k)] for v in per.values())
    return out


def check_summary(got, want, rel=1e-12):
    """detection.summarize's dict against summary(): integers equal, floats to 1e-12 relative (both are host float64 over at most 101
    terms formed from identical integers)."""
    from pytest import approx
    assert got["images_skipped"] == want["images_skipped"] and got["n_gt"] == want["n_gt"] and got["n_pred"] == want["n_pred"]
    for k in ("mAP", "AR", "AP50", "AP75"):
        assert (k in got) == (k in want), k
        if k in want:
            assert got[k] == approx(want[k], rel=rel, abs=0.0, nan_ok=True), (k, got[k], want[k])
    for c, w in want["per_class"].items():
        g = got["per_class"][c]
        assert (g["n_gt"], g["n_pred"]) == (w["n_gt"], w["n_pred"]), c
        assert g["AP"] == approx(w["AP"], rel=rel, abs=0.0, nan_ok=True) and g["AR"] == approx(w["AR"], rel=rel, abs=0.0, nan_ok=True), c
        assert g["AP_at"] == approx(w["AP_at"], rel=rel, abs=0.0, nan_ok=True), c


def confidence(shape, seed=5):
    """A confidence plane float32 [B,H,W] in (0, 1]; coarse values (multiples of 1/8) in the left half so that mean scores tie."""
    rng = np.random.default_rng(seed + shape[1] * 7 + shape[2])
    conf = rng.random(shape, dtype=np.float32) * np.float32(0.999) + np.float32(0.001)
    conf[:, :, : shape[2] // 2] = np.ceil(conf[:, :, : shape[2] // 2] * 8) / 8
    return conf.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, shape, connectivity, mp=MP, mg=MG):
    """-> (pred mask, gt mask, confidence, label_batch of the prediction (with the confidence sums) and of the ground truth)."""
    pred, gt = M.masks(name, shape)
    conf = confidence(shape)
    return pred, gt, conf, R.label_batch(pred, (conf,), connectivity, 0, 1, mp), R.label_batch(gt, (), connectivity, 0, 1, mg)


@functools.lru_cache(maxsize=None)
def reference(name, shape, connectivity, thresholds=COCO, agnostic=False, max_dets=None, mp=MP, mg=MG):
    _, _, _, ref_p, ref_g = case(name, shape, connectivity, mp, mg)
    return detect_batch(ref_p, ref_g, 4, thresholds, agnostic, max_dets)


def figure(boxes_p, boxes_g, shape, scores_map=None):
    """Masks from lists of (class, y0, x0, y1, x1) boxes, in the order their numbers will be given (raster order of first pixels is the
    caller's business), and a confidence plane that is `scores_map[k]` over prediction box k (default 0.5)."""
    pred, gt = np.zeros((1,) + shape, dtype=np.int64), np.zeros((1,) + shape, dtype=np.int64)
    conf = np.full((1,) + shape, 0.5, dtype=np.float32)
    for k, (c, y0, x0, y1, x1) in enumerate(boxes_p):
        pred[0, y0:y1, x0:x1] = c
        if scores_map is not None:
            conf[0, y0:y1, x0:x1] = scores_map[k]
    for c, y0, x0, y1, x1 in boxes_g:
        gt[0, y0:y1, x0:x1] = c
    return pred, gt, conf

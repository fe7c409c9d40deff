"""The reference of the matching tests (tests/test_match_host.py, tests/test_gpu_match.py): a brute-force statement of the definitions
of defect matching.  Per image it loops over the components of both sides and counts np.logical_and(lp == p, lg == g) (inside the box
of p, over the g that occur there); the class rule and the float64 comparison are applied literally.  It shares no code with
uaps_amd/matching.py and takes the label maps and tables of instances_ref.label_batch (scipy).  Every comparison of tables built on it
is exact."""
import functools
import math

import numpy as np
from pytest import approx

import instances_ref as R

SHAPES = ((1, 1, 1), (1, 1, 45), (1, 7, 300), (3, 37, 53), (2, 130, 70), (2, 256, 256))       # the instance tests' set
MP, MG = 512, 300                                   # table rows of the prediction and of the ground truth: different strides
PATTERNS = ("noise", "blobs", "full_full", "full_empty", "empty_empty", "diagonal", "checkerboard")

NAN = float("nan")


def match_image(lp, lg, np_all, ng_all, tp, tg, num_classes, thr=0.5, agnostic=False):
    """One image.  lp, lg: label maps; np_all, ng_all: the true component counts; tp [Mp,9], tg [Mg,9]: the tables.
    -> pred int64 [Mp,4], target int64 [Mg,4], counts int64 [C,3], valid."""
    Mp, Mg = tp.shape[0], tg.shape[0]
    n_p, n_g = max(0, min(int(np_all), Mp)), max(0, min(int(ng_all), Mg))      # (a negative count: no rows)
    inter = np.zeros((n_p + 1, n_g + 1), dtype=np.int64)
    for p in range(1, n_p + 1):
        y0, x0, y1, x1 = (int(v) for v in tp[p - 1, 2:6])       # the component's box: no pixel of p lies outside it
        mp, box_g = lp[y0:y1, x0:x1] == p, lg[y0:y1, x0:x1]
        for g in np.unique(box_g[mp]):                          # every other g has an empty intersection with p
            if 1 <= g <= n_g and (agnostic or tp[p - 1, 0] == tg[g - 1, 0]):
                inter[p, g] = int(np.logical_and(mp, box_g == g).sum())
    pred = np.zeros((Mp, 4), dtype=np.int64)
    target = np.zeros((Mg, 4), dtype=np.int64)

    def is_match(i, area_a, area_b):
        return float(i) > float(thr) * float(area_a + area_b - i)
    for p in range(1, n_p + 1):
        best, best_i = 0, 0
        for g in range(1, n_g + 1):
            if inter[p, g] > best_i:
                best, best_i = g, inter[p, g]
        m = best > 0 and is_match(best_i, int(tp[p - 1, 1]), int(tg[best - 1, 1]))
        pred[p - 1] = (best, best_i, inter[p].sum(), int(m))
    for g in range(1, n_g + 1):
        best, best_i = 0, 0
        for p in range(1, n_p + 1):
            if inter[p, g] > best_i:
                best, best_i = p, inter[p, g]
        m = best > 0 and is_match(best_i, int(tp[best - 1, 1]), int(tg[g - 1, 1]))
        target[g - 1] = (best, best_i, inter[:, g].sum(), int(m))
    counts = np.zeros((num_classes, 3), dtype=np.int64)
    for p in range(n_p):
        if 0 <= tp[p, 0] < num_classes:
            counts[tp[p, 0], 1] += 1
    for g in range(n_g):
        if 0 <= tg[g, 0] < num_classes:
            counts[tg[g, 0], 2] += 1
            counts[tg[g, 0], 0] += target[g, 3]
    return pred, target, counts, (np_all <= Mp and ng_all <= Mg)


def match_batch(ref_p, ref_g, num_classes, thr=0.5, agnostic=False):
    """ref_p, ref_g: (labels, count, table) of instances_ref.label_batch -> pred [B,Mp,4], target [B,Mg,4], counts [B,C,3], valid [B]."""
    out = [match_image(ref_p[0][b], ref_g[0][b], ref_p[1][b], ref_g[1][b], ref_p[2][b], ref_g[2][b], num_classes, thr, agnostic)
           for b in range(ref_p[0].shape[0])]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), np.array([o[3] for o in out]))


def assert_tables(res, ref, what=""):
    """Exact equality of a MatchResult with match_batch's tuple."""
    for name, got, want in (("pred", res.pred, ref[0]), ("target", res.target, ref[1]), ("counts", res.counts, ref[2])):
        got = got.cpu().numpy()
        assert got.dtype == np.int64 and got.shape == want.shape, (what, name, got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (what, name, bad[:5], got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])
    assert np.array_equal(res.valid.cpu().numpy(), ref[3]), (what, "valid")


def iou_gt(ref, ref_p, ref_g):
    """float64 [B,Mg]: the IoU of every ground-truth defect with its partner, 0 without one."""
    target = ref[1]
    out = np.zeros(target.shape[:2], dtype=np.float64)
    for b in range(target.shape[0]):
        for g in range(target.shape[1]):
            partner, inter = int(target[b, g, 0]), int(target[b, g, 1])
            if partner:
                out[b, g] = inter / (int(ref_p[2][b, partner - 1, 1]) + int(ref_g[2][b, g, 1]) - inter)
    return out


def sums(ref, ref_p, ref_g, classes):
    """float64 [K,7]: tp, fp, fn, sum IoU over the matched pairs, sum covered/area over the ground-truth and over the predicted defects,
    images used; invalid images left out.  math.fsum: the correctly rounded sums."""
    pred, target, counts, valid = ref
    iou = iou_gt(ref, ref_p, ref_g)
    rows = []
    for c in classes:
        tp = fp = fn = 0
        t_iou, t_pro, t_pur = [], [], []
        for b in np.nonzero(valid)[0]:
            tp += int(counts[b, c, 0]); fp += int(counts[b, c, 1] - counts[b, c, 0]); fn += int(counts[b, c, 2] - counts[b, c, 0])
            for g in range(min(int(ref_g[1][b]), target.shape[1])):
                if ref_g[2][b, g, 0] == c:
                    t_pro.append(int(target[b, g, 2]) / int(ref_g[2][b, g, 1]))
                    if target[b, g, 3]:
                        t_iou.append(iou[b, g])
            for p in range(min(int(ref_p[1][b]), pred.shape[1])):
                if ref_p[2][b, p, 0] == c:
                    t_pur.append(int(pred[b, p, 2]) / int(ref_p[2][b, p, 1]))
        rows.append([tp, fp, fn, math.fsum(t_iou), math.fsum(t_pro), math.fsum(t_pur), int(valid.sum())])
    return np.array(rows, dtype=np.float64).reshape(len(classes), 7)


def _div(a, b):
    return a / b if b else NAN


def summary(ref, ref_p, ref_g, classes):
    """Per class and overall (the mean over the classes with a defect on either side, those where the ratio is NaN left out) PQ, SQ, RQ,
    precision, recall, F1, PRO, purity."""
    rows = sums(ref, ref_p, ref_g, classes)
    per = {}
    for c, (tp, fp, fn, s_iou, s_pro, s_pur, _) in zip(classes, rows):
        per[c] = {"tp": int(tp), "fp": int(fp), "fn": int(fn), "n_pred": int(tp + fp), "n_gt": int(tp + fn),
                  "PQ": _div(s_iou, tp + fp / 2 + fn / 2), "SQ": _div(s_iou, tp), "RQ": _div(tp, tp + fp / 2 + fn / 2),
                  "precision": _div(tp, tp + fp), "recall": _div(tp, tp + fn), "F1": _div(2 * tp, 2 * tp + fp + fn),
                  "PRO": _div(s_pro, tp + fn), "purity": _div(s_pur, tp + fp)}
    out = {"per_class": per}
    present = [c for c in classes if per[c]["n_pred"] + per[c]["n_gt"] > 0]
    for k in ("PQ", "SQ", "RQ", "precision", "recall", "F1", "PRO", "purity"):
        defined = [per[c][k] for c in present if not math.isnan(per[c][k])]
        out[k] = sum(defined) / len(defined) if defined else NAN
    out["images_skipped"] = int((~ref[3]).sum())
    return out


def redraw(mask, fraction, C=4, seed=0):
    """A prediction made from a ground-truth mask by re-drawing a fraction of its pixels (class uniform in 0..C-1)."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(mask.shape) < fraction, rng.integers(0, C, mask.shape), mask).astype(np.int64)


def masks(name, shape, C=4):
    """(prediction mask, ground-truth mask) int64 [B,H,W]: the ground truth is class noise, the prediction the same with 15 % of the
    pixels drawn again (thousands of small components: most images overflow their tables); image 0 is the pattern `name`, so that
    images must not leak into each other."""
    B, H, W = shape
    if name == "blobs":                             # every image: square cells of random classes against the same moved by (3, 5) --
        cell = 16 if min(H, W) >= 64 else 4         # a few hundred components at most, spread over the whole image, large overlaps
        rng = np.random.default_rng(H + W)
        gt = rng.integers(0, C, (B, H // cell + 1, W // cell + 1)).repeat(cell, axis=1).repeat(cell, axis=2).astype(np.int64)
        return np.ascontiguousarray(np.roll(gt, (3, 5), axis=(1, 2))[:, :H, :W]), np.ascontiguousarray(gt[:, :H, :W])
    gt = R.noise(B, H, W, 0.8, C, seed=H + 3 * W)
    pred = redraw(gt, 0.15, C, seed=H * W)
    if name == "full_full":                         # one blob on either side: every add of the image lands on one word
        pred[0], gt[0] = 2, 2
    elif name == "full_empty":
        pred[0], gt[0] = 2, 0
    elif name == "empty_empty":
        pred[0], gt[0] = 0, 0
    elif name == "diagonal":                        # many components (4-connectivity) against one (8-connectivity)
        pred[0] = gt[0] = R.diagonal(H, W)[0]
    elif name == "checkerboard":                    # a checkerboard against its complement: no overlap at all
        pred[0] = R.checkerboard(H, W)[0]
        gt[0] = 1 - pred[0]
    return pred, gt


@functools.lru_cache(maxsize=None)
def case(name, shape, connectivity, mp=MP, mg=MG):
    """-> (pred mask, gt mask, connectivity of the prediction, of the ground truth, label_batch of either side)."""
    pred, gt = masks(name, shape)
    cp, cg = (4, 8) if name == "diagonal" else (connectivity, connectivity)
    return pred, gt, cp, cg, R.label_batch(pred, (), cp, 0, 1, mp), R.label_batch(gt, (), cg, 0, 1, mg)


def check_scores(res, ref, ref_p, ref_g, rel=1e-12):
    """iou(), sums() and summary() against the reference's float64 values.  Each is a sum of at most 4096 non-negative terms, each
    within one rounding of the reference's: any summation order stays within 4096 * 2^-53 = 4.6e-13 relative."""
    assert np.allclose(res.iou().cpu().numpy(), iou_gt(ref, ref_p, ref_g), rtol=rel, atol=0.0)
    for classes in ([1, 2, 3], [2], [0, 3]):
        assert np.allclose(res.sums(classes).cpu().numpy(), sums(ref, ref_p, ref_g, classes), rtol=rel, atol=0.0), classes
        got, want = res.summary(classes), summary(ref, ref_p, ref_g, classes)
        assert got["images_skipped"] == want["images_skipped"]
        for k in ("PQ", "SQ", "RQ", "precision", "recall", "F1", "PRO", "purity"):
            assert got[k] == approx(want[k], rel=rel, abs=0.0, nan_ok=True), (k, classes)
            for c in classes:
                assert got["per_class"][c][k] == approx(want["per_class"][c][k], rel=rel, abs=0.0, nan_ok=True), (k, c)
        for c in classes:
            assert all(got["per_class"][c][k] == want["per_class"][c][k] for k in ("tp", "fp", "fn", "n_pred", "n_gt"))
    assert np.allclose(res.sums().cpu().numpy(), sums(ref, ref_p, ref_g, [1, 2, 3]), rtol=rel, atol=0.0)

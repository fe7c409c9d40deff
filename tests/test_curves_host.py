"""Threshold-sweep metrics without a GPU: the package's numpy restatement (uaps_amd/curves.py) against the brute-force reference
(tests/curves_ref.py), a hand-worked image, the bin, ignore, tie and sigmoid rules, the scores against sklearn and hand-worked
histograms, evaluate(curves=...) around a stub network, and the C ABI's argument checks (they return before any launch).  Every
comparison of histograms is exact."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import curves_ref as CR
import instances_ref as R
from conftest import ROOT

EINVAL, ERANGE = -1, -2
F32 = np.float32


def _t(a):
    return torch.from_numpy(np.array(a))


def _inst(ref):
    from uaps_amd import InstanceResult
    labels, count, table = ref
    return InstanceResult(torch.from_numpy(labels), torch.from_numpy(count), torch.from_numpy(table), 0)


@pytest.mark.parametrize("Cn", CR.CLASSES)
@pytest.mark.parametrize("shape", CR.SHAPES[:5], ids=lambda s: "x".join(map(str, s)))
def test_cpu_path_equals_the_brute_force_reference(shape, Cn):
    from uaps_amd import score_curves
    for i, name in enumerate(CR.PATTERNS):
        bins = CR.BINS[(i + Cn) % 4]
        S, t = CR.scores(name, shape, Cn), CR.targets(shape, Cn, ignored=name == "ignored")
        res = score_curves(_t(S), _t(t), bins=bins, want_sums=True)
        K = 1 if Cn == 1 else Cn - 1
        assert res.hist.shape == (shape[0], K + 1, 2, bins) and res.classes == tuple([1] if Cn == 1 else range(1, Cn)) and res.has_top
        CR.assert_result(res, CR.curves(S, t, bins=bins, want_sums=True), f"{name} {shape} C{Cn} bins{bins}")
    z = CR.logits(shape, Cn)
    t = CR.targets(shape, Cn, ignored=True)
    for bins in (15, 4096):
        res = score_curves(_t(z), _t(t), bins=bins, from_logits=True, classes=[Cn - 1] if Cn > 1 else None, top=Cn != 2)
        CR.assert_result(res, CR.curves(z, t, [Cn - 1] if Cn > 1 else None, bins, Cn != 2, True), f"logits {shape} C{Cn} bins{bins}")


@pytest.mark.parametrize("name", ("blobs", "full", "noise"))
def test_cpu_regions_equal_the_reference(name):
    from uaps_amd import score_curves
    for shape, Cn in (((3, 37, 53), 4), ((2, 7, 300), 1), ((2, 130, 70), 2)):
        t, reg = CR.region_case(name, shape, Cn)
        S = CR.scores("one_bin" if name == "full" else "uniform", shape, Cn)
        res = score_curves(_t(S), _t(t), bins=15, regions=_inst(reg))
        ref = CR.curves(S, t, bins=15, regions=reg)
        CR.assert_result(res, ref, f"{name} {shape} C{Cn}")
        assert int(ref["n_regions"].sum()) > 0
        if name == "noise" and shape[1] > 7:
            assert not ref["valid"].all()


def test_hand_worked_image():
    """2 x 3, C = 3, bins = 4 over [0, 1]: edges 0.25, 0.5, 0.75."""
    from uaps_amd import label_instances, score_curves
    t = np.array([[[0, 1, 1], [2, 1, 7]]])                                     # the last pixel is ignored
    S = np.zeros((1, 3, 2, 3), dtype=F32)
    S[0, 0] = [[0.70, 0.10, 0.30], [0.20, 0.45, 0.9]]
    S[0, 1] = [[0.20, 0.80, 0.30], [0.30, 0.50, 0.9]]                           # (0,2): classes 0 and 1 tie, the arg-max is 0: wrong
    S[0, 2] = [[0.10, 0.10, 0.26], [0.50, 0.05, 0.9]]
    reg = label_instances(torch.where(_t(t) > 2, 0, _t(t)), max_instances=4)    # the 1s form one region (8-connected), the 2 another
    assert reg.count.tolist() == [2] and reg.table[0, :2, :2].tolist() == [[1, 3], [2, 1]]
    res = score_curves(_t(S), _t(t), bins=4, regions=reg, want_sums=True)
    assert res.classes == (1, 2) and res.bins == 4 and (res.lo, res.hi) == (0.0, 1.0) and res.has_top
    # class 1: positives 0.8 -> 3, 0.3 -> 1, 0.5 -> 2; negatives 0.2 -> 0, 0.3 -> 1
    assert res.hist[0, 0].tolist() == [[1, 1, 0, 0], [0, 1, 1, 1]]
    # class 2: positive 0.5 -> 2; negatives 0.1, 0.1 -> 0, 0.26 -> 1, 0.05 -> 0
    assert res.hist[0, 1].tolist() == [[3, 1, 0, 0], [0, 0, 1, 0]]
    # top: 0.7 right -> 2, 0.8 right -> 3, 0.3 wrong -> 1, 0.5 right -> 2, 0.5 right -> 2
    assert res.hist[0, 2].tolist() == [[0, 1, 0, 0], [0, 0, 3, 1]]
    q = lambda *v: int(sum(int(np.rint(F32(x) * F32(16777216.0))) for x in v))
    assert res.qsum[0, 2].tolist() == [[0, q(0.3), 0, 0], [0, 0, q(0.7, 0.5, 0.5), q(0.8)]]
    assert res.qsum[0, 0].tolist() == [[q(0.2), q(0.3), 0, 0], [0, q(0.3), q(0.5), q(0.8)]]
    assert res.nan.tolist() == [[0, 0, 0]] and res.valid.tolist() == [True]
    # region 1 (class 1, area 3): bins 3, 1, 2 -> suffix 3, 3, 2, 1; region 2 (class 2, area 1): bin 2 -> suffix 1, 1, 1, 0
    assert res.n_regions.tolist() == [[1, 1]]
    assert res.pro_sum[0].tolist() == [[1.0, 1.0, 2 / 3, 1 / 3], [1.0, 1.0, 1.0, 0.0]]
    s = res.summary(ece_bins=4)
    # class 1: pairs (pos, neg): 3 x 2, the 0.3 / 0.3 pair ties: (5 + 0.5) / 6
    assert s["per_class"][1]["AUROC"] == pytest.approx(5.5 / 6, rel=1e-15) and s["per_class"][2]["AUROC"] == 1.0
    assert s["AUROC"] == pytest.approx((5.5 / 6 + 1.0) / 2, rel=1e-15)
    # class 1 AP, descending bins: (tp 1, fp 0), (2, 0), (3, 1), (3, 2) -> 1/3 + 1/3 + 1/3 * 3/4
    assert s["per_class"][1]["AP"] == pytest.approx(2 / 3 + 0.25, rel=1e-15) and s["per_class"][2]["AP"] == 1.0
    assert s["per_class"][1]["F1"] == pytest.approx(2 * 3 / (2 * 3 + 1 + 0)) and s["per_class"][1]["F1_threshold"] == 0.25
    assert s["top_accuracy"] == 0.8 and s["images"] == 1 and s["images_skipped"] == 0
    conf = lambda *v: q(*v) / 16777216.0 / len(v)
    gaps = [(1, abs(0.0 - conf(0.3))), (3, abs(1.0 - conf(0.7, 0.5, 0.5))), (1, abs(1.0 - conf(0.8)))]
    assert s["ECE"] == pytest.approx(sum(n / 5 * g for n, g in gaps), rel=1e-14) and s["MCE"] == pytest.approx(max(g for _, g in gaps))
    assert [r["n"] for r in s["reliability"]] == [0, 1, 3, 1] and math.isnan(s["reliability"][0]["accuracy"])
    # class 2 AUPRO: FPR of "bin >= i" for i = 4 .. 0: 0, 0, 0, 1/4, 1; PRO: 0, 0, 1, 1, 1 -> the area up to 0.3 is 0.3
    assert s["per_class"][2]["AUPRO"] == pytest.approx(1.0, rel=1e-14)


def test_bin_rule_on_edge_scores():
    from uaps_amd import curves, score_curves
    e = CR.edge_values()
    for bins in (2, 15, 1024, 4096):
        got = curves.bin_index(e, bins)
        want = [CR.bin_scalar(v, bins) for v in e]
        assert got.tolist() == [-1 if w is None else w for w in want]
        # exactly: a product of two fp32 values is exact in float64, so one rounding to fp32 is the correctly rounded fp32 product
        inv = F32(bins) / F32(1)
        fin = e[np.isfinite(e)]
        with np.errstate(over="ignore"):
            exact = np.clip(np.floor((fin.astype(np.float64) * np.float64(inv)).astype(F32)), 0, bins - 1).astype(np.int64)
        assert curves.bin_index(fin, bins).tolist() == exact.tolist()
    assert curves.bin_index(F32(1.0), 1024) == 1023 and curves.bin_index(np.nextafter(F32(1), F32(0)), 1024) == 1023
    assert curves.bin_index((np.arange(1024) / 1024).astype(F32), 1024).tolist() == list(range(1024))          # a power of two: exact
    assert curves.bin_index(np.nextafter(F32(0.5), F32(0)), 1024) == 511 and curves.bin_index(F32(0.5), 1024) == 512
    assert curves.bin_index(np.array([np.inf, -np.inf, -0.0, 1e-45, 7.0, -7.0], dtype=F32), 15).tolist() == [14, 0, 0, 0, 14, 0]
    assert curves.bin_index(F32(np.nan), 15) == -1
    for lo, hi in ((-2.5, 7.0), (0.25, 0.26)):
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.concatenate([e, (e * F32(hi - lo) + F32(lo)).astype(F32)])
        want = [CR.bin_scalar(x, 15, lo, hi) for x in v]
        assert curves.bin_index(v, 15, lo, hi).tolist() == [-1 if w is None else w for w in want]
    # through the public function: one pixel per edge value, class 1 everywhere
    S = np.stack([np.zeros_like(e), e])[None, :, None, :]
    res = score_curves(_t(S), torch.ones((1, 1, len(e)), dtype=torch.int64), bins=15, top=False)
    idx = curves.bin_index(e, 15)
    assert res.hist[0, 0, 1].tolist() == np.bincount(idx[idx >= 0], minlength=15).tolist() and int(res.hist[0, 0, 0].sum()) == 0
    assert res.nan.tolist() == [[int(np.isnan(e).sum())]]


def test_ignore_rule():
    from uaps_amd import plane_curves, score_curves
    S = CR.scores("uniform", (1, 1, 45), 4)
    t = np.full((1, 1, 45), 4, dtype=np.int64)
    t[0, 0, :5] = [-1, 255, 0, 3, 1]
    res = score_curves(_t(S), _t(t), bins=15)
    assert res.hist.sum(dim=(2, 3)).tolist() == [[3, 3, 3, 3]]                 # three counted pixels in every row
    S2 = S.copy()
    S2[0, :, 0, 0] = np.nan                                                     # a NaN on an ignored pixel is not counted
    S2[0, 2, 0, 2] = np.nan                                                     # class 2's score of a counted pixel: row 1 and the top row
    res = score_curves(_t(S2), _t(t), bins=15)
    assert res.nan.tolist() == [[0, 1, 0, 1]] and res.hist.sum(dim=(2, 3)).tolist() == [[3, 2, 3, 2]]
    for dt in (torch.uint8, torch.int32, torch.int16, torch.bool):
        tt = _t(t).clamp(0, 1).to(dt)
        assert torch.equal(score_curves(_t(S), tt, bins=15).hist, score_curves(_t(S), _t(t).clamp(0, 1), bins=15).hist)
    p = plane_curves(_t(S[:, 0]), torch.zeros((1, 1, 45), dtype=torch.int64), _t(t) - 4, bins=15)        # targets -5, 251, -4, -1, -3, 0 ...
    assert int(p.hist.sum()) == 41 and int(p.hist[0, 0, 1].sum()) == 40 and p.plane and p.classes == ()


def test_ties_of_the_arg_max_take_the_lowest_index():
    from uaps_amd import score_curves
    S = np.full((1, 3, 1, 3), 0.25, dtype=F32)
    S[0, :, 0, 1] = [0.1, 0.4, 0.4]
    S[0, :, 0, 2] = [0.4, 0.1, 0.4]
    res = score_curves(_t(S), _t([[[0, 1, 2]]]), bins=4, classes=[])
    assert res.hist[0, 0].tolist() == [[0, 1, 0, 0], [0, 2, 0, 0]]             # 0 == 0 right, 1 == 1 right, pixel 2: arg-max 0, wrong
    z = np.log(S) + F32(3.0)
    res = score_curves(_t(z), _t([[[0, 1, 2]]]), bins=4, classes=[], from_logits=True)
    assert res.hist[0, 0].sum(dim=1).tolist() == [1, 2]


def test_sigmoid_head():
    from uaps_amd import score_curves
    p = np.array([[[[0.1, 0.6, 0.5, 0.9, 0.3, 0.7]]]], dtype=F32)
    t = _t([[[0, 1, 1, 0, 2, -1]]])
    res = score_curves(_t(p), t, bins=4)
    assert res.classes == (1,)
    assert res.hist[0, 0].tolist() == [[1, 0, 0, 1], [0, 0, 2, 0]]             # event target == 1
    # top: max(p, 1 - p) = 0.9, 0.6, 0.5, 0.9; (p > 0.5) == target: yes, yes, no (0.5 is not above), no
    assert res.hist[0, 1].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1]]
    z = np.log(p.astype(np.float64) / (1 - p.astype(np.float64))).astype(F32)
    z[0, 0, 0, 2] = 1e-3                                                        # z > 0: class 1, right
    res = score_curves(_t(z), t, bins=4, from_logits=True)
    assert res.hist[0, 0].tolist() == [[1, 0, 0, 1], [0, 0, 2, 0]] and res.hist[0, 1].tolist() == [[0, 0, 0, 1], [0, 0, 2, 1]]
    with pytest.raises(ValueError):
        score_curves(_t(p), t, classes=[0])


def test_scores_equal_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    from uaps_amd import curves, score_curves
    shape, Cn = (3, 37, 53), 4
    t = CR.targets(shape, Cn)
    rng = np.random.default_rng(5)
    S = CR.softmax64(3.0 * np.eye(Cn)[t].transpose(0, 3, 1, 2) + 2.0 * rng.standard_normal((3, Cn, 37, 53))).astype(F32)
    for bins in (15, 1024):
        s = score_curves(_t(S), _t(t), bins=bins, classes=[0, 1, 2, 3]).summary()
        for c in range(Cn):
            idx, y = curves.bin_index(S[:, c], bins).reshape(-1), (t == c).reshape(-1)
            assert s["per_class"][c]["AUROC"] == pytest.approx(skm.roc_auc_score(y, idx), abs=1e-12)
            assert s["per_class"][c]["AP"] == pytest.approx(skm.average_precision_score(y, idx), abs=1e-12)
            pr, rc, _ = skm.precision_recall_curve(y, idx)
            assert s["per_class"][c]["F1"] == pytest.approx(np.nanmax(2 * pr * rc / np.maximum(pr + rc, 1e-300)), abs=1e-12)
        assert s["AUROC"] == pytest.approx(np.mean([s["per_class"][c]["AUROC"] for c in range(Cn)]), rel=1e-15) and 0.7 < s["AUROC"] < 1


def test_aupro_of_a_perfect_and_of_a_random_predictor():
    from uaps_amd import label_instances, score_curves
    t, reg = CR.region_case("blobs", (3, 37, 53), 4)
    perfect = np.eye(4, dtype=F32)[t].transpose(0, 3, 1, 2).copy()
    s = score_curves(_t(perfect), _t(t), regions=_inst(reg)).summary()
    assert s["AUPRO"] == 1.0 and s["AUROC"] == 1.0 and s["AP"] == 1.0 and all(v["AUPRO"] == 1.0 for v in s["per_class"].values() if v["regions"])
    # independent uniform scores: PRO = FPR in expectation, so the area up to fpr_limit is fpr_limit^2 / 2 and AUPRO -- that area
    # divided by fpr_limit -- is fpr_limit / 2: AUPRO / fpr_limit lies within 0.02 of 0.5 (0.1559 / 0.3 = 0.520 with this seed)
    rng = np.random.default_rng(11)
    tt = np.zeros((1, 336, 336), dtype=np.int64)                               # more than 10^5 negatives
    for k in range(40):
        y, x = rng.integers(0, 300, 2)
        tt[0, y:y + 8, x:x + 8] = 1
    S = rng.random((1, 2, 336, 336), dtype=F32)
    r = score_curves(_t(S), _t(tt), regions=label_instances(_t(tt)))
    s = r.summary()
    assert s["per_class"][1]["negatives"] > 10 ** 5 and s["per_class"][1]["regions"] > 20
    assert abs(s["AUPRO"] / 0.3 - 0.5) < 0.02 and abs(s["AUROC"] - 0.5) < 0.02
    wide = r.summary(fpr_limit=1.0)
    assert abs(wide["AUPRO"] / 1.0 - 0.5) < 0.02
    none = score_curves(_t(S), _t(tt)).summary()
    assert math.isnan(none["AUPRO"]) and none["AUROC"] == s["AUROC"]


def test_ece_and_aurc_on_hand_worked_histograms():
    from uaps_amd import curves
    one = 16777216
    # four fine bins over [0, 1], two groups.  group 0: 4 pixels, 1 right, confidences 0.1, 0.2, 0.3, 0.4; group 1: 6 pixels, 3 right,
    # confidences 0.5 x 2, 0.75 x 2, 1.0 x 2
    false, true = [2, 1, 1, 2], [0, 1, 1, 2]
    qf, qt = [int(0.3 * one), int(0.4 * one), int(0.5 * one), int(1.75 * one)], [0, int(0.3 * one), int(0.5 * one), int(1.75 * one)]
    c = curves.calibration(false, true, qf, qt, 0.0, 1.0, ece_bins=2)
    conf0, conf1 = (qf[0] + qf[1] + qt[1]) / one / 4, (qf[2] + qf[3] + qt[2] + qt[3]) / one / 6
    assert c["ECE"] == pytest.approx(0.4 * abs(0.25 - conf0) + 0.6 * abs(0.5 - conf1), rel=1e-15)
    assert c["MCE"] == pytest.approx(max(abs(0.25 - conf0), abs(0.5 - conf1)), rel=1e-15)
    assert [r["n"] for r in c["reliability"]] == [4, 6] and c["reliability"][1]["lo"] == 0.5 and c["reliability"][0]["accuracy"] == 0.25
    with pytest.raises(ValueError):
        curves.calibration(false, true, qf, qt, 0.0, 1.0, ece_bins=3)
    # risk-coverage, ascending score: bin 0: 4 right; bin 1 empty; bin 2: 2 right, 2 wrong; bin 3: 2 wrong
    false, true = [0, 0, 2, 2], [4, 0, 2, 0]
    assert curves.aurc(false, true) == pytest.approx(0.4 * 0.0 + 0.4 * (2 / 8) + 0.2 * (4 / 10), rel=1e-15)
    # error detection: "wrong" is the positive class.  pairs (wrong, right): 4 x 6 = 24; a wrong pixel of bin 2 beats the 4 rights of
    # bin 0 and ties with 2: 2 x (4 + 1); one of bin 3 beats all 6: 2 x 6
    assert curves.auroc(false, true) == pytest.approx((2 * 5 + 2 * 6) / 24, rel=1e-15)
    assert math.isnan(curves.aurc([0, 0], [0, 0])) and math.isnan(curves.auroc([0, 0], [1, 2])) and math.isnan(curves.average_precision([0], [3]))
    # through plane_curves and its summary
    from uaps_amd import plane_curves
    score = _t(np.array([[[0.1] * 4 + [0.6] * 4 + [0.9] * 2]], dtype=F32))
    pred = _t([[[1, 1, 1, 1, 1, 1, 0, 0, 0, 0]]])
    s = plane_curves(score, pred, torch.ones((1, 1, 10), dtype=torch.int64), bins=4).summary()
    assert s["AURC"] == pytest.approx(0.4 * (2 / 8) + 0.2 * (4 / 10), rel=1e-15) and s["AUROC"] == pytest.approx(22 / 24, rel=1e-15) and s["error_rate"] == 0.4


def test_sums_of_two_batches_equal_the_concatenated_batch():
    from uaps_amd import CurveSums, score_curves
    shape, Cn = (3, 37, 53), 4
    ta, ra = CR.region_case("blobs", shape, Cn)
    tb, rb = CR.region_case("noise", shape, Cn)                                 # its images overflow: left out of the sums
    Sa, Sb = CR.scores("uniform", shape, Cn), CR.scores("nans", shape, Cn)
    a = score_curves(_t(Sa), _t(ta), bins=15, regions=_inst(ra), want_sums=True)
    b = score_curves(_t(Sb), _t(tb), bins=15, regions=_inst(rb), want_sums=True)
    both = score_curves(_t(np.concatenate([Sa, Sb])), _t(np.concatenate([ta, tb])), bins=15, want_sums=True,
                        regions=_inst(tuple(np.concatenate([x, y]) for x, y in zip(ra, rb))))
    assert a.valid.all() and not b.valid.any()
    x, y = a.sums() + b.sums(), both.sums()
    assert isinstance(x, CurveSums) and x.images.tolist() == [3, 6] == y.images.tolist()
    for name in ("hist", "qsum", "nan", "n_regions"):
        assert torch.equal(getattr(x, name), getattr(y, name)), name
    assert torch.allclose(x.pro_sum, y.pro_sum, rtol=1e-12, atol=0)
    assert torch.equal(x.hist, a.hist.sum(0)) and int(x.hist.sum()) > 0
    with pytest.raises(ValueError):
        a.sums() + score_curves(_t(Sa), _t(ta), bins=15).sums()


def test_overflow_marks_the_image_and_summary_skips_it():
    from uaps_amd import label_instances, score_curves
    m = np.concatenate([R.checkerboard(9, 11), R.checkerboard(9, 11) * 0])
    m[1, 2:5, 2:5] = 1
    S = CR.scores("uniform", (2, 9, 11), 2)
    reg = label_instances(_t(m), connectivity=4, max_instances=16)             # 50 one-pixel regions in image 0
    res = score_curves(_t(S), _t(m), bins=15, regions=reg)
    assert res.valid.tolist() == [False, True]
    CR.assert_result(res, CR.curves(S, m, bins=15, regions=R.label_batch(m, (), 4, 0, 1, 16)))
    assert res.n_regions.tolist() == [[16], [1]]                               # the in-table regions of the overflowed image are still counted
    s = res.summary()
    assert (s["images"], s["images_skipped"]) == (1, 1) and s["per_class"][1]["positives"] == 9 and s["per_class"][1]["regions"] == 1
    assert s == score_curves(_t(S[1:]), _t(m[1:]), bins=15, regions=label_instances(_t(m[1:]), connectivity=4)).summary() | {"images_skipped": 1}


def test_refusals():
    from uaps_amd import label_instances, plane_curves, score_curves
    S, t = torch.rand(2, 3, 4, 4), torch.zeros((2, 4, 4), dtype=torch.int64)
    for kw in ({"bins": 1}, {"bins": 4097}, {"classes": [3]}, {"classes": [-1]}, {"classes": [], "top": False}, {"classes": [1] * 9}):
        with pytest.raises(ValueError):
            score_curves(S, t, **kw)
    for bad_s, bad_t in ((S.double(), t), (S[0], t), (S, t[:1]), (S, t[:, :3]), (torch.rand(2, 9, 4, 4), t), (S.to("meta"), t)):
        with pytest.raises(ValueError):
            score_curves(bad_s, bad_t)
    with pytest.raises(TypeError):
        score_curves(S, t.float())
    with pytest.raises(TypeError):
        score_curves(S, t, regions=t)
    with pytest.raises(ValueError):
        score_curves(S, t, regions=label_instances(torch.zeros((2, 4, 5), dtype=torch.int64)))
    with pytest.raises(ValueError, match="max_instances"):
        from uaps_amd import InstanceResult
        r = label_instances(t)
        score_curves(S, t, bins=4096, regions=InstanceResult(r.labels, r.count, torch.zeros((2, 65536, 9), dtype=torch.int64)))
    p = torch.rand(2, 4, 4)
    for kw in ({"bins": 1}, {"lo": 1.0, "hi": 1.0}, {"lo": 2.0}, {"hi": float("inf")}, {"lo": float("nan")}, {"lo": 0.0, "hi": 1e-44}):
        with pytest.raises(ValueError):
            plane_curves(p, t, t, **kw)
    with pytest.raises(ValueError):
        plane_curves(p, t[:1], t)
    with pytest.raises(ValueError):
        plane_curves(S, t, t)
    with pytest.raises(ValueError):
        score_curves(S, t, bins=16, want_sums=True).summary(ece_bins=5)
    assert score_curves(S, t, bins=4096, classes=[0, 1, 2]).hist.shape == (2, 4, 2, 4096)


class Stub(torch.nn.Module):
    """A seeded 1x1 convolution with `heads` outputs: a "network" that runs at any size."""

    def __init__(self, cin, classes, heads=1):
        super().__init__()
        torch.manual_seed(3)
        self.convs = torch.nn.ModuleList([torch.nn.Conv2d(cin, classes, 1) for _ in range(heads)])

    def forward(self, x):
        out = tuple(4.0 * c(x) for c in self.convs)
        return out if len(out) > 1 else out[0]


def _host_confusion(scored, labels):
    B, Cc = scored.shape[:2]
    return torch.stack([torch.bincount(labels[b].flatten() * Cc + scored[b].argmax(0).flatten(), minlength=Cc * Cc).view(Cc, Cc)
                        for b in range(B)])


def _host_uncertainty(main, aux):
    """consistency.uncertainty_map needs the GPU: sum_c KLDivLoss('none')(log_softmax(main), softmax(aux))."""
    q = torch.softmax(aux, dim=1)
    return (q * (torch.log(q) - torch.log_softmax(main, dim=1))).sum(dim=1)


def test_evaluate_with_curves_around_a_stub(monkeypatch):
    from uaps_amd import consistency, curves, inference, label_instances, metrics, plane_curves, score_curves
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    monkeypatch.setattr(consistency, "uncertainty_map", _host_uncertainty)
    net = Stub(3, 4, heads=2)
    gen = torch.Generator().manual_seed(2)
    smooth = lambda v: torch.nn.functional.avg_pool2d(v, 5, 1, 2)
    batches = []
    for _ in range(2):
        x = smooth(torch.randn(2, 3, 24, 31, generator=gen))
        with torch.no_grad():
            y = (net(x)[0] + 0.6 * smooth(torch.randn(2, 4, 24, 31, generator=gen))).argmax(1)
        batches.append((x, y))
    plain = inference.evaluate(net, batches)
    out = inference.evaluate(net, batches, curves=True)
    new = {"AUROC(%)", "AP(%)", "AUPRO(%)", "ECE(%)", "curve_images_skipped"}
    assert list(out)[:4] == list(plain) and all(out[k] == plain[k] for k in plain) and set(out) - set(plain) == new

    def by_hand(bins=1024, classes=None, fpr_limit=0.3, ece_bins=16, **lab):
        total = None
        with torch.no_grad():
            for x, y in batches:
                part = score_curves(net(x)[0], y, bins=bins, classes=classes, from_logits=True, regions=label_instances(y, **lab),
                                    want_sums=True).sums()
                total = part if total is None else total + part
        return curves.summarize(total, [1, 2, 3] if classes is None else classes, fpr_limit=fpr_limit, ece_bins=ece_bins)
    s = by_hand()
    assert out["curve_images_skipped"] == 0 and 50 < out["AUROC(%)"] <= 100 and 0 <= out["ECE(%)"] < 100 and 0 < out["AUPRO(%)"] <= 100
    for key in ("AUROC", "AP", "AUPRO", "ECE"):
        assert out[key + "(%)"] == pytest.approx(100 * s[key], rel=1e-12, nan_ok=True), key
    kw = {"bins": 64, "fpr_limit": 0.1, "ece_bins": 8, "classes": [2], "max_instances": 64, "connectivity": 4, "min_area": 3}
    one = inference.evaluate(net, batches, curves=kw)
    s = by_hand(**kw)
    for key in ("AUROC", "AP", "AUPRO", "ECE"):
        assert one[key + "(%)"] == pytest.approx(100 * s[key], rel=1e-12, nan_ok=True), key
    assert one["AUPRO(%)"] != out["AUPRO(%)"]
    assert inference.evaluate(net, batches, curves={"max_instances": 1})["curve_images_skipped"] > 0
    unc = inference.evaluate(net, batches, curves={"uncertainty": True, "hi": 2.0})
    assert set(unc) - set(out) == {"UncAUROC(%)", "AURC"} and all(unc[k] == out[k] for k in out)
    total = None
    with torch.no_grad():
        for x, y in batches:
            main, aux = net(x)
            part = plane_curves(_host_uncertainty(main, aux), main.argmax(1), y, hi=2.0).sums()
            total = part if total is None else total + part
    u = curves.summarize(total, (), hi=2.0, plane=True)
    assert unc["UncAUROC(%)"] == pytest.approx(100 * u["AUROC"], rel=1e-12) and unc["AURC"] == pytest.approx(u["AURC"], rel=1e-12)
    assert 0 < unc["AURC"] < 1
    assert inference.evaluate(net, batches, curves=None) == plain == inference.evaluate(net, batches, curves=False)
    assert repr(inference.evaluate(net, batches, curves={})) == repr(out)                  # an empty dict: the defaults, not "off"
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, curves={"percentile": 95})
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, curves=0.5)
    with pytest.raises(ValueError):
        inference.evaluate(net, batches, curves={"uncertainty": True}, tta=(1.0,))
    with pytest.raises(ValueError):
        inference.evaluate(net, batches, curves={"uncertainty": True}, tiled=True)
    with pytest.raises(ValueError, match="auxiliary"):
        inference.evaluate(Stub(3, 4), batches, curves={"uncertainty": True})


def _fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    return names


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_curves_workspace_bytes", "uaps_score_curves", "uaps_plane_curves"}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uaps_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    assert _fields(hdr, "uaps_curves_call") == [f[0] for f in _lib.CurvesCall._fields_]
    assert _fields(hdr, "uaps_plane_curves_call") == [f[0] for f in _lib.PlaneCurvesCall._fields_]
    assert "#define UAPS_CURVES_MAX_BINS 4096" in hdr and _lib.CURVES_MAX_BINS == 4096
    # the library reads exactly up to `stream`: a struct 8 bytes shorter is refused, a longer one (a later header's) passes the size check
    assert _lib.CurvesCall.stream.offset + 8 == C.sizeof(_lib.CurvesCall) and _lib.PlaneCurvesCall.stream.offset + 8 == C.sizeof(_lib.PlaneCurvesCall)
    L = _lib.lib()
    assert L.uaps_score_curves(_call(C=0)) == ERANGE
    assert L.uaps_score_curves(_call(C=0, struct_size=C.sizeof(_lib.CurvesCall) - 8)) == EINVAL
    assert L.uaps_score_curves(_call(C=0, struct_size=C.sizeof(_lib.CurvesCall) + 64)) == ERANGE
    assert L.uaps_plane_curves(_plane(bins=1, struct_size=C.sizeof(_lib.PlaneCurvesCall) + 64)) == ERANGE
    assert L.uaps_plane_curves(_plane(bins=1, struct_size=C.sizeof(_lib.PlaneCurvesCall) - 8)) == EINVAL


def _call(regions=False, **kw):
    from uaps_amd import _lib
    c = _lib.CurvesCall()
    c.struct_size = C.sizeof(_lib.CurvesCall)
    c.B, c.C, c.H, c.W, c.bins, c.from_logits, c.top_row, c.n_classes = 1, 4, 8, 8, 16, 0, 1, 2
    c.classes[0], c.classes[1] = 1, 3
    c.target_dtype, c.lo, c.hi = 8, 0.0, 1.0
    # never dereferenced: every call below returns before a launch
    c.scores = c.target = c.hist = c.qsum = c.nan = 4096
    if regions:
        c.region_labels = c.region_count = c.region_table = c.pro_sum = c.n_regions = c.workspace = 4096
        c.max_regions, c.workspace_bytes = 8, 1 << 40
    for k, v in kw.items():
        if k == "classes":
            for i, x in enumerate(v):
                c.classes[i] = x
        else:
            setattr(c, k, v)
    return C.byref(c)


def _plane(**kw):
    from uaps_amd import _lib
    c = _lib.PlaneCurvesCall()
    c.struct_size = C.sizeof(_lib.PlaneCurvesCall)
    c.B, c.H, c.W, c.bins, c.from_logits, c.pred_dtype, c.target_dtype, c.lo, c.hi = 1, 8, 8, 16, 0, 8, 8, 0.0, 1.0
    c.score = c.pred = c.target = c.hist = c.qsum = c.nan = 4096
    for k, v in kw.items():
        setattr(c, k, v)
    return C.byref(c)


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    n = C.c_size_t()
    ws = L.uaps_curves_workspace_bytes
    assert ws(16, 256, 1024, C.byref(n)) == 0 and n.value == 16 * 256 * 1024 * 4
    assert ws(1, 1, 2, C.byref(n)) == 0 and n.value == 256
    assert ws(3, 0, 15, C.byref(n)) == 0 and n.value == 0                                    # no regions: no workspace
    assert ws(3, 300, 15, C.byref(n)) == 0 and n.value >= 3 * 300 * 15 * 4 and n.value % 256 == 0
    assert ws(1, 8, 16, None) == EINVAL and ws(0, 8, 16, C.byref(n)) == EINVAL and ws(1, -1, 16, C.byref(n)) == EINVAL
    assert ws(1, 8, 1, C.byref(n)) == ERANGE and ws(1, 8, 4097, C.byref(n)) == ERANGE
    assert ws(2, 65536, 4096, C.byref(n)) == ERANGE and ws(2, 65535, 4096, C.byref(n)) == 0     # 2 GiB exactly
    run = L.uaps_score_curves
    assert run(None) == EINVAL
    for field in ("scores", "target", "hist", "nan"):
        assert run(_call(**{field: None})) == EINVAL, field
    assert run(_call(struct_size=0)) == EINVAL and run(_call(struct_size=C.sizeof(_lib.CurvesCall) - 8)) == EINVAL
    for dim in ("B", "H", "W"):
        assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL, dim
    for flag in ("from_logits", "top_row"):
        assert run(_call(**{flag: 2})) == EINVAL and run(_call(**{flag: -1})) == EINVAL, flag
    assert run(_call(target_dtype=2)) == EINVAL
    assert run(_call(n_classes=0, top_row=0)) == EINVAL and run(_call(n_classes=9)) == EINVAL and run(_call(n_classes=-1)) == EINVAL
    assert run(_call(classes=[1, 4])) == EINVAL and run(_call(classes=[-1, 1])) == EINVAL
    assert run(_call(C=1, n_classes=1, classes=[0])) == EINVAL                               # the sigmoid head scores class 1
    for lo, hi in ((1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (0.0, 1e-44)):
        assert run(_call(lo=lo, hi=hi)) == EINVAL, (lo, hi)
    for field in ("region_labels", "region_count", "region_table", "pro_sum", "n_regions", "workspace"):
        assert run(_call(regions=True, **{field: None})) == EINVAL, field
    assert run(_call(region_count=4096)) == EINVAL and run(_call(max_regions=4)) == EINVAL   # a part of the regions alone
    assert run(_call(regions=True, max_regions=0)) == EINVAL
    assert run(_call(regions=True, workspace_bytes=8 * 16 * 4 - 1)) == EINVAL                # too small
    assert run(_call(regions=True, workspace=4096 + 128)) == EINVAL                          # not 256-byte aligned
    assert run(_call(C=0)) == ERANGE and run(_call(C=9)) == ERANGE
    assert run(_call(bins=1)) == ERANGE and run(_call(bins=4097)) == ERANGE and run(_call(bins=0)) == ERANGE
    assert run(_call(H=65536, W=32768)) == ERANGE                                            # H * W = 2^31
    assert run(_call(B=2, H=8192, W=8192)) == ERANGE                                         # 2 * 4 * 2^26 * 4 bytes of scores
    assert run(_call(B=4096, H=256, W=256, C=1, n_classes=1, classes=[1])) == ERANGE         # int64 labels: 2^28 * 8 bytes
    assert run(_call(B=32768, H=1, W=1, bins=4096, n_classes=1)) == ERANGE                   # hist: 2^15 * 2 * 2 * 4096 * 8 bytes
    assert run(_call(regions=True, B=2, bins=4096, max_regions=65536)) == ERANGE             # the region histograms reach 2 GiB
    run = L.uaps_plane_curves
    assert run(None) == EINVAL
    for field in ("score", "pred", "target", "hist", "nan"):
        assert run(_plane(**{field: None})) == EINVAL, field
    assert run(_plane(struct_size=0)) == EINVAL
    for dim in ("B", "H", "W"):
        assert run(_plane(**{dim: 0})) == EINVAL, dim
    assert run(_plane(from_logits=1)) == EINVAL and run(_plane(pred_dtype=3)) == EINVAL and run(_plane(target_dtype=0)) == EINVAL
    for lo, hi in ((1.0, 1.0), (2.0, -2.0), (float("nan"), 1.0), (0.0, float("inf"))):
        assert run(_plane(lo=lo, hi=hi)) == EINVAL, (lo, hi)
    assert run(_plane(bins=1)) == ERANGE and run(_plane(bins=4097)) == ERANGE
    assert run(_plane(H=65536, W=32768)) == ERANGE and run(_plane(B=8, H=8192, W=8192)) == ERANGE

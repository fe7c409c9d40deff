"""Hand-worked detection figures, run by tests/test_detect_host.py on the CPU path and by tests/test_gpu_detect.py on the device.
`run(pred mask, gt mask, confidence, num_classes, **keywords of detection_match)` labels both masks (8-connectivity, 16 rows against 12)
and returns the DetectionResult; `scores` is passed as a list of per-label values and placed by `run`.  Every expectation below was
worked out by hand from the rule, none was read off the code."""
import math

import numpy as np
from pytest import approx

import detect_ref as D

INF = float("inf")


def _tables(res):
    g = lambda t: t.cpu().numpy()
    return g(res.score), g(res.rank), g(res.pred_match), g(res.target_match), g(res.counts)


def full_candidate_list(run):
    """One 2 x 20 prediction (area 40) over ten touching 2 x 2 ground-truth tiles of alternating classes: every intersection is 4, every
    union 40 + 4 - 4 = 40, every IoU exactly 1/10 -- ten candidates, all tied; the lowest number is taken at 0.1, nothing at 0.101."""
    boxes_g = [(1 + k % 2, 1, 1 + 2 * k, 3, 3 + 2 * k) for k in range(10)]
    pred, gt, conf = D.figure([(1, 1, 1, 3, 21)], boxes_g, (4, 23))
    res = run(pred, gt, conf, 3, iou_thresholds=(0.1, 0.101, 0.2), class_agnostic=True)
    score, rank, pm, tm, counts = _tables(res)
    assert pm[0, 0].tolist() == [1, 0, 0] and rank[0, 0] == 0 and rank[0, 1] == -1
    assert tm[0, :10].tolist() == [[1, 0, 0]] + [[0, 0, 0]] * 9
    assert counts[0].tolist() == [[1, 0, 0, 1, 10], [0] * 5, [0] * 5]          # class_agnostic: everything is class 0
    assert res.iou()[0, 0].tolist() == [0.1, 0.0, 0.0] and res.pred_inter[0, 0].tolist() == [4, 0, 0]
    assert score[0, 0] == 0.5 * 16777216.0                                     # float64(sum0) / float64(area): the 2^24 scale is kept
    # class-aware: only the five tiles of class 1 are candidates, each still at 1/10
    res = run(pred, gt, conf, 3, iou_thresholds=(0.1, 0.2))
    assert res.pred_match[0, 0].tolist() == [1, 0] and res.counts[0].tolist() == [[0] * 4, [1, 0, 1, 5], [0, 0, 0, 5]]


def three_candidates(run):
    """A 2 x 20 prediction over three 2 x 6 tiles one column apart: intersections 12, unions 40, IoU 0.3 each."""
    pred, gt, conf = D.figure([(2, 0, 0, 2, 20)], [(2, 0, 0, 2, 6), (2, 0, 7, 2, 13), (2, 0, 14, 2, 20)], (2, 20))
    res = run(pred, gt, conf, 3, iou_thresholds=(0.1, 0.3, 0.301))
    assert res.pred_match[0, 0].tolist() == [1, 1, 0] and res.target_match[0, :3].tolist() == [[1, 1, 0], [0, 0, 0], [0, 0, 0]]
    assert res.counts[0, 2].tolist() == [1, 1, 0, 1, 3] and res.iou()[0, 0].tolist() == [0.3, 0.3, 0.0]


def _two_on_one():
    """G1 = columns 0..9, G2 = columns 11..16 of one row; P1 = columns 0..2 (IoU 3/10 with G1), P2 = columns 5..13 (5/14 with G1, 3/12
    with G2).  3/10 + 5/14 < 1, as it must be."""
    return [(1, 0, 0, 1, 3), (1, 0, 5, 1, 14)], [(1, 0, 0, 1, 10), (1, 0, 11, 1, 17)]


THR_TWO = (0.1, 0.25, 0.3, 0.35)
# P1 first: it takes G1 wherever 3/10 passes (0.3 included: COCO's >=), P2 falls back on G2 wherever 1/4 passes (0.25 included)
WAY_A = {"pm": [[1, 1, 1, 0], [2, 2, 0, 1]], "tm": [[1, 1, 1, 2], [2, 2, 0, 0]], "tp": [2, 2, 1, 1], "rank": [0, 1]}
# P2 first: it takes G1, its largest IoU, everywhere; P1 has no other candidate
WAY_B = {"pm": [[0, 0, 0, 0], [1, 1, 1, 1]], "tm": [[2, 2, 2, 2], [0, 0, 0, 0]], "tp": [1, 1, 1, 1], "rank": [1, 0]}


def _is_way(res, way, what):
    _, rank, pm, tm, counts = _tables(res)
    assert pm[0, :2].tolist() == way["pm"] and tm[0, :2].tolist() == way["tm"], (what, pm[0, :2], tm[0, :2])
    assert counts[0, 1].tolist() == way["tp"] + [2, 2] and rank[0, :2].tolist() == way["rank"], (what, counts[0, 1], rank[0, :2])


def two_predictions_on_one_defect(run):
    bp, bg = _two_on_one()
    pred, gt, conf = D.figure(bp, bg, (1, 17), scores_map=(0.75, 0.25))
    res = run(pred, gt, conf, 2, iou_thresholds=THR_TWO)
    _is_way(res, WAY_A, "P1 scored higher")
    assert res.score[0, :2].tolist() == [0.75 * 2 ** 24, 0.25 * 2 ** 24]
    assert res.iou()[0, 1].tolist() == [3 / 12, 3 / 12, 0.0, 5 / 14]
    pred, gt, conf = D.figure(bp, bg, (1, 17), scores_map=(0.25, 0.75))
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO), WAY_B, "P2 scored higher")


def ordering(run):
    bp, bg = _two_on_one()
    pred, gt, conf = D.figure(bp, bg, (1, 17))                                  # equal confidence: the lower label first
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO), WAY_A, "tie")
    res = run(pred, gt, conf, 2, iou_thresholds=THR_TWO, scores=np.array([math.nan, -INF]))
    _is_way(res, WAY_B, "NaN after -inf")
    assert res.score[0, :2].tolist() == [-INF, -INF]
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO, scores=np.array([math.nan, math.nan])), WAY_A, "NaN tie")
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO, scores=np.array([-0.0, 0.0])), WAY_A, "-0 ties with 0")
    # the float32 values tie; read as float64 the second is one float32 step larger
    step = float(np.nextafter(np.float32(0.3), np.float32(1)))
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO, scores=np.array([0.3, 0.3], dtype=np.float32)), WAY_A, "fp32 tie")
    res = run(pred, gt, conf, 2, iou_thresholds=THR_TWO, scores=np.array([0.3, step], dtype=np.float32))
    _is_way(res, WAY_B, "fp32 step")
    assert res.score[0, :2].tolist() == [float(np.float32(0.3)), step]
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO, scores=np.array([0.3, 0.3 + 2 ** -52], dtype=np.float64)), WAY_B, "fp64 step")
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO, scores=np.array([0.3 + 2 ** -52, 0.3], dtype=np.float64)), WAY_A, "fp64 step")


def max_dets(run):
    bp, bg = _two_on_one()
    pred, gt, conf = D.figure(bp, bg, (1, 17), scores_map=(0.75, 0.25))
    _is_way(run(pred, gt, conf, 2, iou_thresholds=THR_TWO, max_dets=2), WAY_A, "max_dets 2")
    res = run(pred, gt, conf, 2, iou_thresholds=THR_TWO, max_dets=1)            # P2 is cut: neither TP nor FP
    _, rank, pm, tm, counts = _tables(res)
    assert rank[0, :2].tolist() == [0, -1] and pm[0, :2].tolist() == [[1, 1, 1, 0], [0, 0, 0, 0]]
    assert tm[0, :2].tolist() == [[1, 1, 1, 0], [0, 0, 0, 0]] and counts[0, 1].tolist() == [1, 1, 1, 0, 1, 2]
    s = res.summary()
    assert s["n_pred"] == 1 and s["n_gt"] == 2


def hand_worked_ap(run):
    """One class, two defects, three detections scored 0.9 (on G1), 0.8 (on nothing), 0.7 (on G2): recall 1/2, 1/2, 1, precision
    1, 1/2, 2/3 -> 1, 2/3, 2/3 from the right; the 51 recall levels 0 .. 0.50 read 1, the 50 levels 0.51 .. 1 read 2/3:
    AP = (51 + 100/3) / 101 = 253/303, AR = 1."""
    boxes = [(1, 0, 0, 2, 3), (1, 0, 5, 2, 8), (1, 0, 10, 2, 13)]
    pred, gt, conf = D.figure(boxes, [boxes[0], boxes[2]], (2, 13), scores_map=(0.9, 0.8, 0.7))
    res = run(pred, gt, conf, 2, iou_thresholds=(0.5, 0.75, 1.0))
    assert res.pred_match[0, :3].tolist() == [[1, 1, 1], [0, 0, 0], [2, 2, 2]] and res.counts[0, 1].tolist() == [2, 2, 2, 3, 2]
    s = res.summary()
    for k in ("mAP", "AP50", "AP75"):
        assert s[k] == approx(253 / 303, rel=1e-12), k
    assert s["AR"] == 1.0 and s["per_class"][1]["AP_at"] == approx([253 / 303] * 3, rel=1e-12)
    assert (s["n_gt"], s["n_pred"], s["images"], s["images_skipped"]) == (2, 3, 1, 0)
    assert math.isnan(res.summary(classes=[0])["mAP"])                          # no ground truth of class 0
    rec = res.records()[0]
    assert [r["label"] for r in rec] == [1, 2, 3] and rec[2]["matched"] == [2, 2, 2] and rec[2]["iou"] == [1.0, 1.0, 1.0]
    assert rec[0]["score"] == approx(0.9, rel=1e-6) and rec[1]["rank"] == 1 and rec[1]["matched"] == [0, 0, 0]
    # at 1.0 only coinciding components match: the two-on-one figure matches nothing there
    bp, bg = _two_on_one()
    pred, gt, conf = D.figure(bp, bg, (1, 17))
    assert run(pred, gt, conf, 2, iou_thresholds=(1.0,)).counts[0, 1].tolist() == [0, 2, 2]


ALL = (full_candidate_list, three_candidates, two_predictions_on_one_defect, ordering, max_dets, hand_worked_ap)

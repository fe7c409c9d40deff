"""Defect detection scores on the GPU (csrc/detect.hip) against the literal reference (tests/detect_ref.py), the hand-worked figures
(tests/detect_figures.py) and the module's CPU path, behind the device's own label_instances.  Every integer table is compared exactly
and `score` bit for bit; the float64 figures of summary() are held to a relative 1e-12.

Shapes: the matching tests' set (one pixel a lane and four; one wave, several waves, several workgroups per image), 512 rows against
300 so that the strides differ; tables of 1, 3, 256 and 257 rows (order_kernel and sweep_kernel walk groups of 64: 256 fills four,
257 starts a fifth); one case with more than 3072 detections in an image, where a thread of order_kernel holds all of its four rows; T of
1, 10 and 32 thresholds, 0.1 and 1.0 among them."""
import numpy as np
import pytest
import torch

import detect_figures as F
import detect_ref as D
import instances_ref as R
import match_ref as M

pytestmark = pytest.mark.gpu
DEV = R.DEV


def _inst(ref, n_maps=0, dev=DEV):
    from uaps_amd import InstanceResult
    labels, count, table = ref
    return InstanceResult(torch.from_numpy(labels).to(dev), torch.from_numpy(count).to(dev), torch.from_numpy(table).to(dev), n_maps)


def _equal(a, b):
    same = all(torch.equal(getattr(a, n).cpu(), getattr(b, n).cpu()) for n in D.NAMES[1:] + ("valid",))
    return same and torch.equal(a.score.cpu().view(torch.int64), b.score.cpu().view(torch.int64))


def _device(pred, gt, conf, connectivity, mp, mg):
    """The device's own labelling in front: the whole path a user runs."""
    from uaps_amd import label_instances
    ip = label_instances(torch.from_numpy(pred).to(DEV), maps=(torch.from_numpy(conf).to(DEV),), connectivity=connectivity, max_instances=mp)
    return ip, label_instances(torch.from_numpy(gt).to(DEV), connectivity=connectivity, max_instances=mg)


def _run(pred, gt, conf, num_classes, scores=None, **kw):
    from uaps_amd import detection_match
    ip, ig = _device(pred, gt, conf, 8, 16, 12)
    if scores is not None:
        full = np.zeros((1, 16), dtype=scores.dtype)
        full[0, :len(scores)] = scores
        scores = torch.from_numpy(full).to(DEV)
    return detection_match(ip, ig, num_classes, scores=scores, **kw)


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_the_reference_and_the_cpu_path(shape):
    from uaps_amd import detection_match
    for name in ("noise", "blobs", "full_full", "full_empty", "empty_empty"):
        pred, gt, conf, ref_p, ref_g = D.case(name, shape, 8)
        ip, ig = _device(pred, gt, conf, 8, D.MP, D.MG)
        res = detection_match(ip, ig, 4)
        assert res.pred_match.is_cuda and res.pred_match.shape == (shape[0], D.MP, 10) and res.counts.shape == (shape[0], 4, 12)
        D.assert_tables(res, D.reference(name, shape, 8), f"{name} {shape}")
        assert _equal(res, detection_match(_inst(ref_p, 1, "cpu"), _inst(ref_g, 0, "cpu"), 4)), name
    pred, gt, conf, ref_p, ref_g = D.case("blobs", shape, 8)
    res = detection_match(*_device(pred, gt, conf, 8, D.MP, D.MG), 4, iou_thresholds=D.LOW, class_agnostic=True, max_dets=3)
    D.assert_tables(res, D.reference("blobs", shape, 8, D.LOW, True, 3), f"agnostic low {shape}")
    pred, gt, conf, ref_p, ref_g = D.case("blobs", shape, 4)
    res = detection_match(*_device(pred, gt, conf, 4, D.MP, D.MG), 4, iou_thresholds=D.T32)
    D.assert_tables(res, D.reference("blobs", shape, 4, D.T32), f"T32 {shape}")
    res = detection_match(*_device(pred, gt, conf, 4, D.MP, D.MG), 4, iou_thresholds=(0.5,))
    D.assert_tables(res, D.reference("blobs", shape, 4, (0.5,)), f"T1 {shape}")


@pytest.mark.parametrize("rows", (1, 3, 256, 257))
def test_table_sizes(rows):
    from uaps_amd import detection_match
    shape = (2, 130, 70)
    for name in ("blobs", "noise"):
        pred, gt, conf, ref_p, ref_g = D.case(name, shape, 8, rows, rows)
        res = detection_match(*_device(pred, gt, conf, 8, rows, rows), 4, iou_thresholds=D.LOW)
        D.assert_tables(res, D.reference(name, shape, 8, D.LOW, False, None, rows, rows), f"{name} {rows}")
    pred, gt, conf, ref_p, ref_g = D.case("blobs", shape, 8, rows, 300)        # a dozen blobs: 1 and 3 rows overflow, 256 and 257 do not
    res = detection_match(*_device(pred, gt, conf, 8, rows, 300), 4, iou_thresholds=D.LOW, class_agnostic=True)
    D.assert_tables(res, D.reference("blobs", shape, 8, D.LOW, True, None, rows, 300), f"agnostic {rows}")


def test_more_than_1024_detections_in_an_image():
    from uaps_amd import detection_match
    shape, thr = (1, 130, 70), (0.1, 0.5)
    pred, gt, conf, ref_p, ref_g = D.case("noise", shape, 4, 4096, 1100)
    assert 3072 < ref_p[1][0] <= 4096 and ref_g[1][0] > 1100                   # the ground truth overflows: still matched, marked invalid
    res = detection_match(*_device(pred, gt, conf, 4, 4096, 1100), 4, iou_thresholds=thr)
    D.assert_tables(res, D.reference("noise", shape, 4, thr, False, None, 4096, 1100))
    assert _equal(res, detection_match(_inst(ref_p, 1, "cpu"), _inst(ref_g, 0, "cpu"), 4, iou_thresholds=thr))
    assert int(res.rank.max()) > 1024 and res.valid.tolist() == [False]          # more than 1024 in ONE class: ranks beyond a group of threads


@pytest.mark.parametrize("figure", F.ALL, ids=lambda f: f.__name__)
def test_hand_worked_figures(figure):
    figure(_run)


def test_caller_scores():
    from uaps_amd import detection_match
    _, _, _, ref_p, ref_g = D.case("noise", (3, 37, 53), 8)
    rng = np.random.default_rng(11)
    sc = np.round(rng.standard_normal((3, D.MP)), 1)                          # many ties
    sc[0, :7] = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 1e30]
    for dtype in (np.float32, np.float64):
        s = sc.astype(dtype)
        res = detection_match(_inst(ref_p), _inst(ref_g), 4, scores=torch.from_numpy(s).to(DEV), iou_thresholds=D.LOW)
        ref = D.detect_batch(ref_p, ref_g, 4, D.LOW, scores=s)
        D.assert_tables(res, ref, str(dtype))
    D.check_summary(res.summary(), D.summary([(ref, ref_p)], [1, 2, 3], D.LOW))


def test_overflow_on_one_side():
    from uaps_amd import detection_match, label_instances
    m = np.concatenate([R.checkerboard(37, 53), R.noise(1, 37, 53, 0.1, 2, seed=4)])
    conf = D.confidence((2, 37, 53))
    dm, dc = torch.from_numpy(m).to(DEV), torch.from_numpy(conf).to(DEV)
    res = detection_match(label_instances(dm, maps=(dc,), connectivity=4, max_instances=256),
                          label_instances(dm, connectivity=4, max_instances=1024), 2, iou_thresholds=D.LOW)
    ref_p, ref_g = R.label_batch(m, (conf,), 4, 0, 1, 256), R.label_batch(m, (), 4, 0, 1, 1024)
    assert ref_p[1][0] == 981 and ref_p[1][1] <= 256
    assert res.valid.tolist() == [False, True]
    ref = D.detect_batch(ref_p, ref_g, 2, D.LOW)
    D.assert_tables(res, ref)                                 # the in-table components of the overflowed image are still matched
    assert res.counts[0, 1].tolist() == [256] * 6 + [256, 981]
    s = res.summary()
    assert (s["images"], s["images_skipped"]) == (1, 1) and s["n_gt"] == int(ref_g[1][1]) and s["mAP"] == 1.0 and s["AR"] == 1.0


def test_stale_workspace():
    """A dense call, then a sparse one with fewer rows on the same cached workspace: what the second reads, it has written."""
    from uaps_amd import detection_match
    _, _, _, ref_p, ref_g = D.case("noise", (2, 130, 70), 4, 512, 512)
    dense = detection_match(_inst(ref_p, 1), _inst(ref_g), 4, iou_thresholds=D.LOW)
    D.assert_tables(dense, D.reference("noise", (2, 130, 70), 4, D.LOW, False, None, 512, 512))
    m = R.noise(2, 130, 70, 0.05, 4, seed=9)
    p = M.redraw(m, 0.02, 4, seed=10)
    conf = D.confidence((2, 130, 70))
    sp, sg = R.label_batch(p, (conf,), 8, 0, 1, 96), R.label_batch(m, (), 8, 0, 1, 160)
    sparse = detection_match(_inst(sp, 1), _inst(sg), 4, iou_thresholds=D.COCO)
    D.assert_tables(sparse, D.detect_batch(sp, sg, 4, D.COCO))
    again = detection_match(_inst(ref_p, 1), _inst(ref_g), 4, iou_thresholds=D.LOW)
    assert _equal(dense, again)


def test_two_runs_same_bits_and_a_side_stream():
    from uaps_amd import detection_match
    _, _, _, ref_p, ref_g = D.case("noise", (2, 256, 256), 8)
    ip, ig = _inst(ref_p, 1), _inst(ref_g)
    a, b = detection_match(ip, ig, 4), detection_match(ip, ig, 4)
    assert _equal(a, b)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = detection_match(ip, ig, 4)
    side.synchronize()
    assert _equal(a, c)


def test_agrees_with_match_instances_at_three_quarters():
    """0.75 is exact in binary.  An IoU of exactly 3/4 would be a pair's largest intersection on both sides (more than half of either
    component), so looking at every prediction's partner shows that no pair sits on the threshold; there the strict rule of
    match_instances and the >= of the sweep agree, and above 0.5 a match is unique, so greedy order cannot matter."""
    from uaps_amd import detection_match, match_instances
    rng = np.random.default_rng(3)                   # square cells of random classes against the same moved by (1, 1): IoUs near 0.78
    gt = rng.integers(0, 4, (2, 17, 17)).repeat(16, axis=1).repeat(16, axis=2).astype(np.int64)
    ref_g = R.label_batch(np.ascontiguousarray(gt[:, :256, :256]), (), 8, 0, 1, D.MG)
    for shift in ((1, 1), (2, 1)):                   # (2, 1): a lone cell falls to 210 / 302, below the threshold; merged cells stay above
        moved = np.ascontiguousarray(np.roll(gt, shift, axis=(1, 2))[:, :256, :256])
        ref_p = R.label_batch(moved, (D.confidence((2, 256, 256)),), 8, 0, 1, D.MP)
        ip, ig = _inst(ref_p, 1), _inst(ref_g)
        m = match_instances(ip, ig, 4, iou_threshold=0.75)
        partner, inter = m.pred[..., 0], m.pred[..., 1]
        area_g = torch.gather(ig.table[..., 1], 1, (partner - 1).clamp(min=0))
        assert not bool(((partner > 0) & (4 * inter == 3 * (ip.table[..., 1] + area_g - inter))).any())
        res = detection_match(ip, ig, 4, iou_thresholds=(0.5, 0.75, 0.9))
        matched = m.pred[..., 3] > 0
        assert int(matched.sum()) > 0
        assert torch.equal(res.pred_match[..., 1], torch.where(matched, partner, torch.zeros_like(partner)))
        assert torch.equal(res.counts[..., 1], m.counts[..., 0])


def test_summary_and_records():
    from uaps_amd import detection, detection_match
    pred, gt, conf, ref_p, ref_g = D.case("blobs", (3, 37, 53), 8)
    res = detection_match(*_device(pred, gt, conf, 8, D.MP, D.MG), 4, iou_thresholds=D.LOW)
    ref = D.reference("blobs", (3, 37, 53), 8, D.LOW)
    assert res.sums().rows.is_cuda and res.iou().is_cuda and res.iou().dtype == torch.float64
    D.check_summary(res.summary(), D.summary([(ref, ref_p)], [1, 2, 3], D.LOW))
    parts = [res.sums([1, 3]), res.sums([1, 3])]
    D.check_summary(detection.summarize(parts, [1, 3], D.LOW, 6), D.summary([(ref, ref_p), (ref, ref_p)], [1, 3], D.LOW))
    rec = res.records()
    assert [len(r) for r in rec] == [min(int(n), D.MP) for n in ref_p[1]]
    assert sum(v > 0 for r in rec for d in r for v in d["matched"]) == int(ref[5][..., :6].sum())


def test_evaluate_with_detection():
    import math

    import uaps_amd
    from uaps_amd import inference
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    gen = torch.Generator().manual_seed(1)
    blocks = lambda: torch.randint(0, 4, (2, 8, 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)
    batches = [(torch.randn(2, 3, 64, 64, generator=gen).to(DEV), blocks().to(DEV)) for _ in range(2)]
    plain = inference.evaluate(model, batches)
    out = inference.evaluate(model, batches, detection={"max_instances": 4096, "iou_thresholds": D.LOW})
    assert all(out[k] == plain[k] for k in plain) and out["detection_images_skipped"] == 0
    for k in ("mAP(%)", "AP50(%)", "AP75(%)", "DefectAR(%)"):
        assert math.isnan(out[k]) or 0.0 <= out[k] <= 100.0, (k, out[k])
    tta = inference.evaluate(model, batches, tta=(1.0,), detection={"max_instances": 4096})
    assert tta["detection_images_skipped"] == 0 and set(tta) - set(plain) == set(out) - set(plain)

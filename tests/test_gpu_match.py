"""Defect matching on the GPU (csrc/match.hip) against the brute-force reference (tests/match_ref.py) and against the module's CPU
path.  Every comparison of tables is exact; the float64 scores derived from them are held to a relative 1e-12.

The pair-count kernel gives a lane four consecutive pixels (16-byte loads) where H * W is a multiple of four -- 7 x 300, 130 x 70,
256 x 256 -- and one pixel otherwise -- 1 x 1, 1 x 45, 37 x 53; a wave walks 256 or 1024 pixels, so every shape but the first two spans
several waves and 256 x 256 several workgroups per image.  The tables have 512 rows on the prediction's side and 300 on the ground
truth's: the strides of the pair matrix differ."""
import numpy as np
import pytest
import torch

import instances_ref as R
import match_ref as M

pytestmark = pytest.mark.gpu
DEV = R.DEV


def _inst(ref, dev=DEV):
    from uaps_amd import InstanceResult
    labels, count, table = ref
    return InstanceResult(torch.from_numpy(labels).to(dev), torch.from_numpy(count).to(dev), torch.from_numpy(table).to(dev), 0)


def _equal(a, b):
    return all(torch.equal(getattr(a, n).cpu(), getattr(b, n).cpu()) for n in ("pred", "target", "counts", "valid"))


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_the_reference_and_the_cpu_path(shape, connectivity):
    from uaps_amd import label_instances, match_instances
    for name in M.PATTERNS:
        pred, gt, cp, cg, ref_p, ref_g = M.case(name, shape, connectivity)
        # the device's own labelling in front: the whole path a user runs
        ip = label_instances(torch.from_numpy(pred).to(DEV), connectivity=cp, max_instances=M.MP)
        ig = label_instances(torch.from_numpy(gt).to(DEV), connectivity=cg, max_instances=M.MG)
        res = match_instances(ip, ig, 4)
        assert res.pred.is_cuda and res.pred.shape == (shape[0], M.MP, 4) and res.target.shape == (shape[0], M.MG, 4)
        M.assert_tables(res, M.match_batch(ref_p, ref_g, 4), f"{name} {shape} c{connectivity}")
        assert _equal(res, match_instances(_inst(ref_p, "cpu"), _inst(ref_g, "cpu"), 4)), name
    _, _, _, _, ref_p, ref_g = M.case("noise", shape, connectivity)
    res = match_instances(_inst(ref_p), _inst(ref_g), 4, iou_threshold=0.75, class_agnostic=True)
    M.assert_tables(res, M.match_batch(ref_p, ref_g, 4, 0.75, True), f"agnostic 0.75 {shape}")


def test_single_address_and_empty_images():
    """Both sides full: every pixel of the image adds to one word; full against empty and empty against empty: nothing to add."""
    from uaps_amd import match_instances
    for shape in ((2, 256, 256), (3, 37, 53)):
        _, _, _, _, ref_p, ref_g = M.case("full_full", shape, 8)
        res = match_instances(_inst(ref_p), _inst(ref_g), 4)
        hw = shape[1] * shape[2]
        assert res.pred[0, 0].tolist() == [1, hw, hw, 1] and res.target[0, 0].tolist() == [1, hw, hw, 1]
        assert res.counts[0].tolist() == [[0, 0, 0], [0, 0, 0], [1, 1, 1], [0, 0, 0]]
        assert float(res.iou()[0, 0]) == 1.0
        _, _, _, _, ref_p, ref_g = M.case("full_empty", shape, 8)
        res = match_instances(_inst(ref_p), _inst(ref_g), 4)
        assert res.pred[0, 0].tolist() == [0, 0, 0, 0] and int(res.target[0].abs().sum()) == 0 and res.counts[0, 2].tolist() == [0, 1, 0]
        _, _, _, _, ref_p, ref_g = M.case("empty_empty", shape, 8)
        res = match_instances(_inst(ref_p), _inst(ref_g), 4)
        assert int(res.pred[0].abs().sum()) == 0 and int(res.target[0].abs().sum()) == 0 and int(res.counts[0].abs().sum()) == 0


def test_overflow_on_one_side():
    from uaps_amd import label_instances, match_instances
    m = np.concatenate([R.checkerboard(37, 53), R.noise(1, 37, 53, 0.1, 2, seed=4)])
    dm = torch.from_numpy(m).to(DEV)
    res = match_instances(label_instances(dm, connectivity=4, max_instances=256), label_instances(dm, connectivity=4, max_instances=1024), 2)
    ref_p, ref_g = R.label_batch(m, (), 4, 0, 1, 256), R.label_batch(m, (), 4, 0, 1, 1024)
    assert ref_p[1][0] == 981 and ref_p[1][1] <= 256
    assert res.valid.tolist() == [False, True]
    ref = M.match_batch(ref_p, ref_g, 2)
    M.assert_tables(res, ref)                                 # the in-table components of the overflowed image are still matched
    assert res.counts[0, 1].tolist() == [256, 256, 981]
    s = res.summary()
    assert (s["images"], s["images_skipped"]) == (1, 1) and s["n_gt"] == int(ref_g[1][1]) and s["PQ"] == 1.0


def test_stale_workspace():
    """A dense call, then a sparse one with fewer rows on the same cached workspace: the zeroing must cover what the second reads."""
    from uaps_amd import match_instances
    _, _, _, _, ref_p, ref_g = M.case("noise", (2, 130, 70), 4, 512, 512)
    dense = match_instances(_inst(ref_p), _inst(ref_g), 4)
    M.assert_tables(dense, M.match_batch(ref_p, ref_g, 4))
    m = R.noise(2, 130, 70, 0.05, 4, seed=9)
    p = M.redraw(m, 0.02, 4, seed=10)
    sp, sg = R.label_batch(p, (), 8, 0, 1, 96), R.label_batch(m, (), 8, 0, 1, 160)
    sparse = match_instances(_inst(sp), _inst(sg), 4)
    M.assert_tables(sparse, M.match_batch(sp, sg, 4))
    again = match_instances(_inst(ref_p), _inst(ref_g), 4)   # and back: the sparse call's words lie inside the dense call's matrix
    assert _equal(dense, again)


def test_two_runs_same_bits_and_a_side_stream():
    from uaps_amd import match_instances
    _, _, _, _, ref_p, ref_g = M.case("noise", (2, 256, 256), 8)
    ip, ig = _inst(ref_p), _inst(ref_g)
    a, b = match_instances(ip, ig, 4), match_instances(ip, ig, 4)
    assert _equal(a, b)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = match_instances(ip, ig, 4)
    side.synchronize()
    assert _equal(a, c)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_derived_scores(connectivity):
    from uaps_amd import match_instances
    _, _, _, _, ref_p, ref_g = M.case("noise", (3, 37, 53), connectivity, 1024, 1024)
    ref = M.match_batch(ref_p, ref_g, 4)
    res = match_instances(_inst(ref_p), _inst(ref_g), 4)
    M.assert_tables(res, ref)
    assert ref[3].all() and res.iou().is_cuda and res.sums().is_cuda and res.sums().dtype == torch.float64
    M.check_scores(res, ref, ref_p, ref_g)
    rec = res.records()
    assert [len(r["target"]) for r in rec] == ref_g[1].tolist() and [len(r["pred"]) for r in rec] == ref_p[1].tolist()
    assert sum(r["matched"] for rr in rec for r in rr["target"]) == int(ref[2][..., 0].sum()) == sum(r["matched"] for rr in rec for r in rr["pred"])


def test_evaluate_with_instances():
    import math

    import uaps_amd
    from uaps_amd import inference, label_instances
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    gen = torch.Generator().manual_seed(1)
    blocks = lambda: torch.randint(0, 4, (2, 8, 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)
    batches = [(torch.randn(2, 3, 64, 64, generator=gen).to(DEV), blocks().to(DEV)) for _ in range(2)]
    plain = inference.evaluate(model, batches)
    out = inference.evaluate(model, batches, instances=True)
    assert all(out[k] == plain[k] for k in plain)
    for k in ("PQ(%)", "SQ(%)", "RQ(%)", "DefectPrecision(%)", "DefectRecall(%)", "PRO(%)"):
        assert math.isnan(out[k]) or 0.0 <= out[k] <= 100.0, (k, out[k])
    # consistent counts: the defects of the images that were used (an untrained network may report more than 256 specks in one)
    n_gt = n_pred = skipped = 0
    for x, y in batches:
        ip, ig = label_instances(inference.predict(model, x)[0]), label_instances(y)
        assert not bool(ig.overflow.any())
        used = ~(ip.overflow | ig.overflow)
        n_gt += int(ig.count[used].sum()); n_pred += int(ip.count[used].sum()); skipped += int((~used).sum())
    assert (out["defects_gt"], out["defects_pred"], out["instance_images_skipped"]) == (n_gt, n_pred, skipped)
    wide = inference.evaluate(model, batches, instances={"max_instances": 4096})       # 64 x 64 pixels: no image can overflow
    assert wide["instance_images_skipped"] == 0 and wide["defects_gt"] == sum(int(label_instances(y).count.sum()) for _, y in batches)
    tta = inference.evaluate(model, batches, tta=(1.0,), instances={"max_instances": 4096})
    assert tta["defects_gt"] == wide["defects_gt"] and tta["instance_images_skipped"] == 0

"""Mask clean-up morphology on the device (csrc/morph.hip) against scipy (tests/morph_ref.py): every op x footprint at the radii 1, 3
and 15 over the shapes where the bit-plane kernel can go wrong -- one-word rows, a word boundary +- 1, a single row or column, the
width limit -- on masks that touch all four borders; band independence, repeatability, chains, and the cleanup= keyword of
inference.predict_instances / inference.evaluate.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import morph_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = ((1, 1), (1, 70), (70, 1), (31, 32), (33, 64), (37, 53), (64, 65), (130, 161), (5, 4096), (4096, 3))
CHECKED = (130, 161)                     # where the generator gives every op x footprint x radius something to do


def _dev(m, steps, num_classes=4, **kw):
    from uaps_amd import morphology
    out = morphology(torch.from_numpy(np.array(m)).to(DEV), steps, num_classes, **kw)
    assert out.dtype == torch.int64 and out.is_cuda and out.shape == m.shape
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(B, H, W, C, r, steps):
    return R.morphology(R.discs(B, H, W, C, r), list(steps), C)


@pytest.mark.parametrize("radius", (1, 3, 15))
@pytest.mark.parametrize("fp", R.FOOTPRINTS)
@pytest.mark.parametrize("op", R.OPS)
def test_device_equals_scipy(op, fp, radius):
    steps = ((op, fp, radius),)
    for H, W in SHAPES:
        m = R.discs(2, H, W, 4, radius)
        ref = _ref(2, H, W, 4, radius, steps)
        if (H, W) == CHECKED:
            assert R.informative(ref, m), "a vacuous case"
            assert all((e != 0).any() for e in (m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1]))     # the masks touch all four borders
        got = _dev(m, steps)
        assert np.array_equal(got, ref), (H, W, int((got != ref).sum()))


def test_eight_classes():
    for steps in (((("close", "disk", 3)),), (("open", "cross", 3),), (("dilate", "square", 3), ("boundary", "disk", 1))):
        m = R.discs(2, 130, 161, 8, 3)
        ref = _ref(2, 130, 161, 8, 3, steps)
        assert R.informative(ref, m) and len(np.unique(m)) == 8
        assert np.array_equal(_dev(m, steps, 8), ref), steps
    m = np.array(R.discs(2, 64, 65, 8, 3))
    m[:, 10:12] = 255                                    # obstacles; a non-zero background; a subset of the classes, out of order
    kw = {"background": 2, "classes": (7, 1, 4, 0)}
    steps = [("close", "square", 3), ("open", "disk", 1)]
    assert np.array_equal(_dev(m, steps, 8, **kw), R.morphology(m, steps, 8, **kw))


@pytest.mark.parametrize("r,steps", ((3, (("open", "disk", 1), ("close", "square", 2))), (15, (("open", "disk", 15),))), ids=("reach6", "open15"))
def test_band_independence(r, steps):
    from uaps_amd.morphology import band_rows, chain_reach
    m = R.discs(2, 130, 161, 4, r)
    ref = _ref(2, 130, 161, 4, r, steps)
    assert R.informative(ref, m)
    assert chain_reach(steps) in (6, 30) and 1 <= band_rows(130, 161, 3, chain_reach(steps)) <= 130
    for rows in (1, 8, 0):                               # (at 1 and 8 rows the halo is larger than the band)
        assert np.array_equal(_dev(m, steps, _band_rows=rows), ref), rows


def test_two_calls_and_a_side_stream_give_the_same_bits():
    from uaps_amd import morphology
    steps = [("open", "disk", 2), ("close", "square", 2)]
    m = torch.from_numpy(np.array(R.discs(2, 130, 161, 4, 2))).to(DEV)
    a, b = morphology(m, steps, 4), morphology(m, steps, 4)
    assert a.data_ptr() != b.data_ptr() != m.data_ptr() and torch.equal(a, b)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = morphology(m, steps, 4)
    side.synchronize()
    assert torch.equal(a, c) and np.array_equal(a.cpu().numpy(), _ref(2, 130, 161, 4, 2, tuple(steps)))


def test_a_chain_equals_its_steps_one_at_a_time():
    steps = (("erode", "cross", 1), ("dilate", "disk", 3), ("close", "square", 2), ("boundary", "disk", 1))
    m = R.discs(2, 130, 161, 4, 3)
    ref = _ref(2, 130, 161, 4, 3, steps)
    assert R.informative(ref, m)
    chain = _dev(m, steps)
    one = np.array(m)
    for s in steps:
        one = _dev(one, [s])
    assert np.array_equal(chain, one) and np.array_equal(chain, ref)


def test_class_groups_and_one_word_tiles():
    """Where the planes of all classes do not fit beside a tall band, the result planes serve a few classes at a time; where the
    longest chain (reach 64) meets a row wider than a tile, tiles shrink to one word with a one-word halo on either side."""
    m = R.discs(2, 130, 161, 8, 15)
    for steps in ((("open", "disk", 15),), (("close", "cross", 15),)):
        ref = _ref(2, 130, 161, 8, 15, steps)
        assert (ref != m).any()
        assert np.array_equal(_dev(m, steps, 8, _band_rows=100), ref), steps      # seven planes in groups of three
    steps = (("close", "square", 15), ("open", "disk", 15), ("erode", "cross", 4))
    m = np.array(R.discs(1, 70, 600, 8, 15))
    m[:, :, 300:303] = 255
    ref = R.morphology(m, steps, 8)
    assert R.informative(ref, m)
    assert np.array_equal(_dev(m, steps, 8), ref)
    assert np.array_equal(_dev(m, steps, 8, _band_rows=64), ref)                  # only one-word tiles hold 64 + 128 rows


def _model_and_batches():
    import uaps_amd
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    gen = torch.Generator().manual_seed(1)
    blocks = lambda: torch.randint(0, 4, (2, 8, 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)
    return model, [(torch.randn(2, 3, 64, 64, generator=gen).to(DEV), blocks().to(DEV)) for _ in range(2)]


def test_predict_instances_with_cleanup():
    from uaps_amd import inference, label_instances, morphology
    model, batches = _model_and_batches()
    x = batches[0][0]
    steps = [("open", "disk", 1)]
    mask, heads = inference.predict(model, x)
    clean = morphology(mask, steps, 4)
    assert np.array_equal(clean.cpu().numpy(), R.morphology(mask.cpu().numpy(), steps, 4)) and not torch.equal(clean, mask)
    conf = torch.softmax(heads[0], dim=1).amax(dim=1)
    res, ref = inference.predict_instances(model, x, cleanup=steps), label_instances(clean, (conf,))
    assert torch.equal(res.labels, ref.labels) and torch.equal(res.count, ref.count) and torch.equal(res.table, ref.table)
    tta = inference.predict_instances(model, x, tta=(1.0,), cleanup=steps)
    tiled = inference.predict_instances(model, x, tiled={"tile": 64, "overlap": 16}, cleanup=steps)
    for r in (tta, tiled):
        assert r.labels.shape == ref.labels.shape and int(r.count.sum()) > 0


def test_evaluate_with_cleanup():
    from uaps_amd import inference, label_instances, morphology
    model, batches = _model_and_batches()
    steps = [("open", "disk", 1)]
    kw = dict(instances={"max_instances": 4096}, surface=True)
    plain = inference.evaluate(model, batches, **kw)
    out = inference.evaluate(model, batches, cleanup=steps, **kw)
    assert set(out) - set(plain) == {"mIoU_clean(%)", "mDice_clean(%)"}
    same = ("mIoU(%)", "mDice(%)", "Accuracy(%)", "images", "defects_gt")
    assert all(out[k] == plain[k] for k in same)
    assert 0.0 <= out["mIoU_clean(%)"] <= 100.0 and 0.0 <= out["mDice_clean(%)"] <= 100.0
    # the defect scores look at the cleaned arg-max mask
    count = lambda clean: sum(int(label_instances(morphology(inference.predict(model, x)[0], steps, 4) if clean else
                                                  inference.predict(model, x)[0], max_instances=4096).count.sum()) for x, _ in batches)
    assert out["defects_pred"] == count(True) and plain["defects_pred"] == count(False) and out["instance_images_skipped"] == 0
    assert out["surface_pairs"] > 0 and out["HD95(px)"] >= 0.0
    bare = inference.evaluate(model, batches)
    with_keys = inference.evaluate(model, batches, cleanup=steps)
    assert set(with_keys) - set(bare) == {"mIoU_clean(%)", "mDice_clean(%)"} and all(with_keys[k] == bare[k] for k in bare)
    assert with_keys["mIoU_clean(%)"] == out["mIoU_clean(%)"]

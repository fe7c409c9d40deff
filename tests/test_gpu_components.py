"""Component clean-up on the device (csrc/components.hip) against scipy (tests/components_ref.py) on the smallest shapes at which each
mechanism can go wrong: one pixel, a single row or column, exactly one 16 x 16 tile, one pixel past a tile seam and a wave word, many
seams, a row longer than a wave's span of 16 x 64 pixels, several workgroup spans and batch offsets.  Long parent chains across seams
(spirals, a comb), eight virtual planes, chains, a recycled workspace, and the components= keyword of inference.predict_instances /
inference.evaluate.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import components_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLANES = ((2, 16, 16), (2, 17, 65), (2, 37, 53), (2, 130, 161), (2, 3, 1100), (2, 256, 256))     # informative for every step
LINES = ((2, 1, 1), (2, 1, 70), (2, 64, 1))
STEPS = ([("area_open", n) for n in (2, 5, 50)] + [("clear_border",)] + [("fill_holes", n) for n in (1, 5, 50, None)])
_ids = lambda s: "-".join(str(v) for v in s)


def _dev(m, steps, num_classes=4, **kw):
    from uaps_amd import components
    src = torch.from_numpy(np.array(m)).to(DEV)
    out = components(src, steps, num_classes, **kw)
    assert out.dtype == torch.int64 and out.is_cuda and out.shape == src.shape and out.data_ptr() != src.data_ptr()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(shape, steps, connectivity, C=4):
    out = R.components(R.rings(*shape, C), list(steps), C, connectivity=connectivity)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("step", STEPS, ids=_ids)
def test_device_equals_scipy(step, connectivity):
    for shape in PLANES:
        m, ref = R.rings(*shape), _ref(shape, (step,), connectivity)
        assert R.informative(ref, m), ("a vacuous case", shape)
        got = _dev(m, [step], connectivity=connectivity)
        assert np.array_equal(got, ref), (shape, int((got != ref).sum()))


@pytest.mark.parametrize("connectivity", (4, 8))
def test_device_equals_scipy_on_one_pixel_rows_and_columns_without_the_informative_claim(connectivity):
    for shape in LINES:
        m = R.rings(*shape)
        for step in STEPS + [("area_open", 1)]:
            got = _dev(m, [step], connectivity=connectivity)
            assert np.array_equal(got, _ref(shape, (step,), connectivity)), (shape, step)
            if step == ("area_open", 1) or step[0] == "fill_holes":       # a line has no holes
                assert np.array_equal(got, m), (shape, step)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_spirals_and_a_comb(connectivity):
    """Long parent chains across seams: the sealed spiral's corridor is one large hole, the open one's is none."""
    fill = [("fill_holes", None)]
    closed, opened, comb = R.closed_spiral(130, 161), R.open_spiral(130, 161), R.comb(130, 161)
    corridor = int((closed == 0).sum())
    ref = R.components(closed, fill, 4, connectivity=connectivity)
    assert corridor > 10000 and (ref == 1).all()
    assert np.array_equal(_dev(closed, fill, connectivity=connectivity), ref)
    assert np.array_equal(_dev(closed, [("fill_holes", corridor - 1)], connectivity=connectivity), closed)       # one hole of that size
    assert np.array_equal(_dev(closed, [("fill_holes", corridor)], connectivity=connectivity), ref)
    assert np.array_equal(_dev(opened, fill, connectivity=connectivity), opened)
    assert np.array_equal(R.components(opened, fill, 4, connectivity=connectivity), opened)
    wall = int((opened == 1).sum())
    for g, n in ((opened, wall), (comb, int((comb == 2).sum()))):                        # ONE component, which touches the border
        assert np.array_equal(_dev(g, [("area_open", n)], connectivity=connectivity), g)
        assert (_dev(g, [("area_open", n + 1)], connectivity=connectivity) == 0).all()
        assert (_dev(g, [("clear_border",)], connectivity=connectivity) == 0).all()
        assert np.array_equal(_dev(g, fill, connectivity=connectivity), R.components(g, fill, 4, connectivity=connectivity))


def test_the_frame():
    for H, W in ((16, 16), (37, 53), (130, 161)):
        m = R.frame(H, W)
        for connectivity in (4, 8):
            assert (_dev(m, [("clear_border",)], connectivity=connectivity) == 0).all()
            assert (_dev(m, [("fill_holes", None)], connectivity=connectivity) == 1).all()
            assert np.array_equal(_dev(m, [("fill_holes", (H - 2) * (W - 2) - 1)], connectivity=connectivity), m)
            assert np.array_equal(R.components(m, [("fill_holes", None)], 4, connectivity=connectivity), np.ones_like(m))


def test_eight_classes_give_eight_virtual_planes():
    m = np.array(R.rings(2, 130, 161, 9))               # the values 0..8 and a few 255
    m[m == 0] = 200
    m[m == 8] = 0                                       # now: background 200 and the classes 0..7, eight selected classes
    kw = dict(background=200, classes=(7, 3, 1, 5, 0, 2, 6, 4))
    assert set(range(8)) <= set(np.unique(m).tolist())
    for connectivity in (4, 8):
        for steps in ((("fill_holes", None),), (("fill_holes", 50), ("area_open", 5), ("fill_holes", None))):
            ref = R.components(m, steps, 8, connectivity=connectivity, **kw)
            assert R.informative(ref, m, background=200)
            assert np.array_equal(_dev(m, steps, 8, connectivity=connectivity, **kw), ref), (connectivity, steps)


def test_a_class_subset_with_obstacles():
    m = np.array(R.rings(2, 130, 161))
    m[:, 50:53, :] = 255                                # an ignore band through rings and holes
    m[:, :, 80:82] = 7                                  # a value >= num_classes
    for steps in ((("fill_holes", None),), (("area_open", 20),), (("clear_border",), ("fill_holes", 50))):
        for kw in ({"classes": (2,)}, {"classes": (3, 1)}, {"background": 2}, {"background": 3, "classes": (0, 1)}):
            ref = R.components(m, steps, 4, **kw)
            assert (ref != m).any(), (steps, kw)
            got = _dev(m, steps, **kw)
            assert np.array_equal(got, ref), (steps, kw)
            assert np.array_equal(got == 255, m == 255) and np.array_equal(got == 7, m == 7)


CHAINS = ((("area_open", 16), ("fill_holes", 64)),
          (("fill_holes", None), ("clear_border",), ("area_open", 50)),
          (("clear_border",), ("fill_holes", 5), ("area_open", 2), ("fill_holes", None)))


@pytest.mark.parametrize("steps", CHAINS, ids=("2", "3", "4"))
def test_a_chain_equals_its_steps_one_at_a_time(steps):
    for shape in ((2, 37, 53), (2, 130, 161)):
        for connectivity in (4, 8):
            m, ref = R.rings(*shape), _ref(shape, steps, connectivity)
            assert R.informative(ref, m)
            one = np.array(m)
            for s in steps:
                one = _dev(one, [s], connectivity=connectivity)
            assert np.array_equal(_dev(m, steps, connectivity=connectivity), ref) and np.array_equal(one, ref)


def test_a_recycled_workspace_two_calls_and_a_side_stream_give_the_same_bits():
    """A large shape, a small one, the large one again on one workspace: stale area / flag words would show."""
    from uaps_amd import components
    steps = [("fill_holes", 64), ("area_open", 16), ("clear_border",)]
    big = torch.from_numpy(np.array(R.rings(2, 256, 256))).to(DEV)
    small = torch.from_numpy(np.array(R.rings(2, 37, 53))).to(DEV)
    a = components(big, steps, 4)
    s = components(small, steps, 4)
    b = components(big, steps, 4)
    s2 = components(small, [("clear_border",)], 4)      # one plane on words the eight-launch chain above left behind
    assert a.data_ptr() != b.data_ptr() != big.data_ptr() and torch.equal(a, b)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = components(big, steps, 4)
    side.synchronize()
    assert torch.equal(a, c) and np.array_equal(a.cpu().numpy(), _ref((2, 256, 256), tuple(steps), 8))
    assert np.array_equal(s.cpu().numpy(), _ref((2, 37, 53), tuple(steps), 8))
    assert np.array_equal(s2.cpu().numpy(), _ref((2, 37, 53), (("clear_border",),), 8))


def test_device_equals_the_cpu_path():
    from uaps_amd import components
    m = torch.from_numpy(np.array(R.rings(2, 37, 53)))
    for connectivity in (4, 8):
        for steps in ([("area_open", 5)], [("clear_border",)], [("fill_holes", None)], [("fill_holes", 5), ("area_open", 50), ("clear_border",)]):
            for kw in ({}, {"classes": (3, 1)}, {"background": 2}):
                cpu = components(m, steps, 4, connectivity=connectivity, **kw)
                assert not torch.equal(cpu, m)
                assert torch.equal(components(m.to(DEV), steps, 4, connectivity=connectivity, **kw).cpu(), cpu), (steps, kw)


@pytest.mark.parametrize("n", (2, 5, 50))
def test_area_open_agrees_with_label_instances_min_area(n):
    from uaps_amd import components, label_instances
    for shape in ((2, 37, 53), (2, 130, 161)):
        for connectivity in (4, 8):
            m = torch.from_numpy(np.array(R.rings(*shape))).to(DEV)
            m[m == 255] = 0
            opened = components(m, [("area_open", n)], 4, connectivity=connectivity)
            a = label_instances(opened, connectivity=connectivity, max_instances=1024)
            b = label_instances(m, connectivity=connectivity, min_area=n, max_instances=1024)
            assert int(b.count.max()) <= 1024 and int(b.count.sum()) < int(label_instances(m, connectivity=connectivity).count.sum())
            assert torch.equal(a.labels, b.labels) and torch.equal(a.count, b.count) and torch.equal(a.table, b.table)
            assert torch.equal(opened, torch.where(b.labels > 0, m, torch.zeros_like(m)))


def _model_and_batches():
    import uaps_amd
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    gen = torch.Generator().manual_seed(1)
    blocks = lambda: torch.randint(0, 4, (2, 8, 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)
    return model, [(torch.randn(2, 3, 64, 64, generator=gen).to(DEV), blocks().to(DEV)) for _ in range(2)]


def test_predict_instances_with_components():
    from uaps_amd import components, inference, label_instances, morphology
    model, batches = _model_and_batches()
    x = batches[0][0]
    steps, morph = [("area_open", 4), ("fill_holes", None)], [("open", "disk", 1)]
    mask, heads = inference.predict(model, x)
    clean = components(mask, steps, 4)
    assert np.array_equal(clean.cpu().numpy(), R.components(mask.cpu().numpy(), steps, 4)) and not torch.equal(clean, mask)
    conf = torch.softmax(heads[0], dim=1).amax(dim=1)
    res, ref = inference.predict_instances(model, x, components=steps), label_instances(clean, (conf,))
    assert torch.equal(res.labels, ref.labels) and torch.equal(res.count, ref.count) and torch.equal(res.table, ref.table)
    both = components(morphology(mask, morph, 4), steps, 4)
    res, ref = inference.predict_instances(model, x, cleanup=morph, components=steps), label_instances(both, (conf,))
    assert torch.equal(res.labels, ref.labels) and torch.equal(res.count, ref.count) and torch.equal(res.table, ref.table)
    tta = inference.predict_instances(model, x, tta=(1.0,), components=steps)
    tiled = inference.predict_instances(model, x, tiled={"tile": 64, "overlap": 16}, cleanup=morph, components=steps)
    for r in (tta, tiled):
        assert r.labels.shape == ref.labels.shape and int(r.count.sum()) > 0
        assert int(r.table[..., 1][r.table[..., 1] > 0].min()) >= 4                       # no defect below the area opening


def test_evaluate_with_components():
    from uaps_amd import components, inference, label_instances, morphology
    model, batches = _model_and_batches()
    steps, morph = [("area_open", 4), ("fill_holes", None)], [("open", "disk", 1)]
    kw = dict(instances={"max_instances": 4096}, surface=True)
    plain = inference.evaluate(model, batches, **kw)
    out = inference.evaluate(model, batches, components=steps, **kw)
    both = inference.evaluate(model, batches, cleanup=morph, components=steps, **kw)
    same = ("mIoU(%)", "mDice(%)", "Accuracy(%)", "images", "defects_gt")
    for d in (out, both):
        assert set(d) - set(plain) == {"mIoU_clean(%)", "mDice_clean(%)"} and all(d[k] == plain[k] for k in same)
        assert 0.0 <= d["mIoU_clean(%)"] <= 100.0 and 0.0 <= d["mDice_clean(%)"] <= 100.0
        assert d["surface_pairs"] > 0 and d["HD95(px)"] >= 0.0 and d["instance_images_skipped"] == 0

    def count(chain):
        return sum(int(label_instances(chain(inference.predict(model, x)[0]), max_instances=4096).count.sum()) for x, _ in batches)

    assert plain["defects_pred"] == count(lambda m: m)
    assert out["defects_pred"] == count(lambda m: components(m, steps, 4))
    assert any(not torch.equal(components(inference.predict(model, x)[0], steps, 4), inference.predict(model, x)[0]) for x, _ in batches)
    assert both["defects_pred"] == count(lambda m: components(morphology(m, morph, 4), steps, 4))
    bare = inference.evaluate(model, batches)
    assert inference.evaluate(model, batches, components=None) == bare
    tta = inference.evaluate(model, batches, tta=(1.0,), components=steps)
    assert set(tta) - set(bare) == {"mIoU_clean(%)", "mDice_clean(%)"} and tta["images"] == bare["images"]

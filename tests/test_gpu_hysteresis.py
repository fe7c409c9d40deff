"""Hysteresis thresholding and binary reconstruction on the device (csrc/hysteresis.hip) against scipy (tests/hysteresis_ref.py) on the
smallest shapes at which each mechanism can go wrong: one pixel, a single row or column, exactly one 16 x 16 tile, one pixel past a
tile seam and a wave word, many seams, a row longer than a wave's span of 16 x 64 pixels, several workgroup spans and batch offsets,
long frames.  Seeds where the flatten pass could lose them -- far from the root, in a non-leading run of a 64-pixel group, in a leading
run carried across groups -- properties checked on the device, a recycled workspace, and the hysteresis= keyword of
inference.predict_instances.  Every comparison is exact: the generated scores keep a margin of 1e-3 from every threshold
(hysteresis_ref), and where a network's logits are thresholded the margin is asserted against the fp32 softmax's error."""
import numpy as np
import pytest
import torch

import components_ref as CR
import hysteresis_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLANES = ((2, 16, 16), (2, 17, 65), (2, 37, 53), (2, 130, 161), (2, 3, 1100), (2, 256, 256))     # informative in every combination
LINES = ((2, 1, 1), (2, 1, 70), (2, 64, 1))
FRAMES = ((1, 8, 4096), (1, 4096, 8))
# an fp32 softmax of up to 8 classes against the float64 one: expf within 2 ulp, at most 7 adds, one division -- below 1e-6 on a
# probability (the reasoning of tests/curves_ref.py); a network's logits are only thresholded where every selected score keeps ten
# times that from the thresholds
NET_MARGIN = 1e-5


def _dev(s, low, high, **kw):
    from uaps_amd import hysteresis
    src = torch.from_numpy(np.array(s)).to(DEV)
    out = hysteresis(src, low, high, **kw)
    assert out.dtype == torch.int64 and out.is_cuda and out.shape == (src.shape[0],) + src.shape[2:]
    return out.cpu().numpy()


def _rec(m, k, num_classes=4, **kw):
    from uaps_amd import reconstruct
    src = torch.from_numpy(np.array(m)).to(DEV)
    out = reconstruct(src, torch.from_numpy(np.array(k)).to(DEV), num_classes, **kw)
    assert out.dtype == torch.int64 and out.is_cuda and out.shape == src.shape and out.data_ptr() != src.data_ptr()
    return out.cpu().numpy()


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("from_logits", (False, True), ids=("scores", "logits"))
@pytest.mark.parametrize("Cn", (4, 1), ids=("C4", "C1"))
def test_device_equals_scipy(Cn, from_logits, connectivity):
    for shape in PLANES + FRAMES:
        s = R.case(shape, Cn, from_logits)                      # (asserts the margin)
        for min_area in (1, 5):
            for per_class in ((False, True) if Cn == 4 else (False,)):
                ref = R.expected(shape, Cn, from_logits, per_class, connectivity, min_area)       # (asserts "informative")
                lo, hi = R.PER_CLASS if per_class else (R.LOW, R.HIGH)
                got = _dev(s, lo, hi, from_logits=from_logits, connectivity=connectivity, min_area=min_area)
                assert np.array_equal(got, ref), (shape, min_area, per_class, int((got != ref).sum()))


@pytest.mark.parametrize("connectivity", (4, 8))
def test_device_equals_scipy_on_one_pixel_rows_and_columns_without_the_informative_claim(connectivity):
    for shape in LINES:
        for Cn in (4, 1):
            for from_logits in (False, True):
                s = R.case(shape, Cn, from_logits)
                ref = R.expected(shape, Cn, from_logits, False, connectivity, 1, check=False)
                assert np.array_equal(_dev(s, R.LOW, R.HIGH, from_logits=from_logits, connectivity=connectivity), ref), (shape, Cn)


def test_class_subsets_and_a_non_zero_background():
    shape = (2, 37, 53)
    s = R.case(shape, 4, False)
    for kw in ({"classes": (2,)}, {"classes": (3, 1)}, {"background": 3, "classes": (1, 2)}, {"background": 7}):
        lo, hi = ((0.3, 0.2), (0.7, 0.5)) if len(kw.get("classes", ())) == 2 else (R.LOW, R.HIGH)
        ref = R.hysteresis(s, lo, hi, **kw)
        assert (ref != kw.get("background", 0)).any()
        assert np.array_equal(_dev(s, lo, hi, **kw), ref), kw
    # eight channels: 4 is a copy of the background's and stays unselected, 5..7 are scaled copies of 2, 3, 1 that win or lose against them
    eight = (np.concatenate([s, s[:, [0, 2, 3, 1]] * np.array([1.0, 1.1, 0.9, 1.1], dtype=np.float32)[None, :, None, None]], axis=1) / 2).astype(np.float32)
    kw = {"classes": (1, 2, 3, 5, 6, 7)}
    ref = R.hysteresis(eight, R.LOW / 2, R.HIGH / 2, **kw)
    assert np.array_equal(_dev(eight, R.LOW / 2, R.HIGH / 2, **kw), ref) and set(np.unique(ref)) == {0, 3, 5, 7}


@pytest.mark.parametrize("connectivity", (4, 8))
def test_a_seed_far_from_its_root(connectivity):
    """ONE component whose parent chain crosses every seam, exactly one seed on its LAST pixel in raster order: kept whole.  The seed
    one pixel off the component: dropped whole."""
    for g in (CR.open_spiral(130, 161), CR.comb(130, 161)):
        g = np.array(g)
        cls = int(g.max())
        H, W = g.shape[1:]
        last = int(np.flatnonzero(g[0].reshape(-1))[-1])
        y, x = divmod(last, W)
        off = [(yy, xx) for yy in (y - 1, y, y + 1) for xx in (x - 1, x, x + 1) if 0 <= yy < H and 0 <= xx < W and g[0, yy, xx] == 0][0]
        on_k, off_k = np.zeros(g.shape, dtype=bool), np.zeros(g.shape, dtype=bool)
        on_k[0, y, x] = True
        off_k[0][off] = True
        # the marker form
        assert np.array_equal(R.reconstruct(g, on_k, 4, connectivity=connectivity), g)
        assert np.array_equal(_rec(g, on_k, connectivity=connectivity), g)
        assert (_rec(g, off_k, connectivity=connectivity) == 0).all()
        assert (_rec(g, on_k, connectivity=connectivity, min_area=int((g != 0).sum()) + 1) == 0).all()
        assert np.array_equal(_rec(g, on_k, connectivity=connectivity, min_area=int((g != 0).sum())), g)
        # the score form: the one strong pixel on the component; then a strong pixel of ANOTHER class beside it
        p, z = R.scores_from_labels(g, 4, seeds=on_k)
        assert R.margin(p, [R.LOW, R.HIGH]) >= R.MARGIN
        ref = R.hysteresis(p, R.LOW, R.HIGH, connectivity=connectivity)
        assert np.array_equal(ref, g)
        assert np.array_equal(_dev(p, R.LOW, R.HIGH, connectivity=connectivity), g)
        assert np.array_equal(_dev(z, R.LOW, R.HIGH, from_logits=True, connectivity=connectivity), g)
        other = 3 if cls != 3 else 1
        g2 = g.copy()
        g2[0][off] = other
        p, _ = R.scores_from_labels(g2, 4, seeds=off_k)
        assert R.margin(p, [R.LOW, R.HIGH]) >= R.MARGIN
        want = np.where(off_k, other, 0)
        assert np.array_equal(R.hysteresis(p, R.LOW, R.HIGH, connectivity=connectivity), want)
        assert np.array_equal(_dev(p, R.LOW, R.HIGH, connectivity=connectivity), want)


def test_a_seed_in_a_non_leading_run():
    """A 64-pixel group with three components, the seed in the middle one: its run is not the group's leading root, so the flag
    travels with the per-run add."""
    m = np.zeros((1, 3, 64), dtype=np.int64)
    m[0, 1, 2:12], m[0, 1, 20:31], m[0, 1, 40:64] = 1, 1, 1
    for at in (20, 25, 30):
        k = np.zeros(m.shape, dtype=bool)
        k[0, 1, at] = True
        want = np.zeros_like(m)
        want[0, 1, 20:31] = 1
        assert np.array_equal(R.reconstruct(m, k, 4), want)
        assert np.array_equal(_rec(m, k), want), at
        p, _ = R.scores_from_labels(m, 4, seeds=k)
        assert np.array_equal(_dev(p, R.LOW, R.HIGH), want), at
    k = np.zeros(m.shape, dtype=bool)
    k[0, 1, 63] = True                                           # ... and in the last one, on the group's last lane
    want = np.zeros_like(m)
    want[0, 1, 40:64] = 1
    assert np.array_equal(_rec(m, k), want)
    k[0, 1, 5] = True                                            # ... and the leading one as well
    want[0, 1, 2:12] = 1
    assert np.array_equal(_rec(m, k), want) and np.array_equal(R.reconstruct(m, k, 4), want)


def test_a_seed_in_a_leading_run_carried_across_several_groups():
    """A component that fills rows is carried by the wave over its span of 16 groups of 64 pixels: the seed sits in one group only,
    first, middle or last of the span, or in the next wave's span; a second component behind it forces the flush."""
    H, W = 6, 512                                                # rows 0..3: 2048 pixels = two spans of 1024
    m = np.zeros((1, H, W), dtype=np.int64)
    m[0, 0:4] = 1
    m[0, 5, 3:9] = 2
    for at in (0, 63, 64, 5 * 64 + 17, 1023, 1024, 2047):
        k = np.zeros(m.shape, dtype=bool)
        k.reshape(-1)[at] = True
        want = np.where(m == 1, 1, 0)
        assert np.array_equal(R.reconstruct(m, k, 4), want)
        assert np.array_equal(_rec(m, k), want), at
        assert np.array_equal(_rec(m, k, connectivity=4, min_area=2048), want) and (_rec(m, k, min_area=2049) == 0).all()
        p, _ = R.scores_from_labels(m, 4, seeds=k)
        assert np.array_equal(_dev(p, R.LOW, R.HIGH), want), at
    k = np.zeros(m.shape, dtype=bool)
    k[0, 5, 8] = True
    assert np.array_equal(_rec(m, k), np.where(m == 2, 2, 0))
    assert (_rec(m, np.zeros(m.shape, dtype=bool)) == 0).all()


def test_diagonal_neighbours_and_touching_classes():
    m = np.zeros((1, 5, 6), dtype=np.int64)
    m[0, 1, 1], m[0, 2, 2] = 1, 1                                # two diagonal neighbours of one class, one seeded
    m[0, 3, 3:5], m[0, 4, 3:5] = 2, 3                            # two touching components of different classes, one seeded
    k = np.zeros(m.shape, dtype=bool)
    k[0, 1, 1], k[0, 4, 4] = True, True
    p, z = R.scores_from_labels(m, 4, seeds=k)
    want8 = np.where((m == 1) | (m == 3), m, 0)
    want4 = want8.copy()
    want4[0, 2, 2] = 0
    for connectivity, want in ((8, want8), (4, want4)):
        assert np.array_equal(R.hysteresis(p, R.LOW, R.HIGH, connectivity=connectivity), want)
        assert np.array_equal(_dev(p, R.LOW, R.HIGH, connectivity=connectivity), want)
        assert np.array_equal(_dev(z, R.LOW, R.HIGH, from_logits=True, connectivity=connectivity), want)
        assert np.array_equal(_rec(m, k, connectivity=connectivity), want)


def test_nan_pixels_and_an_infinite_high_threshold():
    shape = (2, 37, 53)
    s = np.array(R.case(shape, 4, False))
    rng = np.random.default_rng(9)
    s[:, 2][rng.random(s[:, 2].shape) < 0.02] = np.nan          # class 2's score: the pixel is out for every class while 2 is selected
    s[:, 0][rng.random(s[:, 0].shape) < 0.05] = np.nan          # the background's score is never looked at
    ref = R.hysteresis(s, R.LOW, R.HIGH)
    clean = R.expected(shape, 4, False)
    assert (ref != clean).any() and (ref != 0).any() and (ref[np.isnan(s[:, 2])] == 0).all()
    assert np.array_equal(_dev(s, R.LOW, R.HIGH), ref)
    only = R.hysteresis(s, R.LOW, R.HIGH, classes=(1, 3))
    assert (only[np.isnan(s[:, 2])] != 0).any() and np.array_equal(_dev(s, R.LOW, R.HIGH, classes=(1, 3)), only)
    z = np.array(R.case(shape, 4, True))
    z[:, 0][rng.random(z[:, 0].shape) < 0.02] = np.nan          # a NaN logit makes the pixel's whole softmax NaN
    ref = R.hysteresis(z, R.LOW, R.HIGH, from_logits=True)
    assert (ref[np.isnan(z[:, 0])] == 0).all() and np.array_equal(_dev(z, R.LOW, R.HIGH, from_logits=True), ref)
    one = np.array(R.case(shape, 1, True))
    one[rng.random(one.shape) < 0.02] = np.nan
    assert np.array_equal(_dev(one, R.LOW, R.HIGH, from_logits=True), R.hysteresis(one, R.LOW, R.HIGH, from_logits=True))
    for Cn in (4, 1):
        assert (_dev(R.case(shape, Cn, False), R.LOW, float("inf")) == 0).all()
        assert (_dev(R.case(shape, Cn, False), float("inf"), float("inf"), background=5) == 5).all()
    assert (_dev(R.case(shape, 4, False), float("-inf"), float("-inf")) != 0).all()             # everything is a seed


def test_a_recycled_workspace():
    """A dense 256 x 256 call leaves large area words and flags behind; the 16 x 16 call after it must not see them."""
    from uaps_amd import hysteresis
    dense = torch.full((2, 4, 256, 256), 0.1, device=DEV)
    dense[:, 1] = 0.9
    assert (hysteresis(dense, 0.25, 0.5) == 1).all()
    for shape in ((2, 16, 16), (2, 17, 65)):
        for connectivity in (4, 8):
            assert np.array_equal(_dev(R.case(shape, 4, False), R.LOW, R.HIGH, connectivity=connectivity, min_area=5),
                                  R.expected(shape, 4, False, False, connectivity, 5))
    m = torch.from_numpy(np.array(CR.rings(2, 16, 16))).to(DEV)
    from uaps_amd import reconstruct
    assert (reconstruct(m, torch.zeros_like(m, dtype=torch.bool), 4)[(m >= 1) & (m <= 3)] == 0).all()


@pytest.mark.parametrize("connectivity", (4, 8))
def test_properties_on_the_device(connectivity):
    from uaps_amd import components, hysteresis, reconstruct
    for shape in ((2, 37, 53), (2, 130, 161), (2, 256, 256)):
        for Cn in (4, 1):
            s = torch.from_numpy(np.array(R.case(shape, Cn, False))).to(DEV)
            kw = {"connectivity": connectivity}
            sel = s[:, 1:] if Cn == 4 else s
            best, k = sel.max(dim=1)
            cls = k + 1
            zero = torch.zeros_like(cls)
            hyst = hysteresis(s, R.LOW, R.HIGH, **kw)
            # low == high: the plain threshold mask
            for t in (R.LOW, R.HIGH):
                assert torch.equal(hysteresis(s, t, t, **kw), torch.where(best >= t, cls, zero))
            # hysteresis is reconstruction of the candidate mask from the seed mask
            cand, seed = torch.where(best >= R.LOW, cls, zero), best >= R.HIGH
            rec = reconstruct(cand, seed, max(Cn, 2), **kw)
            assert torch.equal(hyst, rec) and not torch.equal(hyst, cand) and (hyst != 0).any()
            assert torch.equal(reconstruct(cand, seed.to(torch.uint8) * 200, max(Cn, 2), **kw), rec)
            assert torch.equal(reconstruct(rec, seed, max(Cn, 2), **kw), rec)                   # idempotent
            assert torch.equal(reconstruct(cand, torch.ones_like(seed), max(Cn, 2), **kw), cand)
            if Cn == 4:
                gone = reconstruct(cand, torch.zeros_like(seed), 4, classes=(1, 3), **kw)
                assert torch.equal(gone, torch.where(cand == 2, cand, zero)) and (gone != 0).any()
            # raising `high` gives a subset
            higher = hysteresis(s, R.LOW, 0.9, **kw)
            assert torch.equal(higher != 0, (higher != 0) & (hyst != 0)) and torch.equal(higher[higher != 0], hyst[higher != 0])
            assert Cn == 1 or int((higher != 0).sum()) < int((hyst != 0).sum())      # (one class: every region keeps a seed above 0.9)
            # min_area = n is area opening afterwards
            for n in (2, 5, 50):
                opened = components(hyst, [("area_open", n)], max(Cn, 2), **kw)
                assert torch.equal(hysteresis(s, R.LOW, R.HIGH, min_area=n, **kw), opened)
            assert Cn == 1 or not torch.equal(opened, hyst)
            # two runs give the same bits
            assert torch.equal(hysteresis(s, R.LOW, R.HIGH, **kw), hyst)


def test_reconstruct_equals_scipy_with_ignore_labels_and_unselected_classes():
    for shape in ((2, 37, 53), (2, 130, 161)):
        m = np.array(CR.rings(*shape))
        k = np.random.default_rng(5).random(m.shape) < 0.03
        for connectivity in (4, 8):
            for kw in ({}, {"classes": (3, 1)}, {"background": 2}, {"min_area": 5}):
                ref = R.reconstruct(m, k, 4, connectivity=connectivity, **kw)
                got = _rec(m, k, connectivity=connectivity, **kw)
                assert np.array_equal(got, ref), (shape, kw)
                assert (ref != m).any() and np.array_equal(got == 255, m == 255)


# ------------------------------------------------------------------------------------------------ inference
def _stub(classes):
    from test_morph_host import Stub, _batches
    x = _batches(Stub(3, 4), 1)[0][0]
    return Stub(3, classes, heads=2).to(DEV), x.to(DEV)


def _same(res, ref):
    assert torch.equal(res.labels, ref.labels) and torch.equal(res.count, ref.count) and torch.equal(res.table, ref.table)


def test_predict_instances_with_hysteresis_on_the_device():
    from uaps_amd import consistency, inference, label_instances
    from uaps_amd.tiled import predict_tiled
    from uaps_amd.tta import predict_tta
    net, x = _stub(4)
    lo, hi = 0.3, 0.6
    with torch.no_grad():
        main, aux = net(x)
    assert R.margin(main.cpu().numpy(), [lo, hi], True) >= NET_MARGIN
    for connectivity in (4, 8):
        ref_mask = R.hysteresis(main.cpu().numpy(), lo, hi, True, connectivity=connectivity)
        assert R.informative(ref_mask, main.cpu().numpy(), lo, hi, True)
        assert (ref_mask != main.argmax(1).cpu().numpy()).any()
        maps = (torch.softmax(main, dim=1).amax(dim=1), consistency.uncertainty_map(main, aux))
        ref = label_instances(torch.from_numpy(ref_mask).to(DEV), maps, connectivity=connectivity)
        _same(inference.predict_instances(net, x, hysteresis=(lo, hi), connectivity=connectivity), ref)
    assert int(ref.count.sum()) > 0
    # tta: the sum of the views' probability maps; tiled: the blended probabilities.  The reference reads the same fp32 maps.
    t = predict_tta(net, x, scales=(1.0, 0.5), want=("probs", "conf"))
    probs = t.probs.cpu().numpy()
    ref_mask = R.hysteresis(probs, 4 * lo, 4 * hi)
    assert R.informative(ref_mask, probs, 4 * lo, 4 * hi)
    ref = label_instances(torch.from_numpy(ref_mask).to(DEV), (t.conf, consistency.uncertainty_map(main, aux)))
    _same(inference.predict_instances(net, x, tta=(1.0, 0.5), hysteresis=(4 * lo, 4 * hi)), ref)
    tl = predict_tiled(net, x, tile=16, overlap=4, uncertainty="auto", want=("probs", "conf"))
    probs = tl.probs.cpu().numpy()
    ref_mask = R.hysteresis(probs, lo, hi, connectivity=4, min_area=2)
    assert R.informative(ref_mask, probs, lo, hi)
    ref = label_instances(torch.from_numpy(ref_mask).to(DEV), (tl.conf,) + tuple(tl.maps), connectivity=4)
    _same(inference.predict_instances(net, x, tiled={"tile": 16, "overlap": 4}, hysteresis={"low": lo, "high": hi, "min_area": 2},
                                      connectivity=4), ref)


def test_one_channel_model_on_the_device():
    from uaps_amd import inference, label_instances
    net, x = _stub(1)
    lo, hi = 0.15, 0.3
    with torch.no_grad():
        main, _ = net(x)
    z = main.cpu().numpy()
    assert R.margin(z, [lo, hi], True) >= NET_MARGIN
    ref_mask = R.hysteresis(z, lo, hi, True)
    assert R.informative(ref_mask, z, lo, hi, True) and set(np.unique(ref_mask)) == {0, 1}
    p = torch.sigmoid(main)[:, 0]
    ref = label_instances(torch.from_numpy(ref_mask).to(DEV), (torch.maximum(p, 1 - p),))
    res = inference.predict_instances(net, x, hysteresis=(lo, hi))
    _same(res, ref)
    assert int(res.count.sum()) > 0
    with pytest.raises(ValueError, match="hysteresis="):
        inference.predict_instances(net, x)
    for kw in ({"tta": True}, {"tiled": {"tile": 16, "overlap": 4}}):
        with pytest.raises(ValueError):
            inference.predict_instances(net, x, hysteresis=(lo, hi), **kw)

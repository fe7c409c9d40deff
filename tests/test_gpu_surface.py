"""Boundary metrics on the GPU (csrc/surface.hip) against scipy (tests/surface_ref.py).  Tables and distance transforms are integers
and are compared bit for bit.

Shapes: 1 x 1 and 1 x 45 are degenerate; 7 x 300 has a row longer than a 256-lane workgroup; 37 x 53 and 130 x 70 are ragged in both
directions, with several images that must not leak into each other; 256 x 256 is the workload's own; 3 x 4096 and 4096 x 2 sit at the
size limit, where the corner-pixel pattern gives d2 = 4095^2 + 4 = 16,769,029.  That is still 8,187 below 2^24 = 16,777,216, so
301 x 4096 is added for that pattern alone: 300^2 + 4095^2 = 16,859,025 is above 2^24 and odd, a squared distance fp32 cannot hold.

The blob patterns must leave at least half of the (image, class) pairs valid, asserted on the reference's table before the device is
asked; seeds 1 and 2 do on every shape that can (0.75 at the least).  A 1 x 1 image holds one label, so at most one of its four pairs
can be valid: seed 1 reaches that."""
import math

import numpy as np
import pytest
import torch

import surface_ref as R

pytestmark = pytest.mark.gpu
DEV = R.DEV
SHAPES = ((1, 1, 1), (1, 1, 45), (1, 7, 300), (3, 37, 53), (2, 130, 70), (2, 256, 256), (1, 3, 4096), (1, 4096, 2))
CASES = [(n, None) for n in R.PATTERNS if n != "blobs"] + [("blobs", 1), ("blobs", 2)]
ident = lambda s: "x".join(map(str, s))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _run(p, t, C=4, **kw):
    from uaps_amd import surface_distances
    res = surface_distances(_dev(p), _dev(t), C, **kw)
    assert res.table.is_cuda and res.table.dtype == torch.int64
    return res.table.cpu().numpy()


def _check_blobs(ref, shape, C=4):
    B, H, W = shape
    if H * W == 1:
        assert int(((ref[..., 0] > 0) & (ref[..., 1] > 0)).sum()) <= 1
    else:
        assert R.valid_fraction(ref) >= 0.5, shape


@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_device_table_equals_scipy(shape):
    for name, seed in CASES:
        (p, t), ref = R.case(name, shape, 4, seed)
        if name == "blobs":
            _check_blobs(ref, shape)
            if shape == (1, 1, 1) and seed == 1:
                assert R.valid_fraction(ref) == 0.25
        got = _run(p, t)
        assert np.array_equal(got, ref), (name, seed, shape, np.argwhere(got != ref)[:4].tolist())
    if shape[1:] in ((3, 4096), (4096, 2)):
        _, ref = R.case("corners", shape)
        assert ref[0, 1, 2] == ref[0, 1, 3] == (shape[1] - 1) ** 2 + (shape[2] - 1) ** 2


def test_a_squared_distance_above_two_to_the_24():
    from uaps_amd import distance_transform_sq
    shape = (1, 301, 4096)
    (p, t), ref = R.case("corners", shape, 2)
    d2 = 300 ** 2 + 4095 ** 2
    assert d2 > 2 ** 24 and float(np.float32(d2)) != d2 and ref[0, 1].tolist()[:4] == [1, 1, d2, d2] and ref[0, 1, 10] == d2
    assert np.array_equal(_run(p, t, 2), ref)
    edt = distance_transform_sq(_dev(p) == 0)                   # the distance to the one pixel in the corner
    assert int(edt[0, 300, 4095]) == d2 and int(edt.max()) == d2 and int(edt[0, 0, 0]) == 0


@pytest.mark.parametrize("C", (1, 8))
def test_one_and_eight_classes(C):
    shape = (3, 37, 53)
    for name, seed in (("blobs", 1), ("blobs", 2), ("noise", None), ("absent", None), ("filled", None)):
        (p, t), ref = R.case(name, shape, C, seed)
        if name == "blobs":
            _check_blobs(ref, shape, C)
        assert ref.shape == (3, C, 12) and np.array_equal(_run(p, t, C), ref), (name, seed, C)


@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_distance_transform_equals_scipy(shape):
    from uaps_amd import distance_transform_sq
    B, H, W = shape
    rng = np.random.default_rng(H + W)
    for density in (0.5, 0.97):
        m = rng.random((B + 1, H, W)) < density
        m[B] = True                                             # an image without a zero pixel
        want = np.stack([R.edt_sq(x) for x in m])
        assert bool((want[B] == R.NO_FEATURE).all())
        got = distance_transform_sq(_dev(m))
        assert got.dtype == torch.int32 and got.shape == m.shape
        assert np.array_equal(got.cpu().numpy(), want), (shape, density)
    for dtype in (torch.uint8, torch.int32, torch.int64):
        assert torch.equal(distance_transform_sq(_dev(m, dtype) * 3), got)
    assert torch.equal(distance_transform_sq(_dev(m[0])), got[0])


def test_label_dtypes_and_scores_give_the_same_bits():
    from uaps_amd import surface_distances
    for shape in ((3, 37, 53), (2, 130, 70)):
        (p, t), ref = R.case("blobs", shape, 4, 1)
        for dp in (torch.uint8, torch.int32, torch.int64):
            for dt in (torch.uint8, torch.int32, torch.int64):
                assert np.array_equal(surface_distances(_dev(p, dp), _dev(t, dt), 4).table.cpu().numpy(), ref), (dp, dt)
        scores = torch.nn.functional.one_hot(_dev(p), 4).permute(0, 3, 1, 2).float() * 0.5 + 0.25
        scores[:, 3] = scores.amax(dim=1)                       # ties: the lowest index wins
        assert np.array_equal(surface_distances(scores, _dev(t), 4).table.cpu().numpy(), ref)
    q = np.array(p)
    q[q == 3] = 200                                             # a label outside [0, C) belongs to no class
    assert np.array_equal(_run(q, t), R.table(q, t, 4))


@pytest.mark.parametrize("tolerance", (None, 1.0, 2.5))
@pytest.mark.parametrize("percentile", (50.0, 95.0, 100.0))
def test_percentile_and_tolerance(percentile, tolerance):
    for name, shape, seed in (("noise", (3, 37, 53), None), ("blobs", (2, 130, 70), 2), ("shifted", (1, 7, 300), None)):
        (p, t), _ = R.case(name, shape, 4, seed)
        assert np.array_equal(_run(p, t, percentile=percentile, tolerance=tolerance), R.table(p, t, 4, percentile, tolerance)), (name, shape)


def test_result_on_the_device():
    from uaps_amd import surface_distances
    (p, t), ref = R.case("absent", (2, 130, 70))
    res = surface_distances(_dev(p), _dev(t), 4, tolerance=2.5)
    valid = (ref[..., 0] > 0) & (ref[..., 1] > 0)
    assert res.valid.is_cuda and np.array_equal(res.valid.cpu().numpy(), valid) and not valid.all() and valid.any()
    for name in ("hd", "hd95", "asd_pg", "asd_gp", "assd", "nsd"):
        v = getattr(res, name)
        assert v.is_cuda and v.dtype == torch.float64 and np.array_equal(np.isnan(v.cpu().numpy()), ~valid), name
    for b, c in zip(*np.nonzero(valid)):
        want = R.float_metrics(p[b], t[b], c, 95.0, 2.5)
        assert float(res.hd[b, c]) == pytest.approx(want["hd"], rel=1e-14)
        assert float(res.hd95[b, c]) == pytest.approx(want["hd95"], rel=1e-9)
        for side in ("asd_pg", "asd_gp"):
            assert -1e-12 <= want[side] - float(getattr(res, side)[b, c]) <= 2.0 ** -16
        assert float(res.nsd[b, c]) == want["nsd"]
    s = res.summary()
    assert s["pairs"] == int(valid[:, 1:].sum()) and s["hd95"] == pytest.approx(float(np.nanmean(res.hd95.cpu().numpy()[:, 1:])), rel=1e-12)


def test_two_calls_same_bits_and_a_side_stream_with_recycled_workspace():
    from uaps_amd import distance_transform_sq
    (p, t), ref = R.case("blobs", (2, 130, 70), 4, 1)
    (p2, t2), ref2 = R.case("noise", (2, 130, 70))
    a, b = _run(p, t, tolerance=1.0), _run(p, t, tolerance=1.0)
    assert np.array_equal(a, b) and np.array_equal(a[..., :6], ref[..., :6])
    m = _dev(p) > 0
    e0 = distance_transform_sq(m)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        first = _run(p2, t2)                                   # dirties this stream's workspace
        c = _run(p, t, tolerance=1.0)                          # the same buffer again, not cleared in between
        e1 = distance_transform_sq(_dev(p2) > 0)
        e2 = distance_transform_sq(m)
    side.synchronize()
    assert np.array_equal(first, ref2) and np.array_equal(a, c)
    assert torch.equal(e0, e2) and not torch.equal(e0, e1)


def test_evaluate_with_surface():
    import uaps_amd
    from uaps_amd import inference
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    gen = torch.Generator().manual_seed(4)
    batches = [(torch.randn(2, 3, 64, 64, generator=gen).to(DEV), torch.randint(0, 4, (2, 64, 64), generator=gen).to(DEV)) for _ in range(2)]
    plain = inference.evaluate(model, batches)
    out = inference.evaluate(model, batches, surface={"tolerance": 2.0})
    assert all(out[k] == plain[k] for k in plain) and set(out) - set(plain) == {"HD95(px)", "ASSD(px)", "NSD(%)", "surface_pairs"}
    hd95, assd, nsd = [], [], []
    for x, y in batches:
        mask = inference.predict(model, x)[0].cpu().numpy()
        tab = R.table(mask, y.cpu().numpy(), 4, 95.0, 2.0)
        for b in range(2):
            for c in (1, 2, 3):
                r = [int(v) for v in tab[b, c]]
                if r[0] and r[1]:
                    h = float(r[0] + r[1] - 1) * (95.0 / 100.0)
                    hd95.append(math.sqrt(r[10]) + (math.sqrt(r[11]) - math.sqrt(r[10])) * (h - r[8]))
                    assd.append((r[4] / 65536.0 / r[0] + r[5] / 65536.0 / r[1]) / 2.0)
                    nsd.append((r[6] + r[7]) / (r[0] + r[1]))
    assert out["surface_pairs"] == len(hd95) > 0
    assert out["HD95(px)"] == pytest.approx(np.mean(hd95), rel=1e-9) and out["ASSD(px)"] == pytest.approx(np.mean(assd), rel=1e-12)
    assert out["NSD(%)"] == pytest.approx(100 * np.mean(nsd), rel=1e-12)
    # composes with test-time augmentation and with tiles
    tta = inference.evaluate(model, batches, tta=(1.0,), surface=True)
    assert tta["surface_pairs"] > 0 and tta["HD95(px)"] >= 0.0 and "NSD(%)" not in tta
    tiled = inference.evaluate(model, batches, tiled={"tile": 32, "overlap": 8}, surface=True)
    assert tiled["surface_pairs"] > 0 and tiled["ASSD(px)"] >= 0.0

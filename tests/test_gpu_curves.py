"""Threshold-sweep histograms on the GPU (csrc/curves.hip) against the brute-force reference (tests/curves_ref.py) and against the
module's CPU path.  Every integer output is compared exactly, pro_sum bit for bit.

The histogram kernel gives a lane four consecutive pixels (16-byte loads) where H * W is a multiple of four -- 7 x 300, 130 x 70,
256 x 256 -- and one pixel otherwise -- 1 x 1, 1 x 45, 37 x 53; a workgroup walks 1024 or 4096 pixels of one image, so 256 x 256 spans
sixteen workgroups per image and 37 x 53 two.  A workgroup holds floor(65536 / (bins * 4)) row halves in LDS (a third of that with want_sums): at 4096
bins the eight rows of C = 8 run in four groups (sixteen with want_sums), at 1024 bins with want_sums in four.

Logits: the device's expf need not round as the host's does, so the generator (curves_ref.logits) keeps every scored value 2^-18 away
from a bin edge of every bin count used here; the integer outputs then equal the float64 reference exactly.  qsum is left out of that
comparison (it carries the value itself, not its bin) and is held to the same derived error instead: 7.2e-7 * 2^24 + 1 per pixel."""
import math

import numpy as np
import pytest
import torch

import curves_ref as CR
import instances_ref as R

pytestmark = pytest.mark.gpu
DEV = CR.DEV
IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _d(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _h(a):
    return torch.from_numpy(np.array(a))


def _inst(ref, dev=DEV):
    from uaps_amd import InstanceResult
    labels, count, table = ref
    return InstanceResult(torch.from_numpy(labels).to(dev), torch.from_numpy(count).to(dev), torch.from_numpy(table).to(dev), 0)


def _same(a, b):
    for x, y in zip(a[:6], b[:6]):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x.cpu(), y.cpu())


@pytest.mark.parametrize("Cn", CR.CLASSES)
@pytest.mark.parametrize("shape", CR.SHAPES, ids=IDS)
def test_device_equals_the_reference_and_the_cpu_path(shape, Cn):
    from uaps_amd import score_curves
    for i, name in enumerate(CR.PATTERNS):
        S, t = CR.scores(name, shape, Cn), CR.targets(shape, Cn, ignored=name == "ignored")
        dS, dt = _d(S), _d(t)
        for j, bins in enumerate(CR.BINS):
            sums = (i + j) % 2 == 0
            res = score_curves(dS, dt, bins=bins, want_sums=sums)
            assert res.hist.is_cuda and res.hist.shape == (shape[0], max(Cn - 1, 1) + 1, 2, bins)
            what = f"{name} {shape} C{Cn} bins{bins} sums{sums}"
            CR.assert_result(res, CR.curves(S, t, bins=bins, want_sums=sums), what)
            if (i + j) % 3 == 0:
                _same(res, score_curves(_h(S), _h(t), bins=bins, want_sums=sums))


@pytest.mark.parametrize("Cn", CR.CLASSES)
@pytest.mark.parametrize("shape", CR.SHAPES, ids=IDS)
def test_logits_equal_the_float64_reference(shape, Cn):
    from uaps_amd import score_curves
    z, t = CR.logits(shape, Cn), CR.targets(shape, Cn, ignored=True)
    reg = R.label_batch(np.where((t >= 0) & (t < max(Cn, 2)), t, 0), (), 8, 0, 1, 64)
    dz, dt, dreg = _d(z), _d(t), _inst(reg)
    for bins in CR.BINS:
        res = score_curves(dz, dt, bins=bins, from_logits=True, regions=dreg)
        CR.assert_result(res, CR.curves(z, t, bins=bins, from_logits=True, regions=reg), f"logits {shape} C{Cn} bins{bins}")
    # the sums of the values themselves: within the derived error of a probability, per pixel
    res = score_curves(dz, dt, bins=15, from_logits=True, want_sums=True)
    ref = CR.curves(z, t, bins=15, from_logits=True, want_sums=True)
    assert np.array_equal(res.hist.cpu().numpy(), ref["hist"])
    assert np.all(np.abs(res.qsum.cpu().numpy() - ref["qsum"]) <= ref["hist"] * (7.2e-7 * 2 ** 24 + 1))


@pytest.mark.parametrize("name", ("blobs", "full", "noise"))
@pytest.mark.parametrize("shape,Cn", (((1, 1, 45), 2), ((3, 37, 53), 4), ((2, 7, 300), 1), ((2, 130, 70), 8), ((2, 256, 256), 4)), ids=IDS)
def test_regions(shape, Cn, name):
    """Sparse blobs; one region that fills image 0 with every score in one bin (all adds of the image on one word); class noise that
    overflows the 64 rows of the table."""
    from uaps_amd import score_curves
    t, reg = CR.region_case(name, shape, Cn)
    S = CR.scores("one_bin" if name == "full" else ("nans" if name == "blobs" else "uniform"), shape, Cn)
    for bins, sums in ((15, False), (1024, True), (4096, False)):
        res = score_curves(_d(S), _d(t), bins=bins, regions=_inst(reg), want_sums=sums)
        ref = CR.curves(S, t, bins=bins, regions=reg, want_sums=sums)
        CR.assert_result(res, ref, f"{name} {shape} C{Cn} bins{bins}")
        if bins == 15:
            _same(res, score_curves(_h(S), _h(t), bins=bins, regions=_inst(reg, "cpu")))
    if name == "full":
        hw = shape[1] * shape[2]
        k = res.n_regions.shape[1] - 1                                         # the class of the filling region is the last row
        assert res.n_regions[0, k] == 1 and res.pro_sum[0, k, :2049].eq(1.0).all() and res.pro_sum[0, k, 2049:].eq(0.0).all()
        assert int(res.hist[0, k, 1, 2048]) == hw
    if name == "noise" and shape[1] * shape[2] > 2000:
        assert not res.valid.any() and res.summary()["images"] == 0


def test_stale_workspace():
    """A call with many regions, then one with few on the same cached workspace: the zeroing must cover what the second reads."""
    from uaps_amd import score_curves
    shape, Cn = (2, 130, 70), 4
    t, reg = CR.region_case("noise", shape, Cn)
    S = CR.scores("uniform", shape, Cn)
    dense = score_curves(_d(S), _d(t), bins=1024, regions=_inst(reg))
    CR.assert_result(dense, CR.curves(S, t, bins=1024, regions=reg))
    t2, reg2 = CR.region_case("blobs", shape, Cn)
    sparse = score_curves(_d(S), _d(t2), bins=1024, regions=_inst(reg2))
    CR.assert_result(sparse, CR.curves(S, t2, bins=1024, regions=reg2))
    _same(dense, score_curves(_d(S), _d(t), bins=1024, regions=_inst(reg)))


def test_row_groups_at_4096_bins():
    """Seven class rows and the top row at 4096 bins: 16 row halves of 16 KB each, four to a workgroup -- four groups; with the sums
    one half fills a workgroup's LDS -- sixteen groups.  A class list in another order and with a repeat."""
    from uaps_amd import score_curves
    shape, Cn = (2, 130, 70), 8
    for name in ("uniform", "saturated", "nans"):
        S, t = CR.scores(name, shape, Cn), CR.targets(shape, Cn, ignored=True)
        for sums in (False, True):
            res = score_curves(_d(S), _d(t), bins=4096, want_sums=sums)
            assert res.hist.shape[1] == 8
            CR.assert_result(res, CR.curves(S, t, bins=4096, want_sums=sums), f"{name} sums{sums}")
    cl = [7, 0, 3, 3, 5]
    res = score_curves(_d(S), _d(t), bins=4096, classes=cl, top=False, want_sums=True)
    CR.assert_result(res, CR.curves(S, t, cl, 4096, False, want_sums=True))
    res = score_curves(_d(S), _d(t), bins=1024, classes=[], want_sums=True)          # the top row alone
    CR.assert_result(res, CR.curves(S, t, [], 1024, want_sums=True))


@pytest.mark.parametrize("bins", (1001, 1365, 1367, 3001))
def test_sums_at_odd_bin_counts(bins):
    """With the sums a group holds floor(65536 / (12 bins)) units: 5 at 1001 and 3 at 1367 bins -- an odd number of units of an odd
    number of bins, so the counters end on an odd multiple of 4 bytes and the 64-bit sums behind them must be moved to the next
    multiple of 8 -- 4 at 1365 (the neighbour on the other side of the step), 1 at 3001.  Four rows: 2, 3, 2 and 8 groups."""
    from uaps_amd import plane_curves, score_curves
    shape, Cn = (2, 130, 70), 4
    assert (65536 // (12 * bins)) == {1001: 5, 1365: 4, 1367: 3, 3001: 1}[bins]
    for name in ("uniform", "saturated", "nans"):
        S, t = CR.scores(name, shape, Cn), CR.targets(shape, Cn, ignored=True)
        res = score_curves(_d(S), _d(t), bins=bins, want_sums=True)
        CR.assert_result(res, CR.curves(S, t, bins=bins, want_sums=True), f"{name} bins{bins}")
        _same(res, score_curves(_h(S), _h(t), bins=bins, want_sums=True))
        assert torch.equal(res.hist, score_curves(_d(S), _d(t), bins=bins).hist)
    t1, reg = CR.region_case("blobs", (3, 37, 53), Cn)                            # the one-pixel form, with regions
    S1 = CR.scores("uniform", (3, 37, 53), Cn)
    res = score_curves(_d(S1), _d(t1), bins=bins, regions=_inst(reg), want_sums=True)
    CR.assert_result(res, CR.curves(S1, t1, bins=bins, regions=reg, want_sums=True), f"regions bins{bins}")
    pred = CR.targets(shape, Cn, seed=5)
    res = plane_curves(_d(S[:, 0]), _d(pred), _d(t), bins=bins, want_sums=True)   # one row: a single unit per group at 3001 bins
    CR.assert_result(res, CR.plane(S[:, 0], pred, t, bins, 0.0, 1.0, True), f"plane bins{bins}")


@pytest.mark.parametrize("lo,hi", ((0.0, 1.0), (-2.5, 7.0)))
@pytest.mark.parametrize("shape", CR.SHAPES, ids=IDS)
def test_plane_mode(shape, lo, hi):
    from uaps_amd import plane_curves
    rng = np.random.default_rng(shape[1] + shape[2])
    t = CR.targets(shape, 4, ignored=True)
    pred = np.where(rng.random(shape) < 0.3, rng.integers(0, 4, shape), t).astype(np.int64)
    e = CR.edge_values()
    with np.errstate(over="ignore", invalid="ignore"):
        edges = (e[rng.integers(0, len(e), shape)] * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)
    planes = {"uniform": (rng.random(shape, dtype=np.float32) * np.float32(hi - lo + 1) + np.float32(lo - 0.5)).astype(np.float32),
              "saturated": np.where(rng.random(shape) < 0.5, np.float32(lo), np.float32(hi)).astype(np.float32),
              "edges": edges}
    for j, (name, s) in enumerate(planes.items()):
        for i, bins in enumerate(CR.BINS):
            sums = (i + j) % 2 == 0
            for dt_p, dt_t in ((torch.int64, torch.int64), (torch.uint8, torch.int32)) if bins == 15 else ((torch.int64, torch.int64),):
                res = plane_curves(_d(s), _d(pred).to(dt_p), _d(t).to(dt_t), bins=bins, lo=lo, hi=hi, want_sums=sums)
                tt = t if dt_t == torch.int64 else t.astype(np.int32)
                CR.assert_result(res, CR.plane(s, pred, tt, bins, lo, hi, sums), f"{name} {shape} bins{bins} [{lo},{hi}]")
            if bins == 1024:
                _same(res, plane_curves(_h(s), _h(pred), _h(t), bins=bins, lo=lo, hi=hi, want_sums=sums))


def test_two_runs_same_bits_sums_on_and_off_and_a_side_stream():
    from uaps_amd import score_curves
    shape, Cn = (2, 256, 256), 4
    t, reg = CR.region_case("blobs", shape, Cn)
    z = CR.logits(shape, Cn)
    args = dict(bins=1024, from_logits=True, regions=_inst(reg), want_sums=True)
    a, b = score_curves(_d(z), _d(t), **args), score_curves(_d(z), _d(t), **args)
    _same(a, b)
    off = score_curves(_d(z), _d(t), **{**args, "want_sums": False})
    assert off.qsum is None and torch.equal(off.hist, a.hist) and torch.equal(off.pro_sum, a.pro_sum) and torch.equal(off.nan, a.nan)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    dz, dt = _d(z), _d(t)
    with torch.cuda.stream(side):
        c = score_curves(dz, dt, **args)
    side.synchronize()
    _same(a, c)
    # a view that is not 16-byte aligned takes the one-pixel form: the same histograms
    pad = torch.zeros(z.size + 1, dtype=torch.float32, device=DEV)
    pad[1:] = _d(z).reshape(-1)
    _same(a, score_curves(pad[1:].view(z.shape), dt, **args))


def test_summary_on_the_device_equals_the_host():
    from uaps_amd import score_curves
    shape, Cn = (3, 37, 53), 4
    t, reg = CR.region_case("blobs", shape, Cn)
    S = CR.scores("uniform", shape, Cn)
    dev = score_curves(_d(S), _d(t), regions=_inst(reg), want_sums=True)
    assert dev.sums().hist.is_cuda and dev.sums().pro_sum.dtype == torch.float64
    a, b = dev.summary(), score_curves(_h(S), _h(t), regions=_inst(reg, "cpu"), want_sums=True).summary()
    assert repr(a["per_class"]) == repr(b["per_class"]) and a["ECE"] == b["ECE"] and a["AUPRO"] == b["AUPRO"] and a["images"] == 3


def test_evaluate_with_curves():
    import uaps_amd
    from uaps_amd import curves, inference, label_instances, score_curves
    from uaps_amd.tiled import predict_tiled
    from uaps_amd.tta import predict_tta
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    gen = torch.Generator().manual_seed(1)
    blocks = lambda: torch.randint(0, 4, (2, 8, 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)
    batches = [(torch.randn(2, 3, 64, 64, generator=gen).to(DEV), blocks().to(DEV)) for _ in range(2)]
    plain = inference.evaluate(model, batches)
    tile = dict(tile=(32, 32), overlap=8)
    paths = (({}, True, lambda x: inference.predict(model, x)[1][0]),
             ({"tta": (1.0,)}, False, lambda x: predict_tta(model, x, scales=(1.0,), want=("probs",)).probs),
             ({"tiled": tile}, False, lambda x: predict_tiled(model, x, **tile, want=("probs",)).probs))
    for kw, from_logits, scored in paths:
        out = inference.evaluate(model, batches, curves=True, **kw)
        if not kw:
            assert all(out[k] == plain[k] for k in plain)
        total = None
        for x, y in batches:
            part = score_curves(scored(x).float(), y, from_logits=from_logits, regions=label_instances(y), want_sums=True).sums()
            total = part if total is None else total + part
        s = curves.summarize(total, [1, 2, 3])
        assert out["curve_images_skipped"] == s["images_skipped"] == 0
        for key in ("AUROC", "AP", "AUPRO", "ECE"):
            assert out[key + "(%)"] == pytest.approx(100 * s[key], rel=1e-12, nan_ok=True), (kw, key)
            assert math.isnan(out[key + "(%)"]) or 0.0 <= out[key + "(%)"] <= 100.0
        assert not math.isnan(out["AUROC(%)"]) and not math.isnan(out["ECE(%)"])
    with pytest.raises(ValueError, match="auxiliary"):                         # "unet" has the main head alone
        inference.evaluate(model, batches, curves={"uncertainty": True})
    with pytest.raises(ValueError):
        inference.evaluate(model, batches, curves={"uncertainty": True}, tta=(1.0,))
    two = uaps_amd.net_factory("unet_uaps", 3, 4, n_aux=1).to(DEV)
    unc = inference.evaluate(two, batches, curves={"uncertainty": True, "bins": 256, "hi": 4.0})
    assert 0.0 <= unc["UncAUROC(%)"] <= 100.0 and 0.0 <= unc["AURC"] <= 1.0 and 0.0 <= unc["AUROC(%)"] <= 100.0

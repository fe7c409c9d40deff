"""Boundary metrics without a GPU: the package's numpy restatement (uaps_amd/surface.py, a separable transform; no scipy) against
scipy (tests/surface_ref.py), the SurfaceResult formulas, evaluate(surface=...) around a stub network, and the C ABI's argument checks
(they return before any launch).  Tables and distance transforms are compared bit for bit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import surface_ref as R
from conftest import ROOT

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
SHAPES = ((1, 1, 1), (1, 7, 300), (3, 37, 53))
CASES = [(n, None) for n in R.PATTERNS if n != "blobs"] + [("blobs", 1), ("blobs", 2)]


def _t(a):
    return torch.from_numpy(np.array(a))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_path_equals_scipy(shape):
    from uaps_amd import SURFACE_COLUMNS, surface_distances
    assert SURFACE_COLUMNS == R.COLUMNS
    for name, seed in CASES:
        (p, t), ref = R.case(name, shape, 4, seed)
        res = surface_distances(_t(p), _t(t), 4)
        assert res.table.dtype == torch.int64 and res.table.shape == (shape[0], 4, 12)
        assert np.array_equal(res.table.numpy(), ref), (name, seed, shape)
        if name == "blobs" and shape[1] * shape[2] > 1:
            assert R.valid_fraction(ref) >= 0.5, (seed, shape)
    (p, t), _ = R.case("noise", shape)
    for q, tol in ((50.0, 1.0), (100.0, 2.5), (95.0, 0.0)):
        res = surface_distances(_t(p), _t(t), 4, percentile=q, tolerance=tol)
        assert np.array_equal(res.table.numpy(), R.table(p, t, 4, q, tol)), (q, tol, shape)


def test_known_distances():
    from uaps_amd import surface_distances
    (p, t), ref = R.case("shifted", (3, 37, 53))
    res = surface_distances(_t(p), _t(t), 4)
    assert ref[0, 1, 2] == ref[0, 1, 3] == 25 and float(res.hd[0, 1]) == pytest.approx(5.0, rel=1e-14)                # moved by (3, 4)
    (p, t), ref = R.case("corners", (1, 7, 300))
    res = surface_distances(_t(p), _t(t), 4, tolerance=1.0)
    d2 = 6 * 6 + 299 * 299
    assert res.table[0, 1].tolist() == [1, 1, d2, d2, math.isqrt(d2 << 32), math.isqrt(d2 << 32), 0, 0, 0, 1, d2, d2]
    assert float(res.nsd[0, 1]) == 0.0
    (p, t), _ = R.case("same", (3, 37, 53))
    res = surface_distances(_t(p), _t(t), 4, tolerance=0.0)
    assert int(res.table[..., 2:6].abs().sum()) == 0 and int(res.table[..., 10:].abs().sum()) == 0
    assert torch.equal(res.table[..., 6], res.table[..., 0]) and bool((res.nsd[res.valid] == 1.0).all())
    # a class that fills the image: its surface is the edge ring
    (p, t), _ = R.case("filled", (3, 37, 53))
    assert surface_distances(_t(p), _t(t), 4).table[:, 1, 0].tolist() == [2 * 37 + 2 * 53 - 4] * 3


def test_labels_dtypes_scores_and_refusals():
    from uaps_amd import surface_distances
    (p, t), ref = R.case("blobs", (3, 37, 53), 4, 1)
    for dp, dt in ((torch.uint8, torch.int64), (torch.int32, torch.uint8), (torch.int64, torch.int32)):
        assert np.array_equal(surface_distances(_t(p).to(dp), _t(t).to(dt), 4).table.numpy(), ref)
    scores = torch.nn.functional.one_hot(_t(p), 4).permute(0, 3, 1, 2).float() * 0.5 + 0.25
    scores[:, 3] = scores.amax(dim=1)                                                       # ties: the lowest index wins
    assert np.array_equal(surface_distances(scores, _t(t), 4).table.numpy(), ref)
    # a label outside [0, C) belongs to no class
    q = np.array(p)
    q[q == 3] = 200
    want = R.table(q, t, 4)
    assert np.array_equal(surface_distances(_t(q), _t(t), 4).table.numpy(), want) and int(want[:, 3, 0].sum()) == 0
    for bad in (0, 9):
        with pytest.raises(ValueError):
            surface_distances(_t(p), _t(t), bad)
    with pytest.raises(ValueError):
        surface_distances(torch.zeros(1, 4097, 2, dtype=torch.int64), torch.zeros(1, 4097, 2, dtype=torch.int64), 2)
    with pytest.raises(ValueError):
        surface_distances(_t(p), _t(t), 4, percentile=101.0)
    with pytest.raises(ValueError):
        surface_distances(_t(p), _t(t), 4, tolerance=-1.0)
    with pytest.raises(TypeError):
        surface_distances(_t(p).float(), _t(t), 4)
    with pytest.raises(TypeError):
        surface_distances(_t(p)[:, :5], _t(t), 4)


@pytest.mark.parametrize("shape", ((1, 1), (1, 45), (7, 300), (37, 53)), ids=lambda s: "x".join(map(str, s)))
def test_distance_transform_equals_scipy(shape):
    from uaps_amd import distance_transform_sq, surface
    assert surface.NO_FEATURE == R.NO_FEATURE == 2 ** 30
    rng = np.random.default_rng(shape[0] + shape[1])
    for density in (0.5, 0.97):
        m = rng.random((2,) + shape) < density
        m[1, 0, 0] = False
        got = distance_transform_sq(_t(m))
        assert got.dtype == torch.int32 and got.shape == m.shape
        assert np.array_equal(got.numpy(), np.stack([R.edt_sq(x) for x in m]))
        assert torch.equal(distance_transform_sq(_t(m.astype(np.int64) * 7)), got)
        assert torch.equal(distance_transform_sq(_t(m[1])), got[1])                         # [H,W]
    full = distance_transform_sq(torch.ones((2,) + shape, dtype=torch.uint8))
    assert bool((full == R.NO_FEATURE).all())
    with pytest.raises(ValueError):
        distance_transform_sq(torch.ones(1, 2, 4097, dtype=torch.uint8))
    with pytest.raises(TypeError):
        distance_transform_sq(torch.ones(3, 3))


def test_result_formulas_nan_valid_and_summary():
    from uaps_amd import SurfaceResult, surface_distances
    (p, t), ref = R.case("absent", (3, 37, 53))
    tol = 2.5
    res = surface_distances(_t(p), _t(t), 4, tolerance=tol)
    assert isinstance(res, SurfaceResult) and res.percentile == 95.0 and res.tolerance == tol
    valid = (ref[..., 0] > 0) & (ref[..., 1] > 0)
    assert res.valid.dtype == torch.bool and np.array_equal(res.valid.numpy(), valid) and not valid[:, 0].any() and not valid[:, 3].any()
    assert int(res.table[:, 0, 2:].abs().sum()) == 0 and int(res.table[:, 0, 1].sum()) == 0 and int(res.table[:, 0, 0].sum()) > 0
    tab = res.table.numpy()
    for name in ("hd", "hd95", "asd_pg", "asd_gp", "assd", "nsd"):
        v = getattr(res, name)
        assert v.dtype == torch.float64 and v.shape == (3, 4) and np.array_equal(np.isnan(v.numpy()), ~valid), name
    for b, c in zip(*np.nonzero(valid)):
        row = [int(v) for v in tab[b, c]]
        want = R.float_metrics(p[b], t[b], c, 95.0, tol)
        # torch's float64 sqrt is good to an ulp, not correctly rounded: a few ulps on the formulas that take roots
        assert float(res.hd[b, c]) == pytest.approx(math.sqrt(max(row[2], row[3])), rel=1e-14) and math.sqrt(max(row[2], row[3])) == want["hd"]
        h = float(row[0] + row[1] - 1) * (95.0 / 100.0)
        formula = math.sqrt(row[10]) + (math.sqrt(row[11]) - math.sqrt(row[10])) * (h - row[8])
        assert float(res.hd95[b, c]) == pytest.approx(formula, rel=1e-14)
        # float64 both, the two differ in the order of one interpolation
        assert abs(float(res.hd95[b, c]) - want["hd95"]) <= 1e-9 * max(want["hd95"], 1.0)
        assert float(res.asd_pg[b, c]) == row[4] / 65536.0 / row[0] and float(res.asd_gp[b, c]) == row[5] / 65536.0 / row[1]
        # every term of sum16 is the floor of 2^16 times the distance: the mean is below the float64 mean by less than 2^-16
        for side in ("asd_pg", "asd_gp"):
            assert -1e-12 <= want[side] - float(getattr(res, side)[b, c]) <= 2.0 ** -16
        assert float(res.assd[b, c]) == (float(res.asd_pg[b, c]) + float(res.asd_gp[b, c])) / 2.0
        assert float(res.nsd[b, c]) == (row[6] + row[7]) / (row[0] + row[1]) == want["nsd"]
    s = res.summary()
    assert s["pairs"] == int(valid[:, 1:].sum()) and set(s) == {"hd95", "assd", "hd", "nsd", "pairs"}
    for name in ("hd95", "assd", "hd", "nsd"):
        assert s[name] == pytest.approx(float(np.nanmean(getattr(res, name).numpy()[:, 1:])), rel=1e-12)
    only = res.summary(classes=[2])
    assert only["pairs"] == int(valid[:, 2].sum()) and only["hd"] == pytest.approx(float(np.nanmean(res.hd.numpy()[:, 2])), rel=1e-12)
    none = res.summary(classes=[0, 3])
    assert none["pairs"] == 0 and math.isnan(none["hd95"])
    plain = surface_distances(_t(p), _t(t), 4)
    assert "nsd" not in plain.summary() and int(plain.table[..., 6:8].abs().sum()) == 0
    with pytest.raises(ValueError):
        plain.nsd
    with pytest.raises(ValueError):
        res.summary(classes=[4])


class Stub(torch.nn.Module):
    """A seeded 1x1 convolution: a one-head "network" that runs at any size."""

    def __init__(self, cin, classes):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv2d(cin, classes, 1)

    def forward(self, x):
        return 4.0 * self.conv(x)


def _host_confusion(scored, labels):
    """The metrics kernel needs the GPU: count on the host what evaluate hands it."""
    B, Cc = scored.shape[:2]
    return torch.stack([torch.bincount(labels[b].flatten() * Cc + scored[b].argmax(0).flatten(), minlength=Cc * Cc).view(Cc, Cc)
                        for b in range(B)])


def test_evaluate_with_surface_around_a_stub(monkeypatch):
    from uaps_amd import inference, metrics, surface_distances
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    net = Stub(3, 4)
    gen = torch.Generator().manual_seed(2)
    batches = [(torch.randn(2, 3, 24, 31, generator=gen), torch.randint(0, 4, (2, 24, 31), generator=gen)) for _ in range(2)]
    plain = inference.evaluate(net, batches)
    out = inference.evaluate(net, batches, surface=True)
    assert list(out)[:4] == list(plain) and all(out[k] == plain[k] for k in plain)
    assert set(out) - set(plain) == {"HD95(px)", "ASSD(px)", "surface_pairs"}
    hd95, assd, nsd, pairs = [], [], [], 0
    with torch.no_grad():
        for x, y in batches:
            pred = net(x).argmax(1).numpy()
            for b in range(2):
                for c in (1, 2, 3):
                    if R.directed(pred[b], y[b].numpy(), c)[2] is not None:
                        m = R.float_metrics(pred[b], y[b].numpy(), c, 95.0, 2.0)
                        hd95.append(m["hd95"]); assd.append((m["asd_pg"] + m["asd_gp"]) / 2); nsd.append(m["nsd"]); pairs += 1
    assert out["surface_pairs"] == pairs > 0
    assert out["HD95(px)"] == pytest.approx(np.mean(hd95), rel=1e-9) and abs(out["ASSD(px)"] - np.mean(assd)) <= 2.0 ** -16
    both = inference.evaluate(net, batches, surface={"tolerance": 2.0, "percentile": 95.0})
    assert both["NSD(%)"] == pytest.approx(100 * np.mean(nsd), rel=1e-12) and both["HD95(px)"] == out["HD95(px)"]
    one = inference.evaluate(net, batches, surface={"classes": [2], "percentile": 100.0})
    want = [surface_distances(net(x).detach(), y, 4, percentile=100.0) for x, y in batches]
    hd = torch.cat([w.hd95[:, 2] for w in want])
    assert one["surface_pairs"] == int((~hd.isnan()).sum()) and one["HD95(px)"] == pytest.approx(float(hd.nanmean()), rel=1e-12)
    assert torch.equal(torch.cat([w.hd95 for w in want]).nan_to_num(-1), torch.cat([w.hd for w in want]).nan_to_num(-1))    # percentile 100
    assert inference.evaluate(net, batches, surface=None) == plain == inference.evaluate(net, batches, surface=False)
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, surface={"connectivity": 8})
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, surface=95)


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_edt_workspace_bytes", "uaps_edt_sq", "uaps_surface_workspace_bytes", "uaps_surface_distances"}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uaps_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    for struct, cname in ((_lib.EdtCall, "uaps_edt_call"), (_lib.SurfaceCall, "uaps_surface_call")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
        assert names == [f[0] for f in struct._fields_], (cname, names)
    assert "#define UAPS_EDT_NO_FEATURE 1073741824" in hdr and "#define UAPS_SURFACE_COLUMNS 12" in hdr


def _edt(**kw):
    from uaps_amd import _lib
    c = _lib.EdtCall()
    c.struct_size = C.sizeof(_lib.EdtCall)
    c.B, c.H, c.W, c.mask_dtype = 1, 8, 8, 1
    c.mask = c.out = c.workspace = 4096                     # never dereferenced: every call below returns before a launch
    c.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(c, k, v)
    return C.byref(c)


def _surf(**kw):
    from uaps_amd import _lib
    c = _lib.SurfaceCall()
    c.struct_size = C.sizeof(_lib.SurfaceCall)
    c.B, c.C, c.H, c.W, c.pred_dtype, c.target_dtype = 1, 4, 8, 8, 8, 8
    c.pred = c.target = c.table = c.workspace = 4096
    c.percentile_frac, c.workspace_bytes = 0.95, 1 << 40
    for k, v in kw.items():
        setattr(c, k, v)
    return C.byref(c)


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    n = C.c_size_t()
    assert L.uaps_edt_workspace_bytes(16, 256, 256, C.byref(n)) == 0 and n.value >= 2 * 16 * 256 * 256 and n.value % 256 == 0
    assert L.uaps_edt_workspace_bytes(1, 1, 1, C.byref(n)) == 0 and n.value > 0
    assert L.uaps_edt_workspace_bytes(1, 4096, 4096, C.byref(n)) == 0
    assert L.uaps_edt_workspace_bytes(0, 8, 8, C.byref(n)) == EINVAL and L.uaps_edt_workspace_bytes(1, 8, 8, None) == EINVAL
    assert L.uaps_edt_workspace_bytes(1, 4097, 8, C.byref(n)) == ERANGE and L.uaps_edt_workspace_bytes(1, 8, 4097, C.byref(n)) == ERANGE
    assert L.uaps_edt_workspace_bytes(64, 2048, 2048, C.byref(n)) == ERANGE                 # B * H * W * 8 = 2 GiB
    assert L.uaps_edt_sq(None) == EINVAL
    for field in ("mask", "out", "workspace"):
        assert L.uaps_edt_sq(_edt(**{field: None})) == EINVAL, field
    assert L.uaps_edt_sq(_edt(mask_dtype=2)) == EINVAL and L.uaps_edt_sq(_edt(W=0)) == EINVAL
    assert L.uaps_edt_sq(_edt(struct_size=C.sizeof(_lib.EdtCall) - 8)) == EINVAL           # a header without `stream`
    assert L.uaps_edt_sq(_edt(H=4097)) == ERANGE and L.uaps_edt_sq(_edt(workspace_bytes=64)) == EWORKSPACE

    assert L.uaps_surface_workspace_bytes(16, 4, 256, 256, C.byref(n)) == 0 and n.value >= 12 * 16 * 4 * 256 * 256 and n.value % 256 == 0
    assert L.uaps_surface_workspace_bytes(1, 1, 1, 1, C.byref(n)) == 0 and n.value > 0
    assert L.uaps_surface_workspace_bytes(1, 8, 4096, 4096, C.byref(n)) == 0 and n.value < 2 ** 31
    assert L.uaps_surface_workspace_bytes(1, 4, 8, 8, None) == EINVAL and L.uaps_surface_workspace_bytes(1, 4, 0, 8, C.byref(n)) == EINVAL
    assert L.uaps_surface_workspace_bytes(1, 4, 4097, 8, C.byref(n)) == ERANGE
    assert L.uaps_surface_workspace_bytes(1, 9, 8, 8, C.byref(n)) == ERANGE and L.uaps_surface_workspace_bytes(1, 0, 8, 8, C.byref(n)) == ERANGE
    assert L.uaps_surface_workspace_bytes(2, 8, 4096, 4096, C.byref(n)) == ERANGE           # a workspace beyond 2 GiB
    run = L.uaps_surface_distances
    assert run(None) == EINVAL
    for field in ("target", "table", "workspace", "pred"):
        assert run(_surf(**{field: None})) == EINVAL, field
    assert run(_surf(pred_scores=4096)) == EINVAL                                           # both forms of the prediction
    assert run(_surf(pred=None, pred_scores=4096, H=4097)) == ERANGE                        # (the scores form alone passes the pointer checks)
    assert run(_surf(pred_dtype=2)) == EINVAL and run(_surf(target_dtype=0)) == EINVAL
    assert run(_surf(percentile_frac=1.5)) == EINVAL and run(_surf(percentile_frac=float("nan"))) == EINVAL
    assert run(_surf(has_tolerance=2)) == EINVAL and run(_surf(has_tolerance=1, tol_d2=-1)) == EINVAL
    assert run(_surf(struct_size=C.sizeof(_lib.SurfaceCall) - 8)) == EINVAL
    assert run(_surf(B=0)) == EINVAL
    assert run(_surf(H=4097)) == ERANGE and run(_surf(W=4097)) == ERANGE and run(_surf(C=9)) == ERANGE and run(_surf(C=0)) == ERANGE
    assert run(_surf(workspace_bytes=64)) == EWORKSPACE

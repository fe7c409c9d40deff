"""Splitting of touching defects without a GPU: the package's CPU restatement (uaps_amd/split.py: whole-plane rounds, a union-find)
against the per-marker flood on scipy (tests/split_ref.py), the rule on hand-made maps, conservation, every refusal of the wrapper and
of the C ABI (they return before any launch) and the split= keyword of inference.predict_instances / inference.evaluate around the
stub network of the hysteresis host tests.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import instances_ref as IR
import split_ref as R
from conftest import ROOT
from test_hysteresis_host import _host_uncertainty
from test_morph_host import Stub, _batches, _host_confusion

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
SHAPES = ((1, 1), (2, 2), (1, 70), (70, 1), (3, 200), (37, 53), (64, 64), (65, 129))


def _maps(case, device="cpu"):
    return tuple(torch.from_numpy(v).to(device) for v in case.maps)


def _run(case, form, device="cpu", **kw):
    from uaps_amd import split_instances
    how = {"radius": 5.0} if form == "distance" else {"markers": torch.from_numpy(case.centres).to(device)}
    return split_instances(case.inst(device), maps=_maps(case, device), connectivity=case.connectivity, **how, **kw)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("form", ("distance", "markers"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_cpu_path_equals_the_reference(shape, form, connectivity):
    case = R.case(2, *shape, connectivity)
    for mma in (1, 4):
        ref = case.expected(form, min_marker_area=mma)                      # (asserts "informative" from 37 x 53 on)
        R.assert_equal(_run(case, form, min_marker_area=mma), ref, (shape, form, connectivity, mma))


def test_fewer_splits_at_smaller_radii_and_the_callers_distance_plane():
    from uaps_amd import split_instances
    case = R.case(2, 65, 129, 8)
    pieces = []
    for d2, radius in ((9, 3.0), (16, 4.0), (25, 5.0), (25, 4.5)):          # ceil(4.5^2) = 21 is another rule: checked below
        res = split_instances(case.inst(), radius=radius)
        marker = case.distance >= (21 if radius == 4.5 else d2)
        ref = R.split_batch(case.labels, case.table, marker)
        R.assert_equal(res, ref, radius)
        pieces.append(int((ref["pieces"] >= 2).sum()))
    assert pieces[0] <= pieces[1] <= pieces[2] and pieces[0] < pieces[2]
    plane = torch.from_numpy(case.distance).clone()
    plane[:, :, :64] = 0                                                    # the caller's plane: no core left of column 64
    ref = R.split_batch(case.labels, case.table, plane.numpy() >= 25)
    R.assert_equal(split_instances(case.inst(), radius=5, distance=plane), ref)
    assert not np.array_equal(ref["labels"], case.expected("distance", with_maps=False)["labels"])


def _bar(connectivity=8):
    from uaps_amd import split_instances
    m = np.ones((1, 1, 7), dtype=np.int64)
    inst, labels, table = R.source(m, connectivity)
    mk = np.zeros((1, 1, 7), dtype=bool)
    mk[0, 0, 0] = mk[0, 0, 6] = True
    return split_instances, inst, labels, table, mk


def test_the_tie_on_a_bar_goes_to_the_lower_marker():
    split_instances, inst, labels, table, mk = _bar()
    for connectivity in (4, 8):
        res = split_instances(inst, markers=torch.from_numpy(mk), connectivity=connectivity)
        assert res.instances.labels[0, 0].tolist() == [1, 1, 1, 1, 2, 2, 2]             # the middle pixel is 3 from both ends
        assert res.parent[0, :3].tolist() == [1, 1, 0] and res.pieces[0, :2].tolist() == [2, 0] and bool(res.converged[0])
        assert res.instances.table[0, 0].tolist() == [1, 4, 0, 0, 1, 4, 0, 0, 0] and res.instances.table[0, 1].tolist() == [1, 3, 0, 4, 1, 7, 4, 0, 0]
        R.assert_equal(res, R.split_batch(labels, table, mk, connectivity=connectivity))
        # cut short: two rounds leave the middle unowned, a piece of its own, and say so
        res = split_instances(inst, markers=torch.from_numpy(mk), connectivity=connectivity, max_iters=2)
        assert res.instances.labels[0, 0].tolist() == [1, 1, 1, 2, 3, 3, 3] and not bool(res.converged[0])
        R.assert_equal(res, R.split_batch(labels, table, mk, connectivity=connectivity, max_iters=2))
        res = split_instances(inst, markers=torch.from_numpy(mk), connectivity=connectivity, max_iters=3)
        assert res.instances.labels[0, 0].tolist() == [1, 1, 1, 1, 2, 2, 2] and bool(res.converged[0])     # exactly enough rounds
    recs = split_instances(inst, markers=torch.from_numpy(mk)).records()[0]
    assert [(r["label"], r["parent"], r["pieces_of_parent"], r["area"]) for r in recs] == [(1, 1, 2, 4), (2, 1, 2, 3)]


def test_a_diagonal_neck_is_crossed_by_8_connectivity_alone():
    from uaps_amd import split_instances
    m = np.zeros((1, 9, 9), dtype=np.int64)
    m[0, 0:4, 0:4] = 1
    m[0, 4:9, 4:9] = 1                                                      # the blocks meet at the corner (3, 3) / (4, 4) only
    mk = np.zeros((1, 9, 9), dtype=bool)
    mk[0, 0, 0] = True
    for connectivity, n_src in ((8, 1), (4, 2)):
        inst, labels, table = R.source(m, connectivity)
        assert int(inst.count[0]) == n_src
        res = split_instances(inst, markers=torch.from_numpy(mk), connectivity=connectivity)
        R.assert_equal(res, R.split_batch(labels, table, mk, connectivity=connectivity))
        assert torch.equal(res.instances.labels, inst.labels) and bool(res.converged[0])
    # under 8-connectivity the front crosses the corner: a second marker in the far block cuts the defect there
    mk[0, 8, 8] = True
    inst, labels, table = R.source(m, 8)
    res = split_instances(inst, markers=torch.from_numpy(mk))
    R.assert_equal(res, R.split_batch(labels, table, mk))
    assert int(res.instances.count[0]) == 2 and res.instances.labels[0, 3, 3] == 1
    assert res.instances.labels[0, 4, 4] == 1                               # 4 from both: the front of the lower marker crossed the corner
    assert res.instances.labels[0, 5, 5] == 2                               # 5 from (0, 0), 3 from (8, 8)


def test_no_owner_crosses_a_label():
    from uaps_amd import split_instances
    m = np.zeros((1, 5, 12), dtype=np.int64)
    m[0, :, :6], m[0, :, 6:] = 1, 2                                         # two touching defects of different classes
    mk = np.zeros((1, 5, 12), dtype=bool)
    mk[0, 2, 0] = True                                                      # one marker, in the left one
    inst, labels, table = R.source(m)
    res = split_instances(inst, markers=torch.from_numpy(mk))
    R.assert_equal(res, R.split_batch(labels, table, mk))
    assert torch.equal(res.instances.labels, inst.labels) and res.instances.table[0, :2, 0].tolist() == [1, 2]
    assert res.pieces[0, :2].tolist() == [1, 1] and bool(res.converged[0])
    # the distance form sees the union of touching defects (shape_descriptors' documented thickness): one core over the seam
    res = split_instances(inst, radius=2)
    assert torch.equal(res.instances.labels, inst.labels)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_conservation(connectivity):
    case = R.case(2, 65, 129, connectivity)
    for form in ("distance", "markers"):
        res = _run(case, form)
        src = IR.label_batch(case.mask, case.maps, connectivity, 0, 1, 256)            # the source rows with their sums
        lab, t, parent, pieces = res.instances.labels.numpy(), res.instances.table.numpy(), res.parent.numpy(), res.pieces.numpy()
        assert np.array_equal(lab > 0, case.labels > 0)                                  # the pieces partition the source
        for b in range(2):
            n = int(res.instances.count[b])
            assert n <= 256 and (parent[b, :n] > 0).all() and (parent[b, n:] == 0).all()
            assert np.array_equal(pieces[b], np.bincount(parent[b, :n], minlength=257)[1:])
            for col in (1, 7, 8):                                                        # areas and both fixed-point sums
                total = np.zeros(257, dtype=np.int64)
                np.add.at(total, parent[b, :n], t[b, :n, col])
                assert np.array_equal(total[1:], src[2][b, :, col]), (form, b, col)
            assert np.array_equal(t[b, :n, 0], src[2][b, parent[b, :n] - 1, 0])          # the source's class
            # every piece lies inside its parent
            for k in range(n):
                assert (case.labels[b][lab[b] == k + 1] == parent[b, k]).all()


def test_overflowing_tables_and_min_area():
    from uaps_amd import split_instances
    case = R.case(2, 65, 129, 8)
    for M in (1, 3):
        ref = case.expected("distance", max_instances=M)
        R.assert_equal(_run(case, "distance", max_instances=M), ref, M)
        assert (ref["count"] > M).all()                                      # count is complete whatever max_instances is
    ref = case.expected("distance", min_area=30)
    R.assert_equal(_run(case, "distance", min_area=30), ref)
    assert ref["count"].sum() < case.expected("distance")["count"].sum()
    # a source whose own table overflowed: the class of a source label above its rows is not known
    inst, labels, table = R.source(case.mask, 8, max_instances=2)
    ref = R.split_batch(labels, table, case.distance >= 25, max_instances=64)
    res = split_instances(inst, radius=5, max_instances=64)
    R.assert_equal(res, ref)
    assert (ref["table"][:, :, 0] == -1).any() and ref["pieces"].shape == (2, 2)
    assert any(r["pieces_of_parent"] is None for r in res.records()[0])


def test_argument_checks():
    from uaps_amd import split_instances
    case = R.case(2, 37, 53, 8)
    inst, mk = case.inst(), torch.from_numpy(case.centres)
    with pytest.raises(TypeError):
        split_instances(inst.labels, radius=5)
    with pytest.raises(TypeError):
        split_instances(inst._replace(labels=inst.labels.long()), radius=5)
    for kw in ({}, {"radius": 5, "markers": mk}, {"distance": torch.from_numpy(case.distance)},
               {"markers": mk, "distance": torch.from_numpy(case.distance)}, {"radius": 0}, {"radius": -1.0}, {"radius": float("nan")},
               {"radius": float("inf")}, {"radius": "5"}, {"radius": True}, {"radius": 1e6},
               {"radius": 5, "connectivity": 6}, {"radius": 5, "min_marker_area": 0}, {"radius": 5, "min_area": 0},
               {"radius": 5, "min_area": 1.5}, {"radius": 5, "max_iters": 0}, {"radius": 5, "max_iters": 65537},
               {"radius": 5, "max_instances": 0}, {"radius": 5, "_sub_iters": 17}, {"radius": 5, "_sub_iters": -1},
               {"radius": 5, "_band_rows": -1}, {"radius": 5, "maps": (torch.zeros(2, 37, 53),) * 3},
               {"markers": mk[:1]}, {"markers": mk[:, :, :50]}):
        with pytest.raises(ValueError):
            split_instances(inst, **kw)
    for kw in ({"markers": mk.float()}, {"markers": case.centres}, {"radius": 5, "distance": torch.from_numpy(case.distance).long()},
               {"radius": 5, "distance": torch.from_numpy(case.distance)[:1]}, {"radius": 5, "maps": (torch.zeros(2, 37, 53, dtype=torch.float64),)},
               {"radius": 5, "maps": (torch.zeros(2, 37, 50),)}):
        with pytest.raises(TypeError):
            split_instances(inst, **kw)
    big = inst._replace(labels=torch.zeros(1, 1, 4097, dtype=torch.int32), table=inst.table[:1])
    with pytest.raises(ValueError):
        split_instances(big, radius=5)
    from uaps_amd.split import radius_d2
    assert [radius_d2(r) for r in (5, 5.0, 4.5, 3, 0.1, np.float32(2.5))] == [25, 25, 21, 9, 1, 7]


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_split_instances", "uaps_split_workspace_bytes", "uaps_split_band_rows"}
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_split_call \{(.*?)\} uaps_split_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.SplitCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_SPLIT_[A-Z_]+) (\d+)", text))
    assert int(defines["UAPS_SPLIT_MAX_EXTENT"]) == _lib.SPLIT_MAX_EXTENT == 4096
    assert int(defines["UAPS_SPLIT_MAX_ITERS"]) == _lib.SPLIT_MAX_ITERS == 65536
    assert int(defines["UAPS_SPLIT_MAX_SUB_ITERS"]) == _lib.SPLIT_MAX_SUB_ITERS == 16
    assert C.sizeof(_lib.SplitCall) == 8 + 13 * 4 + 4 + 15 * 8              # (4 bytes of padding before the pointers)


def _call(marker_form=False, **kw):
    from uaps_amd import _lib
    c = _lib.SplitCall()
    c.struct_size = C.sizeof(_lib.SplitCall)
    c.B, c.H, c.W, c.connectivity, c.d2, c.min_marker_area, c.max_iters, c.min_area = 1, 8, 8, 8, 25, 1, 256, 1
    c.max_instances, c.source_rows = 16, 16
    # never dereferenced: every call returns before a launch
    c.source_labels, c.source_table, c.labels, c.count, c.table, c.parent, c.pieces, c.converged = (4096 * k for k in range(1, 9))
    c.workspace, c.workspace_bytes = 65536, 1 << 20
    if marker_form:
        c.markers = 40960
    else:
        c.distance = 40960
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    run = lambda c: L.uaps_split_instances(C.byref(c))
    assert L.uaps_split_instances(None) == EINVAL
    need = C.c_size_t()
    assert L.uaps_split_workspace_bytes(1, 8, 8, C.byref(need)) == 0 and need.value % 256 == 0 and need.value == 512 + 3 * 256 + 2 * 256 + 256
    for markers in (False, True):
        for name in ("source_labels", "source_table", "labels", "count", "table", "parent", "pieces", "converged", "workspace"):
            assert run(_call(markers, **{name: None})) == EINVAL, name
        assert run(_call(markers, distance=None, markers=None)) == EINVAL                   # neither form
        assert run(_call(markers, distance=40960, markers=40960)) == EINVAL                 # both
        assert run(_call(markers, map1=4096)) == EINVAL                                     # map1 without map0
        for dim in ("B", "H", "W"):
            assert run(_call(markers, **{dim: 0})) == EINVAL and run(_call(markers, **{dim: -3})) == EINVAL
        assert run(_call(markers, connectivity=5)) == EINVAL and run(_call(markers, connectivity=0)) == EINVAL
        for name in ("min_marker_area", "min_area", "max_iters", "max_instances", "source_rows"):
            assert run(_call(markers, **{name: 0})) == EINVAL and run(_call(markers, **{name: -1})) == EINVAL, name
        assert run(_call(markers, max_iters=65537)) == EINVAL
        assert run(_call(markers, d2=-1)) == EINVAL
        assert run(_call(markers, sub_iters=17)) == EINVAL and run(_call(markers, sub_iters=-2)) == EINVAL
        assert run(_call(markers, band_rows=-1)) == EINVAL and run(_call(markers, tile_cols=-1)) == EINVAL
        assert run(_call(markers, struct_size=C.sizeof(_lib.SplitCall) - 8)) == EINVAL      # a header without `stream`
        assert run(_call(markers, H=4097, workspace_bytes=1 << 40)) == ERANGE and run(_call(markers, W=4097, workspace_bytes=1 << 40)) == ERANGE
        assert run(_call(markers, B=64, H=2048, W=2048, workspace_bytes=1 << 40)) == ERANGE  # B * H * W * 8 = 2 GiB
        assert run(_call(markers, B=8, H=4096, W=4096, workspace_bytes=1 << 40)) == ERANGE   # the workspace: 24 bytes a pixel
        assert run(_call(markers, max_instances=1 << 25)) == ERANGE and run(_call(markers, source_rows=1 << 25)) == ERANGE   # tables of 2 GiB
        assert run(_call(markers, H=4096, W=4096, band_rows=4096, tile_cols=4096, workspace_bytes=1 << 40)) == ERANGE        # no such tile in LDS
        assert run(_call(markers, H=256, W=256, band_rows=64, tile_cols=64, sub_iters=16, workspace_bytes=1 << 40)) == ERANGE
        assert run(_call(markers, workspace_bytes=need.value - 1)) == EWORKSPACE             # too small
        assert run(_call(markers, workspace=65536 + 128)) == EWORKSPACE                      # misaligned
        ok = dict(workspace_bytes=need.value - 1)                                            # these pass every check but the workspace's
        assert run(_call(markers, d2=0, sub_iters=16, max_iters=65536, **ok)) == EWORKSPACE
        assert run(_call(markers, map0=4096, map1=8192, connectivity=4, band_rows=8, tile_cols=8, **ok)) == EWORKSPACE
    assert L.uaps_split_workspace_bytes(1, 8, 8, None) == EINVAL and L.uaps_split_workspace_bytes(0, 8, 8, C.byref(need)) == EINVAL
    assert L.uaps_split_workspace_bytes(1, 4097, 8, C.byref(need)) == ERANGE and L.uaps_split_workspace_bytes(8, 4096, 4096, C.byref(need)) == ERANGE
    big = C.c_size_t()
    assert L.uaps_split_workspace_bytes(2, 1024, 1024, C.byref(big)) == 0 and big.value == 2 ** 21 * 24 + 2 * 4096 * 4 + 256
    rows, cols = C.c_int(), C.c_int()
    assert L.uaps_split_band_rows(256, 256, 0, C.byref(rows), C.byref(cols)) == 0 and rows.value >= 1 and cols.value >= 1
    assert L.uaps_split_band_rows(5, 7, 16, C.byref(rows), C.byref(cols)) == 0 and (rows.value, cols.value) == (5, 7)
    assert L.uaps_split_band_rows(0, 7, 0, C.byref(rows), C.byref(cols)) == EINVAL and L.uaps_split_band_rows(8, 8, 17, C.byref(rows), C.byref(cols)) == EINVAL
    assert L.uaps_split_band_rows(8, 8, 0, None, C.byref(cols)) == EINVAL and L.uaps_split_band_rows(4097, 8, 0, C.byref(rows), C.byref(cols)) == ERANGE


RADIUS = 1.5                            # d2 = 3: the stub's blobs are a few pixels thick


def test_predict_instances_with_split(monkeypatch):
    from uaps_amd import consistency, inference, label_instances, split_instances
    from uaps_amd.split import SplitInstances
    monkeypatch.setattr(consistency, "uncertainty_map", _host_uncertainty)
    net = Stub(3, 4, heads=2)
    x = _batches(Stub(3, 4), 1)[0][0]
    main, aux = net(x)
    maps = (torch.softmax(main, dim=1).amax(dim=1), consistency.uncertainty_map(main, aux))
    plain = inference.predict_instances(net, x)
    assert all(torch.equal(a, b) for a, b in zip(inference.predict_instances(net, x, split=None)[:3], plain[:3]))
    res = inference.predict_instances(net, x, split=RADIUS)
    cut = split_instances(plain, radius=RADIUS, maps=maps)
    assert isinstance(res, SplitInstances) and res.n_maps == 2
    for a, b in zip(res[:3], cut.instances[:3]):
        assert torch.equal(a, b)
    assert torch.equal(res.split.parent, cut.parent) and torch.equal(res.split.pieces, cut.pieces) and res.split.converged.all()
    assert torch.equal(res.split.source.labels, plain.labels) and (cut.pieces >= 2).any() and not torch.equal(res.labels, plain.labels)
    # against the reference of the reference mask
    mask = inference.predict(net, x)[0].numpy()
    src, labels, table = R.source(mask)
    ref = R.split_batch(labels, table, R.distance_sq(labels) >= 3, [m.detach().numpy() for m in maps])
    R.assert_equal(res.split._replace(instances=InstanceOf(res)), ref)
    # a dict, the call's connectivity and min_area, after the clean-up chains and before the descriptors
    kw = {"radius": 1.5, "min_marker_area": 2, "max_iters": 1}
    steps = [("area_open", 4)]
    from uaps_amd import components
    clean = label_instances(components(torch.from_numpy(mask), steps, 4), maps, connectivity=4, min_area=2)
    cut = split_instances(clean, maps=maps, connectivity=4, min_area=2, **kw)
    res = inference.predict_instances(net, x, split=kw, components=steps, connectivity=4, min_area=2, shapes=True, contours=True)
    assert torch.equal(res.also.instances.labels, cut.instances.labels) and torch.equal(res.also.instances.table, cut.instances.table)
    assert not cut.converged.all() and torch.equal(res.also.instances.split.converged, cut.converged)
    from uaps_amd.tiled import predict_tiled
    from uaps_amd.tta import predict_tta
    t = predict_tta(net, x, scales=(1.0,), want=("mask", "conf"))          # (one scale and its flip: more scales smooth the necks away)
    res = inference.predict_instances(net, x, tta=(1.0,), split=RADIUS)
    cut = split_instances(label_instances(t.mask, (t.conf, maps[1])), radius=RADIUS, maps=(t.conf, maps[1]))
    assert torch.equal(res.labels, cut.instances.labels) and torch.equal(res.table, cut.instances.table) and (cut.pieces >= 2).any()
    tl = predict_tiled(net, x, tile=16, overlap=4, want=("mask", "conf"))
    res = inference.predict_instances(net, x, tiled={"tile": 16, "overlap": 4, "uncertainty": None}, split=RADIUS)
    cut = split_instances(label_instances(tl.mask, (tl.conf,)), radius=RADIUS, maps=(tl.conf,))
    assert torch.equal(res.labels, cut.instances.labels) and torch.equal(res.table, cut.instances.table) and (cut.pieces >= 2).any()
    for bad in (0, -1.0, "ab", (1.5, 2), {"min_marker_area": 2}, {"radius": 1.5, "connectivity": 4}, {"radius": float("nan")}):
        with pytest.raises(ValueError):
            inference.predict_instances(net, x, split=bad)


def InstanceOf(res):
    from uaps_amd.instances import InstanceResult
    return InstanceResult(*res[:4])


def test_evaluate_with_split(monkeypatch):
    from uaps_amd import inference, metrics
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    net = Stub(3, 4, heads=2)
    batches = _batches(Stub(3, 4))
    big = {"max_instances": 4096}
    plain = inference.evaluate(net, batches)
    inst = inference.evaluate(net, batches, instances=big)
    det = inference.evaluate(net, batches, instances=big, detection=big)
    assert inference.evaluate(net, batches, instances=big, split=None) == inst             # without the keyword every key keeps its value
    out = inference.evaluate(net, batches, instances=big, split=RADIUS)
    assert list(out) == list(inst) and all(out[k] == plain[k] for k in plain)
    assert out["defects_gt"] == inst["defects_gt"] and out["defects_pred"] > inst["defects_pred"]      # the ground truth is left alone
    both = inference.evaluate(net, batches, instances=big, detection=big, split={"radius": RADIUS, "min_marker_area": 1})
    assert list(both) == list(det) and all(both[k] == out[k] for k in out)
    assert any(both[k] != det[k] for k in ("mAP(%)", "AP50(%)", "DefectAR(%)"))
    for bad in (0, "ab", {"min_marker_area": 2}, {"radius": 1.5, "min_area": 2}):
        with pytest.raises(ValueError):
            inference.evaluate(net, batches, instances=big, split=bad)
    with pytest.raises(ValueError, match="split="):
        inference.evaluate(net, batches, split=RADIUS)                                      # nothing to split

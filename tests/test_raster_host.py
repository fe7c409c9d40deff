"""Polygon rasterisation without a GPU: the package's CPU restatement (uaps_amd/raster.py: sorted crossing keys paired into runs)
against the brute-force reference (tests/raster_ref.py: crossings counted per pixel centre) bit for bit on the traced rings of the
contour case table at both connectivities and M = 1, 3, 256, 257, on the same rings simplified at four tolerances, and on the F = 4
polygon table; the round trip rasterize(contours(inst)) == inst.labels; the partition of a convex quad into two triangles; the ring
builders; the argument checks, the C ABI's refusals (they return before any launch) and the raster= keyword of
inference.predict_instances around a stub network."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import contours_ref as R
import raster_ref as X
from conftest import ROOT
from test_bn_ref import norm_act_kernel_symbols
from test_contours_host import _inst
from test_hull_host import Stub, stub_mask
from test_simplify_host import HOST_IDS

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
FRAME_IDS = [c[0] for c in R.CASES if c[2] is None or c[2] in R.FRAMES[:5]]      # frames up to 3 x 17 x 129
assert set(FRAME_IDS) <= set(HOST_IDS)


def ring_set(tables, B, M, H, W, F, dev=None, classes=None):
    from uaps_amd import RingSet
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)) if dev is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cls = np.zeros((B, M), dtype=np.int64) if classes is None else classes
    return RingSet(put(tables[0]), put(tables[1]), put(tables[2]), put(cls), (H, W), F)


def arrays(res):
    return tuple(None if t is None else t.cpu().numpy() for t in (res.labels, res.mask, res.stats, res.overlap))


def assert_equal(got, ref, what):
    for name, a, b in zip(("labels", "mask", "stats", "overlap"), got, ref[:4]):
        if b is None:
            assert a is None, (what, name)
            continue
        assert a is not None and a.dtype == np.int64 and a.shape == b.shape, (what, name)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, name, bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])


def class_table(B, M):
    return (np.arange(B * M, dtype=np.int64).reshape(B, M) * 7 + 3) % 11


def check_case_traced(cid, dev=None, Ms=R.MS, **kw):
    """The traced rings of a contour case: the reference, the round trip and the instance table's areas."""
    from uaps_amd import contours, rasterize_contours
    case = R.case(cid)
    B, H, W = case.labels.shape
    for conn in (8, 4):
        for M in Ms:
            inst = _inst(case, M, dev)
            res = contours(inst, connectivity=conn)
            cls = class_table(B, M)
            put = torch.from_numpy(cls) if dev is None else torch.from_numpy(cls).to(dev)
            got = rasterize_contours(res, reference=True, classes=put, background=-5, **kw)
            assert got.contours is res and got.frac_bits == 0 and got.labels.device == res.points.device
            g = arrays(got)
            assert_equal(g, X.case_reference(cid, conn, None, M, -5, cls), (cid, conn, M, kw))
            inside = (case.labels >= 1) & (case.labels <= M)
            assert np.array_equal(g[0], np.where(inside, case.labels, -5))                     # the round trip
            area = case.instances(M)[1][..., 1]
            assert not g[3].any() and np.array_equal(g[2][..., 0], area) and np.array_equal(g[2][..., 1], area)
            assert np.array_equal(got.reference_area.cpu().numpy(), area)
            iou = got.iou().cpu().numpy()
            assert iou.dtype == np.float64 and np.array_equal(np.isnan(iou), area == 0) and (iou[area > 0] == 1.0).all()


def check_case_simplified(cid, dev=None, Ms=R.MS, conns=(8, 4), **kw):
    """The simplified rings of a contour case at the four tolerances, at every M; returns the overlap seen at M = 3."""
    from uaps_amd import contours, rasterize_contours, simplify_contours
    case = R.case(cid)
    seen = 0
    for conn in conns:
        for M in Ms:
            res = contours(_inst(case, M, dev), connectivity=conn)
            for e16 in X.E16S:
                s = simplify_contours(res, e16 / 16.0)
                got = rasterize_contours(s, reference=True, **kw)
                assert got.contours is s and got.mask is None
                ref = X.case_reference(cid, conn, e16, M)
                g = arrays(got)
                assert_equal(g, ref, (cid, conn, M, e16, kw))
                if M == 3:
                    seen += int(g[3].sum())
                check_iou(got, ref[2], case.instances(M)[1][..., 1])
    return seen


def check_iou(got, stats, ref_area):
    """iou() against the exact fractions, to float64 rounding (one division of exactly represented integers)."""
    iou = got.iou().cpu().numpy()
    for b, row in enumerate(X.iou_fractions(stats, ref_area)):
        for k, f in enumerate(row):
            if f is None:
                assert math.isnan(iou[b, k])
            else:
                assert iou[b, k] == f.numerator / f.denominator, (b, k, iou[b, k], f)


def check_polygon_case(name, dev=None, **kw):
    from uaps_amd import rasterize_contours
    tables, B, M, H, W = X.polygon_cases()[name]
    cls = class_table(B, M)
    planes = X.label_planes(*tables, B, H, W, M, X.F4)
    ref = X.compose(planes, B, H, W, M, 0, None, cls)
    got = rasterize_contours(ring_set(tables, B, M, H, W, X.F4, dev, cls), **kw)
    assert got.frac_bits == 4 and got.reference_area is None
    assert_equal(arrays(got), ref, (name, kw))
    return planes, ref


def check_quads(seed, dev=None, **kw):
    """Two triangles that share a diagonal cover exactly the pixels of their quad, once each, in either orientation."""
    from uaps_amd import rasterize_contours
    B, H, W = 16, 11, 13
    for reverse in (False, True):
        for diagonal in (0, 1):
            tris, quads = X.quad_tables(seed, B, H, W, reverse, diagonal)
            t = rasterize_contours(ring_set(tris, B, 2, H, W, X.F4, dev), **kw)
            q = rasterize_contours(ring_set(quads, B, 2, H, W, X.F4, dev), **kw)
            tg, qg = arrays(t), arrays(q)
            none = np.zeros((B, 2), dtype=np.int64)                     # (a RingSet carries classes: the class map is written)
            tref = X.compose(X.label_planes(*tris, B, H, W, 2, X.F4), B, H, W, 2, 0, None, none)
            qref = X.compose(X.label_planes(*quads, B, H, W, 2, X.F4), B, H, W, 2, 0, None, none)
            assert_equal(tg, tref, (seed, reverse, diagonal))
            assert_equal(qg, qref, (seed, reverse, diagonal))
            assert np.array_equal(tg[0] > 0, qg[0] > 0) and not tg[3].any() and int(tref[4].max()) == 1
            assert np.array_equal(tg[2][..., 0].sum(axis=1), qg[2][:, 0, 0]) and int(qg[2][:, 0, 0].sum()) > 100


@pytest.mark.parametrize("cid", FRAME_IDS)
def test_cpu_path_equals_the_reference_on_traced_rings_and_round_trips(cid):
    check_case_traced(cid)


@pytest.mark.parametrize("conn", (8, 4))
@pytest.mark.parametrize("cid", FRAME_IDS)
def test_cpu_path_equals_the_reference_on_simplified_rings(cid, conn):
    check_case_simplified(cid, conns=(conn,))


def test_simplified_rings_of_the_case_table_overlap():
    assert check_case_simplified("gap-3x17x129", Ms=(3,)) > 0 and check_case_simplified("noise3-3x17x129", Ms=(3,)) > 0


@pytest.mark.parametrize("cid", ("gap-3x17x129", "noise3-3x17x129"))
def test_the_array_reference_equals_the_python_integer_count_on_contour_cases(cid):
    B, H, W = R.case(cid).labels.shape
    for conn in (8, 4):
        for e16 in (None, 12, 32):                                      # traced, and where the labels overlap
            planes = X.case_planes(cid, conn, e16)
            edges = X.by_label(*X.case_tables(cid, conn, e16), B, max(R.MS))
            assert sorted(edges) == sorted(planes) and len(planes) >= 3
            for key, mine in edges.items():
                assert np.array_equal(X.plane_python_by_rows(mine, H, W, 0), planes[key]), (cid, conn, e16, key)


@pytest.mark.parametrize("name", sorted(X.polygon_cases()))
def test_cpu_path_equals_the_reference_on_the_polygon_table(name):
    planes, ref = check_polygon_case(name)
    tables, B, M, H, W = X.polygon_cases()[name]
    slow = X.label_planes(*tables, B, H, W, M, X.F4, python=True)        # the count with Python integers, a pixel at a time
    assert sorted(slow) == sorted(planes) and all(np.array_equal(slow[k], planes[k]) for k in planes)
    rows = {k: X.plane_python_by_rows(e, H, W, X.F4) for k, e in X.by_label(*tables, B, M).items()}
    assert all(np.array_equal(rows[k], planes[k]) for k in planes)


def test_the_polygon_table_is_informative():
    cases = X.polygon_cases()
    _, ref = check_polygon_case("outside")
    assert ref[0][1].min() == 1 and (ref[0][0] == 2).sum() == 0 and ref[2][0, 1, 0] == 0 and ref[2][0, 2, 0] > 0      # wholly right of the frame
    _, ref = check_polygon_case("two-points")
    assert ref[2][0, :, 0].tolist()[:2] == [0, 0] and ref[2][0, 2, 0] > 0
    planes, ref = check_polygon_case("centres")
    assert ref[0][1, 1:6, 1:6].min() == 1 and ref[2][1, 0, 0] == 25                              # [1.5, 6.5): centres on the near sides are in
    assert ref[2][2, 0, 0] + ref[2][2, 1, 0] == 64 and ref[3][2] == 0                            # the diagonal's centres go to one side
    _, rev = check_polygon_case("centres-reversed")
    assert all(np.array_equal(a, b) for a, b in zip(ref[:4], rev[:4]))                           # orientation is irrelevant
    planes, ref = check_polygon_case("even-odd")
    assert ref[0][0, 8, 8] == 0 and ref[0][0, 8, 11] == 1 and ref[2][0, 0, 0] == 36              # the pentagram's centre is out
    assert ref[0][2, 7, 7] == 5 and ref[0][2, 8, 5] == 0 and ref[0][2, 2, 2] == 2                # a label inside the hole of another
    assert ref[0][3, 8, 8] == 1 and ref[3][3] == 16 and ref[2][3, 3, 0] == 0                     # the lowest label; a ring drawn twice
    _, ref = check_polygon_case("stack")
    assert int(ref[4].max()) == 4 and ref[0][0, 5, 5] == 1 and ref[0][0, 6, 1] == 2 and ref[0][0, 1, 1] == 3 and ref[3][0] > 36
    _, ref = check_polygon_case("wide")
    assert ref[0][0, 0, 62:66].tolist() == [0, 1, 1, 1] and ref[0][0, 1, 63:67].tolist() == [1, 1, 1, 1] and ref[2][0, 1, 0] == 4
    assert ref[3][0] > 0 and ref[0].max() == 3


@pytest.mark.parametrize("seed", (1, 2, 3, 4))
def test_two_triangles_partition_their_quad(seed):
    check_quads(seed)


def test_rings_from_polygons_round_trips():
    from uaps_amd import RingSet, contours, rasterize_contours, rings_from_polygons
    case = R.case("nested-3x17x129")
    for conn in (8, 4):
        inst = _inst(case, 3)
        res = contours(inst, connectivity=conn)
        rs = rings_from_polygons(res.polygons(), size=case.labels.shape[1:], max_instances=3)
        assert isinstance(rs, RingSet) and rs.frac_bits == 0 and rs.points.dtype == torch.int32 and rs.rings.shape == (len(res.rings), 2)
        key = lambda p, o, r: sorted((int(r[i, 0]), int(r[i, 1]), tuple(map(tuple, p[o[i]:o[i + 1]].tolist()))) for i in range(len(r)))
        assert key(rs.points.numpy(), rs.ring_offsets.numpy(), rs.rings.numpy()) == key(res.points.numpy(), res.ring_offsets.numpy(), res.rings.numpy())
        got = rasterize_contours(rs, reference=inst.labels)
        assert np.array_equal(got.labels.numpy(), case.labels) and torch.equal(got.mask, torch.zeros_like(got.labels))
        assert np.array_equal(got.stats[..., 1].numpy(), case.instances(3)[1][..., 1])
        # the same polygons at F = 4: integer pixel coordinates scale exactly
        fine = rings_from_polygons(res.polygons(), 4, size=case.labels.shape[1:], max_instances=3)
        assert torch.equal(fine.points, rs.points * 16) and np.array_equal(rasterize_contours(fine).labels.numpy(), case.labels)
        recs = got.records()
        assert [r["label"] for r in recs[0]] == [1, 2, 3] and recs[0][0]["raster_area"] == int(case.instances(3)[1][0, 0, 1])
        assert recs[0][0]["raster_iou"] == 1.0


def test_rings_from_coco_quantises_and_clamps():
    from uaps_amd import rasterize_contours, rings_from_coco
    from uaps_amd.raster import quantise_points
    anns = [{"image_id": "b", "category_id": 7, "segmentation": [[1.0, 2.0, 5.03125, 2.0, 5.0, 6.09375], [0.0, 0.0, 1.0, 0.0, 1.0, 1.0]]},
            {"image_id": "a", "category_id": 9, "segmentation": [[-3.0, 1.0, 50.0, 1.0, 50.0, 40.0]]},
            {"image_id": "zz", "category_id": 7, "segmentation": [[0.0, 0.0, 1.0, 0.0, 1.0, 1.0]]},
            {"image_id": "b", "category_id": 9, "segmentation": [[2.0, 2.0, 4.0, 2.0, 4.0, 4.0]]}]
    rs = rings_from_coco(anns, ["a", "b"], {7: 1, 9: 2}, size=(8, 10))
    assert rs.frac_bits == 4 and rs.size == (8, 10) and rs.rings.tolist() == [[1, 1], [1, 1], [0, 1], [1, 2]]
    assert rs.classes.tolist() == [[2, 0], [1, 2]] and rs.ring_offsets.tolist() == [0, 3, 6, 9, 12]
    # (x, y) pairs become (y, x); floor(v 16 + 0.5): 5.03125 -> 81 (80.5 + 0.5), 6.09375 -> 98 (97.5 + 0.5); clamped into 8 x 10
    assert rs.points[:3].tolist() == [[32, 16], [32, 81], [98, 80]]
    assert rs.points[6:9].tolist() == [[16, 0], [16, 160], [128, 160]]
    assert quantise_points(np.array([[0.03125, 0.0312], [4096.5, -1.0]]), 4).tolist() == [[1, 0], [65536, 0]]
    assert quantise_points(np.array([[3, 70000]]), 2, (8, 10)).tolist() == [[12, 40]]
    same = rings_from_coco(anns, ["a", "b"], lambda c: {7: 1, 9: 2}[c], size=(8, 10))
    assert torch.equal(same.points, rs.points) and torch.equal(same.classes, rs.classes)
    got = rasterize_contours(rs)
    planes = X.label_planes(rs.points.numpy(), rs.ring_offsets.numpy(), rs.rings.numpy(), 2, 8, 10, 2, 4)
    ref = X.compose(planes, 2, 8, 10, 2, 0, None, rs.classes.numpy())
    assert_equal(arrays(got), ref, "coco")
    assert got.mask.max() == 2 and got.records()[1][0] == {"label": 1, "raster_area": int(ref[2][1, 0, 0])}
    with pytest.raises(ValueError, match="RLE"):
        rings_from_coco([{"image_id": "a", "category_id": 7, "segmentation": {"counts": "x", "size": [8, 10]}}], ["a"], {7: 1})
    with pytest.raises(ValueError, match="distinct"):
        rings_from_coco([], ["a", "a"], {})
    with pytest.raises(ValueError, match="max_instances"):
        rings_from_coco(anns, ["a", "b"], {7: 1, 9: 2}, max_instances=1)
    for bad in (5, -1, 1.0, True):
        with pytest.raises(ValueError, match="frac_bits"):
            rings_from_coco(anns, ["a", "b"], {7: 1, 9: 2}, bad)


def test_argument_checks():
    from uaps_amd import contours, label_instances, rasterize_contours
    inst = label_instances(torch.ones(1, 4, 4, dtype=torch.int64))
    res = contours(inst)
    got = rasterize_contours(res)
    assert got.labels.tolist() == [[[1] * 4] * 4] and got.mask is None and got.reference_area is None and got.stats[0, 0].tolist() == [16, 0]
    assert rasterize_contours(res, classes=True).mask.unique().tolist() == [1]
    assert rasterize_contours(res, size=(2, 6)).labels.tolist() == [[[1, 1, 1, 1, 0, 0]] * 2]
    with pytest.raises(ValueError, match="without a reference"):
        got.iou()
    for bad in (inst, None, (res.points, res.ring_offsets, res.rings)):
        with pytest.raises(TypeError, match="rasterize_contours: a contours.ContourResult"):
            rasterize_contours(bad)
    with pytest.raises(TypeError, match="points int32"):
        rasterize_contours(res._replace(points=res.points.long()))
    for size in ((0, 4), (4, 4097)):
        with pytest.raises(ValueError, match="1 <= H, W <= 4096"):
            rasterize_contours(res, size=size)
    with pytest.raises(TypeError, match="size is"):
        rasterize_contours(res, size=5)
    for ref in (inst.labels[0], inst.labels.float(), torch.zeros(1, 4, 5, dtype=torch.int32)):
        with pytest.raises(TypeError, match="the reference is an integer"):
            rasterize_contours(res, reference=ref)
    with pytest.raises(TypeError, match="classes is an integer"):
        rasterize_contours(res, classes=torch.zeros(1, 3, dtype=torch.int64))
    for cut in (-1, 4097, 1.5, True):
        with pytest.raises(ValueError, match="edge_wave_rows"):
            rasterize_contours(res, edge_wave_rows=cut)
    with pytest.raises(TypeError, match="background"):
        rasterize_contours(res, background=0.5)
    with pytest.raises(ValueError, match="2 GiB"):
        rasterize_contours(res._replace(summary=res.summary.expand(17, 256, 4)), size=(4096, 4096))      # labels of 2 GiB
    with pytest.raises(ValueError, match="ring_offsets ascend"):
        rasterize_contours(res._replace(ring_offsets=torch.tensor([2, 4], dtype=torch.int32)))


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    import uaps_amd
    from uaps_amd import raster
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("uaps_raster_workspace_bytes", "uaps_raster_plan", "uaps_raster_fill"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_raster_call \{(.*?)\} uaps_raster_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.RasterCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_RASTER_[A-Z_]+) \(?(-?\d+)\)?", text))
    assert int(defines["UAPS_RASTER_COLUMNS"]) == _lib.RASTER_COLUMNS == len(raster.RASTER_COLUMNS) == 2
    assert int(defines["UAPS_RASTER_MAX_EXTENT"]) == _lib.RASTER_MAX_EXTENT == raster.MAX_EXTENT == 4096
    assert int(defines["UAPS_RASTER_MAX_FRAC_BITS"]) == _lib.RASTER_MAX_FRAC_BITS == 4
    assert int(defines["UAPS_RASTER_WAVE_ROWS"]) == _lib.RASTER_WAVE_ROWS == raster.WAVE_ROWS
    assert int(defines["UAPS_RASTER_ALL_WAVE"]) == _lib.RASTER_ALL_WAVE == -1
    assert C.sizeof(_lib.RasterCall) == 8 * 4 + 2 * 8 + 4 * 8 + 8 + 3 * 8 + 8 + 4 * 8 + 3 * 8
    assert uaps_amd.rasterize_contours is raster.rasterize_contours and uaps_amd.RASTER_COLUMNS == ("area", "inter")
    assert uaps_amd.RasterResult._fields == ("labels", "mask", "stats", "overlap", "contours", "reference_area", "frac_bits")
    # no existing result type grew a field
    assert uaps_amd.ContourResult._fields == ("points", "ring_offsets", "rings", "summary", "instances", "connectivity", "also", "rounds")
    assert uaps_amd.SimplifiedContours._fields == ("contours", "source", "epsilon", "epsilon16", "ring_stats")


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.RasterCall()
    c.struct_size = C.sizeof(_lib.RasterCall)
    c.B, c.H, c.W, c.max_instances, c.frac_bits, c.ring_stride, c.edge_wave_rows = 1, 8, 8, 4, 0, 7, 0
    c.n_points, c.n_rings, c.n_words = 8, 2, 16
    # never dereferenced: every call below returns before a launch
    c.points, c.ring_offsets, c.rings, c.totals, c.workspace, c.workspace_bytes = 4096, 8192, 12288, 16384, 65536, 1 << 20
    c.planes, c.labels, c.stats, c.overlap = 20480, 24576, 28672, 32768
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    plan, fill = (lambda c: L.uaps_raster_plan(C.byref(c))), (lambda c: L.uaps_raster_fill(C.byref(c)))
    assert L.uaps_raster_plan(None) == EINVAL and L.uaps_raster_fill(None) == EINVAL
    for run in (plan, fill):
        for ptr in ("points", "ring_offsets", "rings", "workspace"):
            assert run(_call(**{ptr: None})) == EINVAL
        assert run(_call(ring_offsets=4096)) == EINVAL and run(_call(rings=8192)) == EINVAL            # aliased inputs
        for dim in ("B", "H", "W", "max_instances", "n_points", "n_rings"):
            assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL
        assert run(_call(frac_bits=-1)) == EINVAL and run(_call(frac_bits=5)) == EINVAL
        assert run(_call(ring_stride=1)) == EINVAL and run(_call(edge_wave_rows=-2)) == EINVAL and run(_call(edge_wave_rows=4097)) == EINVAL
        assert run(_call(struct_size=C.sizeof(_lib.RasterCall) - 8)) == EINVAL                          # a header without `stream`
        assert run(_call(H=4097)) == ERANGE and run(_call(W=4097)) == ERANGE
        assert run(_call(B=16, H=4096, W=4096)) == ERANGE                                               # labels of 2 GiB
        assert run(_call(B=32768, max_instances=4096)) == ERANGE                                        # sums of 2 GiB
        assert run(_call(n_points=2 ** 30)) == ERANGE and run(_call(n_rings=2 ** 30)) == ERANGE
    assert plan(_call(totals=None)) == EINVAL and plan(_call(totals=4096)) == EINVAL and plan(_call(totals=12288)) == EINVAL
    for ptr in ("planes", "labels", "stats", "overlap"):
        assert fill(_call(**{ptr: None})) == EINVAL
    assert fill(_call(classes=36864)) == EINVAL and fill(_call(mask=40960)) == EINVAL                   # one without the other
    assert fill(_call(labels=4096)) == EINVAL and fill(_call(stats=24576)) == EINVAL and fill(_call(overlap=20480)) == EINVAL
    assert fill(_call(classes=36864, mask=24576)) == EINVAL and fill(_call(reference=28672)) == EINVAL
    assert fill(_call(n_words=0)) == EINVAL and fill(_call(n_words=2 ** 28)) == ERANGE                  # planes of 2 GiB
    need = C.c_size_t()
    assert L.uaps_raster_workspace_bytes(8, 2, 1, 8, 8, 4, C.byref(need)) == 0 and need.value % 256 == 0
    assert 8 * 8 + 4 * 64 + 24 * 4 <= need.value <= 8 * 8 + 4 * 64 + 24 * 4 + 8 + 7 * 256             # 8 a point, 4 a pixel, 24 a label
    for run in (plan, fill):
        assert run(_call(workspace_bytes=need.value - 1)) == EWORKSPACE and run(_call(workspace=65536 + 128)) == EWORKSPACE
    assert L.uaps_raster_workspace_bytes(8, 2, 1, 8, 8, 4, None) == EINVAL and L.uaps_raster_workspace_bytes(0, 2, 1, 8, 8, 4, C.byref(need)) == EINVAL
    assert L.uaps_raster_workspace_bytes(8, 2, 1, 8, 8, 0, C.byref(need)) == EINVAL
    assert L.uaps_raster_workspace_bytes(8, 2, 1, 4097, 8, 4, C.byref(need)) == ERANGE
    assert L.uaps_raster_workspace_bytes(8, 2, 16, 4096, 4096, 4, C.byref(need)) == ERANGE


def test_census_the_raster_kernels():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libuaps_hip.so is not built")
    pattern = re.compile(r"^(?:void )?\(anonymous namespace\)::(raster_\w+(?:<[^>]*>)?)\(")
    built = norm_act_kernel_symbols(_lib.LIB_PATH, pattern)
    assert built == {"raster_zero_kernel", "raster_extent_kernel", "raster_scan_kernel", "raster_clear_kernel", "raster_edges_kernel",
                     "raster_long_kernel", "raster_paint_kernel", "raster_finish_kernel"}, sorted(built)


def check_predict_instances(net, x, ref_labels=None, **path):
    """raster=True with and without simplify=: filled against the instance labels, `.contours` what the call returned before."""
    from uaps_amd import ContourResult, RasterResult, SimplifiedContours, inference, rasterize_contours
    traced = inference.predict_instances(net, x, contours=True, hull=True, **path)
    r = inference.predict_instances(net, x, contours=True, hull=True, raster=True, **path)
    assert isinstance(r, RasterResult) and isinstance(r.contours, ContourResult) and type(r.contours.also) is type(traced.also)
    assert all(torch.equal(a, b) for a, b in zip(r.contours[:4], traced[:4]))
    labels = traced.instances.labels
    inside = (labels >= 1) & (labels <= 256)
    assert torch.equal(r.labels, torch.where(inside, labels, torch.zeros_like(labels)).long()) and not bool(r.overlap.any())
    assert torch.equal(r.stats[..., 0], traced.instances.table[..., 1]) and torch.equal(r.stats[..., 1], r.stats[..., 0])
    s = inference.predict_instances(net, x, contours=True, hull=True, simplify=1.5, raster=True, **path)
    assert isinstance(s, RasterResult) and isinstance(s.contours, SimplifiedContours) and s.contours.epsilon16 == 24
    assert all(torch.equal(a, b) for a, b in zip(s.contours.source[:4], traced[:4]))
    direct = rasterize_contours(s.contours, reference=True)
    assert s.mask is None and all(torch.equal(a, b) for a, b in zip((s.labels, s.stats, s.overlap), (direct.labels, direct.stats, direct.overlap)))
    assert torch.equal(s.reference_area, traced.instances.table[..., 1])
    fid = s.fidelity()
    assert fid["iou"].shape == (x.shape[0], 256) and len(fid["mean"]) == len(fid["min"]) == len(fid["overlap"]) == x.shape[0]
    rec = s.records()
    assert {"raster_area", "raster_iou", "rings", "solidity", "area"} <= set(rec[0][0])
    return r, s


def test_predict_instances_with_raster():
    from uaps_amd import inference
    net = Stub(stub_mask(), 4)
    x = torch.zeros(2, 3, 37, 53)
    r, s = check_predict_instances(net, x)
    fid = s.fidelity()
    # the rims of image 0 are rectangles, which epsilon 1.5 leaves as they are; the noise of image 1 is not
    assert fid["min"][0] == fid["mean"][0] == 1.0 and 0.0 <= fid["min"][1] <= fid["mean"][1] < 1.0 and np.nanmax(fid["iou"]) == 1.0
    # against the reference, from the rings the call returned
    c = s.contours.contours
    planes = X.label_planes(c.points.numpy(), c.ring_offsets.numpy(), c.rings.numpy(), 2, 37, 53, 256, 0)
    ref = X.compose(planes, 2, 37, 53, 256, 0, c.instances.labels.numpy())
    assert_equal(arrays(s), ref, "stub")
    assert isinstance(inference.predict_instances(net, x, contours=True, raster=False), type(inference.predict_instances(net, x, contours=True)))
    with pytest.raises(ValueError, match="predict_instances: raster needs contours=True"):
        inference.predict_instances(net, x, raster=True)
    for bad in ("x", 1, None):
        with pytest.raises(ValueError, match="predict_instances: raster is False or True"):
            inference.predict_instances(net, x, contours=True, raster=bad)

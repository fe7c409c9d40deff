"""Defect contours without a GPU: the package's CPU restatement (uaps_amd/contours.py: edge planes, pointer doubling, one lexsort)
against the sequential tracer (tests/contours_ref.py: a dictionary of directed edges walked ring by ring) bit for bit on the case
table, at both connectivities and M = 1, 3, 256, 257; the identities that tie every output to the instance table's area, to
shape_descriptors' crack perimeter and Euler number, to an even-odd rasterisation and to scipy's component counts; polygons(),
records() and to_coco() on a hand-written example; the argument checks, the C ABI's refusals (they return before any launch) and the
contours= keyword of inference.predict_instances around a stub network."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import contours_ref as R
from conftest import ROOT
from test_bn_ref import norm_act_kernel_symbols
from test_hull_host import Stub, stub_mask

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3


def _inst(case, M, dev=None):
    from uaps_amd.instances import InstanceResult
    count, table = case.instances(M)
    put = (lambda a: torch.from_numpy(a)) if dev is None else (lambda a: torch.from_numpy(a).to(dev))
    return InstanceResult(put(case.labels), put(count), put(table), 0)


def arrays(res):
    return (res.points.cpu().numpy(), res.ring_offsets.cpu().numpy(), res.rings.cpu().numpy(), res.summary.cpu().numpy())


def assert_equals_reference(res, case, M, conn):
    got, ref = arrays(res), case.tables(M, conn)
    B = case.labels.shape[0]
    assert [a.dtype for a in got] == [np.int32, np.int32, np.int64, np.int64]
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape and got[2].shape == ref[2].shape and got[3].shape == (B, M, 4)
    for name, a, b in zip(("points", "ring_offsets", "rings", "summary"), got, ref):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (case.id, M, conn, name, bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])
    return got


def assert_identities(got, case, M, conn, dev=None):
    from uaps_amd import shape_descriptors
    inst = _inst(case, M, dev)
    props = shape_descriptors(inst, connectivity=conn).props()
    R.check_identities(case.labels, M, conn, *got, case.instances(M)[1], props)


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_cpu_path_equals_the_reference_and_the_identities_hold(cid):
    from uaps_amd import contours, ContourResult
    case = R.case(cid)
    for conn in (8, 4):
        for M in R.MS:
            res = contours(_inst(case, M), connectivity=conn)
            assert isinstance(res, ContourResult) and res.also is None and res.connectivity == conn
            got = assert_equals_reference(res, case, M, conn)
            if M == 256:
                assert_identities(got, case, M, conn)


def test_the_case_table_is_informative():
    ids = R.CASE_IDS
    assert len(ids) == len(set(ids))
    t = lambda cid, M, conn: R.case(cid).tables(M, conn)
    # the spiral and the comb: one ring whose doubling needs every round a frame of that size can need
    for cid in ("spiral-3x17x129", "comb-3x17x129"):
        rings = t(cid, 1, 8)[2]
        assert len(rings) == 3 and rings[0, 5] > 17 * 129 and 2 ** 11 < rings[0, 5]
    assert t("comb-1x8x4096", 1, 8)[2][0, 5] > 2 ** 15 and t("spiral-1x4096x8", 1, 4)[2][0, 5] > 2 ** 15
    # the checkerboard: every interior vertex a saddle, so the connectivity changes every ring
    c8, c4 = t("checker-3x17x129", 1, 8)[2], t("checker-3x17x129", 1, 4)[2]
    assert len(c4) == 3 * ((17 * 129 + 1) // 2) and (c4[:, 5] == 4).all() and (c4[:, 6] == 2).all()
    assert (c8[:, 6] > 0).sum() == 3 and (c8[:, 6] < 0).sum() > 3 * 900 and c8[:, 5].sum() == c4[:, 5].sum()
    # both diagonal pairs: one ring of 8 edges (the saddle vertex twice among its 8 points) or two rings of 4
    for cid in ("diag-main", "diag-anti"):
        p8, o8, r8, _ = t(cid, 3, 8)
        first = p8[o8[0]:o8[1]].tolist()
        assert r8[0].tolist()[4:] == [8, 8, 4] and first.count([1, 1]) == 2
        assert [r[4:] for r in t(cid, 3, 4)[2].tolist() if r[0] == 0] == [[4, 4, 2], [4, 4, 2]]
    # nested: the hole of one label and the outer ring of the next start at the same vertex, the outer ring first
    n = t("nested-3x17x129", 3, 8)[2]
    assert n[:5, 1:4].tolist() == [[1, 0, 0], [2, 1, 1], [1, 1, 1], [3, 3, 3], [2, 3, 3]] and (n[[2, 4], 6] < 0).all() and (n[[0, 1, 3], 6] > 0).all()
    far = t("far-3x17x129", 3, 8)[3]
    assert far[0, 1].tolist() == [2, 8, 8, 4]                          # one label on two far-apart pixels: two rings
    out = R.case("outside-3x17x129")
    assert out.labels.min() == -2 ** 31 and out.labels.max() == 2 ** 31 - 1 and not t("outside-3x17x129", 257, 8)[3][:, 2:].any()
    gap = t("gap-3x17x129", 3, 8)
    assert not (gap[2][:, 0] == 1).any() and not gap[3][1].any() and gap[3][2, 0].tolist() == [1, 4, 2 * (17 + 129), 2 * 17 * 129]
    empty = t("empty-2x17x129", 3, 8)
    assert empty[0].shape == (0, 2) and empty[1].tolist() == [0] and empty[2].shape == (0, 7) and not empty[3].any()


def example():
    """6 x 7: label 1 a 4 x 5 block with a 2 x 2 hole, label 2 one pixel in that hole's top left corner, label 3 a diagonal pair."""
    m = np.zeros((1, 6, 7), dtype=np.int32)
    m[0, 0:4, 0:5] = 1
    m[0, 1:3, 1:3] = 0
    m[0, 1, 1] = 2
    m[0, 4, 5] = m[0, 5, 6] = 3
    return m


class _Example:
    id = "example"
    labels = example()

    @staticmethod
    def instances(M):
        import hull_ref
        return hull_ref.instance_table(example(), M)


def test_polygons_records_and_coco_of_a_hand_written_example():
    from uaps_amd import contours
    res = contours(_inst(_Example, 4), connectivity=8)
    assert res.rings.tolist() == [[0, 1, 0, 0, 4, 18, 40], [0, 2, 1, 1, 4, 4, 2], [0, 1, 1, 1, 4, 8, -8], [0, 3, 4, 5, 8, 8, 4]]
    assert res.ring_offsets.tolist() == [0, 4, 8, 12, 20]
    assert res.points.tolist() == [[0, 0], [0, 5], [4, 5], [4, 0],
                                   [1, 1], [1, 2], [2, 2], [2, 1],
                                   [1, 1], [3, 1], [3, 3], [1, 3],
                                   [4, 5], [4, 6], [5, 6], [5, 7], [6, 7], [6, 6], [5, 6], [5, 5]]
    assert res.summary[0].tolist() == [[2, 8, 26, 32], [1, 4, 4, 2], [1, 8, 8, 4], [0, 0, 0, 0]]
    polys = res.polygons()
    assert len(polys) == 1 and [p["label"] for p in polys[0]] == [1, 2, 3]
    assert [[a.tolist() for a in p["outer"]] for p in polys[0]] == [
        [[[0, 0], [0, 5], [4, 5], [4, 0]]], [[[1, 1], [1, 2], [2, 2], [2, 1]]],
        [[[4, 5], [4, 6], [5, 6], [5, 7], [6, 7], [6, 6], [5, 6], [5, 5]]]]
    assert [[a.tolist() for a in p["holes"]] for p in polys[0]] == [[[[1, 1], [3, 1], [3, 3], [1, 3]]], [], []]
    assert all(a.dtype == np.int32 for p in polys[0] for a in p["outer"] + p["holes"])
    recs = res.records()
    assert [(r["label"], r["area"], r["rings"], r["contour_points"], r["perimeter_crack"], r["holes_traced"]) for r in recs[0]] == [
        (1, 16, 2, 8, 26, 1), (2, 1, 1, 4, 4, 0), (3, 2, 1, 8, 8, 0)]
    coco = res.to_coco(image_ids=[41], category_of={0: 9})
    assert coco == [
        {"id": 1, "image_id": 41, "category_id": 9, "segmentation": [[0.0, 0.0, 5.0, 0.0, 5.0, 4.0, 0.0, 4.0]],
         "bbox": [0.0, 0.0, 5.0, 4.0], "area": 16.0, "iscrowd": 1},
        {"id": 2, "image_id": 41, "category_id": 9, "segmentation": [[1.0, 1.0, 2.0, 1.0, 2.0, 2.0, 1.0, 2.0]],
         "bbox": [1.0, 1.0, 1.0, 1.0], "area": 1.0, "iscrowd": 0},
        {"id": 3, "image_id": 41, "category_id": 9,
         "segmentation": [[5.0, 4.0, 6.0, 4.0, 6.0, 5.0, 7.0, 5.0, 7.0, 6.0, 6.0, 6.0, 6.0, 5.0, 5.0, 5.0]],
         "bbox": [5.0, 4.0, 2.0, 2.0], "area": 2.0, "iscrowd": 0}]
    assert [a["image_id"] for a in res.to_coco()] == [0, 0, 0] and res.to_coco(category_of=lambda c: c + 5)[0]["category_id"] == 5
    four = contours(_inst(_Example, 4), connectivity=4)                 # the diagonal pair separates
    assert four.rings.tolist()[3:] == [[0, 3, 4, 5, 4, 4, 2], [0, 3, 5, 6, 4, 4, 2]] and four.records()[0][2]["rings"] == 2


class Shaped:
    """Stands for a HullResult / ShapeResult / SkeletonStats in `also`: records() of its own."""

    def __init__(self, inst):
        self.inst = inst

    def records(self):
        recs = self.inst.records()
        for rows in recs:
            for r in rows:
                r["extra"] = 7.0
        return recs


def test_records_merge_with_also():
    from uaps_amd import contours
    res = contours(_inst(R.case("nested-3x17x129"), 3))
    recs = res.records()
    assert len(recs) == 3 and [r["label"] for r in recs[0]] == [1, 2, 3] and "extra" not in recs[0][0]
    assert [(r["rings"], r["holes_traced"]) for r in recs[1]] == [(2, 1), (2, 1), (1, 0)]
    merged = res._replace(also=Shaped(res.instances)).records()
    assert merged[1][2]["extra"] == 7.0 and merged[1][2]["perimeter_crack"] == recs[1][2]["perimeter_crack"]
    assert set(recs[0][0]) < set(merged[0][0])


def test_argument_checks():
    from uaps_amd import contours, label_instances
    from uaps_amd.instances import InstanceResult
    inst = label_instances(torch.ones(1, 4, 4, dtype=torch.int64))
    res = contours(inst)
    assert res.summary.shape == (1, 256, 4) and res.rings.tolist() == [[0, 1, 0, 0, 4, 16, 32]]
    for bad in (inst.labels, (inst.labels, inst.count, inst.table), None):
        with pytest.raises(TypeError, match="contours: an instances.InstanceResult expected"):
            contours(bad)
    for labels in (inst.labels.long(), inst.labels[0], inst.labels.float()):
        with pytest.raises(TypeError, match=r"contours: int32 \[B,H,W\] labels expected"):
            contours(InstanceResult(labels, inst.count, inst.table))
    with pytest.raises(TypeError, match="the instance table is int64"):
        contours(InstanceResult(inst.labels, inst.count, inst.table[..., :8]))
    for conn in (6, 0, "8", None):
        with pytest.raises(ValueError, match="contours: connectivity is 4 or 8"):
            contours(inst, connectivity=conn)
    with pytest.raises(ValueError, match="contours: H and W up to 4096"):
        contours(InstanceResult(torch.zeros(1, 1, 4097, dtype=torch.int32), inst.count, inst.table))
    with pytest.raises(ValueError, match="contours: empty labels"):
        contours(InstanceResult(torch.zeros(1, 0, 4, dtype=torch.int32), inst.count, inst.table))
    big = torch.zeros(1, 1, 1, dtype=torch.int32).expand(16, 2048, 2048)
    with pytest.raises(ValueError, match="2 GiB"):
        contours(InstanceResult(big, inst.count.expand(16), inst.table.expand(16, 256, 9)))


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    import uaps_amd
    from uaps_amd.contours import contours as fn, ContourResult, RING_COLUMNS, CONTOUR_COLUMNS, MAX_EXTENT
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("uaps_contours_workspace_bytes", "uaps_contours_trace", "uaps_contours_write"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_contour_call \{(.*?)\} uaps_contour_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.ContourCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_CONTOUR_[A-Z_]+) (\d+)", text))
    assert int(defines["UAPS_CONTOUR_COLUMNS"]) == _lib.CONTOUR_COLUMNS == len(CONTOUR_COLUMNS) == 4
    assert int(defines["UAPS_CONTOUR_RING_COLUMNS"]) == _lib.CONTOUR_RING_COLUMNS == len(RING_COLUMNS) == 7
    assert int(defines["UAPS_CONTOUR_MAX_EXTENT"]) == _lib.CONTOUR_MAX_EXTENT == MAX_EXTENT == 4096
    assert C.sizeof(_lib.ContourCall) == 6 * 4 + 3 * 8 + 4 * 8 + 3 * 8 + 3 * 8
    assert uaps_amd.contours is fn and uaps_amd.ContourResult is ContourResult
    assert uaps_amd.RING_COLUMNS == ("image", "label", "y", "x", "points", "length", "area2")
    assert uaps_amd.CONTOUR_COLUMNS == ("rings", "points", "perimeter", "area2")
    assert ContourResult._fields[:7] == ("points", "ring_offsets", "rings", "summary", "instances", "connectivity", "also")


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.ContourCall()
    c.struct_size = C.sizeof(_lib.ContourCall)
    c.B, c.H, c.W, c.max_instances, c.connectivity = 1, 8, 8, 4, 8
    # never dereferenced: every call below returns before a launch
    c.labels, c.summary, c.totals, c.workspace, c.workspace_bytes = 4096, 8192, 12288, 65536, 1 << 20
    c.points, c.ring_offsets, c.rings = 16384, 20480, 24576
    c.n_rings, c.n_points, c.ring_capacity, c.point_capacity = 2, 8, 2, 8
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    trace, write = (lambda c: L.uaps_contours_trace(C.byref(c))), (lambda c: L.uaps_contours_write(C.byref(c)))
    assert L.uaps_contours_trace(None) == EINVAL and L.uaps_contours_write(None) == EINVAL
    for run in (trace, write):
        assert run(_call(labels=None)) == EINVAL and run(_call(workspace=None)) == EINVAL
        for dim in ("B", "H", "W", "max_instances"):
            assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL
        for conn in (0, 6, -8):
            assert run(_call(connectivity=conn)) == EINVAL
        assert run(_call(struct_size=C.sizeof(_lib.ContourCall) - 8)) == EINVAL               # a header without `stream`
        assert run(_call(H=4097)) == ERANGE and run(_call(W=4097)) == ERANGE
        assert run(_call(B=4, H=4096, W=4096)) == ERANGE                                        # B * H * W * 32 = 2 GiB
        assert run(_call(B=4096, max_instances=16384)) == ERANGE                                # a summary of 2 GiB
    assert trace(_call(summary=None)) == EINVAL and trace(_call(totals=None)) == EINVAL
    assert trace(_call(summary=4096)) == EINVAL and trace(_call(totals=4096)) == EINVAL and trace(_call(totals=8192)) == EINVAL
    assert write(_call(points=None)) == EINVAL and write(_call(ring_offsets=None)) == EINVAL and write(_call(rings=None)) == EINVAL
    assert write(_call(n_rings=0)) == EINVAL and write(_call(n_points=3)) == EINVAL and write(_call(n_rings=2 ** 31, ring_capacity=2 ** 31)) == EINVAL
    assert write(_call(ring_capacity=1)) == EINVAL and write(_call(point_capacity=7)) == EINVAL      # smaller than the totals
    need = C.c_size_t()
    assert L.uaps_contours_workspace_bytes(1, 8, 8, 4, C.byref(need)) == 0 and need.value % 256 == 0
    assert 48 * 256 + 4 * 81 <= need.value <= 48 * 256 + 4 * 81 + 13 * 256                         # 48 bytes an edge slot, 4 a vertex
    for run in (trace, write):
        assert run(_call(workspace_bytes=need.value - 1)) == EWORKSPACE and run(_call(workspace=65536 + 128)) == EWORKSPACE
    assert L.uaps_contours_workspace_bytes(1, 8, 8, 4, None) == EINVAL and L.uaps_contours_workspace_bytes(0, 8, 8, 4, C.byref(need)) == EINVAL
    assert L.uaps_contours_workspace_bytes(1, 8, 8, 0, C.byref(need)) == EINVAL
    assert L.uaps_contours_workspace_bytes(1, 4097, 8, 4, C.byref(need)) == ERANGE
    assert L.uaps_contours_workspace_bytes(4, 4096, 4096, 4, C.byref(need)) == ERANGE


def test_census_the_contour_kernels():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libuaps_hip.so is not built")
    pattern = re.compile(r"^(?:void )?\(anonymous namespace\)::(contour_\w+(?:<[^>]*>)?)\(")
    built = norm_act_kernel_symbols(_lib.LIB_PATH, pattern)
    scans = {f"contour_{k}_kernel<{s}>" for k in ("sum", "base", "apply") for s in range(3)}
    assert built == scans | {"contour_zero_kernel", "contour_link_kernel", "contour_jump_kernel", "contour_rounds_kernel",
                             "contour_scatter_kernel", "contour_rings_kernel", "contour_write_kernel"}, sorted(built)


def test_predict_instances_with_contours():
    from uaps_amd import ContourResult, HullResult, ShapeResult, SkeletonStats, contours, inference, label_instances
    m = stub_mask()
    net = Stub(m, 4)
    x = torch.zeros(2, 3, 37, 53)
    plain = inference.predict_instances(net, x)
    assert isinstance(inference.predict_instances(net, x, contours=False), type(plain))
    for conn in (8, 4):
        base = inference.predict_instances(net, x, connectivity=conn)
        c = inference.predict_instances(net, x, contours=True, connectivity=conn)
        assert isinstance(c, ContourResult) and c.also is None and c.connectivity == conn and torch.equal(c.instances.labels, base.labels)
        direct = contours(base, connectivity=conn)
        assert all(torch.equal(a, b) for a, b in zip(c[:4], direct[:4])) and len(c.rings) > 10
        ref = R.tables(base.labels.numpy(), 256, conn)
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(c[:4], ref))
        # labelled at the same connectivity: one outer ring a defect, and the holes shape_descriptors counts
        count = base.count.numpy()
        props = inference.predict_instances(net, x, shapes=True, connectivity=conn).props()
        for b in range(2):
            rows = c.rings[c.rings[:, 0] == b].numpy()
            for k in range(1, min(int(count[b]), 256) + 1):            # (the noise image has more components than rows)
                mine = rows[rows[:, 1] == k]
                assert (mine[:, 6] > 0).sum() == 1 and (mine[:, 6] < 0).sum() == props["holes"][b, k - 1]
    assert {"rings", "contour_points", "perimeter_crack", "holes_traced", "area"} <= set(c.records()[0][0])
    ch = inference.predict_instances(net, x, contours=True, hull=True, shapes=True, skeleton=True)
    assert isinstance(ch.also, HullResult) and isinstance(ch.also.also, SkeletonStats) and isinstance(ch.also.also.shapes, ShapeResult)
    assert {"rings", "solidity", "length", "centroid_y", "area"} <= set(ch.records()[1][0])
    cs = inference.predict_instances(net, x, contours=True, shapes=True)
    assert isinstance(cs.also, ShapeResult) and torch.equal(cs.rings, inference.predict_instances(net, x, contours=True).rings)
    assert [r["perimeter_crack"] for r in cs.records()[0]] == [int(v) for v in cs.also.props()["perimeter_crack"][0, :len(cs.records()[0])]]
    for bad in ("x", 1, None, {"a": 1}):
        with pytest.raises(ValueError, match="predict_instances: contours is False or True"):
            inference.predict_instances(net, x, contours=bad)

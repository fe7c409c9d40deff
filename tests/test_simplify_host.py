"""Contour simplification without a GPU: the package's CPU restatement (uaps_amd/simplify.py: numpy arg-max, an explicit stack per
ring) against the reference (tests/simplify_ref.py: Python integers) bit for bit on the case table of the contour tests, at both
connectivities, M = 3 and 257 and eight tolerances; the properties P1-P4 that tie every output to its source without the reference;
hand-written figures with their expected outputs written out; the quantisation of epsilon, the refusals, the C ABI's refusals
(they return before any launch), the host methods and the simplify= keyword of inference.predict_instances."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import contours_ref as R
import simplify_ref as S
from conftest import ROOT
from test_bn_ref import norm_act_kernel_symbols
from test_contours_host import _Example, _inst
from test_hull_host import Stub, stub_mask

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
HOST_FRAMES = R.FRAMES[:6]                                              # up to 3 x 17 x 129 and 1 x 2 x 2100
HOST_IDS = [c[0] for c in R.CASES if c[2] is None or c[2] in HOST_FRAMES]


def arrays(s):
    c = s.contours
    return tuple(t.cpu().numpy() for t in (c.points, c.ring_offsets, c.rings, c.summary, s.ring_stats))


def assert_equal(got, ref, what):
    assert [a.dtype for a in got] == [np.int32, np.int32, np.int64, np.int64, np.int64]
    for name, a, b in zip(("points", "ring_offsets", "rings", "summary", "ring_stats"), got, ref):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)


def result_of(tables, dev=None, labels_shape=(1, 1, 1)):
    """A ContourResult around reference tables (the instances are not looked at by simplify_contours)."""
    from uaps_amd import ContourResult
    from uaps_amd.instances import InstanceResult
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if dev is None else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    B, M = tables[3].shape[:2]
    inst = InstanceResult(torch.zeros(labels_shape, dtype=torch.int32), torch.zeros(B, dtype=torch.int32), torch.zeros((B, M, 9), dtype=torch.int64), 0)
    return ContourResult(put(tables[0]), put(tables[1]), put(tables[2]), put(tables[3]), inst, 8, None, 0)


@pytest.mark.parametrize("cid", HOST_IDS)
def test_cpu_path_equals_the_reference_and_the_properties_hold(cid):
    from uaps_amd import SimplifiedContours, contours, simplify_contours
    case = R.case(cid)
    for conn in (8, 4):
        for M in (3, 257):
            res = contours(_inst(case, M), connectivity=conn)
            src = case.tables(M, conn)
            finer = None
            for e16 in S.E16S:
                got = simplify_contours(res, e16 / 16.0)
                assert isinstance(got, SimplifiedContours) and got.source is res and got.epsilon16 == e16 and got.epsilon == e16 / 16.0
                assert got.contours.instances is res.instances and got.contours.connectivity == conn and got.contours.rounds == res.rounds
                g = arrays(got)
                assert_equal(g, S.simplified(src, e16), (cid, conn, M, e16))
                if M == 3:
                    S.check_properties(src, g, e16, finer)
                    finer = g


def points_at(labels, epsilon, connectivity=8):
    from uaps_amd import simplify_contours
    t = S.ring_tables(labels, 1, connectivity)
    got = simplify_contours(result_of(t), epsilon)
    assert_equal(arrays(got), S.simplified(t, got.epsilon16), epsilon)
    return [got.contours.points[a:b].tolist() for a, b in zip(got.contours.ring_offsets[:-1].tolist(), got.contours.ring_offsets[1:].tolist())]


def test_the_staircase_collapses_to_its_corners():
    stairs = [[0, 0]] + [[y, x] for k in range(6) for (y, x) in ((k, k + 1), (k + 1, k + 1))] + [[6, 0]]
    assert points_at(S.staircase(6), 0.0) == [stairs] and len(stairs) == 14
    assert points_at(S.staircase(6), 0.75) == [[[0, 0], [6, 6], [6, 0]]]
    # the outer corners lie 1 / sqrt(2) off the diagonal (0, 0) -> (6, 6), so 0.5 keeps the steps -- all but the last one: once
    # (4, 5) is kept, (5, 5) and (5, 6) lie 1 / sqrt(5) = 0.447 off the segment (4, 5) -> (6, 6), which 0.5 does not split
    assert points_at(S.staircase(6), 0.5) == [stairs[:10] + [[6, 6], [6, 0]]]
    assert points_at(S.staircase(6), 0.4375) == [stairs]


def test_the_rectangle_stays_and_never_falls_below_a_triangle():
    box = [[0, 0], [0, 14], [6, 14], [6, 0]]
    for eps in (0.0, 0.75, 1.0, 2.0, 3.0):                              # up to its half-width
        assert points_at(S.rectangle(6, 14), eps) == [box]
    # both corners lie 84 / sqrt(232) = 5.51 off the diagonal; beyond that neither top-level interval splits and the triangle rule
    # keeps the corner of the lower index
    assert points_at(S.rectangle(6, 14), 5.5) == [box] and points_at(S.rectangle(6, 14), 5.5625) == [box[:3]]
    assert points_at(S.rectangle(6, 14), 64.0) == [box[:3]]


def test_the_plus_and_the_diamond_take_the_lowest_index_among_the_equal():
    # plus: p_0 = (0, 3), anchor b = (9, 6).  Against the segment p_0 -> p_b the points (3, 9), index 3 of (0, b), and (6, 0), index
    # 9 of (b, n), both have num = 45^2: the triangle rule's arg-max over both intervals is a tie, the lower index wins
    ring = S.ring_tables(S.plus(3))[0].tolist()
    assert ring[3] == [3, 9] and ring[6] == [9, 6] and ring[9] == [6, 0]
    assert S.deviation((3, 9), (0, 3), (9, 6)) == S.deviation((6, 0), (9, 6), (0, 3)) == (2025, 90)
    assert points_at(S.plus(3), 64.0) == [[[0, 3], [3, 9], [9, 6]]]
    assert points_at(S.plus(3), 1.0) == [ring]
    # diamond: p_0 = (0, 4), anchor b = (9, 5); (4, 9) and (5, 0) tie at num = 41^2 in the same way
    assert S.deviation((4, 9), (0, 4), (9, 5)) == S.deviation((5, 0), (9, 5), (0, 4)) == (1681, 82)
    assert points_at(S.diamond(4), 0.75) == [[[0, 4], [4, 9], [9, 5], [5, 0]]]
    assert points_at(S.diamond(4), 64.0) == [[[0, 4], [4, 9], [9, 5]]]
    # a square: the two corners next to p_0 are equally far from the diagonal
    assert points_at(np.ones((1, 5, 5), dtype=np.int32), 64.0) == [[[0, 0], [0, 5], [5, 5]]]
    # anchor b: (2, 4), index 2, and (4, 2), index 4, are equally far from p_0 = (0, 0); b is the lower index
    eq = np.zeros((1, 4, 4), dtype=np.int32)
    eq[0, :2, :] = 1
    eq[0, :, :2] = 1
    assert S.ring_tables(eq)[0].tolist() == [[0, 0], [0, 4], [2, 4], [2, 2], [4, 2], [4, 0]]
    assert points_at(eq, 64.0) == [[[0, 0], [2, 4], [4, 0]]] and points_at(eq, 1.0) == [[[0, 0], [0, 4], [2, 4], [4, 0]]]
    assert points_at(eq, 0.5) == [[[0, 0], [0, 4], [2, 4], [2, 2], [4, 2], [4, 0]]]


def test_the_checkerboard_has_segments_of_zero_length():
    labels = R.case("checker-1x2x2").labels
    t = S.ring_tables(labels, 1, 8)
    ring = t[0].tolist()
    assert len(ring) == 8 and ring.count([1, 1]) == 2                   # the saddle vertex twice
    for e16 in S.E16S:
        out = points_at(labels, e16 / 16.0)
        S.check_properties(t, S.simplified(t, e16), e16)
        assert len(out) == 1 and out[0][0] == [0, 0] and len(out[0]) >= 3
    # the definition's case for a segment of zero length, two visits of one saddle vertex: the distance to that vertex
    assert S.deviation((1, 2), (1, 1), (1, 1)) == (1, 1) and S.deviation((3, 0), (1, 1), (1, 1)) == (5, 1)
    # ... which no interval of kept points can be: against a segment that starts (or ends) at the vertex its other visit has num 0,
    # is never the arg-max of a split, and so a kept point always lies between two kept visits.  The outer ring of the large
    # checkerboard visits hundreds of saddles twice and keeps none of them twice in a row
    big = R.case("checker-3x17x129").tables(3, 8)
    p = [tuple(v) for v in big[0][big[1][0]:big[1][1]].tolist()]
    assert len(p) == 580 and len(set(p)) < len(p)
    for e16 in S.E16S:
        kept, _ = S.simplify_ring(p, e16)
        assert not [(i, j) for i, j in zip(kept, kept[1:]) if p[i] == p[j]]


def test_the_ramp_comb_has_linear_depth():
    from uaps_amd import simplify_contours
    t = S.ring_tables(S.ramp_comb(64))
    p = [tuple(v) for v in t[0].tolist()]
    assert len(t[2]) == 1 and len(p) == 256
    for e16 in (0, 12, 32):
        kept, depth = S.simplify_ring(p, e16)
        assert depth > 2 * math.log2(len(p)) and depth >= 64, (e16, depth)     # a tooth a round, not a halving
        got = simplify_contours(result_of(t), e16 / 16.0)
        assert_equal(arrays(got), S.simplified(t, e16), e16)
        S.check_properties(t, arrays(got), e16)
    assert S.simplify_ring(p, 0)[0] == list(range(256)) and len(S.simplify_ring(p, 1024)[0]) == 3


def test_quantisation_and_refusals():
    from uaps_amd import contours, inference, simplify_contours
    from uaps_amd.simplify import quantise
    assert [quantise(e) for e in (0.0, 0.03, 0.04, 0.75, 1, 2.0, 63.97, 64.0)] == [0, 0, 1, 12, 16, 32, 1024, 1024]
    res = contours(_inst(_Example, 4))
    assert simplify_contours(res, 0.03).epsilon16 == 0 and simplify_contours(res, 0.04).epsilon16 == 1
    assert simplify_contours(res).epsilon == 1.0 and simplify_contours(res, 0.04).epsilon == 0.0625
    for bad in (-0.01, float("nan"), 64.5, float("inf")):
        with pytest.raises(ValueError, match="0 <= epsilon <= 64"):
            simplify_contours(res, bad)
    for bad in ("1", None, True):
        with pytest.raises(TypeError):
            simplify_contours(res, bad)
    with pytest.raises(TypeError, match="ContourResult expected"):
        simplify_contours(res.points, 1.0)
    for kw in ({"wave_max": 65}, {"lds_max": 2049}, {"wave_max": -1}, {"lds_max": 1.5}):
        with pytest.raises(ValueError):
            simplify_contours(res, 1.0, **kw)
    net, x = Stub(stub_mask(), 4), torch.zeros(2, 3, 37, 53)
    for kw in ({}, {"contours": False}, {"hull": True}):
        with pytest.raises(ValueError, match="simplify needs contours=True"):
            inference.predict_instances(net, x, simplify=1.0, **kw)
    with pytest.raises(ValueError, match="0 <= epsilon <= 64"):
        inference.predict_instances(net, x, contours=True, simplify=-1.0)
    with pytest.raises(ValueError, match="contours is False or True"):
        inference.predict_instances(net, x, contours=1, simplify=1.0)


def test_polygons_records_and_coco_of_the_hand_written_example():
    from uaps_amd import contours, simplify_contours
    res = contours(_inst(_Example, 4), connectivity=8)
    # at 0.75 a single pixel (its corners lie 1 / sqrt(2) off its diagonal) is a triangle, by the triangle rule
    coarse = simplify_contours(res, 0.75)
    assert coarse.contours.rings[:, 4].tolist() == [4, 3, 4, 3] and coarse.contours.points[4:7].tolist() == [[1, 1], [1, 2], [2, 2]]
    assert coarse.ring_stats.tolist() == [[4, 40], [4, 1], [4, -8], [8, 2]] and coarse.contours.summary[0, :, 1].tolist() == [8, 3, 3, 0]
    s = simplify_contours(res, 0.5)
    # label 3, a diagonal pair of pixels (eight points, the saddle vertex twice), becomes the quadrilateral of its far corners
    assert s.contours.rings.tolist() == [[0, 1, 0, 0, 4, 18, 40], [0, 2, 1, 1, 4, 4, 2], [0, 1, 1, 1, 4, 8, -8], [0, 3, 4, 5, 4, 8, 4]]
    assert s.contours.ring_offsets.tolist() == [0, 4, 8, 12, 16] and s.contours.points[12:].tolist() == [[4, 5], [4, 6], [6, 7], [6, 6]]
    assert s.ring_stats.tolist() == [[4, 40], [4, 2], [4, -8], [8, 4]]
    assert s.contours.summary[0].tolist() == [[2, 8, 26, 32], [1, 4, 4, 2], [1, 4, 8, 4], [0, 0, 0, 0]]
    assert torch.equal(res.summary[0, 2], torch.tensor([1, 8, 8, 4])) and s.source is res           # the source is not touched
    polys = s.polygons()
    assert [[a.tolist() for a in p["outer"]] for p in polys[0]][2] == [[[4, 5], [4, 6], [6, 7], [6, 6]]]
    assert [[a.tolist() for a in p["holes"]] for p in polys[0]] == [[[[1, 1], [3, 1], [3, 3], [1, 3]]], [], []]   # by the source's area2
    assert [(r["label"], r["rings"], r["contour_points"], r["perimeter_crack"], r["holes_traced"]) for r in s.records()[0]] == [
        (1, 2, 8, 26, 1), (2, 1, 4, 4, 0), (3, 1, 4, 8, 0)]
    coco = s.to_coco(image_ids=[41], category_of={0: 9})
    assert coco[2] == {"id": 3, "image_id": 41, "category_id": 9, "segmentation": [[5.0, 4.0, 6.0, 4.0, 7.0, 6.0, 6.0, 6.0]],
                       "bbox": [5.0, 4.0, 2.0, 2.0], "area": 2.0, "iscrowd": 0}
    assert coco[:2] == res.to_coco(image_ids=[41], category_of={0: 9})[:2]
    assert s.reduction() == {"source_points": 20, "points": 16, "ratio": 0.8, "per_image": [(20, 16)]}
    same = simplify_contours(res, 0.0)
    assert all(torch.equal(a, b) for a, b in zip(same.contours[:4], res[:4])) and same.reduction()["ratio"] == 1.0


def test_empty_inputs_return_empty_tensors():
    from uaps_amd import contours, simplify_contours
    res = contours(_inst(R.case("empty-2x17x129"), 3))
    s = simplify_contours(res, 1.0)
    assert s.contours.points.shape == (0, 2) and s.contours.ring_offsets.tolist() == [0] and s.contours.rings.shape == (0, 7)
    assert s.ring_stats.shape == (0, 2) and not s.contours.summary.any() and s.polygons() == [[], []]
    assert s.reduction() == {"source_points": 0, "points": 0, "ratio": 1.0, "per_image": [(0, 0), (0, 0)]}


def test_predict_instances_with_simplify():
    from uaps_amd import ContourResult, HullResult, SimplifiedContours, inference, simplify_contours
    net, x = Stub(stub_mask(), 4), torch.zeros(2, 3, 37, 53)
    for conn in (8, 4):
        traced = inference.predict_instances(net, x, contours=True, hull=True, connectivity=conn)
        s = inference.predict_instances(net, x, contours=True, hull=True, simplify=1.0, connectivity=conn)
        assert isinstance(s, SimplifiedContours) and isinstance(s.source, ContourResult) and isinstance(s.contours.also, HullResult)
        assert all(torch.equal(a, b) for a, b in zip(s.source[:4], traced[:4])) and s.epsilon16 == 16
        direct = simplify_contours(traced, 1.0)
        assert all(torch.equal(a, b) for a, b in zip(s.contours[:4], direct.contours[:4])) and torch.equal(s.ring_stats, direct.ring_stats)
        src = R.tables(traced.instances.labels.numpy(), 256, conn)
        assert_equal(arrays(s), S.simplified(src, 16), conn)
        S.check_properties(src, arrays(s), 16)
        red = s.reduction()
        assert red["points"] < red["source_points"] and {"rings", "contour_points", "solidity"} <= set(s.records()[0][0])
    assert isinstance(inference.predict_instances(net, x, contours=True, simplify=None), ContourResult)


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    import uaps_amd
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("uaps_contours_simplify_workspace_bytes", "uaps_contours_simplify_mark", "uaps_contours_simplify_write"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_simplify_call \{(.*?)\} uaps_simplify_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.SimplifyCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_SIMPLIFY_[A-Z0-9_]+) \(?(-?\d+)\)?", text))
    assert int(defines["UAPS_SIMPLIFY_WAVE_MAX"]) == _lib.SIMPLIFY_WAVE_MAX == uaps_amd.simplify.WAVE_MAX == 64
    assert int(defines["UAPS_SIMPLIFY_LDS_MAX"]) == _lib.SIMPLIFY_LDS_MAX == uaps_amd.simplify.LDS_MAX == 2048
    assert int(defines["UAPS_SIMPLIFY_MAX_E16"]) == _lib.SIMPLIFY_MAX_E16 == 1024 and int(defines["UAPS_SIMPLIFY_OFF"]) == _lib.SIMPLIFY_OFF == -1
    assert C.sizeof(_lib.SimplifyCall) == 6 * 4 + 2 * 8 + 6 * 8 + 3 * 8 + 4 * 8 + 3 * 8
    assert uaps_amd.SimplifiedContours._fields == ("contours", "source", "epsilon", "epsilon16", "ring_stats")


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.SimplifyCall()
    c.struct_size = C.sizeof(_lib.SimplifyCall)
    c.B, c.max_instances, c.e16, c.n_points, c.n_rings = 1, 4, 16, 40, 3
    # never dereferenced: every call below returns before a launch
    c.points, c.ring_offsets, c.rings, c.summary_in, c.summary_out, c.totals = 4096, 8192, 12288, 16384, 20480, 24576
    c.points_out, c.ring_offsets_out, c.rings_out, c.ring_stats = 28672, 32768, 36864, 40960
    c.workspace, c.workspace_bytes = 65536, 1 << 20
    c.n_points_out, c.ring_capacity, c.point_capacity = 20, 3, 20
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    mark, write = (lambda c: L.uaps_contours_simplify_mark(C.byref(c))), (lambda c: L.uaps_contours_simplify_write(C.byref(c)))
    assert L.uaps_contours_simplify_mark(None) == EINVAL and L.uaps_contours_simplify_write(None) == EINVAL
    for run in (mark, write):
        for ptr in ("points", "ring_offsets", "rings", "workspace"):
            assert run(_call(**{ptr: None})) == EINVAL
        for dim in ("B", "max_instances", "n_points", "n_rings"):
            assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL
        assert run(_call(e16=-1)) == EINVAL and run(_call(e16=1025)) == EINVAL
        assert run(_call(wave_max=65)) == EINVAL and run(_call(lds_max=2049)) == EINVAL and run(_call(wave_max=-2)) == EINVAL
        assert run(_call(struct_size=C.sizeof(_lib.SimplifyCall) - 8)) == EINVAL                # a header without `stream`
        assert run(_call(n_points=2 ** 30)) == ERANGE and run(_call(n_rings=41)) == ERANGE and run(_call(B=4096, max_instances=16384)) == ERANGE
    assert mark(_call(summary_in=None)) == EINVAL and mark(_call(summary_out=None)) == EINVAL and mark(_call(totals=None)) == EINVAL
    assert mark(_call(summary_out=16384)) == EINVAL and mark(_call(totals=16384)) == EINVAL and mark(_call(totals=20480)) == EINVAL
    for ptr in ("points_out", "ring_offsets_out", "rings_out", "ring_stats"):
        assert write(_call(**{ptr: None})) == EINVAL
    assert write(_call(n_points_out=0)) == EINVAL and write(_call(n_points_out=41, point_capacity=41)) == EINVAL
    assert write(_call(ring_capacity=2)) == EINVAL and write(_call(point_capacity=19)) == EINVAL     # smaller than the totals
    need = C.c_size_t()
    assert L.uaps_contours_simplify_workspace_bytes(40, 3, C.byref(need)) == 0 and need.value % 256 == 0
    assert 28 * 40 + 24 * 3 <= need.value <= 28 * 40 + 24 * 3 + 14 * 256
    for run in (mark, write):
        assert run(_call(workspace_bytes=need.value - 1)) == EWORKSPACE and run(_call(workspace=65536 + 128)) == EWORKSPACE
    assert L.uaps_contours_simplify_workspace_bytes(40, 3, None) == EINVAL and L.uaps_contours_simplify_workspace_bytes(0, 3, C.byref(need)) == EINVAL
    assert L.uaps_contours_simplify_workspace_bytes(40, 0, C.byref(need)) == EINVAL
    assert L.uaps_contours_simplify_workspace_bytes(2 ** 30, 3, C.byref(need)) == ERANGE


def test_census_the_simplify_kernels():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libuaps_hip.so is not built")
    pattern = re.compile(r"^(?:void )?\(anonymous namespace\)::(simplify_\w+(?:<[^>]*>)?)\(")
    built = norm_act_kernel_symbols(_lib.LIB_PATH, pattern)
    assert built == {"simplify_copy_kernel", "simplify_classify_kernel", "simplify_wave_kernel", "simplify_block_kernel<true, 256>",
                     "simplify_block_kernel<false, 1024>", "simplify_sum_kernel", "simplify_base_kernel", "simplify_apply_kernel",
                     "simplify_write_kernel"}, sorted(built)

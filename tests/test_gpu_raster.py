"""Polygon rasterisation on the device (csrc/raster.hip) against the brute-force reference (tests/raster_ref.py), bit for bit: the
traced rings of the contour case table and the same rings simplified at four tolerances (where labels overlap), the F = 4 polygon
table and the quad partition, plus the frames the host tests leave out -- the extent limit in each direction (8 x 4096: 64 words a
box row and the carry across all of them; 4096 x 8: edges of 4096 rows), boxes that start at columns 63, 64 and 65.  Every case runs
through the default edge cut, with every edge on the lane form and with every edge on the wave form.  iou() against exact fractions;
garbage-filled buffers, two runs, a recycled workspace and a side stream; the raw C ABI's refusals; empty inputs; real
label_instances + contours output against the CPU path; inference.predict_instances(raster=True) under the plain, tta= and tiled=
paths."""
import ctypes as C

import numpy as np
import pytest
import torch

import contours_ref as R
import hull_ref as HR
import raster_ref as X
from test_contours_host import _inst
from test_hull_host import Stub, stub_mask
from test_raster_host import (FRAME_IDS, arrays, assert_equal, check_case_simplified, check_case_traced, check_iou, check_polygon_case,
                              check_predict_instances, check_quads, class_table, ring_set)
from test_simplify_host import HOST_IDS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
SENTINEL = 0x1234567
FORMS = ({}, {"edge_wave_rows": 4096}, {"edge_wave_rows": 0})          # the default cut; every edge by its lane; every edge by a wave
BIG_IDS = [f"{name}-1x{h}x{w}" for name in ("spiral", "comb", "noise3", "checker") for (h, w) in ((8, 4096), (4096, 8))]
WIDE_IDS = [c for c in HOST_IDS if c not in FRAME_IDS]                  # the 1 x 2 x 2100 frames: many words a row


@pytest.mark.parametrize("cid", FRAME_IDS)
def test_device_equals_the_reference_on_traced_rings_in_every_form(cid):
    for form in FORMS:
        check_case_traced(cid, DEV, **form)


@pytest.mark.parametrize("cid", WIDE_IDS + BIG_IDS)
def test_device_equals_the_reference_on_the_larger_frames_in_every_form(cid):
    from uaps_amd import contours, rasterize_contours
    case = R.case(cid)
    inside = (case.labels >= 1) & (case.labels <= 3)
    res = contours(_inst(case, 3, DEV), connectivity=8)
    ref = X.case_reference(cid, 8, None, 3)
    assert np.array_equal(ref[0], np.where(inside, case.labels, 0))
    for form in FORMS:
        got = rasterize_contours(res, reference=True, **form)
        assert_equal(arrays(got), ref, (cid, form))
        assert torch.equal(got.stats[..., 0], got.reference_area) and torch.equal(got.stats[..., 1], got.reference_area)


@pytest.mark.parametrize("cid", FRAME_IDS)
def test_device_equals_the_reference_on_simplified_rings_in_every_form(cid):
    seen = [check_case_simplified(cid, DEV, **form) for form in FORMS]
    assert seen[0] == seen[1] == seen[2]
    if cid in ("gap-3x17x129", "noise3-3x17x129"):
        assert seen[0] > 0                                              # labels overlap there: the lowest-label rule is at work


@pytest.mark.parametrize("cid", ("spiral-1x8x4096", "comb-1x4096x8", "noise3-1x2x2100"))
def test_simplified_rings_of_the_larger_frames(cid):
    from uaps_amd import contours, rasterize_contours, simplify_contours
    case = R.case(cid)
    res = contours(_inst(case, 3, DEV), connectivity=8)
    for e16 in (12, 1024):
        s = simplify_contours(res, e16 / 16.0)
        ref = X.case_reference(cid, 8, e16, 3)
        for form in FORMS:
            got = rasterize_contours(s, reference=True, **form)
            assert_equal(arrays(got), ref, (cid, e16, form))
        check_iou(got, ref[2], case.instances(3)[1][..., 1])


@pytest.mark.parametrize("name", sorted(X.polygon_cases()))
def test_device_equals_the_reference_on_the_polygon_table_in_every_form(name):
    for form in FORMS:
        check_polygon_case(name, DEV, **form)


def test_two_triangles_partition_their_quad_in_every_form():
    for seed in (1, 2, 3):
        for form in FORMS:
            check_quads(seed, DEV, **form)


def test_boxes_that_start_at_columns_63_64_and_65():
    from uaps_amd import contours, rasterize_contours
    from uaps_amd.instances import InstanceResult
    lab = np.zeros((2, 5, 200), dtype=np.int32)
    lab[0, 0, 63:130], lab[0, 1:3, 64:66], lab[0, 3:5, 65:200] = 1, 2, 3
    lab[1, :, 63], lab[1, 1, 64], lab[1, 2:4, 65:129] = 1, 2, 3
    count, table = HR.instance_table(lab, 3)
    put = lambda a: torch.from_numpy(a).to(DEV)
    res = contours(InstanceResult(put(lab), put(count), put(table), 0))
    planes = X.label_planes(*(t.cpu().numpy() for t in res[:3]), 2, 5, 200, 3, 0)
    ref = X.compose(planes, 2, 5, 200, 3, 0, lab)
    assert np.array_equal(ref[0], lab)
    for form in FORMS:
        assert_equal(arrays(rasterize_contours(res, reference=True, **form)), ref, form)


# ---- the raw C ABI ----------------------------------------------------------------------------------------------------------------------
def _need(N, L, B, H, W, M):
    from uaps_amd import _lib
    return _lib.workspace_bytes("uaps_raster_workspace_bytes", N, L, B, H, W, M)


def _raw(entry, src, dims, ws, stream=None, **kw):
    """A C entry point on caller-owned tensors; the code.  src: (points, ring_offsets, rings) on the device; dims: B, H, W, M, F."""
    from uaps_amd import _lib
    call = _lib.RasterCall()
    call.struct_size = C.sizeof(_lib.RasterCall)
    call.B, call.H, call.W, call.max_instances, call.frac_bits = dims
    call.ring_stride, call.n_points, call.n_rings = src[2].shape[1], src[0].shape[0], src[2].shape[0]
    call.points, call.ring_offsets, call.rings = (t.data_ptr() for t in src)
    call.workspace, call.workspace_bytes = ws.data_ptr(), ws.numel()
    call.stream = _lib.current_stream(DEV) if stream is None else stream
    for k, v in kw.items():
        setattr(call, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return getattr(_lib.lib(), entry)(C.byref(call))


def _run_raw(src, dims, fill, reference, classes, stream=None, ws=None, **form):
    """plan, the host read, fill -- on buffers filled with `fill`; (labels, mask, stats, overlap) as numpy, the totals, the workspace."""
    B, H, W, M, _ = dims
    full = lambda shape, dtype=torch.int64: torch.full(shape, fill, dtype=torch.int64, device=DEV).view(dtype)
    if ws is None:
        ws = full((_need(src[0].shape[0], src[2].shape[0], B, H, W, M) // 8,), torch.uint8)
    totals = full((4,))
    assert _raw("uaps_raster_plan", src, dims, ws, stream, totals=totals, **form) == 0
    tot = totals.tolist()
    planes, labels, mask, stats, overlap = full((tot[0],)), full((B, H, W)), full((B, H, W)), full((B, M, 2)), full((B,))
    assert _raw("uaps_raster_fill", src, dims, ws, stream, n_words=tot[0], planes=planes, reference=reference, classes=classes,
                background=-7, labels=labels, mask=mask, stats=stats, overlap=overlap, **form) == 0
    return tuple(t.cpu().numpy() for t in (labels, mask, stats, overlap)), tot, ws


def _simplified_case(cid, M, conn, e16):
    """(device tensors of the rings, dims, the reference, device reference labels and classes) of a simplified contour case."""
    case = R.case(cid)
    B, H, W = case.labels.shape
    cls = class_table(B, M)
    tables = X.rings_upto(X.case_tables(cid, conn, e16), M)
    src = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tables)
    ref = X.case_reference(cid, conn, e16, M, -7, cls)
    return src, (B, H, W, M, 0), ref, torch.from_numpy(case.labels).to(DEV), torch.from_numpy(cls).to(DEV)


@pytest.mark.parametrize("cid", ("noise3-3x17x129", "checker-3x17x129", "nested-3x17x129", "spiral-3x17x129", "gap-3x17x129"))
def test_garbage_buffers_two_runs_a_recycled_workspace_and_a_side_stream_give_the_same_bits(cid):
    for M, conn, e16 in ((3, 8, 12), (257, 4, 32)):
        src, dims, ref, labels, cls = _simplified_case(cid, M, conn, e16)
        for form in ({}, {"edge_wave_rows": 2}, {"edge_wave_rows": -1}):
            a, tot, ws = _run_raw(src, dims, 0x5a5a5a5a5a5a5a5a, labels, cls, **form)
            b, tot_b, _ = _run_raw(src, dims, -1, labels, cls, **form)
            again, _, _ = _run_raw(src, dims, 0x5a5a5a5a5a5a5a5a, labels, cls, ws=ws, **form)      # a recycled workspace
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                c, _, _ = _run_raw(src, dims, 7, labels, cls, stream=side.cuda_stream, **form)
            for got in (a, b, again, c):
                assert_equal(got, ref, (cid, M, conn, form))
            assert tot == tot_b and tot[0] >= tot[2] >= tot[1] >= int((ref[2][..., 0] > 0).sum()) > 0 and tot[3] == 0


def test_every_refusal_returns_its_code_and_leaves_the_outputs_untouched():
    from uaps_amd import _lib
    src, dims, ref, labels_ref, cls = _simplified_case("noise3-3x17x129", 4, 8, 16)
    B, H, W, M, _ = dims
    N, L = src[0].shape[0], src[2].shape[0]
    n = _need(N, L, B, H, W, M)
    ws = torch.empty(n + 256, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    mk = lambda shape: torch.full(shape, SENTINEL, dtype=torch.int64, device=DEV)
    totals = mk((4,))
    plan = lambda **kw: _raw("uaps_raster_plan", src, kw.pop("dims", dims), ws, **{"totals": totals, **kw})
    size = C.sizeof(_lib.RasterCall)
    assert plan(struct_size=size - 8) == EINVAL and plan(struct_size=0) == EINVAL
    assert plan(dims=(B, H, W, M, 5)) == EINVAL and plan(dims=(B, H, W, M, -1)) == EINVAL           # frac_bits outside 0 .. 4
    assert plan(dims=(B, 0, W, M, 0)) == EINVAL and plan(dims=(B, H, 4097, M, 0)) == ERANGE and plan(dims=(0, H, W, M, 0)) == EINVAL
    assert plan(ring_stride=1) == EINVAL and plan(edge_wave_rows=-2) == EINVAL and plan(edge_wave_rows=4097) == EINVAL
    assert plan(workspace_bytes=n - 1) == EWORKSPACE and plan(workspace=ws.data_ptr() + 128) == EWORKSPACE
    assert plan(points=None) == EINVAL and plan(ring_offsets=None) == EINVAL and plan(rings=None) == EINVAL and plan(workspace=None) == EINVAL
    assert plan(totals=None) == EINVAL and plan(totals=src[2]) == EINVAL and plan(rings=src[0]) == EINVAL
    assert plan(n_points=0) == EINVAL and plan(n_rings=0) == EINVAL and plan(n_points=2 ** 30) == ERANGE
    torch.cuda.synchronize()
    assert bool((totals == SENTINEL).all())
    assert plan() == 0
    words = totals.tolist()[0]
    assert words > 0
    planes, labels, mask, stats, overlap = mk((words,)), mk((B, H, W)), mk((B, H, W)), mk((B, M, 2)), mk((B,))
    outs = dict(n_words=words, planes=planes, reference=labels_ref, classes=cls, background=-7, labels=labels, mask=mask, stats=stats,
                overlap=overlap)
    fill = lambda **kw: _raw("uaps_raster_fill", src, kw.pop("dims", dims), ws, **{**outs, **kw})
    assert fill(struct_size=size - 8) == EINVAL and fill(dims=(B, H, W, M, 5)) == EINVAL and fill(edge_wave_rows=4097) == EINVAL
    assert fill(planes=None) == EINVAL and fill(labels=None) == EINVAL and fill(stats=None) == EINVAL and fill(overlap=None) == EINVAL
    assert fill(mask=None) == EINVAL and fill(classes=None) == EINVAL                               # one without the other
    assert fill(labels=mask) == EINVAL and fill(stats=labels) == EINVAL and fill(labels=labels_ref) == EINVAL and fill(mask=cls) == EINVAL
    assert fill(planes=src[0]) == EINVAL and fill(overlap=planes) == EINVAL                         # aliased operands
    assert fill(n_words=0) == EINVAL and fill(n_words=2 ** 28) == ERANGE and fill(workspace_bytes=n - 1) == EWORKSPACE
    assert fill(n_words=words - 1) == 0                                 # not the total of this workspace: the launches store nothing
    torch.cuda.synchronize()
    for out in (labels, mask, stats, overlap):
        assert bool((out == SENTINEL).all())
    assert fill() == 0
    assert_equal(tuple(t.cpu().numpy() for t in (labels, mask, stats, overlap)), ref, "after the refusals")
    # without a reference and without classes: inter stays zero, no mask is touched
    assert fill(reference=None, classes=None, mask=None) == 0
    assert np.array_equal(stats.cpu().numpy()[..., 0], ref[2][..., 0]) and not bool(stats[..., 1].any())


def test_empty_inputs():
    from uaps_amd import contours, rasterize_contours
    res = contours(_inst(R.case("empty-2x17x129"), 3, DEV))             # no ring
    got = rasterize_contours(res, reference=True, classes=True, background=9)
    assert got.labels.is_cuda and got.labels.shape == (2, 17, 129) and bool((got.labels == 9).all()) and not bool(got.mask.any())
    assert not bool(got.stats.any()) and not bool(got.overlap.any()) and bool(torch.isnan(got.iou()).all())
    assert got.fidelity()["overlap"] == [0, 0] and got.records() == [[], []]
    # rings that own no pixel: wholly right of the frame, and of two points -- nothing to fill after the plan
    tables = X.tables_of([(0, 1, [(16, 400), (16, 800), (90, 800)]), (0, 2, [(8, 8), (100, 100)])])
    got = rasterize_contours(ring_set(tables, 1, 2, 8, 10, 4, DEV), background=-1)
    assert bool((got.labels == -1).all()) and not bool(got.mask.any()) and not bool(got.stats.any())
    gap = R.case("gap-3x17x129")                                        # an empty image inside a batch, labels without a pixel
    g = rasterize_contours(contours(_inst(gap, 257, DEV)), reference=True)
    assert_equal(arrays(g), X.case_reference("gap-3x17x129", 8, None, 257), "gap")
    assert not bool(g.labels[1].any()) and bool(torch.isnan(g.iou()[1]).all())


def test_device_equals_the_cpu_path_on_real_instances():
    from uaps_amd import contours, label_instances, rasterize_contours, simplify_contours
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 4, size=(2, 12, 16))
    mask = torch.from_numpy(np.kron(blocks, np.ones((1, 5, 7), dtype=np.int64)) * (rng.random((2, 60, 112)) > 0.08))
    for M, conn in ((64, 8), (300, 4)):
        cpu_inst = label_instances(mask, max_instances=M, connectivity=conn)
        dev_inst = label_instances(mask.to(DEV), max_instances=M, connectivity=conn)
        cpu_c, dev_c = contours(cpu_inst, connectivity=conn), contours(dev_inst, connectivity=conn)
        for eps in (None, 0.75, 2.0):
            cpu = rasterize_contours(cpu_c if eps is None else simplify_contours(cpu_c, eps), reference=True, classes=True)
            for form in FORMS:
                dev = rasterize_contours(dev_c if eps is None else simplify_contours(dev_c, eps), reference=True, classes=True, **form)
                assert_equal(arrays(dev), arrays(cpu), (M, conn, eps, form))
            assert torch.equal(dev.iou().cpu().isnan(), cpu.iou().isnan()) and np.array_equal(dev.fidelity()["iou"], cpu.fidelity()["iou"], equal_nan=True)
            assert dev.records() == cpu.records()
            if eps is None:                                             # the class map is the mask that was labelled, within the table
                kept = (cpu_inst.labels >= 1) & (cpu_inst.labels <= M)
                assert torch.equal(cpu.mask, torch.where(kept, mask, torch.zeros_like(mask))) and not bool(cpu.overlap.any())
            else:
                assert float(np.nanmin(dev.fidelity()["iou"])) < 1.0


def test_predict_instances_with_raster_on_the_three_paths():
    import uaps_amd
    m = stub_mask()
    x = torch.zeros(2, 3, 37, 53)
    cpu_r, cpu_s = check_predict_instances(Stub(m, 4), x)
    net = Stub(m, 4)
    net.logits = net.logits.to(DEV)
    dev_r, dev_s = check_predict_instances(net, x.to(DEV))
    assert_equal(arrays(dev_r), arrays(cpu_r), "stub, traced")
    assert_equal(arrays(dev_s), arrays(cpu_s), "stub, simplified")
    assert np.array_equal(dev_s.fidelity()["iou"], cpu_s.fidelity()["iou"], equal_nan=True)
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    for path in ({}, {"tta": (1.0,)}, {"tiled": {"tile": 32, "overlap": 8}}):
        r, s = check_predict_instances(model, x, **path)
        c = s.contours.contours
        planes = X.label_planes(*(t.cpu().numpy() for t in c[:3]), 2, 32, 32, 256, 0)
        assert_equal(arrays(s), X.compose(planes, 2, 32, 32, 256, 0, c.instances.labels.cpu().numpy()), path)

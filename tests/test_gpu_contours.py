"""Defect contours on the device (csrc/contours.hip) against the sequential tracer (tests/contours_ref.py), bit for bit, on the
smallest inputs at which each mechanism can go wrong: one pixel, a row and a column one longer than a wave, a batch whose vertices
and edges fill several workgroups of a scan, rows longer than one workgroup scans, the extent limit in each direction; a
checkerboard (every interior vertex a saddle, the most edges a frame can have), both diagonal pairs, nested labels whose rings share
start vertices, a spiral and a comb whose single ring needs every doubling round, labels outside [1, M], an empty image inside a
batch and an all-empty batch.  Every case runs at both connectivities and at M = 1, 3, 256 and 257; the identities of
contours_ref.check_identities hold without the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import contours_ref as R
from test_contours_host import _Example, _inst, arrays, assert_equals_reference, assert_identities
from test_hull_host import Stub, stub_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
SENTINEL = 0x1234567


def _need(B, H, W, M):
    from uaps_amd import _lib
    return _lib.workspace_bytes("uaps_contours_workspace_bytes", B, H, W, M)


def _raw(entry, lab, M, conn, ws, stream=None, **kw):
    """A C entry point on caller-owned tensors; the code."""
    from uaps_amd import _lib
    B, H, W = lab.shape
    call = _lib.ContourCall()
    call.struct_size = C.sizeof(_lib.ContourCall)
    call.B, call.H, call.W, call.max_instances, call.connectivity = B, H, W, M, conn
    call.labels, call.workspace, call.workspace_bytes = lab.data_ptr(), ws.data_ptr(), ws.numel()
    call.stream = _lib.current_stream(DEV) if stream is None else stream
    for k, v in kw.items():
        setattr(call, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return getattr(_lib.lib(), entry)(C.byref(call))


def _run_raw(lab, M, conn, fill, stream=None, ws=None):
    """trace, the host read, write -- on buffers filled with `fill`; (points, ring_offsets, rings, summary) as numpy, and the workspace.
    With `stream` the caller has made it torch's current stream: the host reads wait for it."""
    B, H, W = lab.shape
    full = lambda shape, dtype: torch.full(shape, fill, dtype=torch.int64, device=DEV).view(dtype)
    if ws is None:
        ws = full((_need(B, H, W, M) // 8,), torch.uint8)
    summary, totals = full((B, M, 4), torch.int64), full((4,), torch.int64)
    assert _raw("uaps_contours_trace", lab, M, conn, ws, stream, summary=summary, totals=totals) == 0
    L, N = (int(v) for v in totals[:2].tolist())
    points, offsets, rings = full((N,), torch.int32).reshape(-1, 2), full(((L + 2) // 2,), torch.int32)[:L + 1], full((L, 7), torch.int64)
    if L > 0:
        assert _raw("uaps_contours_write", lab, M, conn, ws, stream, n_rings=L, n_points=N, ring_capacity=L, point_capacity=N,
                    points=points, ring_offsets=offsets, rings=rings) == 0
    else:
        offsets = torch.zeros(1, dtype=torch.int32, device=DEV)
    return (points.cpu().numpy(), offsets.cpu().numpy(), rings.cpu().numpy(), summary.cpu().numpy()), ws


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_device_equals_the_reference_and_the_identities_hold(cid):
    from uaps_amd import contours
    case = R.case(cid)
    for conn in (8, 4):
        for M in R.MS:
            res = contours(_inst(case, M, DEV), connectivity=conn)
            assert res.points.is_cuda and res.rings.is_cuda and res.summary.is_cuda and res.ring_offsets.is_cuda and res.connectivity == conn
            got = assert_equals_reference(res, case, M, conn)
            if M == 256:
                assert_identities(got, case, M, conn, DEV)


def test_the_long_rings_use_every_round_and_the_short_ones_stop_early():
    from uaps_amd import contours
    long_ring = contours(_inst(R.case("comb-1x8x4096"), 1, DEV))
    length = int(long_ring.rings[0, 5])
    assert length > 2 ** 15 and 2 ** (long_ring.rounds - 1) < 2 * length and 2 ** long_ring.rounds >= length
    short = contours(_inst(R.case("checker-1x8x4096"), 1, DEV), connectivity=4)
    assert int(short.rings[:, 5].max()) == 4 and short.rounds == 3       # two rounds cover four edges, a third finds nothing to lower
    assert contours(_inst(R.case("empty-2x17x129"), 3, DEV)).rounds == 0


@pytest.mark.parametrize("cid", ("noise3-3x17x129", "checker-3x17x129", "nested-3x17x129", "spiral-3x17x129", "comb-1x2x2100", "gap-3x17x129"))
def test_garbage_buffers_two_runs_a_recycled_workspace_and_a_side_stream_give_the_same_bits(cid):
    case = R.case(cid)
    labels = torch.from_numpy(case.labels).to(DEV)
    for M, conn in ((3, 8), (257, 4)):
        ref = case.tables(M, conn)
        a, ws = _run_raw(labels, M, conn, 0x5a5a5a5a5a5a5a5a)
        b, _ = _run_raw(labels, M, conn, -1)
        again, _ = _run_raw(labels, M, conn, 0x5a5a5a5a5a5a5a5a, ws=ws)  # a recycled workspace: the previous run is no part of the next
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            c, _ = _run_raw(labels, M, conn, 7, stream=side.cuda_stream)
        for got in (a, b, again, c):
            for x, y in zip(got, ref):
                assert np.array_equal(x, y), (cid, M, conn)


def test_every_refusal_returns_its_code_and_leaves_the_outputs_untouched():
    from uaps_amd import _lib
    case = R.case("nested-3x17x129")
    labels = torch.from_numpy(case.labels).to(DEV)
    B, H, W = labels.shape
    M, conn = 4, 8
    ref = case.tables(M, conn)
    L, N = len(ref[2]), len(ref[0])
    n = _need(B, H, W, M)
    ws = torch.empty(n + 256, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    mk = lambda shape, dtype=torch.int64: torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
    summary, totals, points, offsets, rings = mk((B, M, 4)), mk((4,)), mk((N, 2), torch.int32), mk((L + 1,), torch.int32), mk((L, 7))
    outs = dict(summary=summary, totals=totals)
    trace = lambda **kw: _raw("uaps_contours_trace", labels, M, conn, ws, **{**outs, **kw})
    assert trace(labels=None) == EINVAL and trace(summary=None) == EINVAL and trace(totals=None) == EINVAL and trace(workspace=None) == EINVAL
    assert trace(summary=labels) == EINVAL and trace(totals=labels) == EINVAL and trace(totals=summary) == EINVAL
    for dim in ("B", "H", "W", "max_instances"):
        assert trace(**{dim: 0}) == EINVAL and trace(**{dim: -1}) == EINVAL
    assert trace(connectivity=6) == EINVAL and trace(struct_size=C.sizeof(_lib.ContourCall) - 8) == EINVAL
    assert trace(H=4097) == ERANGE and trace(W=4097) == ERANGE and trace(B=4, H=4096, W=4096) == ERANGE
    assert trace(workspace_bytes=n - 1) == EWORKSPACE and trace(workspace=ws.data_ptr() + 128) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((summary == SENTINEL).all()) and bool((totals == SENTINEL).all())
    assert trace() == 0 and totals.tolist()[:2] == [L, N] and totals.tolist()[3] == int(ref[2][:, 5].sum())
    assert np.array_equal(summary.cpu().numpy(), ref[3])
    wouts = dict(points=points, ring_offsets=offsets, rings=rings, n_rings=L, n_points=N, ring_capacity=L, point_capacity=N)
    write = lambda **kw: _raw("uaps_contours_write", labels, M, conn, ws, **{**wouts, **kw})
    assert write(points=None) == EINVAL and write(ring_offsets=None) == EINVAL and write(rings=None) == EINVAL and write(labels=None) == EINVAL
    assert write(ring_capacity=L - 1) == EINVAL and write(point_capacity=N - 1) == EINVAL      # a capacity below the totals
    assert write(n_rings=0) == EINVAL and write(n_points=0) == EINVAL and write(connectivity=5) == EINVAL
    assert write(workspace_bytes=n - 1) == EWORKSPACE and write(W=4097) == ERANGE
    assert write(n_rings=L - 1, n_points=N - 4) == 0                     # not the totals of this workspace: the launch stores nothing
    torch.cuda.synchronize()
    for t in (points, offsets, rings):
        assert bool((t == SENTINEL).all())
    big_p, big_o, big_r = mk((N + 3, 2), torch.int32), mk((L + 3,), torch.int32), mk((L + 2, 7))
    assert write(points=big_p, ring_offsets=big_o, rings=big_r, ring_capacity=L + 2, point_capacity=N + 3) == 0     # larger is fine
    assert write() == 0
    for got, want in ((points, ref[0]), (offsets, ref[1]), (rings, ref[2]), (big_p[:N], ref[0]), (big_o[:L + 1], ref[1]), (big_r[:L], ref[2])):
        assert np.array_equal(got.cpu().numpy(), want)
    assert bool((big_p[N:] == SENTINEL).all()) and bool((big_o[L + 1:] == SENTINEL).all()) and bool((big_r[L:] == SENTINEL).all())


def test_device_equals_the_cpu_path_on_real_instances():
    from uaps_amd import contours, label_instances, shape_descriptors
    mask = torch.from_numpy(stub_mask())
    for M, conn in ((64, 8), (300, 4)):
        cpu_inst = label_instances(mask, max_instances=M, connectivity=conn)
        dev_inst = label_instances(mask.to(DEV), max_instances=M, connectivity=conn)
        cpu, dev = contours(cpu_inst, connectivity=conn), contours(dev_inst, connectivity=conn)
        assert torch.equal(dev_inst.labels.cpu(), cpu_inst.labels) and int(cpu_inst.count.min()) >= 3
        for a, b in zip(arrays(dev), arrays(cpu)):
            assert np.array_equal(a, b)
        for a, b in zip(arrays(dev), R.tables(cpu_inst.labels.numpy(), M, conn)):
            assert np.array_equal(a, b)
        # labels of label_instances at the same connectivity: exactly one outer ring a defect, and shape_descriptors' holes
        props = shape_descriptors(dev_inst, connectivity=conn).props()
        rings, count = dev.rings.cpu().numpy(), dev_inst.count.cpu().numpy()
        for b in range(mask.shape[0]):
            for k in range(1, min(int(count[b]), M) + 1):
                mine = rings[(rings[:, 0] == b) & (rings[:, 1] == k)]
                assert (mine[:, 6] > 0).sum() == 1 and (mine[:, 6] < 0).sum() == props["holes"][b, k - 1]
        assert dev.records() == cpu.records() and dev.to_coco() == cpu.to_coco()
        pd, pc = dev.polygons(), cpu.polygons()
        assert [[(r["label"], [a.tolist() for a in r["outer"]], [a.tolist() for a in r["holes"]]) for r in rows] for rows in pd] == \
               [[(r["label"], [a.tolist() for a in r["outer"]], [a.tolist() for a in r["holes"]]) for r in rows] for rows in pc]


def test_the_hand_written_example_on_the_device():
    from uaps_amd import contours
    res = contours(_inst(_Example, 4, DEV))
    assert res.rings.tolist() == [[0, 1, 0, 0, 4, 18, 40], [0, 2, 1, 1, 4, 4, 2], [0, 1, 1, 1, 4, 8, -8], [0, 3, 4, 5, 8, 8, 4]]
    assert res.ring_offsets.tolist() == [0, 4, 8, 12, 20] and res.points[12:].tolist() == [[4, 5], [4, 6], [5, 6], [5, 7], [6, 7], [6, 6], [5, 6], [5, 5]]
    assert [[a.tolist() for a in p["holes"]] for p in res.polygons()[0]] == [[[[1, 1], [3, 1], [3, 3], [1, 3]]], [], []]
    assert [a["iscrowd"] for a in res.to_coco()] == [1, 0, 0] and [r["holes_traced"] for r in res.records()[0]] == [1, 0, 0]


def test_predict_instances_with_contours_hull_and_shapes():
    from uaps_amd import ContourResult, HullResult, ShapeResult, inference
    m = stub_mask()
    x = torch.zeros(2, 3, 37, 53)
    kw = dict(contours=True, hull=True, shapes=True)
    cpu = inference.predict_instances(Stub(m, 4), x, **kw)
    net = Stub(m, 4)
    net.logits = net.logits.to(DEV)
    dev = inference.predict_instances(net, x.to(DEV), **kw)
    for r in (cpu, dev):
        assert isinstance(r, ContourResult) and isinstance(r.also, HullResult) and isinstance(r.also.also, ShapeResult)
    assert dev.points.is_cuda and len(cpu.rings) > 10
    for a, b in zip(arrays(dev) + (dev.also.table.cpu().numpy(), dev.also.also.table.cpu().numpy(), dev.instances.labels.cpu().numpy()),
                    arrays(cpu) + (cpu.also.table.numpy(), cpu.also.also.table.numpy(), cpu.instances.labels.numpy())):
        assert np.array_equal(a, b)
    assert {"rings", "perimeter_crack", "solidity", "centroid_y"} <= set(dev.records()[0][0]) and dev.records() == cpu.records()
    plain = inference.predict_instances(net, x.to(DEV), contours=True)
    assert plain.also is None and torch.equal(plain.rings, dev.rings) and torch.equal(plain.points, dev.points)
    with pytest.raises(ValueError):
        inference.predict_instances(net, x.to(DEV), contours="x")


def test_predict_instances_with_contours_under_the_tta_and_tiled_paths():
    import uaps_amd
    from uaps_amd import ContourResult, ShapeResult, contours, inference
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    clean = dict(cleanup=[("open", "disk", 1)], components=[("area_open", 2), ("fill_holes", None)])
    for path in ({}, {"tta": (1.0,)}, {"tiled": {"tile": 32, "overlap": 8}}):
        for extra in ({}, clean):
            base = inference.predict_instances(model, x, shapes=True, **path, **extra)
            r = inference.predict_instances(model, x, contours=True, shapes=True, **path, **extra)
            assert isinstance(r, ContourResult) and isinstance(r.also, ShapeResult) and r.summary.shape == (2, 256, 4)
            assert torch.equal(r.instances.labels, base.instances.labels) and torch.equal(r.also.table, base.table)
            direct = contours(r.instances)
            assert all(torch.equal(a, b) for a, b in zip(r[:4], direct[:4]))
            for a, b in zip(arrays(r), R.tables(r.instances.labels.cpu().numpy(), 256, 8)):
                assert np.array_equal(a, b)

"""Convex hulls on the device (csrc/hull.hip) against the brute-force reference (tests/hull_ref.py), bit for bit, on the smallest
inputs at which each mechanism can go wrong: one pixel, a row and a column one longer than a wave, more rows than a workgroup holds
and three groups a row, a run longer than the carried span, the extent limit in each direction; a lens with more strict vertices than
a workgroup has threads; figures every column of which is decided by a tie rule; and one frame whose width comparison needs 128 bits.
Every case runs at M = 1, 3, 256 and 257 (the kernels have one form for every M)."""
import ctypes as C

import numpy as np
import pytest
import torch

import hull_ref as R
from test_hull_host import Stub, stub_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, ERANGE, EWORKSPACE = -1, -2, -3


def _inst(case, M):
    from uaps_amd.instances import InstanceResult
    count, table = case.instances(M)
    return InstanceResult(torch.from_numpy(case.labels).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(table).to(DEV), 0)


def _need(B, H, W, M):
    from uaps_amd import _lib
    return _lib.workspace_bytes("uaps_hull_workspace_bytes", B, H, W, M)


def _raw(lab, rows, out, ws, stream=None, **kw):
    """The C entry point on caller-owned tensors (the wrapper allocates its own table and keeps its own workspace); the code."""
    from uaps_amd import _lib
    B, H, W = lab.shape
    call = _lib.HullCall()
    call.struct_size = C.sizeof(_lib.HullCall)
    call.B, call.H, call.W, call.max_instances = B, H, W, rows
    call.labels, call.table, call.workspace, call.workspace_bytes = lab.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()
    call.stream = _lib.current_stream(DEV) if stream is None else stream
    for k, v in kw.items():
        setattr(call, k, v)
    return _lib.lib().uaps_hull_descriptors(C.byref(call))


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_device_equals_the_reference(cid):
    from uaps_amd import hull_descriptors
    case = R.case(cid)
    got = {}
    for M in R.MS:
        res = hull_descriptors(_inst(case, M))
        assert res.table.dtype == torch.int64 and res.table.is_cuda and tuple(res.table.shape) == (case.labels.shape[0], M, 17)
        got[M] = res.table.cpu().numpy()
        ref = case.table(M)
        bad = np.argwhere(got[M] != ref)
        assert len(bad) == 0, (cid, M, bad[:4], got[M][tuple(bad[0][:2])], ref[tuple(bad[0][:2])])
    assert np.array_equal(got[257][:, :256], got[256])                  # rows at and above M in the labels are ignored
    assert np.array_equal(got[3], got[256][:, :3]) and np.array_equal(got[1], got[256][:, :1])


def test_the_comparison_that_needs_128_bits():
    pos, (l, r) = R.wide_positions()                                   # decided on the host, before the GPU is involved
    assert l >= 2 ** 64 and r >= 2 ** 64 and l != r and (l < r) != (l % 2 ** 64 < r % 2 ** 64)
    from uaps_amd import hull_descriptors
    case = R.case("wide")
    res = hull_descriptors(_inst(case, 1))
    assert np.array_equal(res.table.cpu().numpy(), case.table(1)), (res.table.cpu().numpy(), case.table(1))


@pytest.mark.parametrize("cid", ("noise3-3x17x129", "full-1x2x2100", "checker4-3x17x129", "rings-3x17x129", "lens", "gap-3x17x129"))
def test_garbage_buffers_two_runs_a_recycled_workspace_and_a_side_stream_give_the_same_bits(cid):
    case = R.case(cid)
    labels = torch.from_numpy(case.labels).to(DEV)
    B, H, W = labels.shape
    for M in (3, 257):
        ref = case.table(M)
        n = _need(B, H, W, M)
        fill = lambda v, shape: torch.full(shape, v, dtype=torch.int64, device=DEV)
        ws = fill(0x5a5a5a5a5a5a5a5a, (n // 8,)).view(torch.uint8)
        a, b = fill(0x5a5a5a5a5a5a5a5a, (B, M, 17)), fill(-1, (B, M, 17))
        assert _raw(labels, M, a, ws) == 0
        assert _raw(labels, M, b, fill(-1, (n // 8,)).view(torch.uint8)) == 0
        again = a.clone()
        assert _raw(labels, M, again, ws) == 0                          # a recycled table and workspace: the previous run is no part of the next
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        c = fill(7, (B, M, 17))
        with torch.cuda.stream(side):
            assert _raw(labels, M, c, fill(7, (n // 8,)).view(torch.uint8), stream=side.cuda_stream) == 0
        side.synchronize()
        for t in (a, b, again, c):
            assert np.array_equal(t.cpu().numpy(), ref), (cid, M)


def test_every_refusal_returns_its_code_and_leaves_the_table_untouched():
    from uaps_amd import _lib
    case = R.case("rings-3x17x129")
    labels = torch.from_numpy(case.labels).to(DEV)
    B, H, W = labels.shape
    M = 4
    n = _need(B, H, W, M)
    assert n == (B * M * (H + 1) * 8 + 255) // 256 * 256
    table = torch.full((B, M, 17), 0x1234567, dtype=torch.int64, device=DEV)
    ws = torch.empty(n + 256, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    run = lambda **kw: _raw(labels, M, table, ws, **kw)
    assert _lib.lib().uaps_hull_descriptors(None) == EINVAL
    assert run(labels=None) == EINVAL and run(table=None) == EINVAL and run(workspace=None) == EINVAL
    assert run(table=labels.data_ptr()) == EINVAL
    for dim in ("B", "H", "W", "max_instances"):
        assert run(**{dim: 0}) == EINVAL and run(**{dim: -1}) == EINVAL
    assert run(struct_size=C.sizeof(_lib.HullCall) - 8) == EINVAL
    assert run(H=4097) == ERANGE and run(W=4097) == ERANGE and run(B=16, H=4096, W=4096) == ERANGE
    assert run(B=4096, max_instances=3856) == ERANGE and run(H=4096, max_instances=65536) == ERANGE
    assert run(workspace_bytes=n - 1) == EWORKSPACE and run(workspace=ws.data_ptr() + 128) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((table == 0x1234567).all())
    assert run() == 0 and np.array_equal(table.cpu().numpy(), case.table(M))


def test_device_equals_the_cpu_path_on_real_instances():
    from uaps_amd import hull_descriptors, label_instances
    mask = torch.from_numpy(stub_mask())
    for M in (64, 300):
        cpu = hull_descriptors(label_instances(mask, max_instances=M))
        dev = hull_descriptors(label_instances(mask.to(DEV), max_instances=M))
        assert torch.equal(dev.instances.labels.cpu(), cpu.instances.labels) and int(cpu.instances.count.min()) >= 3
        assert torch.equal(dev.table.cpu(), cpu.table)
        assert np.array_equal(cpu.table.numpy(), R.table(cpu.instances.labels.numpy(), M))
        a, b = dev.props(), cpu.props()
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        assert np.array_equal(dev.rect_corners(), cpu.rect_corners(), equal_nan=True) and dev.records() == cpu.records()


def test_predict_instances_with_hull_shapes_and_skeleton():
    from uaps_amd import HullResult, ShapeResult, SkeletonStats, hull_descriptors, inference
    m = stub_mask()
    x = torch.zeros(2, 3, 37, 53)
    kw = dict(hull=True, shapes=True, skeleton=True)
    cpu = inference.predict_instances(Stub(m, 4), x, **kw)
    net = Stub(m, 4)
    net.logits = net.logits.to(DEV)
    dev = inference.predict_instances(net, x.to(DEV), **kw)
    for r in (cpu, dev):
        assert isinstance(r, HullResult) and isinstance(r.also, SkeletonStats) and isinstance(r.also.shapes, ShapeResult)
    assert dev.table.is_cuda and int(cpu.table[..., 0].sum()) > 0
    for a, b in ((dev.table, cpu.table), (dev.instances.labels, cpu.instances.labels), (dev.instances.count, cpu.instances.count),
                 (dev.instances.table[..., :7], cpu.instances.table[..., :7]), (dev.also.table, cpu.also.table),
                 (dev.also.shapes.table, cpu.also.shapes.table), (dev.also.skeleton.mask, cpu.also.skeleton.mask)):
        assert torch.equal(a.cpu(), b)
    assert {"solidity", "length", "centroid_y"} <= set(dev.records()[0][0])
    plain = inference.predict_instances(net, x.to(DEV), hull=True)
    assert plain.also is None and torch.equal(plain.table, dev.table)
    with pytest.raises(ValueError):
        inference.predict_instances(net, x.to(DEV), hull="x")


def test_predict_instances_with_hull_under_the_tta_and_tiled_paths():
    import uaps_amd
    from uaps_amd import HullResult, ShapeResult, hull_descriptors, inference
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    for path in ({}, {"tta": (1.0,)}, {"tiled": {"tile": 32, "overlap": 8}}):
        base = inference.predict_instances(model, x, shapes=True, **path)
        r = inference.predict_instances(model, x, hull=True, shapes=True, **path)
        assert isinstance(r, HullResult) and isinstance(r.also, ShapeResult) and r.table.shape == (2, 256, 17)
        assert torch.equal(r.instances.labels, base.instances.labels) and torch.equal(r.also.table, base.table)
        assert int(r.instances.count.sum()) > 0 and torch.equal(r.table, hull_descriptors(r.instances).table)
        assert np.array_equal(r.table.cpu().numpy(), R.table(r.instances.labels.cpu().numpy(), 256))

"""Shape descriptors on the device (csrc/shapes.hip) against the brute-force reference (tests/shapes_ref.py), bit for bit, on the
smallest shapes at which each mechanism can go wrong: one pixel, a row one pixel longer than a wave, rows of exactly 64 and of 63, more
rows than a workgroup holds and three groups a row, a row longer than the carried span of either flush form (4 x 64 and 16 x 64
pixels).  Every case runs at M = 1, 3, 256 (the LDS flush form) and 257 (the direct one), with and without a plane that holds negative
values and 2^31 - 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import shapes_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _inst(case, M):
    from uaps_amd.instances import InstanceResult
    labels, count, table = case.instances(M)
    return InstanceResult(torch.from_numpy(labels).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(table).to(DEV), 0)


def _raw(labels, plane, M, table, stream=None):
    """The C entry point on caller-owned tensors (the wrapper always allocates its own table)."""
    from uaps_amd import _lib
    B, H, W = labels.shape
    call = _lib.ShapeCall()
    call.struct_size = C.sizeof(_lib.ShapeCall)
    call.B, call.H, call.W, call.max_instances = B, H, W, M
    call.labels, call.plane, call.table = labels.data_ptr(), (None if plane is None else plane.data_ptr()), table.data_ptr()
    call.stream = _lib.current_stream(DEV) if stream is None else stream
    _lib.check(_lib.lib().uaps_shape_descriptors(C.byref(call)), "uaps_shape_descriptors")
    return table


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_device_equals_the_reference_in_both_flush_forms(cid):
    from uaps_amd import shape_descriptors
    case = R.case(cid)
    plane = torch.from_numpy(case.plane).to(DEV)
    got = {}
    for M in R.MS:
        inst = _inst(case, M)
        for with_plane in (False, True):
            res = shape_descriptors(inst, plane if with_plane else None, connectivity=case.connectivity)
            assert res.table.dtype == torch.int64 and res.table.is_cuda and tuple(res.table.shape) == (case.mask.shape[0], M, 11)
            got[M, with_plane] = res.table.cpu().numpy()
            ref = case.table(M, with_plane)
            bad = np.argwhere(got[M, with_plane] != ref)
            assert len(bad) == 0, (cid, M, with_plane, bad[:4], got[M, with_plane][tuple(bad[0][:2])], ref[tuple(bad[0][:2])])
    for with_plane in (False, True):                    # the two forms, on the same labels, against each other
        lds, direct = got[R.LDS_ROWS, with_plane], got[R.LDS_ROWS + 1, with_plane]
        assert np.array_equal(direct[:, :R.LDS_ROWS], lds)
        assert np.array_equal(got[3, with_plane], lds[:, :3]) and np.array_equal(got[1, with_plane], lds[:, :1])


@pytest.mark.parametrize("cid", ("noise-3x17x129", "full-1x2x2100", "checker4-3x17x129", "rings-3x17x129"))
def test_a_garbage_table_two_runs_and_a_side_stream_give_the_same_bits(cid):
    case = R.case(cid)
    plane = torch.from_numpy(case.plane).to(DEV)
    B = case.mask.shape[0]
    for M in (R.LDS_ROWS, R.LDS_ROWS + 1):
        labels = torch.from_numpy(case.instances(M)[0]).to(DEV)
        ref = case.table(M, True)
        a = _raw(labels, plane, M, torch.full((B, M, 11), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=DEV))
        b = _raw(labels, plane, M, torch.full((B, M, 11), -1, dtype=torch.int64, device=DEV))
        again = _raw(labels, plane, M, a.clone())        # a recycled table: the previous result is no part of the next
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            c = _raw(labels, plane, M, torch.full((B, M, 11), 7, dtype=torch.int64, device=DEV), stream=side.cuda_stream)
        side.synchronize()
        for t in (a, b, again, c):
            assert np.array_equal(t.cpu().numpy(), ref), (cid, M)


@pytest.mark.parametrize("cid", ("touch-3x17x129", "noise-1x2x2100", "edges-1x5x63", "diagonals-2x3x64"))
def test_labels_outside_the_table_have_no_row_and_change_no_other(cid):
    """Negative labels, labels above M and the extreme int32 values in place of every 0: no fault, and every row as before."""
    case = R.case(cid)
    rng = np.random.default_rng(3)
    for M in (3, R.LDS_ROWS, R.LDS_ROWS + 1):
        labels = case.instances(M)[0]
        junk = rng.choice(np.array([-1, -7, -2 ** 31, 2 ** 31 - 1, M + 1, M + 2, 2 ** 30], dtype=np.int64), labels.shape).astype(np.int32)
        dirty = np.where(labels == 0, junk, labels).astype(np.int32)
        assert (dirty != labels).any() and (dirty < 0).any() and (dirty > M).any()
        ref = R.table(np.where(labels > M, 0, labels), case.plane, M)
        assert np.array_equal(ref, case.table(M, True))
        B = labels.shape[0]
        got = _raw(torch.from_numpy(dirty).to(DEV), torch.from_numpy(case.plane).to(DEV), M, torch.empty((B, M, 11), dtype=torch.int64, device=DEV))
        assert np.array_equal(got.cpu().numpy(), ref), (cid, M)


def test_thickness_equals_scipy():
    from scipy import ndimage
    from uaps_amd import label_instances, shape_descriptors
    for cid in ("rings-3x17x129", "touch-3x17x129", "noise-1x2x2100"):
        case = R.case(cid)
        mask = torch.from_numpy(case.mask).to(DEV)
        for M in (64, R.LDS_ROWS + 1):
            inst = label_instances(mask, connectivity=case.connectivity, max_instances=M)
            res = shape_descriptors(inst, thickness=True, connectivity=case.connectivity)
            lab, t = inst.labels.cpu().numpy(), res.table.cpu().numpy()
            assert np.array_equal(lab, case.instances(M)[0]) and res.has_plane == "thickness"
            want = np.zeros((lab.shape[0], M, 2), dtype=np.int64)
            for b in range(lab.shape[0]):
                d2 = np.rint(ndimage.distance_transform_edt(lab[b] != 0) ** 2).astype(np.int64)
                for k in range(1, min(M, int(lab[b].max())) + 1):
                    want[b, k - 1] = d2[lab[b] == k].max(), d2[lab[b] == k].sum()
            assert np.array_equal(t[..., 9:], want), (cid, M)
            assert np.array_equal(t[..., :9], case.table(M, False)[..., :9])
            p = res.props()
            assert np.array_equal(p["inradius"][want[..., 0] > 0], np.sqrt(want[..., 0][want[..., 0] > 0]))


def test_device_equals_the_cpu_path_and_props_agree():
    from uaps_amd import label_instances, shape_descriptors
    case = R.case("rings-3x17x129")
    mask = torch.from_numpy(case.mask)
    cpu = shape_descriptors(label_instances(mask, connectivity=4, max_instances=300), torch.from_numpy(case.plane), connectivity=4)
    dev = shape_descriptors(label_instances(mask.to(DEV), connectivity=4, max_instances=300), torch.from_numpy(case.plane).to(DEV), connectivity=4)
    assert torch.equal(dev.table.cpu(), cpu.table) and int(cpu.instances.count.min()) > 0
    a, b = dev.props(), cpu.props()
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    assert dev.records() == cpu.records()


def test_predict_instances_with_shapes():
    import uaps_amd
    from uaps_amd import inference, shape_descriptors
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    plain = inference.predict_instances(model, x)
    for kw in ({}, {"components": [("area_open", 2)]}, {"connectivity": 4, "max_instances": 300}):
        base = inference.predict_instances(model, x, **kw)
        res = inference.predict_instances(model, x, shapes=True, **kw)
        assert isinstance(res, uaps_amd.ShapeResult) and res.has_plane == "none" and res.connectivity == kw.get("connectivity", 8)
        for a, b in zip(res.instances[:3], base[:3]):
            assert torch.equal(a, b)
        assert int(res.instances.count.sum()) > 0
        assert torch.equal(res.table, shape_descriptors(res.instances, connectivity=res.connectivity).table)
        lab = res.instances.labels.cpu().numpy()
        assert np.array_equal(res.table.cpu().numpy(), R.table(lab, None, res.instances.max_instances))
    assert all(torch.equal(a, b) for a, b in zip(inference.predict_instances(model, x, shapes=False)[:3], plain[:3]))
    thick = inference.predict_instances(model, x, shapes="thickness")
    assert thick.has_plane == "thickness" and torch.equal(thick.table, shape_descriptors(thick.instances, thickness=True).table)
    assert len(thick.records()) == 2 and "inradius" in thick.props()
    for kw in ({"tta": (1.0,)}, {"tiled": {"tile": 32, "overlap": 8}}):
        r = inference.predict_instances(model, x, shapes=True, **kw)
        assert torch.equal(r.table, shape_descriptors(r.instances).table) and r.table.shape == (2, 256, 11)
    with pytest.raises(ValueError):
        inference.predict_instances(model, x, shapes="area")

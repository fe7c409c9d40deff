"""Contour simplification on the device (csrc/simplify.hip) against the reference (tests/simplify_ref.py), bit for bit, on the case
table of the contour tests plus the extent-limit frames, every case through the default thresholds, with the wave form off and with
both the wave and the LDS form off; rings of 4, 5..8 and 9+ points on the three forms in one call; rings of exactly 4, 64, 65, 2048
and 2049 points at the seams; the ramp comb, whose rounds are linear in its teeth, in every form; garbage-filled buffers, two runs, a
recycled workspace and a side stream; the raw C ABI's refusals; empty inputs; real label_instances output against the CPU path; and
inference.predict_instances(simplify=...) under the plain, tta= and tiled= paths."""
import ctypes as C

import numpy as np
import pytest
import torch

import contours_ref as R
import simplify_ref as S
from test_contours_host import _inst
from test_hull_host import Stub, stub_mask
from test_simplify_host import HOST_IDS, arrays, assert_equal, result_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
SENTINEL = 0x1234567
E16S = (0, 12, 32, 1024)
FORMS = ({}, {"wave_max": 0}, {"wave_max": 0, "lds_max": 0})           # the defaults; no wave form; the global form for all
BIG_IDS = [f"{name}-1x{h}x{w}" for name in ("spiral", "comb", "noise3", "checker") for (h, w) in ((8, 4096), (4096, 8))]


def _need(N, L):
    from uaps_amd import _lib
    return _lib.workspace_bytes("uaps_contours_simplify_workspace_bytes", N, L)


def _raw(entry, src, e16, ws, stream=None, **kw):
    """A C entry point on caller-owned tensors; the code.  src: (points, ring_offsets, rings, summary) on the device."""
    from uaps_amd import _lib
    call = _lib.SimplifyCall()
    call.struct_size = C.sizeof(_lib.SimplifyCall)
    call.B, call.max_instances, call.e16 = src[3].shape[0], src[3].shape[1], e16
    call.n_points, call.n_rings = src[0].shape[0], src[2].shape[0]
    call.points, call.ring_offsets, call.rings, call.summary_in = (t.data_ptr() for t in src)
    call.workspace, call.workspace_bytes = ws.data_ptr(), ws.numel()
    call.stream = _lib.current_stream(DEV) if stream is None else stream
    for k, v in kw.items():
        setattr(call, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return getattr(_lib.lib(), entry)(C.byref(call))


def _run_raw(src, e16, fill, stream=None, ws=None, **forms):
    """mark, the host read, write -- on buffers filled with `fill`; the five arrays as numpy, the totals and the workspace."""
    N, L = src[0].shape[0], src[2].shape[0]
    full = lambda shape, dtype: torch.full(shape, fill, dtype=torch.int64, device=DEV).view(dtype)
    if ws is None:
        ws = full((_need(N, L) // 8,), torch.uint8)
    summary, totals = full(tuple(src[3].shape), torch.int64), full((4,), torch.int64)
    assert _raw("uaps_contours_simplify_mark", src, e16, ws, stream, summary_out=summary, totals=totals, **forms) == 0
    tot = totals.tolist()
    kept = tot[1]
    points, offsets = full((kept,), torch.int32).reshape(-1, 2), full(((L + 2) // 2,), torch.int32)[:L + 1]
    rings, stats = full((L, 7), torch.int64), full((L, 2), torch.int64)
    assert _raw("uaps_contours_simplify_write", src, e16, ws, stream, n_points_out=kept, ring_capacity=L, point_capacity=kept,
                points_out=points, ring_offsets_out=offsets, rings_out=rings, ring_stats=stats, **forms) == 0
    return tuple(t.cpu().numpy() for t in (points, offsets, rings, summary, stats)), tot, ws


def _on_device(tables):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tables)


def _three_forms_equal_the_reference(res, src, e16, what):
    from uaps_amd import simplify_contours
    ref = S.simplified(src, e16)
    got = None
    for kw in FORMS:
        s = simplify_contours(res, e16 / 16.0, **kw)
        assert all(t.is_cuda for t in s.contours[:4]) and s.ring_stats.is_cuda and s.epsilon16 == e16
        got = arrays(s)
        assert_equal(got, ref, (what, e16, kw))
        if e16 == 0:                                                    # P1
            assert all(torch.equal(a, b) for a, b in zip(s.contours[:4], res[:4]))
    return got


@pytest.mark.parametrize("cid", HOST_IDS + BIG_IDS)
def test_device_equals_the_reference_in_every_form_and_the_properties_hold(cid):
    from uaps_amd import contours
    case = R.case(cid)
    for conn in (8, 4):
        for M in (3, 257) if cid in HOST_IDS else (3,):                 # (one M at the extent-limit frames: a second one repeats seconds of rounds)
            res = contours(_inst(case, M, DEV), connectivity=conn)
            src = case.tables(M, conn)
            finer = None
            for e16 in E16S:
                got = _three_forms_equal_the_reference(res, src, e16, (cid, conn, M))     # (the three are the same bits)
                if M == 3:
                    S.check_properties(src, got, e16, finer)
                    finer = got


@pytest.mark.parametrize("cid", [c for c in HOST_IDS if c.endswith("3x17x129")])
def test_rings_of_4_of_5_to_8_and_of_more_points_on_the_three_forms_in_one_call(cid):
    from uaps_amd import contours, simplify_contours
    case = R.case(cid)
    for conn in (8, 4):
        src = case.tables(3, conn)
        res = contours(_inst(case, 3, DEV), connectivity=conn)
        n = src[2][:, 4]
        for e16 in E16S:
            s = simplify_contours(res, e16 / 16.0, wave_max=4, lds_max=8)
            assert_equal(arrays(s), S.simplified(src, e16), (cid, conn, e16))
            if len(n):
                _, tot, _ = _run_raw(_on_device(src), e16, -1, wave_max=4, lds_max=8)
                assert tot[2] == int(((n > 4) & (n <= 8)).sum()) and tot[3] == int((n > 8).sum())
    if cid == "noise3-3x17x129":                                        # all three forms are in use there
        n = case.tables(3, 8)[2][:, 4]
        assert (n == 4).any() and ((n > 4) & (n <= 8)).any() and (n > 8).any()


def _seam_tables():
    """Rings at the seams of the default thresholds: 4, 64, 65 (a 66-point comb less a point), 66, 2048, 2049, 2050 points."""
    out = {}
    for teeth, past, drop in ((1, False, False), (16, False, False), (16, True, True), (16, True, False), (512, False, False),
                              (512, True, True), (512, True, False)):
        t = S.ring_tables(S.comb(teeth, past))
        if drop:
            t = S.drop_point(t)
        assert len(t[2]) == 1
        out[int(t[2][0, 4])] = t
    return out


def test_ring_sizes_at_the_seams_of_the_forms():
    from uaps_amd import simplify_contours
    seams = _seam_tables()
    assert sorted(seams) == [4, 64, 65, 66, 2048, 2049, 2050]
    for n, t in seams.items():
        assert len(t[0]) == n and t[1].tolist() == [0, n]
        src = _on_device(t)
        finer = None
        for e16 in E16S:
            got = _three_forms_equal_the_reference(result_of(t, DEV), t, e16, n)
            S.check_properties(t, got, e16, finer)
            finer = got
            raw, tot, _ = _run_raw(src, e16, -1)                        # the defaults: which form the ring took
            assert_equal(raw, S.simplified(t, e16), (n, e16))
            assert tot[:2] == [1, len(got[0])] and tot[2:] == [int(64 < n <= 2048), int(n > 2048)], (n, tot)
            # the thresholds as operands, n on either side of each (0: the form is off, UAPS_SIMPLIFY_OFF in the C ABI)
            for wave_max, lds_max in ((n, 0), (n - 1, n), (n - 1, n - 1), (0, n), (0, n - 1)):
                if wave_max <= 64 and lds_max <= 2048:
                    raw, tot, _ = _run_raw(src, e16, 7, wave_max=wave_max or -1, lds_max=lds_max or -1)
                    assert_equal(raw, S.simplified(t, e16), (n, e16, wave_max, lds_max))
                    assert tot[2:] == [int(wave_max < n <= lds_max), int(n > wave_max and n > lds_max)]


def test_the_ramp_comb_in_all_three_forms():
    import math
    from uaps_amd import simplify_contours
    for teeth in (64, 15):                                              # 256 points; 60 points: one wave's ring
        t = S.ring_tables(S.ramp_comb(teeth))
        p = [tuple(v) for v in t[0].tolist()]
        assert len(t[2]) == 1 and len(p) == 4 * teeth
        assert S.simplify_ring(p, 12)[1] > 2 * math.log2(len(p))        # a tooth a round
        for e16 in E16S:
            got = _three_forms_equal_the_reference(result_of(t, DEV), t, e16, teeth)
            S.check_properties(t, got, e16)
        _, tot, _ = _run_raw(_on_device(t), 12, -1)
        assert tot[2:] == ([1, 0] if teeth == 64 else [0, 0])           # the LDS form; the wave form


@pytest.mark.parametrize("cid", ("noise3-3x17x129", "checker-3x17x129", "nested-3x17x129", "spiral-3x17x129", "comb-1x2x2100", "gap-3x17x129"))
def test_garbage_buffers_two_runs_a_recycled_workspace_and_a_side_stream_give_the_same_bits(cid):
    case = R.case(cid)
    for M, conn, e16 in ((3, 8, 12), (257, 4, 32)):
        t = case.tables(M, conn)
        src = _on_device(t)
        ref = S.simplified(t, e16)
        for forms in ({}, {"wave_max": 4, "lds_max": 8}, {"wave_max": -1, "lds_max": -1}):
            a, _, ws = _run_raw(src, e16, 0x5a5a5a5a5a5a5a5a, **forms)
            b, _, _ = _run_raw(src, e16, -1, **forms)
            again, _, _ = _run_raw(src, e16, 0x5a5a5a5a5a5a5a5a, ws=ws, **forms)     # a recycled workspace
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                c, _, _ = _run_raw(src, e16, 7, stream=side.cuda_stream, **forms)
            for got in (a, b, again, c):
                assert_equal(got, ref, (cid, M, conn, forms))


def test_every_refusal_returns_its_code_and_leaves_the_outputs_untouched():
    from uaps_amd import _lib
    t = R.case("noise3-3x17x129").tables(4, 8)
    src = _on_device(t)
    e16 = 16
    ref = S.simplified(t, e16)
    N, L, K = len(t[0]), len(t[2]), len(ref[0])
    n = _need(N, L)
    ws = torch.empty(n + 256, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0 and K < N
    mk = lambda shape, dtype=torch.int64: torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
    summary, totals = mk(tuple(t[3].shape)), mk((4,))
    points, offsets, rings, stats = mk((K, 2), torch.int32), mk((L + 1,), torch.int32), mk((L, 7)), mk((L, 2))
    outs = dict(summary_out=summary, totals=totals)
    mark = lambda **kw: _raw("uaps_contours_simplify_mark", src, kw.pop("e16", e16), ws, **{**outs, **kw})
    size = C.sizeof(_lib.SimplifyCall)
    assert mark(struct_size=size - 8) == EINVAL and mark(struct_size=0) == EINVAL                   # a bad struct size
    assert mark(e16=1025) == EINVAL and mark(e16=-1) == EINVAL
    assert mark(wave_max=65) == EINVAL and mark(lds_max=2049) == EINVAL and mark(wave_max=-2) == EINVAL    # above the form's capacity
    assert mark(workspace_bytes=n - 1) == EWORKSPACE and mark(workspace=ws.data_ptr() + 128) == EWORKSPACE  # a short workspace
    assert mark(points=None) == EINVAL and mark(ring_offsets=None) == EINVAL and mark(rings=None) == EINVAL and mark(workspace=None) == EINVAL
    assert mark(summary_in=None) == EINVAL and mark(summary_out=None) == EINVAL and mark(totals=None) == EINVAL
    assert mark(summary_out=src[3]) == EINVAL and mark(totals=summary) == EINVAL
    assert mark(n_points=0) == EINVAL and mark(n_rings=0) == EINVAL and mark(B=0) == EINVAL and mark(max_instances=0) == EINVAL
    assert mark(n_rings=N + 1) == ERANGE and mark(n_points=2 ** 30) == ERANGE
    torch.cuda.synchronize()
    assert bool((summary == SENTINEL).all()) and bool((totals == SENTINEL).all())
    assert mark() == 0 and totals.tolist()[:2] == [L, K]
    assert np.array_equal(summary.cpu().numpy(), ref[3])
    wouts = dict(points_out=points, ring_offsets_out=offsets, rings_out=rings, ring_stats=stats, n_points_out=K, ring_capacity=L, point_capacity=K)
    write = lambda **kw: _raw("uaps_contours_simplify_write", src, kw.pop("e16", e16), ws, **{**wouts, **kw})
    assert write(struct_size=size - 8) == EINVAL and write(e16=1025) == EINVAL and write(wave_max=65) == EINVAL and write(lds_max=2049) == EINVAL
    assert write(points_out=None) == EINVAL and write(ring_offsets_out=None) == EINVAL and write(rings_out=None) == EINVAL
    assert write(ring_stats=None) == EINVAL and write(points=None) == EINVAL
    assert write(ring_capacity=L - 1) == EINVAL and write(point_capacity=K - 1) == EINVAL           # capacities below the totals
    assert write(n_points_out=0) == EINVAL and write(n_points_out=N + 1, point_capacity=N + 1) == EINVAL
    assert write(workspace_bytes=n - 1) == EWORKSPACE
    assert write(n_points_out=K - 1) == 0                               # not the total of this workspace: the launch stores nothing
    torch.cuda.synchronize()
    for out in (points, offsets, rings, stats):
        assert bool((out == SENTINEL).all())
    big_p, big_o, big_r, big_s = mk((K + 3, 2), torch.int32), mk((L + 3,), torch.int32), mk((L + 2, 7)), mk((L + 2, 2))
    assert write(points_out=big_p, ring_offsets_out=big_o, rings_out=big_r, ring_stats=big_s, ring_capacity=L + 2, point_capacity=K + 3) == 0
    assert write() == 0
    for got, want in ((points, ref[0]), (offsets, ref[1]), (rings, ref[2]), (stats, ref[4]), (big_p[:K], ref[0]), (big_o[:L + 1], ref[1]),
                      (big_r[:L], ref[2]), (big_s[:L], ref[4])):
        assert np.array_equal(got.cpu().numpy(), want)
    assert bool((big_p[K:] == SENTINEL).all()) and bool((big_o[L + 1:] == SENTINEL).all()) and bool((big_r[L:] == SENTINEL).all())
    assert bool((big_s[L:] == SENTINEL).all())


def test_empty_input_and_an_all_empty_batch():
    from uaps_amd import contours, simplify_contours
    res = contours(_inst(R.case("empty-2x17x129"), 3, DEV))
    s = simplify_contours(res, 1.0)
    assert s.contours.points.is_cuda and s.contours.points.shape == (0, 2) and s.contours.ring_offsets.tolist() == [0]
    assert s.contours.rings.shape == (0, 7) and s.ring_stats.shape == (0, 2) and not bool(s.contours.summary.any())
    assert s.polygons() == [[], []] and s.reduction()["ratio"] == 1.0
    gap = R.case("gap-3x17x129")                                        # an empty image inside a batch
    g = simplify_contours(contours(_inst(gap, 3, DEV)), 1.0)
    assert_equal(arrays(g), S.simplified(gap.tables(3, 8), 16), "gap")
    assert not bool(g.contours.summary[1].any()) and g.reduction()["per_image"][1] == (0, 0)


def test_device_equals_the_cpu_path_on_real_instances():
    from uaps_amd import contours, label_instances, simplify_contours
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 4, size=(2, 12, 16))
    mask = torch.from_numpy(np.kron(blocks, np.ones((1, 5, 7), dtype=np.int64)) * (rng.random((2, 60, 112)) > 0.08))
    for M, conn in ((64, 8), (300, 4)):
        cpu_inst = label_instances(mask, max_instances=M, connectivity=conn)
        dev_inst = label_instances(mask.to(DEV), max_instances=M, connectivity=conn)
        cpu_c, dev_c = contours(cpu_inst, connectivity=conn), contours(dev_inst, connectivity=conn)
        src = R.tables(cpu_inst.labels.numpy(), M, conn)
        assert int(src[2][:, 4].max()) >= 64 and int(src[2][:, 4].min()) == 4 and int(cpu_inst.count.min()) >= 3
        for eps in (0.75, 2.0):
            cpu, dev = simplify_contours(cpu_c, eps), simplify_contours(dev_c, eps)
            assert_equal(arrays(dev), arrays(cpu), (M, conn, eps))
            assert_equal(arrays(dev), S.simplified(src, dev.epsilon16), (M, conn, eps))
            S.check_properties(src, arrays(dev), dev.epsilon16)
            assert dev.records() == cpu.records() and dev.to_coco() == cpu.to_coco() and dev.reduction() == cpu.reduction()
            assert dev.reduction()["points"] < dev.reduction()["source_points"]


def test_predict_instances_with_simplify_hull_and_shapes():
    import uaps_amd
    from uaps_amd import ContourResult, HullResult, ShapeResult, SimplifiedContours, inference, simplify_contours
    m = stub_mask()
    x = torch.zeros(2, 3, 37, 53)
    kw = dict(contours=True, simplify=1.0, hull=True, shapes=True)
    cpu = inference.predict_instances(Stub(m, 4), x, **kw)
    net = Stub(m, 4)
    net.logits = net.logits.to(DEV)
    dev = inference.predict_instances(net, x.to(DEV), **kw)
    assert isinstance(dev, SimplifiedContours) and isinstance(dev.contours.also, HullResult) and isinstance(dev.contours.also.also, ShapeResult)
    assert_equal(arrays(dev), arrays(cpu), "stub")
    assert dev.records() == cpu.records() and dev.to_coco() == cpu.to_coco()
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    clean = dict(cleanup=[("open", "disk", 1)], components=[("area_open", 2), ("fill_holes", None)])
    for path in ({}, {"tta": (1.0,)}, {"tiled": {"tile": 32, "overlap": 8}}):
        for extra in ({}, clean):
            traced = inference.predict_instances(model, x, contours=True, hull=True, shapes=True, **path, **extra)
            s = inference.predict_instances(model, x, **kw, **path, **extra)
            assert isinstance(s, SimplifiedContours) and isinstance(s.source, ContourResult) and isinstance(s.contours.also, HullResult)
            assert all(torch.equal(a, b) for a, b in zip(s.source[:4], traced[:4])) and torch.equal(s.contours.also.table, traced.also.table)
            direct = simplify_contours(traced, 1.0)
            assert all(torch.equal(a, b) for a, b in zip(s.contours[:4], direct.contours[:4]))
            src = R.tables(s.source.instances.labels.cpu().numpy(), 256, 8)
            assert_equal(arrays(s), S.simplified(src, 16), (path, extra))
            S.check_properties(src, arrays(s), 16)

"""-m gpu: every kernel form of uaps_amd/csrc/conv_strided.hip against the references of tests/strided_ref.py, through the C ABI.

Every input, output, packed weight and workspace is a view into a buffer pre-filled with a sentinel, most of them 1..3 floats off
16-byte alignment (dy only where the case says so: its alignment picks the weight-gradient form).  After every launch the sentinels in
front of and behind every buffer must be untouched -- the workspace's too, which is exactly as large as the query says -- no sentinel
may be left inside an output, and a second launch into re-dirtied outputs and workspace must give the same bits.  The integer-valued run
must equal the int64 reference in every element; the real-valued run stays under the derived bar; packed weights, pooling, sampling and
phase tensors match bit for bit; every refusal leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import strided_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL, ERANGE, EWORKSPACE = 0, -1, -2, -3
GUARD = 16                                    # sentinel elements in front of and behind every view
SENT = {torch.float32: R.SENT, torch.uint8: 0xA5}
DIRT = 7.25                                   # what a workspace is re-dirtied with before the second launch


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    return _lib.lib()


def _stream():
    from uaps_amd import _lib
    return _lib.current_stream(torch.device(DEV))


class Buf:
    """A device tensor `off` elements into a sentinel-filled buffer, GUARD sentinels on both sides (the idea of
    tests/test_gpu_ops_forms.py: the buffer is 256-byte aligned and GUARD floats keep 16 bytes, so off % 4 != 0 misaligns a float view)."""

    def __init__(self, shape, off: int = 0, data=None, dtype=torch.float32):
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        n = int(np.prod(shape))
        self.lo, self.n, self.shape, self.dtype = GUARD + off, n, shape, dtype
        self.buf = torch.full((self.lo + n + GUARD,), SENT[dtype], dtype=dtype, device=DEV)
        self.v = self.buf[self.lo:self.lo + n]
        if data is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))

    @property
    def ptr(self):
        return self.v.data_ptr()

    def fetch(self):
        return self.v.cpu().numpy().reshape(self.shape).copy()

    def guards_ok(self) -> bool:
        s = SENT[self.dtype]
        return bool((self.buf[:self.lo] == s).all() and (self.buf[self.lo + self.n:] == s).all())

    def dirty(self, value=None):
        self.v.fill_(SENT[self.dtype] if value is None else value)

    def untouched(self) -> bool:
        return bool((self.buf == SENT[self.dtype]).all())


def _guards(bufs: dict, where: str):
    return [f"{where}: the sentinels around {k} were written" for k, b in bufs.items() if b is not None and not b.guards_ok()]


def _twice(launch, outs: dict, ws: Buf = None):
    """Launch, fetch the outputs, re-dirty them (and the workspace), launch again: (first results, names whose bits changed)."""
    assert launch() == OK
    torch.cuda.synchronize()
    first = {k: b.fetch() for k, b in outs.items()}
    for b in outs.values():
        b.dirty()
    if ws is not None:
        ws.dirty(DIRT)
    assert launch() == OK
    torch.cuda.synchronize()
    return first, [k for k, b in outs.items() if b.fetch().tobytes() != first[k].tobytes()]


def run_conv(L, c, kind):
    """(ratios, failed checks) of one convolution case with one kind of input: pack, forward, input gradient, weight gradient."""
    inp = R.conv_inputs(c, kind)
    ops = c.ops if kind == "int" else R.real_ops(c)
    bad, ratios, g, st = [], {}, c.geom, _stream()
    x, w = Buf(inp["x"].shape, c.off("x"), inp["x"]), Buf(inp["w"].shape, c.off("w"), inp["w"])
    dy = Buf(inp["dy"].shape, c.off("dy"), inp["dy"])
    assert (dy.ptr % 16 == 0) == (c.offdy % 4 == 0)
    live = dict(x=x, w=w, dy=dy)

    def compare(op, got, changed):
        ref = R.conv_reference(c, inp, op, bar=kind == "real")
        ratio, b = R.check_conv(c, op, kind, got, inp, ref)
        if ratio is not None:
            ratios[op] = ratio
        bad.extend(b + [f"{op}/{kind}: the second launch gave other bits"] * bool(changed) + _guards(live, f"{op}/{kind}"))

    if set(ops) & {"fwd", "dx"}:
        nf, nb = C.c_size_t(), C.c_size_t()
        assert L.uaps_convs_pack_floats(c.Cout, c.Cin, c.ks, C.byref(nf), C.byref(nb)) == OK
        rf, rb = R.pack_weights(inp["w"])
        assert (nf.value, nb.value) == (rf.size, rb.size)
        wf, wb = Buf(nf.value, c.off("wf")), Buf(nb.value, c.off("wb"))
        live.update(wf=wf, wb=wb)
        got, changed = _twice(lambda: L.uaps_convs_pack_weights(w.ptr, c.Cout, c.Cin, c.ks, wf.ptr, wb.ptr, st), dict(wf=wf, wb=wb))
        for k, ref in (("wf", rf), ("wb", rb)):
            if R.bits_differ(got[k], ref):
                bad.append(f"pack/{kind}: {R.bits_differ(got[k], ref)} elements of {k} differ from the reference layout")
        bad.extend([f"pack/{kind}: the second launch gave other bits"] * bool(changed) + _guards(live, "pack"))
    if "fwd" in ops:
        y = Buf(inp["dy"].shape, c.off("y"))
        live["y"] = y
        got, changed = _twice(lambda: L.uaps_convs_fwd(x.ptr, wf.ptr, y.ptr, *g, st), dict(y=y))
        compare("fwd", got["y"], changed)
    if "dx" in ops:
        dx = Buf(inp["x"].shape, c.off("dx"))
        live["dx"] = dx
        got, changed = _twice(lambda: L.uaps_convs_bwd_data(dy.ptr, wb.ptr, dx.ptr, *g, st), dict(dx=dx))
        compare("dx", got["dx"], changed)
    if "dw" in ops and c.ks != 5:
        n = C.c_size_t()
        assert L.uaps_convs_wrw_workspace_bytes(*g, C.byref(n)) == OK and n.value == c.plan["query"] and n.value % 4 == 0
        ws, dw = Buf(n.value // 4, c.off("ws")), Buf(inp["w"].shape, c.off("dw"))
        live.update(ws=ws, dw=dw)
        got, changed = _twice(lambda: L.uaps_convs_bwd_weight(dy.ptr, x.ptr, dw.ptr, *g, ws.ptr, n.value, st), dict(dw=dw), ws)
        compare("dw", got["dw"], changed)
    for k in ("x", "w", "dy"):                     # the inputs are still what they were
        if R.bits_differ(live[k].fetch(), inp[k]):
            bad.append(f"{kind}: the input {k} was written")
    return ratios, bad


def _hip_guard(fn, cid):
    try:
        return fn()
    except RuntimeError as e:                      # a HIP error is sticky: launch nothing more on a device that has faulted
        if "hip" in str(e).lower():
            pytest.exit(f"{cid}: {e}", returncode=3)
        raise


@pytest.mark.parametrize("cid", [c.id for c in R.CONV])
def test_strided_convolution(L, cid):
    c = R.BY_ID[cid]
    bad = []
    for kind in ("int", "real"):
        ratios, b = _hip_guard(lambda: run_conv(L, c, kind), cid)
        print(cid, kind, " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())) or "-")
        bad += b
    assert not bad, bad


def run_plane(L, c):
    """The pooling, sampling and phase kernels: name -> (got, reference), and the failed structural checks."""
    inp = R.pool_inputs(c) if c.entry == "pool" else R.plane_inputs(c)
    ref = R.plane_reference(c, inp)
    B, Cc, H, W = inp["x"].shape
    st, bad = _stream(), []
    x = Buf(inp["x"].shape, c.offx, inp["x"])
    if c.entry == "pool":
        y, idx = Buf(ref["y"].shape), Buf(ref["idx"].shape, dtype=torch.uint8)
        got, ch = _twice(lambda: L.uaps_maxpool3x3s2_fwd(x.ptr, y.ptr, idx.ptr, B * Cc, H, W, st), dict(y=y, idx=idx))
        dy, dx = Buf(inp["dy"].shape, 1, inp["dy"]), Buf(inp["x"].shape, 3)
        got2, ch2 = _twice(lambda: L.uaps_maxpool3x3s2_bwd(dy.ptr, idx.ptr, dx.ptr, B * Cc, H, W, st), dict(dx=dx))
        live = dict(x=x, y=y, idx=idx, dy=dy, dx=dx)
    elif c.entry == "sub":
        y = Buf(ref["y"].shape, c.offy)
        got, ch = _twice(lambda: L.uaps_subsample2_fwd(x.ptr, y.ptr, B * Cc, H, W, st), dict(y=y))
        dy, dx = Buf(inp["dy"].shape, c.offx, inp["dy"]), Buf(inp["x"].shape, c.offy)
        got2, ch2 = _twice(lambda: L.uaps_subsample2_bwd(dy.ptr, dx.ptr, B * Cc, H, W, st), dict(dx=dx))
        live = dict(x=x, y=y, dy=dy, dx=dx)
    else:
        xs, back = Buf(ref["xs"].shape), Buf(inp["x"].shape)
        got, ch = _twice(lambda: L.uaps_space_to_depth2(x.ptr, xs.ptr, B, Cc, H, W, 0, st), dict(xs=xs))
        got2, ch2 = _twice(lambda: L.uaps_space_to_depth2(xs.ptr, back.ptr, B, Cc, H, W, 1, st), dict(back=back))
        live = dict(x=x, xs=xs, back=back)
    got.update(got2)
    bad += [f"the second launch gave other bits of {k}" for k in ch + ch2] + _guards(live, c.entry)
    for k, r in ref.items():
        if R.bits_differ(got[k], r) or R.unwritten(got[k]):
            bad.append(f"{k}: {R.bits_differ(got[k], r)} of {r.size} elements differ in their bits, {R.unwritten(got[k])} never written")
    if c.entry == "pool" and not c.special:        # torch on the CPU: values, arg-max positions, routed gradient
        t = torch.from_numpy(inp["x"]).requires_grad_(True)
        to = F.max_pool2d(t, 3, 2, 1)
        to.backward(torch.from_numpy(inp["dy"]))
        if R.bits_differ(got["y"], to.detach().numpy()) or R.bits_differ(got["dx"], t.grad.numpy()):
            bad.append("differs from torch.nn.functional.max_pool2d and its backward")
    return bad


@pytest.mark.parametrize("cid", [c.id for c in R.CASES if c.entry != "conv"])
def test_pooling_sampling_phases(L, cid):
    bad = _hip_guard(lambda: run_plane(L, R.BY_ID[cid]), cid)
    assert not bad, bad


# ---- refusals: nothing launched, nothing written -----------------------------------------------------------------------------------
def _refused(rc, outs, want):
    torch.cuda.synchronize()
    assert rc == want, rc
    wrote = [k for k, b in outs.items() if not b.untouched()]
    assert not wrote, f"a refused call wrote {wrote}"


def _conv_bufs(g):
    B, Cin, Cout, H, W, ks, s, p = g
    OH, OW = max(R.out_size(H, ks, s, p), 1), max(R.out_size(W, ks, s, p), 1)
    one = lambda *shape: np.ones(shape, np.float32)
    return dict(x=Buf((B, Cin, H, W), 0, one(B, Cin, H, W)), dy=Buf((B, Cout, OH, OW), 0, one(B, Cout, OH, OW)),
                wp=Buf(49 * R.round_up(Cin, 16) * R.round_up(Cout, 16), 0, one(1)), y=Buf((B, Cout, OH, OW)), dx=Buf((B, Cin, H, W)),
                dw=Buf((Cout, Cin, ks, ks)), ws=Buf(1 << 16))


# ks even, ks > 7, stride 3, padding above ks / 2 + 3, negative padding -> UAPS_ERANGE; no output left -> UAPS_EINVAL
@pytest.mark.parametrize("g,want", [((2, 3, 4, 8, 8, 2, 1, 1), ERANGE), ((2, 3, 4, 12, 12, 9, 1, 4), ERANGE), ((2, 3, 4, 8, 8, 3, 3, 1), ERANGE),
                                    ((2, 3, 4, 8, 8, 3, 1, 5), ERANGE), ((2, 3, 4, 8, 8, 3, 2, -1), ERANGE), ((2, 3, 4, 1, 8, 3, 1, 0), EINVAL),
                                    ((0, 3, 4, 8, 8, 3, 1, 1), EINVAL)])
def test_convolutions_refuse_shapes(L, g, want):
    b, st = _conv_bufs((max(g[0], 1),) + g[1:]), _stream()
    outs = dict(y=b["y"], dx=b["dx"], dw=b["dw"], ws=b["ws"])
    _refused(L.uaps_convs_fwd(b["x"].ptr, b["wp"].ptr, b["y"].ptr, *g, st), outs, want)
    _refused(L.uaps_convs_bwd_data(b["dy"].ptr, b["wp"].ptr, b["dx"].ptr, *g, st), outs, want)
    _refused(L.uaps_convs_bwd_weight(b["dy"].ptr, b["x"].ptr, b["dw"].ptr, *g, b["ws"].ptr, b["ws"].n * 4, st), outs, want)
    n = C.c_size_t(12345)
    assert L.uaps_convs_wrw_workspace_bytes(*g, C.byref(n)) == want and n.value == 12345


def test_convolutions_refuse_null_pointers(L):
    g = (2, 3, 4, 8, 8, 3, 1, 1)
    b, st = _conv_bufs(g), _stream()
    outs = dict(y=b["y"], dx=b["dx"], dw=b["dw"], ws=b["ws"])
    x, dy, wp, y, dx, dw, ws = (b[k].ptr for k in ("x", "dy", "wp", "y", "dx", "dw", "ws"))
    for args in ((None, wp, y), (x, None, y), (x, wp, None)):
        _refused(L.uaps_convs_fwd(*args, *g, st), outs, EINVAL)
    for args in ((None, wp, dx), (dy, None, dx), (dy, wp, None)):
        _refused(L.uaps_convs_bwd_data(*args, *g, st), outs, EINVAL)
    for args, w in (((None, x, dw), ws), ((dy, None, dw), ws), ((dy, x, None), ws), ((dy, x, dw), None)):
        _refused(L.uaps_convs_bwd_weight(*args, *g, w, b["ws"].n * 4, st), outs, EINVAL)
    wf, wb = Buf(9 * 4 * 16), Buf(9 * 4 * 16)
    for args in ((None, 4, 3, 3, wf.ptr, wb.ptr), (b["dw"].ptr, 4, 3, 3, None, wb.ptr), (b["dw"].ptr, 4, 3, 3, wf.ptr, None),
                 (b["dw"].ptr, 4, 3, 2, wf.ptr, wb.ptr), (b["dw"].ptr, 0, 3, 3, wf.ptr, wb.ptr)):
        _refused(L.uaps_convs_pack_weights(*args, st), dict(wf=wf, wb=wb), EINVAL)


def test_weight_gradient_refuses_5x5_and_leaves_dw_untouched(L):
    c = R.BY_ID["c5s2"]
    b, st = _conv_bufs(c.geom), _stream()
    _refused(L.uaps_convs_bwd_weight(b["dy"].ptr, b["x"].ptr, b["dw"].ptr, *c.geom, b["ws"].ptr, b["ws"].n * 4, st), dict(dw=b["dw"], ws=b["ws"]),
             ERANGE)


@pytest.mark.parametrize("cid,aligned_plan", [("c3s1-nw1", False), ("stem-c1-o8", False), ("wrw-s2-tiles", False), ("stem-c3-o80-dyoff", False),
                                              ("stem-c3-o80-dyoff", True)])
def test_weight_gradient_refuses_a_short_workspace(L, cid, aligned_plan):
    """One byte less than the form that would run needs -> UAPS_EWORKSPACE, nothing written.  aligned_plan: a dy one float off
    alignment with the workspace the STEM form needs, which is less than the general form that this call runs needs."""
    c = R.BY_ID[cid]
    inp = R.conv_inputs(c, "int")
    need = R.plan_wrw(*c.geom, dy_aligned=True)["ws_bytes"] if aligned_plan else c.plan["ws_bytes"] - 1
    assert need < c.plan["ws_bytes"]
    x, dy = Buf(inp["x"].shape, 0, inp["x"]), Buf(inp["dy"].shape, c.offdy, inp["dy"])
    dw, ws = Buf(inp["w"].shape), Buf(c.plan["query"] // 4)
    _refused(L.uaps_convs_bwd_weight(dy.ptr, x.ptr, dw.ptr, *c.geom, ws.ptr, need, _stream()), dict(dw=dw, ws=ws), EWORKSPACE)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("shape,offs", [((2, 3, 4, 8), (1, 0)), ((2, 3, 4, 8), (0, 2)), ((2, 3, 3, 8), (0, 0)), ((2, 3, 4, 12), (0, 0))])
def test_space_to_depth_refuses(L, shape, offs, inverse):
    """A source or destination off 16 bytes, an odd H, W % 8 != 0 -> UAPS_ERANGE, the destination untouched."""
    B, Cc, H, W = shape
    src, dst = Buf(shape, offs[0], np.ones(shape, np.float32)), Buf(shape, offs[1])
    _refused(L.uaps_space_to_depth2(src.ptr, dst.ptr, B, Cc, H, W, inverse, _stream()), dict(dst=dst), ERANGE)


def test_plane_kernels_refuse_null_and_empty(L):
    shape = (2, 3, 4, 8)
    x, y, idx = Buf(shape, 0, np.ones(shape, np.float32)), Buf(shape), Buf(shape, dtype=torch.uint8)
    outs, st = dict(y=y, idx=idx), _stream()
    for args in ((None, y.ptr, idx.ptr, 6, 4, 8), (x.ptr, None, idx.ptr, 6, 4, 8), (x.ptr, y.ptr, None, 6, 4, 8), (x.ptr, y.ptr, idx.ptr, 0, 4, 8),
                 (x.ptr, y.ptr, idx.ptr, 6, 0, 8), (x.ptr, y.ptr, idx.ptr, 6, 4, 0)):
        _refused(L.uaps_maxpool3x3s2_fwd(*args, st), outs, EINVAL)
        _refused(L.uaps_maxpool3x3s2_bwd(args[0], args[2], args[1], *args[3:], st), outs, EINVAL)
    for args in ((None, y.ptr, 6, 4, 8), (x.ptr, None, 6, 4, 8), (x.ptr, y.ptr, 0, 4, 8), (x.ptr, y.ptr, 6, 0, 8), (x.ptr, y.ptr, 6, 4, 0)):
        _refused(L.uaps_subsample2_fwd(*args, st), outs, EINVAL)
        _refused(L.uaps_subsample2_bwd(*args, st), outs, EINVAL)
    for args in ((None, y.ptr, 2, 3, 4, 8), (x.ptr, None, 2, 3, 4, 8), (x.ptr, y.ptr, 0, 3, 4, 8), (x.ptr, y.ptr, 2, 0, 4, 8)):
        _refused(L.uaps_space_to_depth2(*args, 0, st), outs, EINVAL)


# ---- through the wrappers --------------------------------------------------------------------------------------------------------
def _offset_view(data: np.ndarray, floats: int = 1) -> torch.Tensor:
    """A contiguous device tensor `floats` floats into its storage: .contiguous() returns it as it is."""
    big = torch.zeros(data.size + 8, dtype=torch.float32, device=DEV)
    v = big[floats:floats + data.size].view(data.shape)
    v.copy_(torch.from_numpy(data))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * floats and v.contiguous().data_ptr() == v.data_ptr()
    return v


def test_conv2d_strided_stem_with_a_dy_one_float_into_its_storage(L):
    """The stem's shape with a gradient that is a contiguous view at a 4-byte storage offset: the weight gradient runs the general
    form with the general plan (it used to run it with the stem's: the first 16 ceil(Cout / 64) channels only, and a slab 49 times
    the workspace).  Integer-valued data: the float64 gradient must be met exactly, on every output channel."""
    from uaps_amd.conv import conv2d_strided
    c = R.BY_ID["stem-c3-o80-dyoff"]
    inp = R.conv_inputs(c, "int")
    x = torch.from_numpy(inp["x"]).to(DEV).requires_grad_(True)
    w = torch.from_numpy(inp["w"]).to(DEV).requires_grad_(True)
    y = conv2d_strided(x, w, c.s, c.p)
    seen = []
    y.register_hook(lambda g: seen.append(g.data_ptr() % 16))
    y.backward(_offset_view(inp["dy"]))
    torch.cuda.synchronize()
    assert seen == [4]                                                              # the gradient arrived where it was
    xr, wr = torch.from_numpy(inp["x"]).double().requires_grad_(True), torch.from_numpy(inp["w"]).double().requires_grad_(True)
    F.conv2d(xr, wr, None, c.s, c.p).backward(torch.from_numpy(inp["dy"]).double())
    dw = w.grad.cpu().numpy()
    ref = R.conv_dw(inp["dy"], inp["x"], c.ks, c.s, c.p)
    assert np.array_equal(ref, wr.grad.numpy())
    wrong = sorted(set(np.nonzero(dw.astype(np.float64) != ref)[0].tolist()))
    assert not wrong, f"output channels {wrong} of {c.Cout} differ"
    assert R.int_mismatch(x.grad.cpu().numpy(), xr.grad.numpy()) == 0 and R.int_mismatch(y.detach().cpu().numpy(), R.conv_fwd(inp["x"], inp["w"], c.s, c.p)) == 0


def test_conv3x3s2_supported_follows_the_entry_point_and_res_uaps_takes_the_general_path(L, monkeypatch):
    """uaps_space_to_depth2 refuses a pointer off 16 bytes, so conv3x3s2_supported is false for a contiguous x at a storage offset and
    res_uaps.conv_bn_act runs layer2.0.conv2 on the general strided kernels: the convolution exact on integer data, the BatchNorm +
    ReLU behind it within the bar the suite holds fused.bn_act to (rtol 1e-4, atol 2e-5: tests/test_gpu_fused_ops.py)."""
    from uaps_amd import conv, res_uaps
    B, Cin, Cout, H, W = 2, 6, 20, 6, 16
    rng = np.random.default_rng(11)
    xd, wd = rng.integers(-3, 4, (B, Cin, H, W)).astype(np.float32), rng.integers(-3, 4, (Cout, Cin, 3, 3)).astype(np.float32)
    x_al, x_off = torch.from_numpy(xd).to(DEV), _offset_view(xd)
    assert conv.conv3x3s2_supported(x_al) and not conv.conv3x3s2_supported(x_off)
    assert conv.conv3x3s2_supported(x_off.transpose(2, 3).contiguous().transpose(2, 3))                # not contiguous: copied, so aligned
    assert not conv.conv3x3s2_supported(x_al[:, :, :5]) and not conv.conv3x3s2_supported(x_al[:, :, :, :12].contiguous())
    assert L.uaps_space_to_depth2(x_off.data_ptr(), torch.empty_like(x_al).data_ptr(), B, Cin, H, W, 0, _stream()) == ERANGE
    cv = torch.nn.Conv2d(Cin, Cout, 3, stride=2, padding=1, bias=False).to(DEV)
    with torch.no_grad():
        cv.weight.copy_(torch.from_numpy(wd))
    calls = []
    general, phases = conv.conv2d_strided, conv.conv3x3s2
    monkeypatch.setattr(conv, "conv2d_strided", lambda *a, **k: calls.append(("general", general(*a, **k))) or calls[-1][1])
    monkeypatch.setattr(conv, "conv3x3s2", lambda *a, **k: calls.append(("phases", phases(*a, **k))) or calls[-1][1])
    yref = R.conv_fwd(xd, wd, 2, 1)
    ref = F.relu(F.batch_norm(torch.from_numpy(yref), None, None, torch.ones(Cout, dtype=torch.float64), torch.zeros(Cout, dtype=torch.float64), True))
    for x, path in ((x_off, "general"), (x_al, "phases")):
        calls.clear()
        bn = torch.nn.BatchNorm2d(Cout).to(DEV)
        out = res_uaps.conv_bn_act(x, cv, bn, True, True)
        torch.cuda.synchronize()
        assert [k for k, _ in calls] == [path]
        y = (calls[0][1][0] if isinstance(calls[0][1], tuple) else calls[0][1]).detach().cpu().numpy()
        if path == "general":                      # the exact-f32 kernels: equal; the phase form keeps the bar of tests/test_gpu_strided.py
            assert R.int_mismatch(y, yref) == 0
        else:
            assert np.abs(y - yref).max() <= 2e-5 * np.abs(yref).max()
        torch.testing.assert_close(out.detach().cpu().double(), ref, rtol=1e-4, atol=2e-5)

"""-m gpu: the backward of a ConvBlock's second convolution (3x3, 16 -> 16, 256-wide maps) and the BatchNorm-backward sums of the layer in
front as one full-width-row pass (csrc/mid_bwd_row.hip, include/uaps_hip.h: uaps_mid_bwd_fused) against the three launches it
replaces -- the weight gradient that forms the true dy from the pending transform and writes it through
(uaps_conv_bwd_weight_partial_bn with dyt_*), the input gradient (uaps_conv_bwd_data) and the sums pass of uaps_bn_act_bwd_prepare --
against float64, on the image border and the run boundary, outside its form, and inside a trainer step."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import bn_ref as R
import conv_form_cases as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.01          # LeakyReLU behind BatchNorm 1 (between the two convolutions)
SLOPE2 = 0.01         # LeakyReLU behind BatchNorm 2 (the pending transform of the incoming gradient)
ENOFORM = -4


@pytest.fixture(autouse=True)
def _h16_mode():
    """The kernel exists in the fp16-split arithmetic only: every test runs in that mode whatever an earlier test left behind."""
    from uaps_amd import conv
    conv.set_mode("h16")
    yield
    conv.set_mode("h16")


def _stats(y, groups):
    B = y.shape[0]
    Bg = B // groups
    yd = y.double()
    mean = torch.stack([yd[i * Bg:(i + 1) * Bg].mean((0, 2, 3)) for i in range(groups)]).float()
    var = torch.stack([yd[i * Bg:(i + 1) * Bg].var((0, 2, 3), unbiased=False) for i in range(groups)])
    return mean.contiguous(), (var + 1e-5).rsqrt().float().contiguous()


def _kinkfree(y, mean, invstd, gamma, beta, groups):
    """Against float64 the sign of a BatchNorm output must not hinge on fp32 rounding: no z within 1e-3 of the kink."""
    B = y.shape[0]
    gi = torch.arange(B) // (B // groups)
    mu, ist = mean.double()[gi][:, :, None, None], invstd.double()[gi][:, :, None, None]
    ga, be = gamma.double()[None, :, None, None], beta.double()[None, :, None, None]
    z = (y.double() - mu) * ist * ga + be
    z = torch.where(z.abs() < 1e-3, torch.where(z < 0, -1e-3, 1e-3).double(), z)
    return (mu + (z - be) / (ga * ist)).float()


def _inputs(B, H, groups, seed, W=256, Cin=16, Cout=16, mask=None, kinkfree=False, cfg=0, pending=True):
    """Seeded operands as the decoder's nodes hand them over: d(act2) with its pending transform (the record lazybn.prepare makes of
    (d(act2), y2): coefficient table and the bound of the true dy2), the raw output y1 of the convolution in front with its saved
    statistics and (scale, shift) table, and the activation's bound.  mask [H, W]: every tensor operand is zero outside it."""
    from uaps_amd import bounds, conv, fused, lazybn
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(seed)
    y1 = torch.randn(B, Cin, H, W, generator=g) * 1.5 + 0.2
    y2 = torch.randn(B, Cout, H, W, generator=g) * 1.2 - 0.1
    da = torch.randn(B, Cout, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 10
    gamma, beta = torch.rand(Cin, generator=g) + 0.5, torch.rand(Cin, generator=g) * 0.8 - 0.4
    gamma2, beta2 = torch.rand(Cout, generator=g) + 0.5, torch.rand(Cout, generator=g) * 0.8 - 0.4
    if mask is not None:
        y1, y2, da = y1 * mask, y2 * mask, da * mask
    mean, invstd = _stats(y1, groups)
    mean2, invstd2 = _stats(y2, groups)
    if kinkfree:
        y1 = _kinkfree(y1, mean, invstd, gamma, beta, groups)
        y2 = _kinkfree(y2, mean2, invstd2, gamma2, beta2, groups)
    sc = gamma[None] * invstd
    xf = torch.stack([sc, beta[None] - mean * sc], -1).contiguous()
    s = dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, groups=groups, cfg=cfg)      # cfg: the weight gradient's pixel-split count (0: the plan's)
    for k, v in dict(y=y1, y2=y2, da=da, w=w, gamma=gamma, beta=beta, mean=mean, invstd=invstd, xf=xf, gamma2=gamma2, beta2=beta2,
                     mean2=mean2, invstd2=invstd2).items():
        s[k] = v.to(dev)
    gi = torch.arange(B, device=dev) // (B // groups)
    zz = s["y"] * s["xf"][gi][:, :, 0, None, None] + s["xf"][gi][:, :, 1, None, None]
    s["xb"] = (bounds.from_value(torch.maximum(zz, SLOPE * zz).abs().max() * 1.001 + 1e-30), 1.0)
    s["wb"] = conv.pack_weights(s["w"])[1]
    s["lz"] = None
    if pending:
        dg, db, dc = (torch.empty(Cout, device=dev) for _ in range(3))
        ws = fused._bn_ws(dev, B, Cout, H, W)
        lz = lazybn.prepare(s["da"], s["y2"], s["gamma2"], s["beta2"], s["mean2"], s["invstd2"], SLOPE2, groups, dg, db, dc, ws)
        assert lazybn.take(s["da"]) is lz
        s["lz"] = lz
    return s


def _ws_bytes(s):
    from uaps_amd import _lib
    n = C.c_size_t()
    _lib.check(_lib.lib().uaps_conv_wrw_workspace_bytes(s["B"], s["Cin"], s["Cout"], s["H"], s["W"], 3, s["cfg"], C.byref(n)), "workspace")
    return n.value


def _reduce(s, ws, want_bias):
    from uaps_amd import _lib
    dev = torch.device(DEV)
    dw = torch.empty(s["Cout"], s["Cin"], 3, 3, device=dev)
    db = torch.empty(s["Cout"], device=dev) if want_bias else None
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_conv_bwd_weight_reduce(ws.data_ptr(), dw.data_ptr(), db.data_ptr() if want_bias else None, s["B"], s["Cin"],
                                                    s["Cout"], s["H"], s["W"], 3, s["cfg"], _lib.current_stream(dev))
    _lib.check(rc, "reduce")
    return dw, db


def _finish(s, g, partials=None, maxes=None):
    """BatchNorm 1's reductions of (g, y1): the sums pass, or the finalize alone on the fused kernel's partials."""
    from uaps_amd import bounds, fused, lazybn
    dev = torch.device(DEV)
    dg, db, dc = (torch.empty(s["Cin"], device=dev) for _ in range(3))
    if partials is None:
        ws = fused._bn_ws(dev, s["B"], s["Cin"], s["H"], s["W"])
        lz = lazybn.prepare(g, s["y"], s["gamma"], s["beta"], s["mean"], s["invstd"], SLOPE, s["groups"], dg, db, dc, ws)
    else:
        lz = lazybn.prepare_from_partials(g, s["y"], s["gamma"], s["beta"], s["mean"], s["invstd"], SLOPE, s["groups"], dg, db, dc, partials, maxes)
    assert lazybn.take(g) is lz
    return dict(coef=lz.coef, dgamma=dg, dbeta=db, bound=float(bounds.value(lz.bound[0])), lz=lz)


def _three_launches(s, want_bias):
    from uaps_amd import _lib, conv
    dev = torch.device(DEV)
    lz = s["lz"]
    dy2 = torch.empty_like(s["da"])
    ws = torch.zeros(_ws_bytes(s), dtype=torch.uint8, device=dev)
    with _lib.device_guard(dev):
        hh = _lib.mk_hints((lz.bound, s["xb"]), dyt=(lz.y, lz.coef, dy2, lz.slope, lz.groups))
        rc = _lib.lib().uaps_conv_bwd_weight_partial_bn_h(hh, s["da"].data_ptr(), s["y"].data_ptr(), s["xf"].data_ptr(), SLOPE, s["groups"],
                                                          int(want_bias), s["B"], s["Cin"], s["Cout"], s["H"], s["W"], 3, s["cfg"],
                                                          ws.data_ptr(), ws.numel(), _lib.current_stream(dev))
    _lib.check(rc, "uaps_conv_bwd_weight_partial_bn")
    dw, db = _reduce(s, ws, want_bias)
    g = conv.conv_bwd_data_raw(dy2, s["wb"], s["Cin"], 3, 0, dyb=lz.bound)
    return dict(g=g, dw=dw, db=db, ws=ws, dy2=dy2, **_finish(s, g))


def _fused(s, want_bias):
    from uaps_amd import conv
    ws = torch.zeros(_ws_bytes(s), dtype=torch.uint8, device=torch.device(DEV))
    out = conv.mid_bwd_fused(s["da"], s["lz"], s["y"], s["xf"], s["xb"], s["wb"], s["mean"], s["invstd"], s["gamma"], s["beta"], SLOPE,
                             s["groups"], want_bias, s["cfg"], ws)
    assert out is not None, "the call is inside the kernel's form"
    g, partials, maxes = out
    dw, db = _reduce(s, ws, want_bias)
    return dict(g=g, dw=dw, db=db, ws=ws, partials=partials, maxes=maxes, **_finish(s, g, partials, maxes))


def _compare(s, got, ref, want_bias):
    """Bit for bit: d(act1), the slabs, dW (db), the coefficient table, dgamma, dbeta and the bound."""
    for k in ("ws", "dw", "g", "coef", "dgamma", "dbeta"):  # (the figures first: pytest shows them beside a failure)
        a, b = (got[k].view(torch.float32), ref[k].view(torch.float32)) if k == "ws" else (got[k], ref[k])
        print(k, "differing", int((a != b).sum()), "of", a.numel(), "max |diff|", float((a.double() - b.double()).abs().max()))
    print("bound", got["bound"], ref["bound"])
    assert torch.equal(got["ws"], ref["ws"])               # same run partition, per-run order and dy2 pieces as conv_hrwrw_bn_dt_kernel<1>
    assert torch.equal(got["dw"], ref["dw"])
    if want_bias:
        assert torch.equal(got["db"], ref["db"])
    assert torch.equal(got["g"], ref["g"])                 # the same fp16 pieces of the same dy2 in conv_hr16_kernel<2>'s k order
    for k in ("coef", "dgamma", "dbeta"):                  # a run is the sums pass's 4096-float chunk, summed in that kernel's order
        assert torch.equal(got[k], ref[k]), k
    assert got["bound"] == ref["bound"]


# (B, H, groups): one run per image; a run boundary inside the image (the halo dy2 rows are real data) and two statistics groups; an
# odd image count
SHAPES = [(2, 16, 1), (4, 32, 2), (3, 32, 1)]


@pytest.mark.parametrize("want_bias", [False, True])
@pytest.mark.parametrize("B,H,groups", SHAPES)
def test_one_pass_equals_the_three_launches_and_repeats(B, H, groups, want_bias):
    from uaps_amd import lazybn
    s = _inputs(B, H, groups, seed=21 + B + H)
    ref = _three_launches(s, want_bias)
    got = _fused(s, want_bias)
    _compare(s, got, ref, want_bias)
    again = _fused(s, want_bias)                           # a second launch: the same bits everywhere
    for k in ("g", "ws", "dw", "partials", "maxes", "coef", "dgamma", "dbeta"):
        assert torch.equal(got[k], again[k]), k
    if want_bias:
        assert torch.equal(got["db"], again["db"])
    assert got["bound"] == again["bound"]
    lazybn.reset()


@pytest.mark.parametrize("nsplit", [1, 3, 5])
def test_several_runs_per_workgroup(nsplit):
    """(4, 32, 2) = 8 runs with the pixel-split count forced to 1, 3 and 5: a workgroup walks through several runs, images and
    statistics groups (rings re-staged, sums restarted, tap accumulators and maxima carried), and 3 and 5 do not divide 8."""
    from uaps_amd import lazybn
    s = _inputs(4, 32, 2, seed=33, cfg=nsplit)
    assert _ws_bytes(s) == nsplit * (9 * 16 * 16 + 16) * 4
    got = _fused(s, True)
    _compare(s, got, _three_launches(s, True), True)
    again = _fused(s, True)
    for k in ("g", "ws", "partials", "maxes"):
        assert torch.equal(got[k], again[k]), k
    lazybn.reset()


def _border_mask(H, W=256):
    m = torch.zeros(H, W)
    m[0], m[-1], m[:, 0], m[:, -1] = 1, 1, 1, 1
    return m


def _seam_mask(H, W=256):
    m = torch.zeros(H, W)
    m[15], m[16] = 1, 1
    return m


@pytest.mark.parametrize("where", ["border", "run_boundary"])
def test_borders(where):
    """Operands that are zero except in row 0, the last row, column 0 and column 255 (the halo rows outside the image and the margin
    groups carry everything); and operands that are non-zero only in rows 15 and 16 of H = 32, either side of the run boundary: a halo
    row that leaked into the weight gradient, or one missing from the input gradient, shows there."""
    from uaps_amd import lazybn
    s = _inputs(2, 32, 1, seed=9, mask=_border_mask(32) if where == "border" else _seam_mask(32))
    _compare(s, _fused(s, True), _three_launches(s, True), True)
    lazybn.reset()


def test_against_float64():
    """(4, 32, 2) against float64 convolutions of the float64 dy2 and tests/bn_ref.py: d(act1) and dW under the bars of the convolution
    forms replaced (conv_form_cases: conv_hr16_kernel<2> for the input gradient, conv_hrwrw_bn_dt_kernel<1> for the weight gradient),
    the BatchNorm coefficients, dgamma, dbeta and the dy bound under the bars of tests/test_gpu_head_bwd_fused.py::test_against_float64."""
    from uaps_amd import lazybn
    B, H, groups = 4, 32, 2
    s = _inputs(B, H, groups, seed=5, kinkfree=True)
    got = _fused(s, True)
    cpu = {k: s[k].cpu() for k in ("y", "y2", "da", "w", "gamma", "beta", "mean", "invstd", "xf")}
    # weight and bias gradient: x = leaky_relu(fma(y1, xf)), dy2 from (d(act2), y2, the coefficient table)
    cw = F.Case("conv_hrwrw_bn_dt_kernel<1>", F.WRW, "h16", B, 16, 16, H, 256, bounded=(0, 1), xf=(SLOPE, groups), dyt=(SLOPE2, groups), want_bias=True)
    inp = dict(x=cpu["y"], w=cpu["w"], dy=cpu["da"], bias=torch.zeros(16), xf=cpu["xf"], dyt_coef=s["lz"].coef.cpu(), bn=dict(y=cpu["y2"]))
    rw = F.reference(cw, inp, floors=F.h16_floors(cw, inp))
    ok, info = F.check(got["dw"].cpu(), rw, F.TAU_DW, F.fp32_cpu_rms(cw, inp, rw))
    print("dw", info)
    assert ok, info
    dy64 = F.true_dy(cw, inp)
    db64 = dy64.sum((0, 2, 3))
    db_err = float((got["db"].cpu().double() - db64).abs().max())
    print("db", db_err, F.TAU_DW * float(dy64.abs().sum((0, 2, 3)).max()))
    assert db_err <= F.TAU_DW * float(dy64.abs().sum((0, 2, 3)).max())
    # input gradient of the float64 dy2
    cg = F.Case("conv_hr16_kernel<2>", F.BWD_DATA, "h16", B, 16, 16, H, 256, bounded=(0,))
    inp_g = dict(x=cpu["y"], w=cpu["w"], dy=dy64, bias=torch.zeros(16))
    rg = F.reference(cg, inp_g, floors=F.h16_floors(cg, inp_g))
    ok, info = F.check(got["g"].cpu(), rg, F.TAU_Y, F.fp32_cpu_rms(cg, inp_g, rg))
    print("g", info)
    assert ok, info
    # BatchNorm 1's reductions of (g, y1) in float64 from the float64 g
    bw = R.backward(rg["ref"].numpy(), cpu["y"].numpy(), cpu["gamma"].numpy(), cpu["beta"].numpy(), cpu["mean"].numpy(), cpu["invstd"].numpy(),
                    groups=groups, slope=SLOPE)
    coef = torch.tensor(R.two_halves_coef(bw, cpu["mean"].numpy(), cpu["invstd"].numpy(), cpu["gamma"].numpy(), cpu["beta"].numpy()))
    torch.testing.assert_close(got["coef"].cpu().double(), coef, rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(got["dgamma"].cpu().double(), torch.tensor(bw["dgamma"]), rtol=2e-5, atol=1e-3)
    torch.testing.assert_close(got["dbeta"].cpu().double(), torch.tensor(bw["dbeta"]), rtol=2e-5, atol=1e-3)
    b64 = R.dy_bound(bw)
    assert float(np.abs(bw["dy"]).max()) <= got["bound"] and abs(got["bound"] - b64) <= 1e-4 * b64
    lazybn.reset()


def _raw_call(s, dzb=True, xb=True, pending=True):
    """uaps_mid_bwd_fused on sentinel-filled outputs: (return code, were the outputs left alone)."""
    from uaps_amd import _lib, bounds
    dev = torch.device(DEV)
    lz = s["lz"]
    g = torch.full_like(s["y"], 7.0)
    partials = torch.full((s["Cin"], s["B"], max(s["H"] // 16, 1), 2), 7.0, device=dev)
    maxes = torch.full((2 * bounds.FLOATS,), 7.0, device=dev)
    ws = torch.full((_ws_bytes(s),), 7, dtype=torch.uint8, device=dev)
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_mid_bwd_fused(s["da"].data_ptr(), lz.y.data_ptr() if pending else None, lz.coef.data_ptr() if pending else None,
                                           SLOPE2, s["groups"], s["y"].data_ptr(), s["xf"].data_ptr(), SLOPE, s["groups"], s["wb"].data_ptr(),
                                           lz.bound[0].data_ptr() if dzb else None, 1.0, s["xb"][0].data_ptr() if xb else None, 1.0,
                                           s["mean"].data_ptr(), s["invstd"].data_ptr(), s["gamma"].data_ptr(), s["beta"].data_ptr(), 1, s["B"],
                                           s["Cin"], s["Cout"], s["H"], s["W"], 3, 0, g.data_ptr(), partials.data_ptr(), maxes.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _lib.current_stream(dev))
    torch.cuda.synchronize()
    untouched = all(bool((t == 7).all()) for t in (g, partials, maxes, ws))
    return rc, untouched


@pytest.mark.parametrize("what", ["W128", "H24", "Cout8", "no_dy_bound", "no_x_bound", "no_pending", "exact"])
def test_outside_its_form_nothing_is_launched_and_the_three_launches_run(what):
    from uaps_amd import conv, lazybn
    B, Cout, H, W = dict(W128=(2, 16, 16, 128), H24=(2, 16, 24, 256), Cout8=(2, 8, 16, 256)).get(what, (2, 16, 16, 256))
    s = _inputs(B, H, 1, seed=3, W=W, Cout=Cout)
    try:
        if what == "exact":
            conv.set_mode("exact")
        rc, untouched = _raw_call(s, dzb=what != "no_dy_bound", xb=what != "no_x_bound", pending=what != "no_pending")
        assert rc == ENOFORM and untouched
        lz = s["lz"]
        if what == "no_dy_bound":
            lz = lazybn.Lazy(lz.y, lz.coef, lz.slope, lz.groups, None)
        ws = torch.zeros(_ws_bytes(s), dtype=torch.uint8, device=torch.device(DEV))
        assert conv.mid_bwd_fused(s["da"], None if what == "no_pending" else lz, s["y"], s["xf"], None if what == "no_x_bound" else s["xb"], s["wb"],
                                  s["mean"], s["invstd"], s["gamma"], s["beta"], SLOPE, 1, True, 0, ws) is None
        assert what in ("no_dy_bound", "no_x_bound", "no_pending") or not conv.mid_bwd_eligible(s["da"], s["y"], 3)
    finally:
        conv.set_mode("h16")
    # the node's backward on such a call: the separate launches, never the fused kernel.  (A pending record always carries the bound
    # of its gradient, so a node never sees `no_dy_bound`: the library call above covers it.)
    if what != "no_dy_bound":
        names = _node_backward(B, Cout, H, W, mode="exact" if what == "exact" else "h16", bound_x=what != "no_x_bound",
                               pending=what != "no_pending")["names"]
        assert names and conv.MID_BWD_KERNEL not in names, names
    lazybn.reset()


def _node_backward(B, Cout, H, W, mode="h16", bound_x=True, pending=True, hook=None):
    """conv1 -> BatchNorm 1 -> LeakyReLU -> conv2 (16 -> Cout) -> BatchNorm 2 -> LeakyReLU -> 3x3 to 4 classes inside lazybn.scope(): the
    kernels the backward timed, and the gradients.  pending False: the gradient reaches conv2's node as it is (no BatchNorm 2).
    bound_x False: the activation between the two convolutions reaches conv2's node without a magnitude bound."""
    import torch.nn as nn
    from uaps_amd import bounds, conv, fused, lazybn
    torch.manual_seed(2)
    x = torch.randn(B, 16, H, W, device=DEV, requires_grad=True)
    w1 = (torch.randn(16, 16, 3, 3, device=DEV) / 10).requires_grad_(True)
    w2 = (torch.randn(Cout, 16, 3, 3, device=DEV) / 10).requires_grad_(True)
    w3 = (torch.randn(4, Cout, 3, 3, device=DEV) / 10).requires_grad_(True)
    bn1, bn2 = nn.BatchNorm2d(16).to(DEV), nn.BatchNorm2d(Cout).to(DEV)
    bounds.refresh([bn1, bn2])
    try:
        conv.set_mode(mode)
        with lazybn.scope():
            y1, st1 = conv.conv2d_with_stats(bounds.put(x, bounds.from_value(x.detach().abs().max())), w1, None)
            if hook is not None:
                y1.register_hook(hook)
            real = bounds.bn_output_bound
            try:
                if not bound_x:
                    bounds.bn_output_bound = lambda *a, **k: None
                if pending:
                    y2, st2 = fused.bn_act_conv(y1, st1, None, bn1, SLOPE, w2, None, want_stats=True)
                else:
                    z = fused.bn_act_conv(y1, st1, None, bn1, SLOPE, w2, None)
            finally:
                bounds.bn_output_bound = real
            if pending:
                z = fused.bn_act_conv(y2, st2, None, bn2, SLOPE2, w3, None)
            g = torch.randn_like(z)
            conv.KERNEL_EVENTS, conv.EVENT_FILTER = {}, None
            z.backward(bounds.put(g, bounds.from_value(g.abs().max())))
            names, conv.KERNEL_EVENTS = set(conv.KERNEL_EVENTS), None
    finally:
        conv.KERNEL_EVENTS = None
        conv.set_mode("h16")
    assert w2.grad is not None and bool(torch.isfinite(w2.grad).all()) and bool(torch.isfinite(x.grad).all())
    return dict(names=names, dx=x.grad, dw1=w1.grad, dw2=w2.grad)


def test_the_node_takes_the_fused_pass_inside_a_scope():
    """The node takes the fused pass and none of the launches it replaces; with the switch off the gradients are the same bits.  A
    hook on y1 keeps the pass off (the observer sees the true gradient, bit for bit what it sees with the switch off)."""
    from uaps_amd import conv
    prev = conv._FUSED_MID
    seen = {}
    try:
        on = _node_backward(2, 16, 16, 256)
        hooked = _node_backward(2, 16, 16, 256, hook=lambda g: seen.__setitem__("on", g.detach().clone()))
        conv._FUSED_MID = False
        off = _node_backward(2, 16, 16, 256)
        _node_backward(2, 16, 16, 256, hook=lambda g: seen.__setitem__("off", g.detach().clone()))
    finally:
        conv._FUSED_MID = prev
    assert conv.MID_BWD_KERNEL in on["names"] and "conv_hrwrw_bn_dt_kernel<1>" not in on["names"], on["names"]
    assert conv.MID_BWD_KERNEL not in off["names"] and "conv_hrwrw_bn_dt_kernel<1>" in off["names"], off["names"]
    for k in ("dx", "dw1", "dw2"):
        assert torch.equal(on[k], off[k]), k
    assert conv.MID_BWD_KERNEL not in hooked["names"], hooked["names"]
    assert torch.equal(seen["on"], seen["off"]) and torch.equal(hooked["dx"], off["dx"])


def test_retain_grad_keeps_the_fused_pass_off():
    from uaps_amd import conv
    kept = {}

    def keep(y):                                           # (called as a hook factory: retain_grad() on y1 itself)
        kept["y"] = y
    import torch.nn as nn
    from uaps_amd import bounds, fused, lazybn
    torch.manual_seed(2)
    x = torch.randn(2, 16, 16, 256, device=DEV, requires_grad=True)
    w1, w2, w3 = ((torch.randn(o, 16, 3, 3, device=DEV) / 10).requires_grad_(True) for o in (16, 16, 4))
    bn1, bn2 = nn.BatchNorm2d(16).to(DEV), nn.BatchNorm2d(16).to(DEV)
    bounds.refresh([bn1, bn2])
    try:
        with lazybn.scope():
            y1, st1 = conv.conv2d_with_stats(bounds.put(x, bounds.from_value(x.detach().abs().max())), w1, None)
            y1.retain_grad()
            y2, st2 = fused.bn_act_conv(y1, st1, None, bn1, SLOPE, w2, None, want_stats=True)
            z = fused.bn_act_conv(y2, st2, None, bn2, SLOPE2, w3, None)
            g = torch.randn_like(z)
            conv.KERNEL_EVENTS, conv.EVENT_FILTER = {}, None
            z.backward(bounds.put(g, bounds.from_value(g.abs().max())))
            names, conv.KERNEL_EVENTS = set(conv.KERNEL_EVENTS), None
    finally:
        conv.KERNEL_EVENTS = None
    assert names and conv.MID_BWD_KERNEL not in names, names
    assert y1.grad is not None and bool(torch.isfinite(y1.grad).all())


def test_trainer_step_with_the_switch_on_and_off():
    """One training step at 2 + 2 images of 32 x 256 with UAPS_FUSED_MID_BWD on and off: the same loss (the forward is untouched) and
    the same state (buffers, Adam moments, parameters) bit for bit; nothing pending; the fused kernel once per decoder and four
    launches fewer of each convolution kernel it replaces."""
    import uaps_amd
    from uaps_amd import conv, lazybn
    torch.manual_seed(6)
    m_on = uaps_amd.UNet_UAPS(3, 4, feature_chns=[16, 16, 32, 32, 64])
    m_off = copy.deepcopy(m_on)
    rng = np.random.default_rng(4)
    xl = torch.tensor(rng.standard_normal((2, 3, 32, 256)).astype(np.float32)).to(DEV)
    xu = torch.tensor(rng.standard_normal((2, 3, 32, 256)).astype(np.float32)).to(DEV)
    yl = torch.tensor(uaps_amd.data.synthetic_masks(rng, 2, 4, 32, 256)).to(DEV)
    res, names, opt = {}, {}, {}
    prev = conv._FUSED_MID
    try:
        for on, m in ((True, m_on), (False, m_off)):
            conv._FUSED_MID = on
            tr = uaps_amd.UAPSTrainer(m.to(DEV), base_lr=1e-3, seed=11)
            uaps_amd.perturb.manual_seed(7, 0)
            np.random.seed(7)
            conv.KERNEL_EVENTS, conv.EVENT_FILTER = {}, None
            res[on] = float(tr.train_step(xl, yl, xu)["loss"])
            names[on], conv.KERNEL_EVENTS = {k: len(v) for k, v in conv.KERNEL_EVENTS.items()}, None
            opt[on] = tr.optimizer
            lazybn.assert_none_pending()
    finally:
        conv._FUSED_MID, conv.KERNEL_EVENTS = prev, None
    assert res[True] == res[False]
    for (n, ba), bb in zip(m_on.named_buffers(), m_off.buffers()):
        assert torch.equal(ba, bb), n                      # running statistics: the forward is the same
    # d(act1), the slabs and the BatchNorm partial sums are the three launches' bit for bit: so is the whole step
    sa, sb = opt[True].state_dict()["state"], opt[False].state_dict()["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    for k in sa:
        assert torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]), k
    for (n, pa), pb in zip(m_on.named_parameters(), m_off.parameters()):
        assert torch.equal(pa, pb), n
    assert names[True].get(conv.MID_BWD_KERNEL) == 4 and conv.MID_BWD_KERNEL not in names[False], (names[True], names[False])
    old = ("conv_hrwrw_bn_dt_kernel<1>", "conv_hr16_kernel<2>")
    assert all(names[False].get(k, 0) >= 4 for k in old), names[False]
    # what the switch-off step ran for the ConvBlock's second convolution is gone: four launches fewer of each
    assert all(names[True].get(k, 0) == names[False][k] - 4 for k in old), (names[True], names[False])

"""-m gpu: out_conv's backward and the BatchNorm-backward sums of the layer in front as one full-width-row pass
(csrc/head_bwd_row.hip, include/uaps_hip.h: uaps_head_bwd_fused) against the three launches it replaces -- the input gradient
(uaps_conv_bwd_data), the weight gradient with the staging-time BatchNorm (uaps_conv_bwd_weight_partial_bn) and the sums pass of
uaps_bn_act_bwd_prepare -- against float64, on the image border, outside its form, and inside a trainer step."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import bn_ref as R
import conv_form_cases as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.01
ENOFORM = -4


@pytest.fixture(autouse=True)
def _h16_mode():
    """The kernel exists in the fp16-split arithmetic only: every test runs in that mode whatever an earlier test left behind."""
    from uaps_amd import conv
    conv.set_mode("h16")
    yield
    conv.set_mode("h16")


def _inputs(B, Cout, H, groups, seed, W=256, Cin=16, border=False, kinkfree=False, cfg=0):
    """Seeded operands shaped like test_backward_sums_in_the_input_gradient_epilogue_match_the_sums_pass, as the decoder's last two
    nodes hand them over: d logits, the raw conv output y with its saved statistics, the (scale, shift) table and both bounds."""
    from uaps_amd import bounds, conv
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, Cin, H, W, generator=g) * 1.5 + 0.2
    dz = torch.randn(B, Cout, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 10
    gamma = torch.rand(Cin, generator=g) + 0.5
    beta = torch.rand(Cin, generator=g) * 0.8 - 0.4
    if border:                                            # only row 0, the last row, column 0 and the last column carry anything
        m = torch.zeros(H, W)
        m[0], m[-1], m[:, 0], m[:, -1] = 1, 1, 1, 1
        y, dz = y * m, dz * m
    Bg = B // groups
    yd = y.double()
    mean = torch.stack([yd[i * Bg:(i + 1) * Bg].mean((0, 2, 3)) for i in range(groups)]).float()
    var = torch.stack([yd[i * Bg:(i + 1) * Bg].var((0, 2, 3), unbiased=False) for i in range(groups)])
    invstd = (var + 1e-5).rsqrt().float()
    if kinkfree:      # against float64 the sign of the BatchNorm output must not hinge on fp32 rounding: no z within 1e-3 of the kink
        gi = torch.arange(B) // Bg
        mu, ist = mean.double()[gi][:, :, None, None], invstd.double()[gi][:, :, None, None]
        ga, be = gamma.double()[None, :, None, None], beta.double()[None, :, None, None]
        z = (yd - mu) * ist * ga + be
        z = torch.where(z.abs() < 1e-3, torch.where(z < 0, -1e-3, 1e-3).double(), z)
        y = (mu + (z - be) / (ga * ist)).float()
    sc = gamma[None] * invstd
    xf = torch.stack([sc, beta[None] - mean * sc], -1).contiguous()
    s = dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, groups=groups, cfg=cfg)      # cfg: the weight gradient's pixel-split count (0: the plan's)
    for k, v in dict(y=y, dz=dz, w=w, gamma=gamma, beta=beta, mean=mean.contiguous(), invstd=invstd.contiguous(), xf=xf).items():
        s[k] = v.to(dev)
    gi = torch.arange(B, device=dev) // Bg
    zz = s["y"] * s["xf"][gi][:, :, 0, None, None] + s["xf"][gi][:, :, 1, None, None]
    s["xb"] = (bounds.from_value(torch.maximum(zz, SLOPE * zz).abs().max() * 1.001 + 1e-30), 1.0)
    s["dzb"] = (bounds.from_value(s["dz"].abs().max() + 1e-30), 1.0)
    s["wb"] = conv.pack_weights(s["w"])[1]
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
    """The BatchNorm's reductions of (g, y): the sums pass, or the finalize alone on the fused kernel's partials."""
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
    g = conv.conv_bwd_data_raw(s["dz"], s["wb"], s["Cin"], 3, 0, dyb=s["dzb"])
    ws = torch.zeros(_ws_bytes(s), dtype=torch.uint8, device=dev)
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_conv_bwd_weight_partial_bn_h(_lib.mk_hints((s["dzb"], s["xb"])), s["dz"].data_ptr(), s["y"].data_ptr(),
                                                          s["xf"].data_ptr(), SLOPE, s["groups"], int(want_bias), s["B"], s["Cin"], s["Cout"],
                                                          s["H"], s["W"], 3, s["cfg"], ws.data_ptr(), ws.numel(), _lib.current_stream(dev))
    _lib.check(rc, "uaps_conv_bwd_weight_partial_bn")
    dw, db = _reduce(s, ws, want_bias)
    return dict(g=g, dw=dw, db=db, ws=ws, **_finish(s, g))


def _fused(s, want_bias):
    from uaps_amd import conv
    ws = torch.zeros(_ws_bytes(s), dtype=torch.uint8, device=torch.device(DEV))
    out = conv.head_bwd_fused(s["dz"], s["dzb"], s["y"], s["xf"], s["xb"], s["wb"], s["mean"], s["invstd"], s["gamma"], s["beta"], SLOPE,
                              s["groups"], want_bias, s["cfg"], ws)
    assert out is not None, "the call is inside the kernel's form"
    g, partials, maxes = out
    dw, db = _reduce(s, ws, want_bias)
    return dict(g=g, dw=dw, db=db, ws=ws, partials=partials, maxes=maxes, **_finish(s, g, partials, maxes))


def _compare(s, got, ref, want_bias):
    from uaps_amd import lazybn
    assert torch.equal(got["g"], ref["g"])                 # the fp32 matrix instruction in the tile kernel's k order
    assert torch.equal(got["dw"], ref["dw"])               # same run partition and per-run order as conv_hrwrw_bn_kernel<1>: the same slabs
    assert torch.equal(got["ws"], ref["ws"])
    if want_bias:
        assert torch.equal(got["db"], ref["db"])
    torch.testing.assert_close(got["coef"], ref["coef"], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(got["dgamma"], ref["dgamma"], rtol=2e-5, atol=1e-3)
    torch.testing.assert_close(got["dbeta"], ref["dbeta"], rtol=2e-5, atol=1e-3)
    dy = lazybn.materialize(got["g"], got["lz"])
    assert float(dy.abs().max()) <= got["bound"] and abs(got["bound"] - ref["bound"]) <= 1e-4 * ref["bound"]
    # more than those bars ask: a run is the sums pass's 4096-float chunk and is summed in that kernel's order, so the same bits
    # (the one-piece backward and a hook on the conv output see what they saw: tests/test_gpu_lazy_bn.py)
    for k in ("coef", "dgamma", "dbeta"):
        assert torch.equal(got[k], ref[k]), k
    assert got["bound"] == ref["bound"]


# (B, Cout, H, groups): one run per image; a run boundary inside the image and two statistics groups; absent output channels and an
# odd image count; one output channel.  (Split counts that do not divide the run count: test_several_runs_per_workgroup.)
SHAPES = [(2, 4, 16, 1), (4, 4, 32, 2), (3, 2, 32, 1), (2, 1, 16, 2)]


@pytest.mark.parametrize("want_bias", [False, True])
@pytest.mark.parametrize("B,Cout,H,groups", SHAPES)
def test_one_pass_equals_the_three_launches_and_repeats(B, Cout, H, groups, want_bias):
    from uaps_amd import conv, lazybn
    s = _inputs(B, Cout, H, groups, seed=21 + B + Cout)
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
    """(4, 4, 32, 2) = 8 runs with the pixel-split count forced to 1, 3 and 5: a workgroup walks through several runs, images and
    statistics groups (rings re-staged, sums restarted, tap accumulators and maxima carried), and 3 and 5 do not divide 8."""
    from uaps_amd import lazybn
    s = _inputs(4, 4, 32, 2, seed=33, cfg=nsplit)
    assert _ws_bytes(s) == nsplit * (9 * 4 * 16 + 4) * 4
    got = _fused(s, True)
    _compare(s, got, _three_launches(s, True), True)
    again = _fused(s, True)
    for k in ("g", "ws", "partials", "maxes"):
        assert torch.equal(got[k], again[k]), k
    lazybn.reset()


def test_against_float64():
    """(4, 4, 32, 2) against a float64 convolution and tests/bn_ref.py: g and dW under the convolution forms' bars (conv_form_cases),
    the BatchNorm coefficients, dgamma, dbeta and the dy bound under the bars of the comparison with the sums pass."""
    from uaps_amd import conv, lazybn
    B, Cout, H, groups = 4, 4, 32, 2
    s = _inputs(B, Cout, H, groups, seed=5, kinkfree=True)
    got = _fused(s, True)
    cpu = {k: s[k].cpu() for k in ("y", "dz", "w", "gamma", "beta", "mean", "invstd", "xf")}
    # input gradient
    cg = F.Case("conv_fwd_kernel<3, 8, 32, 16, 4, 4, 1>", F.BWD_DATA, "exact", B, 16, Cout, H, 256)
    inp = dict(x=cpu["y"], w=cpu["w"], dy=cpu["dz"], bias=torch.zeros(Cout))
    rg = F.reference(cg, inp)
    ok, info = F.check(got["g"].cpu(), rg, F.TAU_Y, F.fp32_cpu_rms(cg, inp, rg))
    print("g", info)
    assert ok, info
    # weight and bias gradient
    cw = F.Case("conv_hrwrw_bn_kernel<1>", F.WRW, "h16", B, 16, Cout, H, 256, bounded=(0, 1), xf=(SLOPE, groups), want_bias=True)
    inp["xf"] = cpu["xf"]
    rw = F.reference(cw, inp, floors=F.h16_floors(cw, inp))
    ok, info = F.check(got["dw"].cpu(), rw, F.TAU_DW, F.fp32_cpu_rms(cw, inp, rw))
    print("dw", info)
    assert ok, info
    db64 = cpu["dz"].double().sum((0, 2, 3))
    assert float((got["db"].cpu().double() - db64).abs().max()) <= F.TAU_DW * float(cpu["dz"].double().abs().sum((0, 2, 3)).max())
    # BatchNorm reductions of (g, y) in float64 from the float64 g
    bw = R.backward(rg["ref"].numpy(), cpu["y"].numpy(), cpu["gamma"].numpy(), cpu["beta"].numpy(), cpu["mean"].numpy(), cpu["invstd"].numpy(),
                    groups=groups, slope=SLOPE)
    coef = torch.tensor(R.two_halves_coef(bw, cpu["mean"].numpy(), cpu["invstd"].numpy(), cpu["gamma"].numpy(), cpu["beta"].numpy()))
    torch.testing.assert_close(got["coef"].cpu().double(), coef, rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(got["dgamma"].cpu().double(), torch.tensor(bw["dgamma"]), rtol=2e-5, atol=1e-3)
    torch.testing.assert_close(got["dbeta"].cpu().double(), torch.tensor(bw["dbeta"]), rtol=2e-5, atol=1e-3)
    b64 = R.dy_bound(bw)
    assert float(np.abs(bw["dy"]).max()) <= got["bound"] and abs(got["bound"] - b64) <= 1e-4 * b64
    lazybn.reset()


def test_borders():
    """Operands that are zero except in row 0, the last row, column 0 and column 255: the halo rows of both rings and the margin
    groups carry everything."""
    from uaps_amd import conv, lazybn
    s = _inputs(2, 4, 32, 1, seed=9, border=True)
    _compare(s, _fused(s, True), _three_launches(s, True), True)
    lazybn.reset()


def _raw_call(s, dzb=True, xb=True):
    """uaps_head_bwd_fused on sentinel-filled outputs: (return code, were the outputs left alone)."""
    from uaps_amd import _lib, bounds
    dev = torch.device(DEV)
    g = torch.full_like(s["y"], 7.0)
    partials = torch.full((s["Cin"], s["B"], max(s["H"] // 16, 1), 2), 7.0, device=dev)
    maxes = torch.full((2 * bounds.FLOATS,), 7.0, device=dev)
    ws = torch.full((_ws_bytes(s),), 7, dtype=torch.uint8, device=dev)
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_head_bwd_fused(s["dz"].data_ptr(), s["y"].data_ptr(), s["xf"].data_ptr(), SLOPE, s["groups"], s["wb"].data_ptr(),
                                            s["dzb"][0].data_ptr() if dzb else None, 1.0, s["xb"][0].data_ptr() if xb else None, 1.0,
                                            s["mean"].data_ptr(), s["invstd"].data_ptr(), s["gamma"].data_ptr(), s["beta"].data_ptr(), 1, s["B"],
                                            s["Cin"], s["Cout"], s["H"], s["W"], 3, 0, g.data_ptr(), partials.data_ptr(), maxes.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _lib.current_stream(dev))
    torch.cuda.synchronize()
    untouched = all(bool((t == 7).all()) for t in (g, partials, maxes, ws))
    return rc, untouched


@pytest.mark.parametrize("what", ["W128", "H24", "Cout5", "no_dy_bound", "no_x_bound", "exact"])
def test_outside_its_form_nothing_is_launched_and_the_three_launches_run(what):
    from uaps_amd import conv, lazybn
    dims = dict(W128=(2, 4, 16, 128), H24=(2, 4, 24, 256), Cout5=(2, 5, 16, 256)).get(what, (2, 4, 16, 256))
    s = _inputs(dims[0], dims[1], dims[2], 1, seed=3, W=dims[3])
    try:
        if what == "exact":
            conv.set_mode("exact")
        rc, untouched = _raw_call(s, dzb=what != "no_dy_bound", xb=what != "no_x_bound")
        assert rc == ENOFORM and untouched
        dzb, xb = (None if what == "no_dy_bound" else s["dzb"]), (None if what == "no_x_bound" else s["xb"])
        ws = torch.zeros(_ws_bytes(s), dtype=torch.uint8, device=torch.device(DEV))
        assert conv.head_bwd_fused(s["dz"], dzb, s["y"], s["xf"], xb, s["wb"], s["mean"], s["invstd"], s["gamma"], s["beta"], SLOPE, 1, True, 0, ws) is None
        assert what in ("no_dy_bound", "no_x_bound") or not conv.head_bwd_eligible(s["dz"], s["y"], 3)
    finally:
        conv.set_mode("h16")
    # the node's backward on such a call: the three launches, never the fused kernel
    names = _node_backward_names(dims[0], dims[1], dims[2], dims[3], mode="exact" if what == "exact" else "h16",
                                 bound_g=what != "no_dy_bound", bound_x=what != "no_x_bound")
    assert names and conv.HEAD_BWD_KERNEL not in names, names
    lazybn.reset()


def _node_backward_names(B, Cout, H, W, mode="h16", bound_g=True, bound_x=True):
    """conv -> BatchNorm -> LeakyReLU -> 3x3 to Cout classes inside lazybn.scope(); the kernels its backward timed.  bound_g / bound_x
    False: the incoming gradient / the activation reaches the node without a magnitude bound."""
    import torch.nn as nn
    from uaps_amd import bounds, conv, fused, lazybn
    torch.manual_seed(2)
    x = torch.randn(B, 16, H, W, device=DEV, requires_grad=True)
    w1 = (torch.randn(16, 16, 3, 3, device=DEV) / 10).requires_grad_(True)
    w2 = (torch.randn(Cout, 16, 3, 3, device=DEV) / 10).requires_grad_(True)
    bn = nn.BatchNorm2d(16).to(DEV)
    bounds.refresh([bn])
    try:
        conv.set_mode(mode)
        with lazybn.scope():
            y1, st1 = conv.conv2d_with_stats(bounds.put(x, bounds.from_value(x.detach().abs().max())), w1, None)
            real = bounds.bn_output_bound
            try:
                if not bound_x:
                    bounds.bn_output_bound = lambda *a, **k: None
                z = fused.bn_act_conv(y1, st1, None, bn, SLOPE, w2, None)
            finally:
                bounds.bn_output_bound = real
            g = torch.randn_like(z)
            conv.KERNEL_EVENTS, conv.EVENT_FILTER = {}, None
            z.backward(bounds.put(g, bounds.from_value(g.abs().max())) if bound_g else g)
            names, conv.KERNEL_EVENTS = set(conv.KERNEL_EVENTS), None
    finally:
        conv.KERNEL_EVENTS = None
        conv.set_mode("h16")
    assert w2.grad is not None and bool(torch.isfinite(w2.grad).all()) and bool(torch.isfinite(x.grad).all())
    return names


def test_the_node_takes_the_fused_pass_inside_a_scope():
    from uaps_amd import conv
    names = _node_backward_names(2, 4, 16, 256)
    assert conv.HEAD_BWD_KERNEL in names and not any(n.startswith("conv_hrwrw_bn_kernel") or n.startswith("conv_fwd_kernel<3, 8, 32, 16, 4") for n in names), names


def test_trainer_step_with_the_switch_on_and_off():
    """One training step at 2 + 2 images of 32 x 256 with UAPS_FUSED_HEAD_BWD on and off: the same loss (the forward is untouched) and
    the same state (buffers, Adam moments, parameters) bit for bit;
    nothing pending; the fused kernel once per decoder and none of the three launches it replaces for out_conv."""
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
    prev = conv._FUSED_HEAD
    try:
        for on, m in ((True, m_on), (False, m_off)):
            conv._FUSED_HEAD = on
            tr = uaps_amd.UAPSTrainer(m.to(DEV), base_lr=1e-3, seed=11)
            uaps_amd.perturb.manual_seed(7, 0)
            np.random.seed(7)
            conv.KERNEL_EVENTS, conv.EVENT_FILTER = {}, None
            res[on] = float(tr.train_step(xl, yl, xu)["loss"])
            names[on], conv.KERNEL_EVENTS = {k: len(v) for k, v in conv.KERNEL_EVENTS.items()}, None
            opt[on] = tr.optimizer
            lazybn.assert_none_pending()
    finally:
        conv._FUSED_HEAD, conv.KERNEL_EVENTS = prev, None
    assert res[True] == res[False]
    for (n, ba), bb in zip(m_on.named_buffers(), m_off.buffers()):
        assert torch.equal(ba, bb), n                      # running statistics: the forward is the same
    # g, the slabs and the BatchNorm partial sums are the three launches' bit for bit: so is the whole step
    sa, sb = opt[True].state_dict()["state"], opt[False].state_dict()["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    for k in sa:
        assert torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]), k
    for (n, pa), pb in zip(m_on.named_parameters(), m_off.parameters()):
        assert torch.equal(pa, pb), n
    assert names[True].get(conv.HEAD_BWD_KERNEL) == 4 and conv.HEAD_BWD_KERNEL not in names[False], (names[True], names[False])
    old = ("conv_fwd_kernel<3, 8, 32, 16, 4, 4, 1>", "conv_hrwrw_bn_kernel<1>")
    assert all(names[False].get(k, 0) >= 4 for k in old), names[False]
    # what the switch-off step ran for out_conv is gone: four launches fewer of each (other layers resolve to the same instantiations)
    assert all(names[True].get(k, 0) == names[False][k] - 4 for k in old), (names[True], names[False])

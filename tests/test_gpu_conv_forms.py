"""Every convolution kernel form of the library (tests/conv_form_cases.py: one case per instantiation, each naming its kernel) run
through uaps_conv_ex with real tensors and held against a float64 reference computed on the CPU as plain math: the concatenation,
bilinear x2 up-sampling (align_corners), the staging-time BatchNorm + LeakyReLU, the dyt transform of the weight gradient.

The bar (conv_form_cases.check): pointwise |got - ref| <= tau * sum|a*b| per element -- wrong, missing or doubled terms, borders
and partial tiles included -- with tau = 5e-6 for y and dx and conv_form_cases.TAU_DW for dw; and the precision RMS((got - ref) / R),
R = sqrt(sum (a*b)^2), within conv_form_cases.RMS_FACTOR of torch float32 on one CPU thread: a lost operand piece averages out
pointwise at large K but not there.  Secondary outputs: bias gradient, BatchNorm partials (as per-channel mean and variance, with
and without stats_mean), the BatchNorm-backward sums and maxima of bsum_*, dyt_out, out_amax, both halves of a two-tensor output;
the sticky error word stays 0 on every legitimate bound.  The measured maxima per case: profiles/conv_forms_dw_tau.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_form_cases as F
from conv_form_cases import BWD_DATA, FWD, WRW

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bound(m: float, loose: bool):
    """A bound >= m: m rounded up to fp32, or a loose power of two above it."""
    from uaps_amd import bounds
    if loose:
        v = 2.0 ** (np.floor(np.log2(max(m, 1e-30))) + 2)
    else:
        v = np.float32(m)
        if float(v) < m:
            v = np.nextafter(v, np.float32(np.inf))
    return bounds.from_value(torch.tensor([float(v)], dtype=torch.float32, device=DEV))


def _amax(t) -> float:
    return float(t.double().abs().max()) if t.numel() else 0.0


def _run(case: F.Case, inp: dict):
    """Runs the case on the GPU; returns the outputs as CPU tensors."""
    from uaps_amd import _lib, bounds, conv
    L = _lib.lib()
    B, Cin, Cout, H, W, ks = case.B, case.Cin, case.Cout, case.H, case.W, case.ks
    st = _lib.current_stream(DEV)
    keep, p, out = [], {}, {}

    def dev(t):
        d = t.to(DEV).contiguous()
        keep.append(d)
        return d

    w = dev(inp["w"])
    wf, wb = conv.pack_weights(w)
    keep += [wf, wb]
    p["w"] = (wf if case.op == FWD else wb).data_ptr()
    cfgw = case.cfg_word() & ~F.X2_UP2
    staged = F.staged_input(case, inp) if case.op != BWD_DATA else None
    C1 = case.C1 if case.C1 else Cin
    if case.op in (FWD, WRW):
        x = inp["x"]
        x1 = x[:, :C1].contiguous() if (case.two_in or case.up2) else x
        buf = torch.full((x1.numel() + 8,), float("nan"), device=DEV)
        xd = buf[case.offset:case.offset + x1.numel()].view(x1.shape)
        xd.copy_(x1.to(DEV))
        keep.append(buf)
        p["x"] = xd.data_ptr()
        if case.up2:
            p["x2"] = dev(inp["x2_low"]).data_ptr()
        elif case.two_in:
            p["x2"] = dev(x[:, C1:]).data_ptr()
        if case.xf is not None:
            p["xf"] = dev(inp["xf"]).data_ptr()
    if case.op == FWD:
        bsrc = {0: _amax(staged[:, :C1])}
        if case.two_in or case.up2:
            bsrc[1] = _amax(inp["x2_low"]) if case.up2 else _amax(staged[:, C1:])
        y = dev(torch.full((B, Cout, H, W), float("nan")))
        p["y"] = y.data_ptr()
        out["y"] = y
        if case.want_bias:
            p["bias"] = dev(inp["bias"]).data_ptr()
        if case.stats:
            parts = C.c_int()
            _lib.check(L.uaps_conv_fwd_stats_parts(B, Cin, Cout, H, W, ks, cfgw, C.byref(parts)), "stats_parts")
            stats = dev(torch.full((Cout, B, parts.value, 2), float("nan")))
            p["stats"] = stats.data_ptr()
            out["stats"] = stats
            if case.stats == "mean":
                p["stats_mean"], p["stats_bias"] = dev(inp["stats_mean"]).data_ptr(), dev(inp["stats_bias"]).data_ptr()
        if case.out_amax:
            am = bounds.new_amax(DEV)
            keep.append(am)
            p["out_amax"] = am.data_ptr()
            out["amax"] = am
    elif case.op == BWD_DATA:
        bsrc = {0: _amax(inp["dy"])}
        p["dy"] = dev(inp["dy"]).data_ptr()
        y = dev(torch.full((B, C1, H, W), float("nan")))
        p["y"] = y.data_ptr()
        out["dx1"] = y
        if case.two_out:
            y2 = dev(torch.full((B, Cin - C1, H, W), float("nan")))
            p["y2"] = y2.data_ptr()
            out["dx2"] = y2
        if case.bsum is not None:
            bn = inp["bn"]
            for k in ("y", "mean", "invstd", "gamma", "beta"):
                p["bsum_" + k] = dev(bn[k]).data_ptr()
            part = dev(torch.full((Cin, B, H // 16, 2), float("nan")))
            mx = dev(torch.zeros(2 * bounds.FLOATS))
            with _lib.device_guard(DEV):
                _lib.check(L.uaps_zero_bounds(mx.data_ptr(), mx.numel(), st), "zero_bounds")
            p["bsum_partials"], p["bsum_max"] = part.data_ptr(), mx.data_ptr()
            out["bsum_partials"], out["bsum_max"] = part, mx
    else:
        dyt = F.true_dy(case, inp)
        # (dyt: the bound of the dy the kernel forms in fp32, as uaps_bn_act_bwd_prepare raises it above the float64 maximum)
        bsrc = {0: _amax(dyt) * (1 + 1e-6 if case.dyt is not None else 1), 1: _amax(staged[:, :C1])}
        if case.two_in or case.up2:
            bsrc[2] = _amax(inp["x2_low"]) if case.up2 else _amax(staged[:, C1:])
        p["dy"] = dev(inp["dy"]).data_ptr()
        n = C.c_size_t()
        _lib.check(L.uaps_conv_wrw_workspace_bytes(B, Cin, Cout, H, W, ks, cfgw, C.byref(n)), "ws")
        ws = dev(torch.full((max(n.value, 16) // 4,), float("nan")))
        p["ws"], p["ws_bytes"] = ws.data_ptr(), ws.numel() * 4
        if case.dyt is not None:
            bn = inp["bn"]
            p["dyt_y"], p["dyt_coef"] = dev(bn["y"]).data_ptr(), dev(inp["dyt_coef"]).data_ptr()
            dto = dev(torch.full((B, Cout, H, W), float("nan")))
            p["dyt_out"] = dto.data_ptr()
            out["dyt_out"] = dto
    for i in case.bounded:
        b = _bound(bsrc[i], case.loose)
        keep.append(b)
        p[f"bound{i}"] = b.data_ptr()
    call = F.make_call(_lib, case, p, st)
    err = _lib.error_word(DEV)
    err.zero_()
    buf = C.create_string_buffer(128)
    assert L.uaps_conv_ex_variant(C.byref(call), buf, 128) == 0 and buf.value.decode() == case.kernel, buf.value
    with _lib.device_guard(DEV):
        _lib.check(L.uaps_conv_ex(C.byref(call)), "uaps_conv_ex")
        if case.op == WRW:
            dw = torch.full((Cout, Cin, ks, ks), float("nan"), device=DEV)
            db = torch.full((Cout,), float("nan"), device=DEV) if case.want_bias else None
            _lib.check(L.uaps_conv_bwd_weight_reduce(ws.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None, B, Cin, Cout,
                                                     H, W, ks, cfgw, st), "reduce")
            out["dw"] = dw
            if db is not None:
                out["db"] = db
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res["err"] = int(err.item())
    return res


@pytest.fixture
def restore_mode():
    from uaps_amd import _lib
    L = _lib.lib()
    L.uaps_conv_get_tuning.restype = C.c_uint
    prev = (L.uaps_conv_get_mode(), L.uaps_conv_get_tuning())
    yield
    L.uaps_conv_set_mode(prev[0])
    L.uaps_conv_set_tuning(prev[1])


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_kernel_form_vs_float64(case, restore_mode):
    from uaps_amd import _lib, bounds
    L = _lib.lib()
    assert L.uaps_conv_set_mode(F.MODES[case.mode]) == 0 and L.uaps_conv_set_tuning(case.tune) == 0
    inp = F.make_inputs(case)
    ref = F.reference(case, inp, floors=F.h16_floors(case, inp))
    got = _run(case, inp)
    if case.op == FWD:
        main = got["y"]
    elif case.op == BWD_DATA:
        main = torch.cat([got["dx1"], got["dx2"]], 1) if case.two_out else got["dx1"]
    else:
        main = got["dw"]
    base = F.fp32_cpu_rms(case, inp, ref)
    tau = F.TAU_DW if case.op == WRW else F.TAU_Y
    ok, st = F.check(main, ref, tau, base)
    print(f"\nFORM {case.id} {st}")
    assert ok, (case, st)
    assert got["err"] == 0, f"error word {got['err']} on a legitimate bound"
    if case.op == WRW and case.want_bias:
        dy = F.true_dy(case, inp)
        db_ref, db_mag = dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
        e = float(((got["db"].double() - db_ref).abs() / db_mag.clamp_min(1e-300)).max())
        print(f"FORM {case.id} db {e:.3e}")
        assert e <= F.TAU_DW, e
    if case.op == WRW and case.dyt is not None:
        tdy, tmag = F.true_dy(case, inp), F.true_dy(case, inp, absolute=True)
        e = float(((got["dyt_out"].double() - tdy).abs() / tmag.clamp_min(1e-300)).max())
        assert e <= F.TAU_Y, ("dyt_out", e)
    if case.op == FWD and case.stats:
        y = ref["ref"]
        s = (inp["stats_mean"].double() - inp["stats_bias"].double()) if case.stats == "mean" else torch.zeros(case.Cout, dtype=torch.float64)
        part = got["stats"].double()
        N = case.B * case.H * case.W
        m1 = part[..., 0].sum((1, 2)) / N
        m2 = part[..., 1].sum((1, 2)) / N
        mean_got, var_got = s + m1, m2 - m1 * m1
        mean_ref, var_ref = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        dev2 = ((y - s[None, :, None, None]) ** 2).mean((0, 2, 3))
        devm = ((y - s[None, :, None, None]).abs() + ref["M"]).mean((0, 2, 3))
        e_mean = float(((mean_got - mean_ref).abs() / devm.clamp_min(1e-300)).max())
        e_var = float(((var_got - var_ref).abs() / dev2.clamp_min(1e-300)).max())
        print(f"FORM {case.id} stats mean {e_mean:.3e} var {e_var:.3e}")
        assert e_mean <= 1e-5 and e_var <= 1e-4, (e_mean, e_var)
    if case.op == FWD and case.out_amax:
        am = float(bounds.value(got["amax"]))
        assert am >= float(got["y"].abs().max()) and np.float32(am) == np.float32(got["y"].abs().max()), (am, float(got["y"].abs().max()))
    if case.op == BWD_DATA and case.bsum is not None:
        bn = inp["bn"]
        gi = torch.arange(case.B) // (case.B // case.bsum[1])
        mu, ist = bn["mean"].double()[gi][:, :, None, None], bn["invstd"].double()[gi][:, :, None, None]
        yc = bn["y"].double() - mu
        z = yc * ist * bn["gamma"].double()[None, :, None, None] + bn["beta"].double()[None, :, None, None]
        dx = ref["ref"]
        d = torch.where(z > 0, dx, dx * case.bsum[0])
        xh = yc * ist
        shp = (case.B, case.Cin, case.H // 16, 16, case.W)
        s_ref = d.reshape(shp).sum((3, 4)).permute(1, 0, 2)
        q_ref = (d * xh).reshape(shp).sum((3, 4)).permute(1, 0, 2)
        s_mag = d.abs().reshape(shp).sum((3, 4)).permute(1, 0, 2)
        q_mag = (d * xh).abs().reshape(shp).sum((3, 4)).permute(1, 0, 2)
        part = got["bsum_partials"].double()
        e_s = float(((part[..., 0] - s_ref).abs() / s_mag.clamp_min(1e-300)).max())
        e_q = float(((part[..., 1] - q_ref).abs() / q_mag.clamp_min(1e-300)).max())
        md, mx = float(bounds.value(got["bsum_max"][:bounds.FLOATS])), float(bounds.value(got["bsum_max"][bounds.FLOATS:]))
        print(f"FORM {case.id} bsum {e_s:.3e} {e_q:.3e} max {md} {float(d.abs().max())} {mx} {float(xh.abs().max())}")
        assert e_s <= 2e-5 and e_q <= 2e-5, (e_s, e_q)
        assert abs(md - float(d.abs().max())) <= 1e-5 * float(d.abs().max())
        assert abs(mx - float(xh.abs().max())) <= 1e-5 * float(xh.abs().max())

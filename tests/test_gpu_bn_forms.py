"""-m gpu: every BatchNorm + LeakyReLU + Dropout kernel form of uaps_amd/csrc/norm_act.hip against the float64 reference of
tests/bn_ref.py, through the C ABI (explicit seed and offset, no step state).

Each output is held pointwise against a bound scaled by its own conditioning (bn_ref.TAU, profiles/bn_forms_tau.txt); the dropout
mask must be the host Philox mask exactly, in the forward and the backward; the conv-bias gradient exactly 0; out_amax exactly
max|out|; dy_bound and the parameter-only output bound must bound what they claim; a second launch must give the same bits; and every
refusal must leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL, ERANGE, EWORKSPACE = 0, -1, -2, -3
MOMENTUM = 0.1


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    lib = _lib.lib()
    prev = lib.uaps_get_step_state()
    lib.uaps_set_step_state(None)                # explicit seed and offset: no step-state key added
    yield lib
    lib.uaps_set_step_state(prev)


def _stream():
    from uaps_amd import _lib
    return _lib.current_stream(torch.device(DEV))


def _hints(**kw):
    from uaps_amd import _lib
    return _lib.mk_hints(**kw)


def _view(a, off: int = 0, fill=None):
    """A device tensor holding the host array `a` (or `fill`), `off` floats into its buffer."""
    a = np.asarray(a)
    buf = torch.empty(a.size + off + 4, dtype=torch.from_numpy(a[:0].copy()).dtype, device=DEV)
    v = buf[off:off + a.size].view(a.shape)
    if fill is None:
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    else:
        v.fill_(fill)
    return v


def _new(shape, off=0, fill=float("nan")):
    return _view(np.zeros(shape, np.float32), off, fill)


def _bound(L):
    b = torch.empty(R.BOUND_FLOATS, dtype=torch.float32, device=DEV)
    assert L.uaps_zero_bounds(b.data_ptr(), b.numel(), _stream()) == OK
    return b


def _bval(b) -> float:
    return float(b[::R.BOUND_STRIDE][:R.BOUND_SLOTS].max())


def _ws(L, case):
    n = C.c_size_t()
    assert L.uaps_bn_workspace_bytes(case.B, case.C, case.H, case.W, C.byref(n)) == OK
    return torch.empty(n.value, dtype=torch.uint8, device=DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _np(t):
    return t.detach().cpu().numpy()


# ---- forward --------------------------------------------------------------------------------------------------------------------
def _run_fwd(L, case, inp):
    """One forward launch on fresh buffers: the outputs as host arrays (+ the return code)."""
    B, Cc, H, W, G = case.B, case.C, case.H, case.W, case.groups
    y = _view(inp["y"], case.off)
    gamma, beta = _view(inp["gamma"]), _view(inp["beta"])
    bias = _view(inp["conv_bias"]) if inp["conv_bias"] is not None else None
    rm = _view(inp["rm"]) if case.running else None
    rv = _view(inp["rv"]) if case.running else None
    nbt = _view(np.array([inp["nbt"]], np.int64)) if case.running else None
    sm, si = _new((G, Cc)), _new((G, Cc))
    amax = _bound(L) if case.amax else None
    d = {}
    if case.entry == R.FINALIZE:
        parts = _view(R.host_partials(inp["y"], B, Cc, case.ppi, R.shift_of(case, inp)))
        xf = _new((G, Cc, 2))
        stats_mean = rm if rm is not None else _view(inp["rm"])
        h = _hints(stats=(stats_mean, bias)) if case.shift else None
        rc = L.uaps_bn_finalize_train_h(h, parts.data_ptr(), case.ppi, _p(bias), gamma.data_ptr(), beta.data_ptr(), _p(rm), _p(rv),
                                        _p(nbt), MOMENTUM, R.EPS, B, Cc, H, W, G, sm.data_ptr(), si.data_ptr(), xf.data_ptr(), _stream())
        d["xf"] = xf
    else:
        out = _new((B, Cc, H, W), case.off)
        res = _view(inp["res"], case.off) if case.residual else None
        ws = _ws(L, case)
        args = (y.data_ptr(), _p(bias), gamma.data_ptr(), beta.data_ptr(), _p(rm), _p(rv), _p(nbt), MOMENTUM, R.EPS, case.slope, case.p,
                case.seed, case.offset, B, Cc, H, W, G, out.data_ptr(), sm.data_ptr(), si.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        if case.entry == R.FWD:
            if amax is not None or res is not None:
                assert L.uaps_next_call_hints(_hints(out_amax=amax, residual=res)) == OK
            rc = L.uaps_bn_act_fwd_train_grouped(*args)
        else:
            parts = _view(R.host_partials(inp["y"], B, Cc, case.ppi, R.shift_of(case, inp)))
            stats_mean = rm if rm is not None else _view(inp["rm"])
            h = _hints(out_amax=amax, residual=res, stats=(stats_mean, bias) if case.shift else None)
            rc = L.uaps_bn_act_fwd_train_partials_h(h, parts.data_ptr(), case.ppi, *args)
        d["out"] = out
    torch.cuda.synchronize()
    got = {k: _np(v) for k, v in d.items()}
    got.update(mean=_np(sm), invstd=_np(si))
    if case.running:
        got.update(rm=_np(rm), rv=_np(rv), nbt=int(nbt[0]))
    if amax is not None:
        got["amax"] = _bval(amax)
    return rc, got


def _check_fwd(L, case):
    inp = R.inputs(case)
    ref = R.forward(inp["y"], inp["gamma"], inp["beta"], groups=case.groups, slope=case.slope, p=case.p, mask=inp["mask"],
                    conv_bias=inp["conv_bias"], rm=inp["rm"] if case.running else None, rv=inp["rv"] if case.running else None,
                    nbt=inp["nbt"] if case.running else None, momentum=MOMENTUM, res=inp.get("res"))
    rc, got = _run_fwd(L, case, inp)
    assert rc == OK, rc
    bad = []
    ratios = R.fwd_ratios(case, inp, ref, got)
    if case.running and got["nbt"] != ref["nbt"]:
        bad.append(f"num_batches_tracked {got['nbt']} != {ref['nbt']}")
    if "out" in got:
        out = got["out"]
        if case.p > 0 and not np.array_equal(out.reshape(-1) != 0, inp["mask"]):
            bad.append(f"forward dropout mask: {int(((out.reshape(-1) != 0) != inp['mask']).sum())} elements differ from host Philox")
        if case.amax and got["amax"] != float(np.abs(out).max()):
            bad.append(f"out_amax {got['amax']} != max|out| {float(np.abs(out).max())}")
        if not case.residual:
            # the parameter-only bound (uaps_bn_param_bounds x sqrt(n) x 1 / (1 - p), bounds.bn_output_bound)
            gb, bb = _view(inp["gamma"]), _view(inp["beta"])
            pb = _bound(L)
            rc2 = L.uaps_bn_param_bounds((C.c_void_p * 1)(gb.data_ptr()), (C.c_void_p * 1)(bb.data_ptr()), (C.c_int * 1)(case.C), 1,
                                         pb.data_ptr(), _stream())
            assert rc2 == OK
            torch.cuda.synchronize()
            if _bval(pb) != float(R.param_bound(inp["gamma"], inp["beta"])):
                bad.append(f"uaps_bn_param_bounds {_bval(pb)} != {float(R.param_bound(inp['gamma'], inp['beta']))}")
            if float(np.abs(out).max()) > _bval(pb) * R.output_bound_factor(case):
                bad.append(f"max|out| {float(np.abs(out).max())} above the parameter bound {_bval(pb) * R.output_bound_factor(case)}")
    rc2, again = _run_fwd(L, case, inp)
    for k, v in got.items():
        if not np.array_equal(np.asarray(v).view(np.uint8) if isinstance(v, np.ndarray) else v,
                              np.asarray(again[k]).view(np.uint8) if isinstance(v, np.ndarray) else again[k]):
            bad.append(f"second launch differs in {k}")
    return ratios, bad


# ---- backward -------------------------------------------------------------------------------------------------------------------
def _run_bwd(L, case, inp):
    B, Cc, H, W, G = case.B, case.C, case.H, case.W, case.groups
    y, dout = _view(inp["y"], case.off), _view(inp["dout"], case.off)
    gamma, beta = _view(inp["gamma"]), _view(inp["beta"])
    sm, si = _view(inp["save_mean"]), _view(inp["save_invstd"])
    dy = _new((B, Cc, H, W), case.off)
    dg, db, dcb = _new((Cc,)), _new((Cc,)), (_new((Cc,)) if case.bias else None)
    amax = _bound(L) if case.amax else None
    got = {}
    if case.entry == R.BWD:
        ws = _ws(L, case)
        tail = (dout.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(), si.data_ptr(), case.slope, case.p,
                case.seed, case.offset, B, Cc, H, W, G, dy.data_ptr(), dg.data_ptr(), db.data_ptr())
        wsa = (ws.data_ptr(), ws.numel(), _stream())
        if case.bias:
            rc = L.uaps_bn_act_bwd_grouped_bias_h(_hints(out_amax=amax), *tail, dcb.data_ptr(), *wsa)
        else:
            rc = L.uaps_bn_act_bwd_grouped_h(_hints(out_amax=amax), *tail, *wsa)
    else:
        coef = _new((G, Cc, 8))
        dyb = _bound(L)
        if case.entry == R.HALVES:
            ws = _ws(L, case)
            rc = L.uaps_bn_act_bwd_prepare(dout.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(), si.data_ptr(),
                                           case.slope, B, Cc, H, W, G, coef.data_ptr(), dg.data_ptr(), db.data_ptr(), _p(dcb),
                                           dyb.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        else:
            parts = _view(R.host_partials(inp["y"], B, Cc, case.ppi, dout=inp["dout"], mean=inp["save_mean"], invstd=inp["save_invstd"],
                                          gamma=inp["gamma"], beta=inp["beta"], slope=case.slope, G=G))
            ref = R.backward(inp["dout"], inp["y"], inp["gamma"], inp["beta"], inp["save_mean"], inp["save_invstd"], groups=G,
                             slope=case.slope)
            maxes = torch.zeros(2 * R.BOUND_FLOATS, dtype=torch.float32, device=DEV)
            maxes[0] = float(np.float32(np.abs(ref["d"]).max()))
            maxes[R.BOUND_FLOATS] = float(np.float32(np.abs(ref["xhat"]).max()))
            rc = L.uaps_bn_act_bwd_finalize(parts.data_ptr(), case.ppi, maxes.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(),
                                            si.data_ptr(), B, Cc, H, W, G, coef.data_ptr(), dg.data_ptr(), db.data_ptr(), _p(dcb),
                                            dyb.data_ptr(), _stream())
        if rc == OK:
            rc = L.uaps_bn_act_bwd_apply_h(_hints(out_amax=amax), dout.data_ptr(), y.data_ptr(), coef.data_ptr(), case.slope, B, Cc, H, W,
                                           G, dy.data_ptr(), _stream())
        torch.cuda.synchronize()
        got.update(coef=_np(coef), dy_bound=_bval(dyb))
    torch.cuda.synchronize()
    got.update(dy=_np(dy), dgamma=_np(dg), dbeta=_np(db))
    if dcb is not None:
        got["dcb"] = _np(dcb)
    if amax is not None:
        got["amax"] = _bval(amax)
    return rc, got


def _check_bwd(L, case):
    inp = R.inputs(case)
    ref = R.backward(inp["dout"], inp["y"], inp["gamma"], inp["beta"], inp["save_mean"], inp["save_invstd"], groups=case.groups,
                     slope=case.slope, p=case.p, mask=inp["mask"])
    rc, got = _run_bwd(L, case, inp)
    assert rc == OK, rc
    bad = []
    ratios = R.bwd_ratios(case, ref, got)
    dy = got["dy"]
    if case.bias and np.any(got["dcb"] != 0):
        bad.append("the conv-bias gradient is not exactly 0")
    if case.amax and got["amax"] != float(np.abs(dy).max()):
        bad.append(f"out_amax {got['amax']} != max|dy| {float(np.abs(dy).max())}")
    if case.p > 0:                         # the mask the backward applied: d recovered from dy, against the host Philox mask
        G = case.groups
        d_rec = R._grouped(dy.astype(np.float64), G) / ref["sc"][..., None] + ref["k2"][..., None] + ref["xhat"] * ref["k3"][..., None]
        scale = 1.0 / (1.0 - float(np.float32(case.p)))
        thr = 0.5 * scale * min(1.0, case.slope) * np.abs(R._grouped(inp["dout"].astype(np.float64), G))
        kept = R._ungrouped(np.abs(d_rec) > thr, dy.shape).reshape(-1)
        if not np.array_equal(kept, inp["mask"]):
            bad.append(f"backward dropout mask: {int((kept != inp['mask']).sum())} elements differ from host Philox")
    if "coef" in got:
        q, qr = got["coef"], R.two_halves_coef(ref, inp["save_mean"], inp["save_invstd"], inp["gamma"], inp["beta"])
        if not np.array_equal(q[..., [0, 1, 2, 3, 6, 7]], qr[..., [0, 1, 2, 3, 6, 7]].astype(np.float32)):
            bad.append("coef columns (mean, invstd, gamma invstd, beta, 0, 0) are not exact")
        bnd = R.dy_bound(ref)
        if not (float(np.abs(dy).max()) <= got["dy_bound"] and abs(got["dy_bound"] - bnd) <= 1e-5 * bnd):
            bad.append(f"dy_bound {got['dy_bound']}: max|dy| {float(np.abs(dy).max())}, formula {bnd}")
    rc2, again = _run_bwd(L, case, inp)
    for k, v in got.items():
        if not np.array_equal(np.asarray(v).view(np.uint8) if isinstance(v, np.ndarray) else v,
                              np.asarray(again[k]).view(np.uint8) if isinstance(v, np.ndarray) else again[k]):
            bad.append(f"second launch differs in {k}")
    return ratios, bad


# ---- eval -------------------------------------------------------------------------------------------------------------------------
def _check_eval(L, case):
    inp = R.inputs(case)
    B, Cc, H, W = case.B, case.C, case.H, case.W
    ref = R.eval_forward(inp["y"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], slope=case.slope, conv_bias=inp["conv_bias"])
    assert float(np.abs(ref["z"]).min()) >= R.DELTA / 4
    y, dout = _view(inp["y"], case.off), _view(inp["dout"], case.off)
    gamma, beta, rm, rv = (_view(inp[k]) for k in ("gamma", "beta", "rm", "rv"))
    bias = _view(inp["conv_bias"]) if inp["conv_bias"] is not None else None
    out, dy, me = _new((B, Cc, H, W), case.off), _new((B, Cc, H, W), case.off), _new((Cc,))
    ws = _ws(L, case)
    rc = L.uaps_bn_act_fwd_eval(y.data_ptr(), _p(bias), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), R.EPS, case.slope,
                                B, Cc, H, W, out.data_ptr(), me.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    assert rc == OK
    rc = L.uaps_bn_act_bwd_eval(dout.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), me.data_ptr(), rv.data_ptr(), R.EPS,
                                case.slope, B, Cc, H, W, dy.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    assert rc == OK
    torch.cuda.synchronize()
    sc4, me4 = ref["sc"][None, :, None, None], ref["mean_eff"][None, :, None, None]
    cond = np.abs(sc4) * (np.abs(inp["y"] - me4) + np.abs(me4)) + np.abs(inp["beta"].astype(np.float64))[None, :, None, None]
    dyr = R.eval_backward(inp["dout"], ref["z"], ref["sc"], case.slope)
    ratios = dict(out=R.ratio(_np(out), ref["out"], cond), dy=R.ratio(_np(dy), dyr, np.abs(sc4 * inp["dout"])))
    bad = [] if np.array_equal(_np(me), (inp["rm"] - (inp["conv_bias"] if inp["conv_bias"] is not None else 0)).astype(np.float32)) \
        else ["eval mean (running_mean - conv bias) is not the fp32 difference"]
    return ratios, bad


def run_case(L, case):
    """(the ratio of every compared quantity to its bar's scale, the failed exact checks)."""
    if case.entry in (R.FWD, R.FWD_PARTIALS, R.FINALIZE):
        return _check_fwd(L, case)
    if case.entry == R.EVAL:
        return _check_eval(L, case)
    return _check_bwd(L, case)


@pytest.mark.parametrize("cid", [c.id for c in R.CASES])
def test_bn_form_against_float64(L, cid):
    case = R.BY_ID[cid]
    ratios, bad = run_case(L, case)
    assert not bad, bad
    over = {k: (v, R.TAU[k]) for k, v in ratios.items() if not v <= R.TAU[k]}
    assert not over, over


# ---- refusals: nothing launched, nothing written -----------------------------------------------------------------------------------
SENTINEL = -12345.0


def _refuse_fwd(L, B=4, Cc=3, H=4, W=4, groups=2, p=0.0, ws_short=False, residual=False):
    case = R.Case("refusal", R.FWD, B, Cc, H, W, 1)
    y = torch.randn(B, Cc, H, W, device=DEV)
    out = torch.full_like(y, SENTINEL)
    gamma, beta = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    rm, rv = torch.full((Cc,), SENTINEL, device=DEV), torch.full((Cc,), SENTINEL, device=DEV)
    nbt = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    G = max(1, groups)
    sm, si = torch.full((8 * Cc,), SENTINEL, device=DEV), torch.full((8 * Cc,), SENTINEL, device=DEV)
    ws = _ws(L, case)
    res = torch.randn_like(y) if residual else None
    if residual:
        assert L.uaps_next_call_hints(_hints(residual=res)) == OK
    rc = L.uaps_bn_act_fwd_train_grouped(y.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(),
                                         0.1, 1e-5, 0.01, p, 1, 0, B, Cc, H, W, groups, out.data_ptr(), sm.data_ptr(), si.data_ptr(),
                                         ws.data_ptr(), ws.numel() - (1 if ws_short else 0), _stream())
    torch.cuda.synchronize()
    untouched = all(bool((t == SENTINEL).all()) for t in (out, rm, rv, sm, si)) and int(nbt[0]) == 5
    return rc, untouched


def _refuse_bwd(L, B=4, Cc=3, H=4, W=4, groups=2, p=0.0, ws_short=False):
    case = R.Case("refusal", R.BWD, B, Cc, H, W, 1)
    y, dout = torch.randn(B, Cc, H, W, device=DEV), torch.randn(B, Cc, H, W, device=DEV)
    dy = torch.full_like(y, SENTINEL)
    gamma, beta = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    sm, si = torch.zeros(8 * Cc, device=DEV), torch.ones(8 * Cc, device=DEV)
    dg, db, dcb = (torch.full((Cc,), SENTINEL, device=DEV) for _ in range(3))
    ws = _ws(L, case)
    rc = L.uaps_bn_act_bwd_grouped_bias(dout.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(), si.data_ptr(), 0.01,
                                        p, 1, 0, B, Cc, H, W, groups, dy.data_ptr(), dg.data_ptr(), db.data_ptr(), dcb.data_ptr(),
                                        ws.data_ptr(), ws.numel() - (1 if ws_short else 0), _stream())
    torch.cuda.synchronize()
    return rc, all(bool((t == SENTINEL).all()) for t in (dy, dg, db, dcb))


def _refuse_halves(L, B=4, Cc=3, H=4, W=4, groups=2):
    case = R.Case("refusal", R.HALVES, B, Cc, H, W, 1)
    y, dout = torch.randn(B, Cc, H, W, device=DEV), torch.randn(B, Cc, H, W, device=DEV)
    gamma, beta = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    sm, si = torch.zeros(8 * Cc, device=DEV), torch.ones(8 * Cc, device=DEV)
    coef = torch.full((8 * Cc * 8,), SENTINEL, device=DEV)
    dg, db, dcb = (torch.full((Cc,), SENTINEL, device=DEV) for _ in range(3))
    dyb = _bound(L)
    dy = torch.full_like(y, SENTINEL)
    ws = _ws(L, case)
    rc1 = L.uaps_bn_act_bwd_prepare(dout.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(), si.data_ptr(), 0.01,
                                    B, Cc, H, W, groups, coef.data_ptr(), dg.data_ptr(), db.data_ptr(), dcb.data_ptr(), dyb.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream())
    rc2 = L.uaps_bn_act_bwd_apply(dout.data_ptr(), y.data_ptr(), coef.data_ptr(), 0.01, B, Cc, H, W, groups, dy.data_ptr(), _stream())
    torch.cuda.synchronize()
    return (rc1, rc2), all(bool((t == SENTINEL).all()) for t in (coef, dg, db, dcb, dy)) and _bval(dyb) == 0.0


@pytest.mark.parametrize("kw,want", [
    (dict(groups=0), EINVAL), (dict(groups=9, B=9), EINVAL), (dict(groups=3), EINVAL),
    (dict(B=256, Cc=256, H=1, W=1, groups=1), ERANGE), (dict(ws_short=True), EWORKSPACE),
    (dict(p=1.0), EINVAL), (dict(p=0.1, residual=True), EINVAL)])
def test_bn_forward_refusals_write_nothing(L, kw, want):
    rc, untouched = _refuse_fwd(L, **kw)
    assert rc == want, rc
    assert untouched, "a refused forward wrote an output"


@pytest.mark.parametrize("kw,want", [
    (dict(groups=0), EINVAL), (dict(groups=9, B=9), EINVAL), (dict(groups=3), EINVAL),
    (dict(B=256, Cc=256, H=1, W=1, groups=1), ERANGE), (dict(ws_short=True), EWORKSPACE), (dict(p=1.0), EINVAL)])
def test_bn_backward_refusals_write_nothing(L, kw, want):
    rc, untouched = _refuse_bwd(L, **kw)
    assert rc == want, rc
    assert untouched, "a refused backward wrote an output"


@pytest.mark.parametrize("kw,want", [(dict(groups=0), EINVAL), (dict(groups=9, B=9), EINVAL), (dict(groups=3), EINVAL),
                                     (dict(B=256, Cc=256, H=1, W=1, groups=1), ERANGE)])
def test_bn_two_halves_refusals_write_nothing(L, kw, want):
    (rc1, rc2), untouched = _refuse_halves(L, **kw)
    assert (rc1, rc2) == (want, want), (rc1, rc2)
    assert untouched, "a refused two-halves backward wrote an output"

"""-m gpu: every loss-block kernel form (uaps_amd/csrc/loss_kernels.hpp: the pair kernels of the product path and the two-branch
kernels, all 56 (D, C), vector and scalar, with and without out_amax) against the float64 reference of tests/loss_ref.py, through the
C ABI.

Each quantity is held against a bound scaled by its own conditioning (loss_ref.TAU, profiles/loss_forms_tau.txt).  Exact: the
pseudo-labels wherever the float64 margin is clear, the class counts, out_amax = max|d logits| bit for bit, gradients with and
without out_amax bit-identical, every output fully overwritten with its guard floats intact, a second launch bit-identical, and
refusals that write nothing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL, ERANGE, EWORKSPACE = 0, -1, -2, -3
GUARD = 8
SENT_F, SENT_I = 777.25, -777


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    lib = _lib.lib()
    prev = lib.uaps_get_step_state()
    lib.uaps_set_step_state(None)                # by-value weights and cw unless a case sets a state of its own
    yield lib
    lib.uaps_set_step_state(prev)


@pytest.fixture(scope="module")
def state_buf():
    return torch.zeros(16, dtype=torch.float32, device=DEV)          # the 64-byte step state (csrc/philox.hpp)


def _stream():
    from uaps_amd import _lib
    return _lib.current_stream(torch.device(DEV))


class Buf:
    """A device tensor `off` elements into a buffer of its own, with GUARD sentinel elements in front of and behind it."""

    def __init__(self, a, off=0, fill=None):
        a = np.asarray(a)
        self.dtype = torch.from_numpy(a[:0].copy()).dtype
        self.sent = SENT_I if self.dtype == torch.int64 else SENT_F
        self.lo, self.n = GUARD + off, a.size
        self.buf = torch.full((self.lo + a.size + GUARD,), self.sent, dtype=self.dtype, device=DEV)
        self.v = self.buf[self.lo:self.lo + a.size].view(a.shape)
        if fill is None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        else:
            self.v.fill_(fill)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def guards_ok(self) -> bool:
        return bool((self.buf[:self.lo] == self.sent).all()) and bool((self.buf[self.lo + self.n:] == self.sent).all())

    def np(self):
        return self.v.detach().cpu().numpy()


def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])


def _bound(L):
    b = torch.empty(R.BOUND_FLOATS, dtype=torch.float32, device=DEV)
    assert L.uaps_zero_bounds(b.data_ptr(), b.numel(), _stream()) == OK
    return b


def _bval(b) -> float:
    return float(b[::R.BOUND_STRIDE][:R.BOUND_SLOTS].max())


def _out(shape, off=0, dtype=np.float32, fill=float("nan")):
    return Buf(np.zeros(shape, dtype), off, fill)


def _collect(case, outs: dict, amax):
    """Synchronise; the outputs as host arrays + the buffers whose guard elements were overwritten."""
    torch.cuda.synchronize()
    spilled = []
    got = {}
    for k, b in outs.items():
        bs = b if isinstance(b, list) else [b]
        spilled += [k for x in bs if x is not None and not x.guards_ok()]
        got[k] = None if b is None else (np.stack([x.np() for x in b]) if isinstance(b, list) else b.np())
    if amax is not None:
        got["amax"] = _bval(amax)
    return got, spilled


def run_pair(L, case, inp, state_buf=None, bound=None, gscale="case"):
    """uaps_pairloss_fwd (+ uaps_pairloss_finalize_sums for SUMS) + uaps_pairloss_bwd_h on fresh, guarded, NaN-filled buffers."""
    from uaps_amd import _lib
    D, B, Cc, H, W, N = case.D, case.B, case.C, case.H, case.W, case.N
    lab = [Buf(a, case.off if k == 0 else 0) for k, a in enumerate(inp["lab"])]
    un = [Buf(a, case.off if k == 0 else 0) for k, a in enumerate(inp["un"])]
    labels = Buf(inp["labels"], case.lab_off)
    pseudo = _out((B, H, W), case.lab_off, np.int64, -1)
    var = _out((D, B, H, W)) if case.want_var else None
    sscal, uscal = _out((R.s_layout(D, Cc)["n"],)), _out((R.u_layout(D, Cc)["n"],))
    dlab = [_out((B, Cc, H, W), case.off if k == 0 else 0) for k in range(D)]
    dun = [_out((B, Cc, H, W), case.off if k == 0 else 0) for k in range(D)]
    nb = C.c_size_t()
    assert L.uaps_pairloss_workspace_bytes(D, Cc, C.byref(nb)) == OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    cw1, cw2 = inp["cw1"], inp["cw2"]
    w = (C.c_double * D)(*[float(x) for x in inp["w"]])
    if case.state:
        st = np.zeros(16, np.float32)
        st[2:2 + D], st[10], st[11] = inp["w"].astype(np.float32), cw1, cw2
        state_buf.copy_(torch.from_numpy(st))
        assert L.uaps_set_step_state(state_buf.data_ptr()) == OK
        w, cw1, cw2 = None, math.nan, math.nan
    outs = dict(pseudo=pseudo, var=var, sscal=sscal, uscal=uscal, dlab=dlab, dun=dun)
    try:
        sums = _out((sum(R.n_sums(D, Cc)),), 0, np.float64) if case.entry == R.SUMS else None
        rc = L.uaps_pairloss_fwd(_ptrs(lab), _ptrs(un), labels.ptr, w, D, B, Cc, H, W, cw1, cw2, R.EPS, pseudo.ptr, None if var is None else var.ptr,
                                 sscal.ptr, uscal.ptr, None if sums is None else sums.ptr, ws.data_ptr(), ws.numel(), case.cfg, _stream())
        assert rc == OK, rc
        nloss = 0
        if sums is not None:
            outs["sums"] = sums
            nloss = N * case.nloss_mult
            total = (sums.v * case.nloss_mult).contiguous()            # as many equal ranks: what the all-reduce would leave
            rc = L.uaps_pairloss_finalize_sums(total.data_ptr(), D, Cc, nloss, cw1, cw2, R.EPS, sscal.ptr, uscal.ptr, _stream())
            assert rc == OK, rc
        gs = case.gscale if gscale == "case" else gscale
        gst = None if gs is None else torch.full((1,), float(gs), dtype=torch.float32, device=DEV)
        amax = (bound if bound is not None else _bound(L)) if case.track else None
        rc = L.uaps_pairloss_bwd_h(_lib.mk_hints(out_amax=amax) if amax is not None else None, _ptrs(lab), _ptrs(un), labels.ptr, pseudo.ptr,
                                   sscal.ptr, uscal.ptr, cw1, cw2, None if gst is None else gst.data_ptr(), D, B, Cc, H, W, nloss,
                                   _ptrs(dlab), _ptrs(dun), case.cfg, _stream())
        assert rc == OK, rc
        got, spilled = _collect(case, outs, amax)
    finally:
        if case.state:
            L.uaps_set_step_state(None)
    ins = dict(lab=lab, un=un, labels=labels)
    spilled += [k for k, b in ins.items() for x in (b if isinstance(b, list) else [b]) if not x.guards_ok()]
    return got, spilled


def run_two(L, case, inp):
    """uaps_unsup_fwd / _bwd and uaps_sup_fwd / _bwd."""
    D, B, Cc, H, W = case.D, case.B, case.C, case.H, case.W
    lab = [Buf(a, case.off if k == 0 else 0) for k, a in enumerate(inp["lab"])]
    un = [Buf(a, case.off if k == 0 else 0) for k, a in enumerate(inp["un"])]
    labels = Buf(inp["labels"], case.lab_off)
    pseudo = _out((B, H, W), case.lab_off, np.int64, -1)
    var = _out((D, B, H, W)) if case.want_var else None
    sscal, uscal = _out((R.s_layout(D, Cc)["n"],)), _out((R.u_layout(D, Cc)["n"],))
    dlab = [_out((B, Cc, H, W), case.off if k == 0 else 0) for k in range(D)]
    dun = [_out((B, Cc, H, W), case.off if k == 0 else 0) for k in range(D)]
    nb = C.c_size_t()
    assert L.uaps_loss_workspace_bytes(D, B, Cc, H, W, C.byref(nb)) == OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    w = (C.c_double * D)(*[float(x) for x in inp["w"]])
    gst = None if case.gscale is None else torch.full((1,), float(case.gscale), dtype=torch.float32, device=DEV)
    gp = None if gst is None else gst.data_ptr()
    coef = 0.5 / D
    assert L.uaps_unsup_fwd(_ptrs(un), w, D, B, Cc, H, W, inp["cw1"], inp["cw2"], R.EPS, pseudo.ptr, None if var is None else var.ptr, uscal.ptr,
                            ws.data_ptr(), ws.numel(), _stream()) == OK
    assert L.uaps_unsup_bwd(_ptrs(un), pseudo.ptr, uscal.ptr, inp["cw1"], inp["cw2"], gp, D, B, Cc, H, W, _ptrs(dun), _stream()) == OK
    assert L.uaps_sup_fwd(_ptrs(lab), labels.ptr, D, B, Cc, H, W, coef, coef, R.EPS, sscal.ptr, ws.data_ptr(), ws.numel(), _stream()) == OK
    assert L.uaps_sup_bwd(_ptrs(lab), labels.ptr, sscal.ptr, coef, coef, gp, D, B, Cc, H, W, _ptrs(dlab), _stream()) == OK
    return _collect(case, dict(pseudo=pseudo, var=var, sscal=sscal, uscal=uscal, dlab=dlab, dun=dun), None)


def run(L, case, inp, state_buf=None, **kw):
    return run_two(L, case, inp) if case.entry == R.TWO_BRANCH else run_pair(L, case, inp, state_buf, **kw)


def _bits(a):
    return None if a is None else (a if not isinstance(a, np.ndarray) else np.ascontiguousarray(a).view(np.uint8))


def differing(a: dict, b: dict, keys=None):
    return [k for k in (keys or a.keys()) if not np.array_equal(_bits(a[k]), _bits(b[k]))]


_refs = {}          # the reference of a case's data and pseudo-labels, computed once (cases that share their data share it)


def _reference(case, inp, pseudo):
    from dataclasses import replace
    if not (0 <= pseudo.min() and pseudo.max() < case.C):               # not overwritten: compare() reports it
        return R.full_reference(case, inp)
    key = (replace(case, id=case.seed_id or case.id, track=False, cfg=0, state=False, want_var=True, gscale=1.0 if case.gscale is None else case.gscale),
           pseudo.tobytes())
    if key not in _refs:
        _refs.clear()
        _refs[key] = R.full_reference(case, inp, pseudo)
    return _refs[key]


def check(L, case, state_buf=None, fails=None, **kw):
    """One case against its reference: prints the ratios, appends what failed to `fails`, returns the outputs."""
    inp = R.inputs(case)
    got, spilled = run(L, case, inp, state_buf, **kw)
    ref = _reference(case, inp, got["pseudo"])
    ratios, bad = R.compare(case, inp, ref, got)
    print("LOSSFORM", f"{case.id:32s}", f"{case.form_sup}/{case.form:7s}", " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())))
    bad += [f"guard elements of {k} overwritten" for k in spilled]
    bad += [f"{k}: {v[0]:.3e} > {v[1]:.1e}" for k, v in R.over_bars(ratios).items()]
    if bad and fails is not None:
        fails.append((case.id, bad))
    return got


# ---- the table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dc", R.ALL_DC, ids=lambda dc: f"{dc[0]}x{dc[1]}")
def test_pair_kernels_against_float64(L, dc):
    """Vector and scalar form, with and without out_amax.  The two runs of a shape share their data: the forward outputs must agree
    bit for bit (a second launch) and so must the gradients (tracking changes no gradient)."""
    fails = []
    for tr, pl in zip(R.PAIR_GROUPS[dc][0::2], R.PAIR_GROUPS[dc][1::2]):
        a, b = check(L, tr, fails=fails), check(L, pl, fails=fails)
        d = differing(a, b, ("pseudo", "var", "sscal", "uscal", "dlab", "dun"))
        if d:
            fails.append((pl.id, f"differs from the out_amax run of the same data in {d}"))
    assert not fails, fails


@pytest.mark.parametrize("dc", R.ALL_DC, ids=lambda dc: f"{dc[0]}x{dc[1]}")
def test_two_branch_kernels_against_float64(L, dc):
    fails = []
    for case in R.TWO_GROUPS[dc]:
        a = check(L, case, fails=fails)
        b, _ = run(L, case, R.inputs(case))
        if differing(a, b):
            fails.append((case.id, f"a second launch differs in {differing(a, b)}"))
    assert not fails, fails


@pytest.mark.parametrize("dc", R.EXTRA_DC, ids=lambda dc: f"{dc[0]}x{dc[1]}")
def test_pair_extras_against_float64(L, state_buf, dc):
    fails = []
    got = {c.id.split("-", 2)[2]: (c, check(L, c, state_buf, fails=fails)) for c in R.EXTRA_GROUPS[dc]}
    base_case, base = got["base"]
    again, _ = run(L, base_case, R.inputs(base_case))
    if differing(base, again):
        fails.append(("base", f"a second launch differs in {differing(base, again)}"))
    for name in ("cfg1x1", "cfg2x3"):                  # another partition of the grid-stride loops: per-pixel outputs keep their bits
        if differing(base, got[name][1], ("pseudo", "var")):
            fails.append((name, "pseudo / var differ from the cfg = 0 run"))
    for name in ("gscale-null", "state"):
        if differing(base, got[name][1]):
            fails.append((name, f"differs from the by-value, gscale = 1 run in {differing(base, got[name][1])}"))
    # a bound above max|d logits| stays: raise it with gscale = 4, then run gscale = 1 into the same bound
    bound = _bound(L)
    hi, _ = run(L, base_case, R.inputs(base_case), bound=bound, gscale=4.0)
    lo, _ = run(L, base_case, R.inputs(base_case), bound=bound)
    if not (hi["amax"] > base["amax"] and lo["amax"] == hi["amax"] and not differing(lo, base, ("dlab", "dun"))):
        fails.append(("raise", f"bound {hi['amax']} became {lo['amax']} after a run whose maximum is {base['amax']}"))
    assert not fails, fails


# ---- refusals: nothing launched, nothing written ------------------------------------------------------------------------------------
def _refuse(L, D=2, B=2, Cc=3, H=4, W=4, null_head=False, ws_short=False, no_w=False):
    Dp, Bp, Cp = min(max(D, 1), 8), max(B, 1), min(max(Cc, 2), 8)          # buffers of a legal size behind the illegal arguments
    z = [torch.randn(Bp, Cp, H, W, device=DEV) for _ in range(9)]
    y = torch.zeros(Bp, H, W, dtype=torch.int64, device=DEV)
    pseudo = torch.full((Bp, H, W), SENT_I, dtype=torch.int64, device=DEV)
    var = torch.full((Dp, Bp, H, W), SENT_F, device=DEV)
    sscal, uscal = torch.full((R.s_layout(8, 8)["n"],), SENT_F, device=DEV), torch.full((R.u_layout(8, 8)["n"],), SENT_F, device=DEV)
    dz = [torch.full((Bp, Cp, H, W), SENT_F, device=DEV) for _ in range(18)]
    nb = C.c_size_t()
    assert L.uaps_pairloss_workspace_bytes(Dp, Cp, C.byref(nb)) == OK
    ws = torch.full((nb.value,), 7, dtype=torch.uint8, device=DEV)
    heads = (C.c_void_p * 9)(*[t.data_ptr() for t in z])
    holed = (C.c_void_p * 9)(*[None if (null_head and k == 1) else t.data_ptr() for k, t in enumerate(z)])
    w = None if no_w else (C.c_double * 9)(*([1.0 / 9] * 9))
    rc_f = L.uaps_pairloss_fwd(heads, holed, y.data_ptr(), w, D, B, Cc, H, W, 0.1, 0.1, R.EPS, pseudo.data_ptr(), var.data_ptr(), sscal.data_ptr(),
                               uscal.data_ptr(), None, ws.data_ptr(), ws.numel() - (1 if ws_short else 0), 0, _stream())
    dl, du = (C.c_void_p * 9)(*[t.data_ptr() for t in dz[:9]]), (C.c_void_p * 9)(*[t.data_ptr() for t in dz[9:]])
    rc_b = L.uaps_pairloss_bwd(heads, holed, y.data_ptr(), y.data_ptr(), sscal.data_ptr(), uscal.data_ptr(), 0.1, 0.1, None, D, B, Cc, H, W, 0, dl, du,
                               0, _stream())
    torch.cuda.synchronize()
    fwd_clean = bool((pseudo == SENT_I).all() and (var == SENT_F).all() and (sscal == SENT_F).all() and (uscal == SENT_F).all() and (ws == 7).all())
    return rc_f, rc_b, fwd_clean, all(bool((t == SENT_F).all()) for t in dz)


@pytest.mark.parametrize("kw,want", [(dict(D=0), ERANGE), (dict(D=9), ERANGE), (dict(Cc=1), ERANGE), (dict(Cc=9), ERANGE), (dict(B=0), EINVAL),
                                     (dict(null_head=True), EINVAL)])
def test_pair_refusals_write_nothing(L, kw, want):
    rc_f, rc_b, fwd_clean, bwd_clean = _refuse(L, **kw)
    assert (rc_f, rc_b) == (want, want)
    assert fwd_clean and bwd_clean, "a refused call wrote an output"


@pytest.mark.parametrize("kw,want", [(dict(ws_short=True), EWORKSPACE), (dict(no_w=True), EINVAL)])
def test_pair_forward_refusals_write_nothing(L, kw, want):
    rc_f, _, fwd_clean, _ = _refuse(L, **kw)
    assert rc_f == want
    assert fwd_clean, "a refused forward wrote an output"


@pytest.mark.parametrize("n_pixels", [0, -5])
def test_finalize_sums_refuses_a_non_positive_pixel_count(L, n_pixels):
    D, Cc = 3, 4
    sums = torch.ones(sum(R.n_sums(D, Cc)), dtype=torch.float64, device=DEV)
    sscal, uscal = torch.full((R.s_layout(D, Cc)["n"],), SENT_F, device=DEV), torch.full((R.u_layout(D, Cc)["n"],), SENT_F, device=DEV)
    assert L.uaps_pairloss_finalize_sums(sums.data_ptr(), D, Cc, n_pixels, 0.1, 0.1, R.EPS, sscal.data_ptr(), uscal.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((sscal == SENT_F).all() and (uscal == SENT_F).all())


# ---- the forms the cases claim to take are the ones launched ------------------------------------------------------------------------
def test_the_profiler_sees_the_predicted_kernel_forms(L):
    """One case per form class.  The kernel names and template arguments a profiler records must be the ones loss_ref's restatement
    of the dispatch predicts: a change of the dispatch then fails here instead of silently testing another form."""
    from torch.profiler import ProfilerActivity, profile
    cases = [R.BY_ID["pair-4x4-vec-plain"], R.BY_ID["pair-3x5-scalar-plain"], R.BY_ID["pair-6x4-vec-track"], R.BY_ID["x-4x4-off1"],
             R.BY_ID["two-5x5-v2"], R.BY_ID["two-2x3-vec"], R.BY_ID["two-8x8-vec"]]
    assert [c.form for c in cases] == ["vec4", "scalar", "vec2", "scalar", "vec2", "vec4", "scalar"]
    seen = {}
    for case in cases:
        inp = R.inputs(case)
        run(L, case, inp)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run(L, case, inp)
        seen[case.id] = [" ".join(e.key.split()) for e in prof.key_averages()]
    names = [n for v in seen.values() for n in v]
    if not any("_fwd_kernel" in n or "_bwd_kernel" in n for n in names):
        pytest.skip("the profiler recorded no device kernels of this package")
    print("LOSSFORM kernels", seen)
    for case in cases:
        ours = [n for n in seen[case.id] if "_fwd_kernel<" in n or "_bwd_kernel<" in n]
        for want in case.kernels:
            assert any(f"uaps::{want}(" in n for n in ours), (case.id, want, ours)
        assert len(ours) == len(case.kernels), (case.id, ours)

"""-m gpu: every kernel form of uaps_amd/csrc/loss_cps.hip and loss_ucc.hip (cut-mix included), and the forms of loss_seg.hip that
tests/test_gpu_seglosses.py lacks, against the references of tests/suploss_ref.py, through the C ABI; and the label edges of every
dense-label entry point.

Every input, output, scalar block and workspace is a view into a buffer pre-filled with a sentinel (Buf of tests/test_gpu_ops_forms.py,
as tests/test_gpu_consistency_forms.py uses it: the Buf of tests/test_gpu_loss_forms.py has no byte sentinel for the pseudo-labels);
every output view is pre-filled with NaN (bytes: 0xEE, labels: -999) and the workspace is exactly the queried size.  After every launch
the sentinels around every buffer must be intact, the outputs fully overwritten, the exact quantities equal to the bit and the others
within their derived bars; a second launch into fresh buffers must give the same bits.  Every misaligned or guarded launch here is a
valid call by the header's contract.

Label edges: labels of -1, C, 255, 2^31, 2^32 + 1, -2^32 + 1, INT64_MIN and INT64_MAX on a few pixels.  The header promises that a
label outside [0, C) enters no term and is counted, so every output must equal, bit for bit, the same call with those labels replaced
by -1, and the count must be the number planted: no reference, no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import suploss_ref as R
from test_gpu_ops_forms import DEV, OK, Buf, _bound, _bval, _hints, _p, _stream

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_IGNORE = -12345                                    # a value no label of a case takes


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    lib = _lib.lib()
    prev = lib.uaps_get_step_state()
    lib.uaps_set_step_state(None)
    yield lib
    lib.uaps_set_step_state(prev)


FILL = {torch.float32: np.nan, torch.uint8: 0xEE, torch.int64: -999}
NP = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int64: np.int64}


def _out(shape, off: int = 0, dtype=torch.float32):
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    return Buf(shape, off, np.full(shape, FILL[dtype], NP[dtype]), dtype)


def _in(a, off: int = 0, dtype=torch.float32):
    return Buf(np.shape(a), off, a, dtype)


def _ws(query):
    """A workspace of exactly the queried size, NaN inside, sentinels around."""
    n = C.c_size_t()
    assert query(C.byref(n)) == OK and n.value % 4 == 0
    return _out(n.value // 4), n.value


def _g(vals, null):
    return [None if null else _in(np.array([v], F32)) for v in vals]


# ---- one runner per family: (outputs as name -> Buf, inputs as name -> Buf) -------------------------------------------------------------
def run_cps(L, c, inp):
    N, Cc, H, W = c.shape
    z1, z2, y = _in(inp["z1"], c.off("z1")), _in(inp["z2"], c.off("z2")), _in(inp["labels"], c.off("labels"), torch.int64)
    p1 = _out((N, H, W), c.off("pseudo1"), torch.uint8) if c.has("pseudo1") else None
    p2 = _out((N, H, W), c.off("pseudo2"), torch.uint8) if c.has("pseudo2") else None
    s = _out(16 + 24 * Cc)
    ws, wsb = _ws(lambda n: L.uaps_cps_workspace_bytes(N, c.B_lab, Cc, H, W, n))
    assert wsb == c.workspace_bytes
    st = _stream()
    assert L.uaps_cps_fwd(z1.ptr, z2.ptr, y.ptr, N, c.B_lab, Cc, H, W, c.eps, _p(p1), _p(p2), s.ptr, ws.ptr, wsb, st) == OK
    g = _g(c.g, c.gnull)
    dz1, dz2 = _out(c.shape, c.off("dz1")), _out(c.shape, c.off("dz2"))
    assert L.uaps_cps_bwd(z1.ptr, z2.ptr, y.ptr, s.ptr, _p(g[0]), _p(g[1]), _p(g[2]), N, c.B_lab, Cc, H, W, dz1.ptr, dz2.ptr, st) == OK
    return dict(pseudo1=p1, pseudo2=p2, s=s, dz1=dz1, dz2=dz2), dict(z1=z1, z2=z2, labels=y, ws=ws, g0=g[0], g1=g[1], g2=g[2])


def run_ucc(L, c, inp):
    B, Cc, H, W = c.shape
    z1, z2, y = _in(inp["z1"], c.off("z1")), _in(inp["z2"], c.off("z2")), _in(inp["labels"], c.off("labels"), torch.int64)
    p1 = _out((B, H, W), c.off("pseudo1"), torch.uint8) if c.has("pseudo1") else None
    p2 = _out((B, H, W), c.off("pseudo2"), torch.uint8) if c.has("pseudo2") else None
    v1 = _out((B, H, W), c.off("var1")) if c.has("var1") else None
    v2 = _out((B, H, W), c.off("var2")) if c.has("var2") else None
    s = _out(20 + 16 * Cc)
    ws, wsb = _ws(lambda n: L.uaps_ucc_workspace_bytes(B, Cc, H, W, n))
    assert wsb == c.workspace_bytes
    st = _stream()
    assert L.uaps_ucc_fwd(z1.ptr, z2.ptr, y.ptr, B, Cc, H, W, c.eps, _p(p1), _p(p2), _p(v1), _p(v2), s.ptr, ws.ptr, wsb, st) == OK
    g = _g((c.g[0], c.g[2]), c.gnull)
    dz1, dz2 = _out((3 * B, Cc, H, W), c.off("dz1")), _out((3 * B, Cc, H, W), c.off("dz2"))
    assert L.uaps_ucc_bwd(z1.ptr, z2.ptr, y.ptr, s.ptr, _p(g[0]), _p(g[1]), B, Cc, H, W, dz1.ptr, dz2.ptr, st) == OK
    return dict(pseudo1=p1, pseudo2=p2, var1=v1, var2=v2, s=s, dz1=dz1, dz2=dz2), dict(z1=z1, z2=z2, labels=y, ws=ws, g0=g[0], g1=g[1])


def run_cutmix(L, c, inp):
    B, _, H, W = c.shape
    Cin = c.Cin
    xl, xwk, xst = (_in(inp[k], c.off(k)) for k in ("x_l", "x_wk", "x_st"))
    y = _in(inp["y_l"], 0, torch.int64)
    out, yout = _out((3 * B, Cin, H, W), c.off("out")), _out((B, H, W), 0, torch.int64)
    rl, ru = np.ascontiguousarray(inp["rl"], np.int32), np.ascontiguousarray(inp["ru"], np.int32)
    bound = _bound(L, 0.0)
    args = (xl.ptr, xwk.ptr, xst.ptr, y.ptr, rl.ctypes.data, ru.ctypes.data, B, Cin, H, W, out.ptr, yout.ptr, _stream())
    if c.hinted:
        assert L.uaps_ucc_cutmix_batch_h(_hints(out_amax=bound), *args) == OK
    else:
        assert L.uaps_next_call_hints(_hints(out_amax=bound)) == OK
        assert L.uaps_ucc_cutmix_batch(*args) == OK
    return dict(out=out, y_out=yout), dict(x_l=xl, x_wk=xwk, x_st=xst, y_l=y, bound=bound)


def _seg_params(c, inp):
    from uaps_amd import _lib
    p = _lib.SegLossParams()
    p.struct_size, p.terms = C.sizeof(_lib.SegLossParams), R.SEG_TERMS
    for i, v in enumerate(R.SEG_COEF):
        p.coef[i] = v
    for i, v in enumerate(inp["class_weight"]):
        p.class_weight[i] = float(v)
    p.focal_gamma, p.focal_mean, p.tversky_alpha, p.tversky_beta, p.eps, p.smooth = 2.0, 1, R.SEG_TVERSKY[0], R.SEG_TVERSKY[1], c.eps, 1e-5
    p.ignore_index = NO_IGNORE if c.ignore is None else c.ignore
    return p


def run_seg(L, c, inp):
    B, Cc, H, W = c.shape
    z, y = _in(inp["z"], c.off("z")), _in(inp["labels"], c.off("labels"), torch.int64)
    prm = _seg_params(c, inp)
    s = _out(16 + 7 * Cc)
    ws, wsb = _ws(lambda n: L.uaps_segloss_workspace_bytes(B, Cc, H, W, n))
    assert wsb == c.workspace_bytes
    st = _stream()
    assert L.uaps_segloss_fwd(z.ptr, y.ptr, C.byref(prm), B, Cc, H, W, s.ptr, ws.ptr, wsb, st) == OK
    g, = _g(c.g[:1], c.gnull)
    dz = _out(c.shape, c.off("dz"))
    assert L.uaps_segloss_bwd(z.ptr, y.ptr, C.byref(prm), s.ptr, _p(g), B, Cc, H, W, dz.ptr, st) == OK
    return dict(s=s, dz=dz), dict(z=z, labels=y, ws=ws, g=g)


RUN = dict(cps=run_cps, ucc=run_ucc, cutmix=run_cutmix, seg=run_seg)


def _split(c, s) -> dict:
    """A scalar block under the reference's names (layouts: include/uaps_hip.h, UAPS_CPS_S_*, UAPS_UCC_S_*, UAPS_SEG_S_*)."""
    Cc = c.C
    if c.entry == "seg":
        r = lambda k: s[16 + k * Cc:16 + (k + 1) * Cc]
        return dict(terms=s[[0, 2, 3, 4, 6]], bad=s[7], n_valid=s[8], wsum=s[9], kce=s[10], A=r(0), I=r(1), N=r(2), GA=r(4), GI=r(5))
    T, b = (6, 16) if c.entry == "cps" else (4, 20)
    r = lambda k: s[b + k * T * Cc:b + (k + 1) * T * Cc]
    d = dict(head=s[:15] if c.entry == "cps" else s[:16], bad=s[b - 1 if c.entry == "cps" else 16], A1=r(0), A2=r(1), I=r(2), CARD=r(3))
    if c.entry == "ucc":
        d["reserved"] = s[17:20]
    return d


def _launch(L, c, inp):
    """One launch on fresh buffers: (the outputs on the host under the reference's names, the failed checks)."""
    outs, ins = RUN[c.entry](L, c, inp)
    torch.cuda.synchronize()
    got, bad = {}, []
    for k, b in outs.items():
        if b is None:
            continue
        h, ok = b.fetch()
        if not ok:
            bad.append(f"the sentinels around {k} were written")
        if k == "s":
            if not np.isfinite(h).all():
                bad.append("a scalar was left unwritten or is not a number")
            got.update(_split(c, h))
        else:
            got[k] = h
    for k, b in ins.items():
        if isinstance(b, Buf) and not b.fetch()[1]:
            bad.append(f"the sentinels around {k} were written")
    if c.entry == "cutmix":
        got["amax"] = _bval(ins["bound"])
        if (got["y_out"] == FILL[torch.int64]).any():
            bad.append("y_out was not fully overwritten")
    return got, bad


def _same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run_case(L, c):
    """(the ratio of every float64-compared quantity to its bar, the failed checks, the reference) of one case."""
    inp = R.inputs(c)
    ref = R.reference(c, inp)
    sw = R.swallowed(ref)
    assert not sw, (c.id, sw)                          # before the device is asked
    got, bad = _launch(L, c, inp)
    ratios, bad2 = R.compare(ref, got)
    again, bad3 = _launch(L, c, inp)
    bad4 = [f"second launch differs in {k}" for k in got if not _same(got[k], again[k])]
    return ratios, bad + bad2 + bad3 + bad4, ref


def group_of(c) -> str:
    kind = c.id.split("-")[1]
    if c.heavy:
        return c.id
    if kind[0] == "c" and kind[1:].isdigit():
        return f"{c.entry}-classes"
    if kind.startswith("outs"):
        return f"{c.entry}-outs"
    if kind in R.REGIMES:
        return f"{c.entry}-regimes"
    if c.entry == "cutmix":
        return "cutmix-ptr" if kind in ("ptr", "b64") else "cutmix-maps"
    return f"{c.entry}-{'ptr' if kind == 'ptr' else 'edges'}"


GROUPS = sorted({group_of(c) for c in R.CASES})


@pytest.mark.parametrize("group", GROUPS)
def test_kernel_forms_against_float64(L, group):
    failed = {}
    for c in (c for c in R.CASES if group_of(c) == group):
        try:
            ratios, bad, ref = run_case(L, c)
        except RuntimeError as e:                      # a HIP error is sticky: launch nothing more on a device that has faulted
            if "hip" in str(e).lower():
                pytest.exit(f"{c.id}: {e}", returncode=3)
            raise
        print("SUPLOSS", c.id, " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())) or "bit-exact")
        if bad:
            failed[c.id] = bad
    assert not failed, failed


# ---- label edges ----------------------------------------------------------------------------------------------------------------------
def _planted(y, C_, rng, keep=()):
    """(labels with the eight edge values on 16 pixels, the same with every label outside [0, C) and not in `keep` as -1, how many of
    the planted count as outside)."""
    y = np.array(y, np.int64)
    flat = y.reshape(-1)
    pix = rng.choice(flat.size, size=min(flat.size, 2 * len(R.EDGE_LABELS)), replace=False)
    flat[pix] = np.resize(R.edge_labels(C_), pix.size)
    out = ((y < 0) | (y >= C_)) & ~np.isin(y, keep)
    return y, np.where(out, -1, y), int(out.sum())


def _edge_dense(L, entry, form):
    c = R.BY_ID[f"{entry}-edges-{form}"]
    inp = R.inputs(c)
    keep = () if c.ignore is None else (c.ignore,)
    y = inp["labels"]
    outside = ((y < 0) | (y >= c.C)) & ~np.isin(y, keep)
    a, bad_a = _launch(L, c, inp)
    b, bad_b = _launch(L, c, dict(inp, labels=np.where(outside, -1, y)))
    assert not bad_a and not bad_b, (bad_a, bad_b)
    assert set(R.edge_labels(c.C).tolist()) <= set(y.reshape(-1).tolist())
    return a, b, int(outside.sum()), float(a["bad"]), float(b["bad"])


def _edge_block(L, cid):
    """uaps_sup_fwd / _bwd (two-branch cases) and uaps_pairloss_fwd / _bwd of the UAPS loss block, through tests/test_gpu_loss_forms.py."""
    import loss_ref as LR
    import test_gpu_loss_forms as T
    case = LR.BY_ID[cid]
    inp = LR.inputs(case)
    y, y1, n = _planted(inp["labels"], case.C, np.random.default_rng(7))
    state = torch.zeros(16, dtype=torch.float32, device=DEV)
    a, sa = T.run(L, case, dict(inp, labels=y), state)
    b, sb = T.run(L, case, dict(inp, labels=y1), state)
    assert not sa and not sb, (sa, sb)
    bad = lambda g: float(LR.slot(g["sscal"], LR.s_layout(case.D, case.C), "bad")[0])
    return a, b, n, bad(a), bad(b)


def _edge_binloss(L, name):
    import binloss_ref as Bn
    import test_gpu_binloss as T
    case = next(c for c in Bn.CASES if c.name == name)
    z, t = Bn.make_inputs(case)
    y, y1, n = _planted(t.numpy(), 2, np.random.default_rng(11))
    a, _ = T.run_c_abi(case, z, torch.from_numpy(y))
    b, _ = T.run_c_abi(case, z, torch.from_numpy(y1))
    return a, b, n, float(a["bad"]), float(b["bad"])


def _edge_confusion(L, which):
    from uaps_amd import binary_losses, metrics
    rng = np.random.default_rng(13)
    Cc = 1 if which == "bin" else 5
    z = torch.from_numpy((rng.standard_normal((2, Cc, 16, 24)) * 2).astype(F32)).to(DEV)
    y, y1, n = _planted(rng.integers(0, max(Cc, 2), (2, 16, 24)), max(Cc, 2), rng)
    f = (lambda t: binary_losses.bin_confusion(z, torch.from_numpy(t).to(DEV))) if which == "bin" else (lambda t: metrics.seg_confusion(z, torch.from_numpy(t).to(DEV)))
    a, b = f(y).cpu().numpy(), f(y1).cpu().numpy()
    return dict(counts=a), dict(counts=b), n, float(y.size - a.sum()), float(y.size - b.sum())


EDGES = [("cps", lambda L: _edge_dense(L, "cps", "v4")), ("cps-v1", lambda L: _edge_dense(L, "cps", "v1")),
         ("ucc", lambda L: _edge_dense(L, "ucc", "v4")), ("ucc-v1", lambda L: _edge_dense(L, "ucc", "v1")),
         ("segloss", lambda L: _edge_dense(L, "seg", "v4")), ("segloss-v1", lambda L: _edge_dense(L, "seg", "v1")),
         ("sup-vec4", lambda L: _edge_block(L, "two-2x3-vec")), ("sup-vec2", lambda L: _edge_block(L, "two-5x5-v2")),
         ("sup-scalar", lambda L: _edge_block(L, "two-8x8-vec")), ("pairloss-vec4", lambda L: _edge_block(L, "pair-4x4-vec-plain")),
         ("pairloss-scalar", lambda L: _edge_block(L, "pair-3x5-scalar-plain")),
         ("binloss", lambda L: _edge_binloss(L, "3x33x19-int")), ("binloss-off1", lambda L: _edge_binloss(L, "1x1x403-off1-int")),
         ("seg_confusion", lambda L: _edge_confusion(L, "seg")), ("bin_confusion", lambda L: _edge_confusion(L, "bin"))]


@pytest.mark.parametrize("name", [n for n, _ in EDGES])
def test_labels_outside_the_classes_enter_no_term_and_are_counted(L, name):
    a, b, n, bad_a, bad_b = dict(EDGES)[name](L)
    differ = [k for k in a if a[k] is not None and not _same(a[k], b[k])]
    print("SUPLOSS edges", name, "planted", n, "counted", bad_a, "differing", differ)
    assert bad_a == n and bad_b == n, (bad_a, bad_b, n)
    assert not differ, differ

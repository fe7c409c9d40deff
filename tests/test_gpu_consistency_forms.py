"""-m gpu: every kernel form of uaps_amd/csrc/loss_mean_teacher.hip, loss_cct_dct.hip and the two-tensor softmax terms of pair_ops.hip
against the references of tests/consistency_ref.py, through the C ABI.

Every tensor is a view `off` elements into a buffer pre-filled with a sentinel; every output view is pre-filled with NaN (bytes: 0xEE).
After every launch the outputs must be fully overwritten, the sentinels in front of and behind every tensor intact, the rows outside a
window still NaN, the bit-exact quantities equal to the bit and the float64-compared ones within their derived bars; a second launch
into fresh buffers must give the same bits (the means included), and every refusal must leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import consistency_ref as R
from test_gpu_ops_forms import DEV, EINVAL, ERANGE, EWORKSPACE, OK, Buf, _bound, _bval, _hints, _p, _stream

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    lib = _lib.lib()
    prev = lib.uaps_get_step_state()
    lib.uaps_set_step_state(None)
    yield lib
    lib.uaps_set_step_state(prev)


def _out(shape, off: int = 0, dtype=torch.float32):
    """An output view: NaN (bytes: 0xEE) inside, sentinels around."""
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    fill = np.full(shape, np.nan, F32) if dtype == torch.float32 else np.full(shape, 0xEE, np.uint8)
    return Buf(shape, off, fill, dtype)


def _in(a, off: int = 0, dtype=torch.float32):
    return Buf(np.shape(a), off, a, dtype)


def _arr(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr if b is not None else None for b in bufs])


def _ws(L, query, short: bool = False):
    n = C.c_size_t()
    assert query(C.byref(n)) == OK and n.value % 4 == 0
    return _out(n.value // 4), n.value - (4 if short else 0)


# ---- one runner per entry-point family: (rc, outputs as name -> Buf, inputs as name -> Buf).  `o` overrides arguments (refusals) -----
def run_ema(L, c, inp, **o):
    n = len(c.numels)
    es = [_in(t["e"], c.offe[i % len(c.offe)]) for i, t in enumerate(inp["t"])]
    ps = [_in(t["p"], c.offp[i % len(c.offp)]) for i, t in enumerate(inp["t"])]
    ea, pa = _arr(es), _arr(ps)
    if "null_e" in o:
        ea[o["null_e"]] = None
    numel = (C.c_long * n)(*[o.get("numel", {}).get(i, m) for i, m in enumerate(c.numels)])
    rc = L.uaps_ema_update(ea, pa, numel, o.get("n", n), inp["alpha"], inp["oma"], _stream())
    return rc, {f"e{i}": b for i, b in enumerate(es)}, {f"p{i}": b for i, b in enumerate(ps)}


def run_noise(L, c, inp, **o):
    B, Ci, H, W = c.shape
    T = o.get("T", c.T)
    x = _in(inp["x"], c.off(0))
    out = _out(((1 + c.T) * B, Ci, H, W), c.off(2 if c.entry == "noise_apply" else 1))
    ins = dict(x=x)
    if c.entry == "noise":
        rc = L.uaps_teacher_noise(x.ptr, o.get("B", B), Ci, H, W, T, c.seed, c.offset, out.ptr, _stream())
    else:
        ins["noise"] = nz = _in(inp["noise"], c.off(1))
        rc = L.uaps_teacher_noise_apply(x.ptr, None if o.get("null") == "noise" else nz.ptr, o.get("B", B), Ci, H, W, T, out.ptr, _stream())
    return rc, dict(out=out), ins


def run_mc_fwd(L, c, inp, **o):
    B, Cc, H, W = c.shape
    masked = c.mode == "mask"
    s, e = _in(inp["s"], c.off(0)), _in(inp["e"], c.off(1))
    mc = _in(inp["mc"], c.off(2)) if masked else None
    mask = _out((B, H, W), c.off(3), torch.uint8) if masked else None
    unc = _out((B, H, W), c.off(4)) if masked and c.unc else None
    out3 = _out(3)
    ws, wsb = _ws(L, L.uaps_mc_consistency_workspace_bytes, o.get("short", False))
    null = o.get("null", "")
    rc = L.uaps_mc_consistency_fwd(s.ptr, e.ptr, _p(mc), o.get("T", c.T), o.get("B", B), o.get("C", Cc), H, W, inp.get("thr", 0.0),
                                   None if null == "mask" else _p(mask), _p(unc), out3.ptr, None if null == "ws" else ws.ptr, wsb, _stream())
    outs = dict(out3=out3)
    if masked:
        outs["mask"] = mask
        if unc is not None:
            outs["unc"] = unc
    return rc, outs, dict(s=s, e=e, mc=mc, ws=ws)


def run_mc_bwd(L, c, inp, **o):
    B, Cc, H, W = c.shape
    masked = c.mode == "mask"
    s, e = _in(inp["s"], c.off(0)), _in(inp["e"], c.off(1))
    mask = _in(inp["mask"], c.off(2), torch.uint8) if masked else None
    out3 = _in(np.array([0.0, 0.0, inp["sum_m"]], F32)) if masked else None
    g, ds = _in(np.array([c.g], F32)), _out(c.shape, c.off(3))
    null = o.get("null", "")
    rc = L.uaps_mc_consistency_bwd(s.ptr, e.ptr, _p(mask), g.ptr, None if null == "out3" else _p(out3), o.get("B", B), o.get("C", Cc), H, W,
                                   ds.ptr, _stream())
    return rc, dict(ds=ds), dict(s=s, e=e, mask=mask, g=g)


def run_cct(L, c, inp, **o):
    B, Cc, H, W = c.shape
    D = c.D
    heads = [_in(h, c.off(k)) for k, h in enumerate(inp["heads"])]
    ha = _arr(heads)
    if o.get("null") == "head":
        ha[D - 1] = None
    ins = {f"h{k}": b for k, b in enumerate(heads)}
    if c.entry == "cct_fwd":
        out = _out(D)
        ws, wsb = _ws(L, L.uaps_cct_dct_workspace_bytes, o.get("short", False))
        rc = L.uaps_cct_consistency_fwd(ha, o.get("D", D), o.get("b0", c.b0), o.get("B", B), o.get("C", Cc), H, W, out.ptr, ws.ptr, wsb, _stream())
        return rc, dict(out=out), dict(ins, ws=ws)
    dh = [_out(h.shape, c.off(D + k)) for k, h in enumerate(inp["heads"])]
    g = _in(np.array([c.g], F32))
    rc = L.uaps_cct_consistency_bwd(ha, o.get("D", D), o.get("b0", c.b0), o.get("B", B), o.get("C", Cc), H, W, g.ptr, _arr(dh), _stream())
    return rc, {f"dz{k}": b for k, b in enumerate(dh)}, ins


def run_rot90(L, c, inp, **o):
    B, Ci, H, W = c.shape
    n = B * Ci * H * W
    xl, xu = _in(inp["xl"], c.off(0)), _in(inp["xu"], c.off(1))
    out = _out((3 if not c.rot_out else 2) * n, c.off(2))
    rot = _out(n, c.off(3)) if c.rot_out else None
    bound = _bound(L, c.amax) if c.amax is not None else None
    k = o.get("k", c.k)
    args = (xl.ptr, xu.ptr, o.get("B", B), Ci, H, W, k, out.ptr, None if o.get("null") == "rot" else _p(rot), _stream())
    if bound is not None and c.hinted:
        rc = L.uaps_rot90_batch_h(_hints(out_amax=bound), *args)
    else:
        if bound is not None:
            assert L.uaps_next_call_hints(_hints(out_amax=bound)) == OK
        rc = L.uaps_rot90_batch(*args)
    outs = dict(out=out)
    if rot is not None:
        outs["rot_out"] = rot
    return rc, outs, dict(xl=xl, xu=xu, bound=bound)


def run_rot(L, c, inp, **o):
    B, Cc, H, W = c.shape
    r, u = _in(inp["r"], c.off(0)), _in(inp["u"], c.off(1))
    k = o.get("k", c.k)
    if c.entry == "rot_fwd":
        out2 = _out(2)
        ws, wsb = _ws(L, L.uaps_cct_dct_workspace_bytes, o.get("short", False))
        rc = L.uaps_rot_consistency_fwd(r.ptr, o.get("r_b0", c.r_b0), u.ptr, c.u_b0, o.get("B", B), o.get("C", Cc), H, W, k, out2.ptr, ws.ptr, wsb,
                                        _stream())
        return rc, dict(out2=out2), dict(r=r, u=u, ws=ws)
    g, dr, du = _in(np.array([c.g], F32)), _out(inp["r"].shape, c.off(2)), _out(inp["u"].shape, c.off(3))
    rc = L.uaps_rot_consistency_bwd(r.ptr, o.get("r_b0", c.r_b0), u.ptr, c.u_b0, o.get("B", B), o.get("C", Cc), H, W, k, g.ptr, dr.ptr,
                                    None if o.get("null") == "du" else du.ptr, _stream())
    return rc, dict(dr=dr, du=du), dict(r=r, u=u)


def run_pair(L, c, inp, **o):
    B, Cc, H, W = c.shape
    Bv, Cv, st = o.get("B", B), o.get("C", Cc), _stream()
    e = c.entry
    if e == "entropy":
        p = _in(inp["p"], c.off(0))
        ent = _out((B, H, W), c.off(1)) if "ent_map" in c.outs else None
        mean = _out(1) if "ent_mean" in c.outs else None
        ws, wsb = _ws(L, L.uaps_pair_workspace_bytes, o.get("short", False))
        none = o.get("null") == "outs"
        rc = L.uaps_entropy_map(p.ptr, Bv, Cv, H, W, None if none else _p(ent), None if none else _p(mean), ws.ptr, wsb, st)
        return rc, {k: b for k, b in dict(ent_map=ent, ent_mean=mean).items() if b is not None}, dict(p=p, ws=ws)
    a, b = _in(inp["a"], c.off(0)), _in(inp["b"], c.off(1))
    ins = dict(a=a, b=b)
    if e == "pair_fwd":
        mse = _out(c.shape, c.off(2)) if "mse_map" in c.outs else None
        klm = _out((B, H, W), c.off(3)) if "kl_map" in c.outs else None
        mean = _out(1) if "kl_mean" in c.outs else None
        ws, wsb = _ws(L, L.uaps_pair_workspace_bytes, o.get("short", False))
        none = o.get("null") == "outs"
        rc = L.uaps_softmax_pair_fwd(a.ptr, b.ptr, int(c.probs), Bv, Cv, H, W, None if none else _p(mse), None if none else _p(klm),
                                     None if none else _p(mean), ws.ptr, wsb, st)
        return rc, {k: v for k, v in dict(mse_map=mse, kl_map=klm, kl_mean=mean).items() if v is not None}, dict(ins, ws=ws)
    if e == "mse_bwd":
        ins["gmap"] = g = _in(inp["gmap"], c.off(2))
        da = _out(c.shape, c.off(3))
        return L.uaps_softmax_mse_bwd(a.ptr, b.ptr, None if o.get("null") == "g" else g.ptr, Bv, Cv, H, W, da.ptr, st), dict(da=da), ins
    if e == "kl_bwd":
        ins["g"] = g = None if c.gnull else _in(np.array([c.g], F32))
        da = _out(c.shape, c.off(2))
        return L.uaps_softmax_kl_bwd(None if o.get("null") == "a" else a.ptr, b.ptr, _p(g), Bv, Cv, H, W, da.ptr, st), dict(da=da), ins
    ins["gmap"] = g = _in(inp["gmap"], c.off(2))
    da = _out(c.shape, c.off(3)) if "da" in c.outs else None
    db = _out(c.shape, c.off(4)) if "db" in c.outs else None
    none = o.get("null") == "outs"
    rc = L.uaps_softmax_klmap_bwd(a.ptr, b.ptr, None if o.get("null") == "g" else g.ptr, Bv, Cv, H, W, None if none else _p(da),
                                  None if none else _p(db), st)
    return rc, {k: v for k, v in dict(da=da, db=db).items() if v is not None}, ins


RUN = dict(ema=run_ema, noise=run_noise, noise_apply=run_noise, mc_fwd=run_mc_fwd, mc_bwd=run_mc_bwd, cct_fwd=run_cct, cct_bwd=run_cct,
           rot90=run_rot90, rot_fwd=run_rot, rot_bwd=run_rot, pair_fwd=run_pair, mse_bwd=run_pair, kl_bwd=run_pair, klmap_bwd=run_pair,
           entropy=run_pair)
SPLIT = dict(out3=("loss", "sum_md", "sum_m"), out2=("loss", "sum"))


def _launch(L, c, inp):
    """One launch on fresh buffers: (the outputs on the host under the reference's names, the failed checks)."""
    rc, outs, ins = RUN[c.entry](L, c, inp)
    assert rc == OK, rc
    torch.cuda.synchronize()
    got, bad = {}, []
    for k, b in outs.items():
        h, ok = b.fetch()
        if not ok:
            bad.append(f"the sentinels around {k} were written")
        if k in SPLIT:
            got.update({name: h[i] for i, name in enumerate(SPLIT[k])})
        elif k == "out" and c.entry == "cct_fwd":
            got["loss"], got["sums"] = h[0], h[1:]
        elif k in ("kl_mean", "ent_mean"):
            got[k] = h[0]
        elif c.entry == "rot90":
            n = int(np.prod(c.shape))
            B, Ci, H, W = c.shape
            rshape = (B, Ci, W, H) if c.k & 1 else c.shape
            if k == "out":
                got["cat"] = h[:2 * n]
                if not c.rot_out:
                    got["rot"] = h[2 * n:].reshape(rshape)
            else:
                got["rot"] = h.reshape(rshape)
        else:
            got[k] = h
    for k, b in ins.items():
        if isinstance(b, Buf) and not b.fetch()[1]:
            bad.append(f"the sentinels around {k} were written")
    if c.entry == "rot90" and c.amax is not None:
        got["amax"] = _bval(ins["bound"])
    return got, bad


def _same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run_case(L, c):
    """(the ratio of every float64-compared quantity to its bar, the failed checks, the reference) of one case."""
    inp = R.inputs(c)
    ref = R.reference(c, inp)                      # (asserts the ambiguity and clamp-edge caps before the device is asked)
    got, bad = _launch(L, c, inp)
    inside, bad1 = R.window_split(ref, got)
    ratios, bad2 = R.compare(ref, inside)
    again, bad3 = _launch(L, c, inp)
    bad4 = [f"second launch differs in {k}" for k in got if not _same(got[k], again[k])]
    return ratios, bad + bad1 + bad2 + bad3 + bad4, ref


def _check(L, entries):
    """Every case of the entry points: one test per entry point keeps the count of tests (and of reference computations) small."""
    failed = {}
    for c in (c for c in R.CASES if c.entry in entries):
        try:
            ratios, bad, ref = run_case(L, c)
        except RuntimeError as e:                  # a HIP error is sticky: launch nothing more on a device that has faulted
            if "hip" in str(e).lower():
                pytest.exit(f"{c.id}: {e}", returncode=3)
            raise
        print(c.id, " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())) or "bit-exact", ref.info or "")
        if bad:
            failed[c.id] = bad
    assert not failed, failed


def test_ema_update(L):
    _check(L, ("ema",))


def test_teacher_noise_draw(L):
    _check(L, ("noise",))


def test_teacher_noise_apply(L):
    _check(L, ("noise_apply",))


def test_mc_consistency_fwd(L):
    _check(L, ("mc_fwd",))


def test_mc_consistency_bwd(L):
    _check(L, ("mc_bwd",))


def test_cct_consistency_fwd(L):
    _check(L, ("cct_fwd",))


def test_cct_consistency_bwd(L):
    _check(L, ("cct_bwd",))


def test_rot90_batch(L):
    _check(L, ("rot90",))


def test_rot_consistency_fwd(L):
    _check(L, ("rot_fwd",))


def test_rot_consistency_bwd(L):
    _check(L, ("rot_bwd",))


def test_softmax_pair_fwd(L):
    _check(L, ("pair_fwd",))


def test_softmax_mse_bwd(L):
    _check(L, ("mse_bwd",))


def test_softmax_kl_bwd(L):
    _check(L, ("kl_bwd",))


def test_softmax_klmap_bwd(L):
    _check(L, ("klmap_bwd",))


def test_entropy_map(L):
    _check(L, ("entropy",))


# ---- refusals: nothing launched, nothing written -----------------------------------------------------------------------------------
REFUSALS = [
    ("ema-step1", dict(n=0), EINVAL), ("ema-step1", dict(null_e=2), EINVAL), ("ema-step1", dict(numel={2: 0}), EINVAL),
    ("ema-step1", dict(numel={1: 1 << 29}), ERANGE), ("ema-n129", dict(null_e=128), EINVAL),
    ("noise-T1", dict(T=17), EINVAL), ("noise-T1", dict(B=0), EINVAL), ("apply-T1", dict(T=-1), EINVAL), ("apply-T1", dict(null="noise"), EINVAL),
    ("uamt-2x16x24-T3", dict(T=17), EINVAL), ("uamt-2x16x24-T3", dict(null="mask"), EINVAL), ("uamt-2x16x24-T3", dict(C=9), ERANGE),
    ("uamt-2x16x24-T3", dict(C=1), ERANGE), ("uamt-2x16x24-T3", dict(short=True), EWORKSPACE), ("uamt-2x16x24-T3", dict(null="ws"), EWORKSPACE),
    ("mt-c3", dict(T=1), EINVAL), ("mt-c3", dict(B=0), EINVAL),
    ("uamtb-c3", dict(null="out3"), EINVAL), ("uamtb-c3", dict(C=9), ERANGE), ("mtb-c3", dict(B=-1), EINVAL),
    ("cct-c3-v4", dict(D=1), EINVAL), ("cct-c3-v4", dict(D=9), EINVAL), ("cct-c3-v4", dict(null="head"), EINVAL), ("cct-c3-v4", dict(b0=-1), EINVAL),
    ("cct-c3-v4", dict(C=9), ERANGE), ("cct-c3-v4", dict(short=True), EWORKSPACE),
    ("cctb-c3-v4", dict(D=1), EINVAL), ("cctb-c3-v4", dict(null="head"), EINVAL), ("cctb-c3-v4", dict(B=0), EINVAL), ("cctb-c3-v4", dict(C=1), ERANGE),
    ("rot90-k1", dict(k=4), EINVAL), ("rot90-k1", dict(null="rot"), EINVAL), ("rot90-k0", dict(B=0), EINVAL), ("rot90-k2", dict(k=-1), EINVAL),
    ("rot-k1", dict(k=4), EINVAL), ("rot-k1", dict(r_b0=-1), EINVAL), ("rot-k1", dict(C=9), ERANGE), ("rot-k1", dict(short=True), EWORKSPACE),
    ("rotb-k1", dict(k=-1), EINVAL), ("rotb-k1", dict(null="du"), EINVAL), ("rotb-k1", dict(C=1), ERANGE), ("rotb-k1", dict(B=0), EINVAL),
    ("pair-outs6", dict(B=0), EINVAL), ("pair-outs6", dict(null="outs"), EINVAL), ("pair-outs6", dict(C=9), ERANGE), ("pair-outs6", dict(C=1), ERANGE),
    ("pair-outs6", dict(short=True), EWORKSPACE),
    ("mseb-c3", dict(null="g"), EINVAL), ("mseb-c3", dict(C=9), ERANGE), ("klb-c4", dict(null="a"), EINVAL), ("klb-c4", dict(C=1), ERANGE),
    ("klmapb-c2", dict(null="outs"), EINVAL), ("klmapb-c2", dict(null="g"), EINVAL), ("klmapb-c2", dict(C=9), ERANGE),
    ("ent-c2", dict(null="outs"), EINVAL), ("ent-c2", dict(B=0), EINVAL), ("ent-c2", dict(C=9), ERANGE), ("ent-c2", dict(short=True), EWORKSPACE)]


def test_refusals_leave_every_output_untouched(L):
    """Every refusal of include/uaps_hip.h with real buffers: the return code, and every output (the EMA's in-place tensors, the
    workspace) exactly as it was."""
    failed = []
    for cid, over, want in REFUSALS:
        c = R.BY_ID[cid]
        inp = R.inputs(c)
        rc, outs, ins = RUN[c.entry](L, c, inp, **over)
        torch.cuda.synchronize()
        if rc != want:
            failed.append((cid, over, f"returned {rc}, not {want}"))
        for k, b in list(outs.items()) + [("ws", ins.get("ws"))]:
            if b is None:
                continue
            h, ok = b.fetch()
            before = inp["t"][int(k[1:])]["e"] if c.entry == "ema" else None
            same = R.bits_differ(h.reshape(-1), before) == 0 if before is not None else bool(
                np.isnan(h).all() if h.dtype == F32 else (h == 0xEE).all())
            if not ok or not same:
                failed.append((cid, over, f"{k} was written"))
    assert not failed, failed


def test_refusal_table_reaches_every_entry_point():
    assert {R.BY_ID[cid].entry for cid, _, _ in REFUSALS} == set(R.ENTRIES)

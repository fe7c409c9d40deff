"""-m gpu: every kernel form of uaps_amd/csrc/perturb.hip, resample.hip, adam.hip and the residual joins of pair_ops.hip against the
references of tests/ops_ref.py, through the C ABI (explicit seed and offset; a step state only where the case sets one).

Every tensor is a view `off` floats into a buffer pre-filled with a sentinel: the floats in front of and behind every output must be
untouched after every launch, a second launch must give the same bits, and every refusal must leave the outputs untouched.  The
bit-exact quantities must match to the bit, the float64-compared ones stay under their derived bars, Adam under ops_ref.TAU_ADAM."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL, ERANGE, EWORKSPACE = 0, -1, -2, -3
GUARD = 16                                    # sentinel elements in front of and behind every view
SENT = {torch.float32: -12345.0, torch.uint8: 0xA5, torch.int64: -7}
BOUND_SLOTS, BOUND_STRIDE = 16, 64


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    lib = _lib.lib()
    prev = lib.uaps_get_step_state()
    lib.uaps_set_step_state(None)
    yield lib
    lib.uaps_set_step_state(prev)


def _stream():
    from uaps_amd import _lib
    return _lib.current_stream(torch.device(DEV))


def _hints(**kw):
    from uaps_amd import _lib
    return _lib.mk_hints(**kw)


class Buf:
    """A device tensor `off` elements into a sentinel-filled buffer, GUARD sentinels on both sides (the buffer is 256-byte aligned
    and GUARD elements keep 16 bytes, so off % 4 != 0 is what misaligns a float view)."""

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
        """(the view on the host, whether the sentinels around it are intact): one copy of the whole buffer."""
        h = self.buf.cpu().numpy()
        s = SENT[self.dtype]
        return h[self.lo:self.lo + self.n].reshape(self.shape).copy(), bool((h[:self.lo] == s).all() and (h[self.lo + self.n:] == s).all())

    def untouched(self) -> bool:
        return bool((self.buf == SENT[self.dtype]).all())


def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr if b is not None else None for b in bufs])


def _p(b):
    return None if b is None else b.ptr


def _bound(L, start: float = 0.0):
    """A zeroed bound, raised to `start` by a one-element uaps_cat2 (plain stores into a bound are not coherent with its atomics)."""
    b = torch.empty(BOUND_SLOTS * BOUND_STRIDE, dtype=torch.float32, device=DEV)
    assert L.uaps_zero_bounds(b.data_ptr(), b.numel(), _stream()) == OK
    if start:
        a, z, o = Buf(1, data=np.array([start], np.float32)), Buf(1, data=np.zeros(1, np.float32)), Buf(2)
        assert L.uaps_cat2_h(_hints(out_amax=b), a.ptr, z.ptr, o.ptr, 1, _stream()) == OK
    return b


def _bval(b) -> float:
    return float(b[::BOUND_STRIDE][:BOUND_SLOTS].max())


def _fdrop_ws(L, shape):
    n = C.c_size_t()
    assert L.uaps_feat_dropout_workspace_bytes(*shape, C.byref(n)) == OK
    return torch.full((n.value,), 0x5A, dtype=torch.uint8, device=DEV)


def _ws_stats(ws, B, HW):
    """(att [B, HW] float32, max [B] float32 decoded from the keys) of a FeatureDropout workspace."""
    torch.cuda.synchronize()
    h = ws.cpu().numpy()
    lo = ((4 * B + 255) // 256) * 256
    return h[lo:lo + 4 * B * HW].view(np.float32).reshape(B, HW).copy(), R.fkey_inv(h[:4 * B].view(np.uint32).copy())


class _State:
    """A step state for the duration of one launch: words 0-1 the key increment, words 12-13 Adam's two scalars."""

    def __init__(self, L, on: bool):
        self.L, self.on = L, on

    def __enter__(self):
        if self.on:
            w = np.zeros(R.STEP_WORDS, np.uint32)
            w[0], w[1] = R.STATE_KEY & 0xFFFFFFFF, R.STATE_KEY >> 32
            w[R.STEP_ADAM:R.STEP_ADAM + 2] = np.array(R.adam_scalars(R.ADAM_HYPER["lr"], R.ADAM_HYPER["b1"], R.ADAM_HYPER["b2"], 7),
                                                      np.float32).view(np.uint32)
            self.t = torch.from_numpy(w.view(np.int32)).to(DEV)
            torch.cuda.synchronize()
            assert self.L.uaps_set_step_state(self.t.data_ptr()) == OK
        return self

    def __exit__(self, *a):
        if self.on:
            torch.cuda.synchronize()
            assert self.L.uaps_set_step_state(None) == OK


# ---- one runner per entry-point family: (rc, outputs as name -> Buf, extra host results, failed checks) ------------------------------
def run_noise(L, c, inp):
    B, Cc, H, W = c.shape
    x, y = Buf(c.shape, c.offx, inp["x"]), Buf(c.shape, c.offy)
    if c.entry == "noise":
        n = Buf(Cc * H * W, c.offn) if c.noise_out else None
        rc = L.uaps_feat_noise(x.ptr, y.ptr, B, Cc, H, W, c.seed, c.offset, c.range, _p(n), _stream())
        return rc, (dict(y=y, noise=n) if n is not None else dict(y=y)), {}, []
    n = Buf(Cc * H * W, c.offn, inp["noise"])
    return L.uaps_feat_noise_apply(x.ptr, n.ptr, y.ptr, B, Cc * H * W, _stream()), dict(y=y), {}, []


def run_bernoulli(L, c, inp, p=None):
    x, y = Buf(c.n, c.offx, inp["x"]), Buf(c.n, c.offy)
    k = Buf(c.n, c.offk, dtype=torch.uint8) if c.keep else None
    rc = L.uaps_feat_bernoulli(x.ptr, y.ptr, c.n, c.seed, c.offset, c.p if p is None else p, _p(k), _stream())
    bad = []
    torch.cuda.synchronize()
    if rc == OK and c.p == 0.0 and R.bits_differ(y.fetch()[0], inp["x"]):
        bad.append("p = 0: y is not x bit for bit")
    return rc, (dict(y=y, keep=k) if k is not None else dict(y=y)), {}, bad


def run_mask_apply(L, c, inp):
    x, k, y = Buf(c.n, 0, inp["x"]), Buf(c.n, 0, inp["keep"], torch.uint8), Buf(c.n)
    return L.uaps_feat_mask_apply(x.ptr, k.ptr, float(inp["scale"]), y.ptr, c.n, _stream()), dict(y=y), {}, []


def run_fdrop(L, c, inp):
    B, Cc, H, W = c.shape
    x, y = Buf(c.shape, c.offx, inp["x"]), Buf(c.shape, c.offy)
    keep = Buf((B, H * W), c.offk, dtype=torch.uint8)
    ws = _fdrop_ws(L, c.shape)
    rc = L.uaps_feat_dropout_fwd(x.ptr, y.ptr, B, Cc, H, W, c.u, keep.ptr, ws.data_ptr(), ws.numel(), _stream())
    if rc != OK:
        return rc, dict(y=y, keep=keep), {}, []
    att, mx = _ws_stats(ws, B, H * W)
    del x
    dy, dx = Buf(c.shape, c.offx, inp["dy"]), Buf(c.shape, c.offy)
    rc = L.uaps_feat_dropout_bwd(dy.ptr, keep.ptr, dx.ptr, B, Cc, H, W, _stream())
    return rc, dict(y=y, keep=keep, dx=dx), dict(att=att, max=mx), []


def run_fdrop_stats(L, c, inp):
    B, Cc, H, W = c.shape
    x = Buf(c.shape, c.offx, inp["x"])
    ws = _fdrop_ws(L, c.shape)
    rc = L.uaps_feat_dropout_stats(x.ptr, B, Cc, H, W, ws.data_ptr(), ws.numel(), _stream())
    att, mx = _ws_stats(ws, B, H * W)
    return rc, {}, dict(att=att, max=mx, att64=att), []


def run_fanout(L, c, inp):
    B, Cc, H, W = c.shape
    n, G = len(c.modes), c.groups
    x = Buf(c.shape, 0, inp["x"])
    outs = [Buf(c.shape) for _ in range(n)]
    keeps = [Buf((B, H * W), dtype=torch.uint8) if m == 3 else None for m in c.modes]
    ws = None
    with _State(L, c.state):
        if 3 in c.modes:
            ws = _fdrop_ws(L, c.shape)
            assert L.uaps_feat_dropout_stats(x.ptr, B, Cc, H, W, ws.data_ptr(), ws.numel(), _stream()) == OK
        offs = (C.c_uint64 * (n * G))(*[o for row in R.fan_offsets(c) for o in row])
        rc = L.uaps_fanout_perturbed(x.ptr, _ptrs(outs), (C.c_int * n)(*c.modes), _ptrs(keeps), offs, (C.c_float * G)(*c.u),
                                     ws.data_ptr() if ws is not None else None, n, G, c.seed, c.range, c.p, B, Cc, H, W, _stream())
    d = {f"out{k}": outs[k] for k in range(n)}
    d.update({f"keep{k}": keeps[k] for k in range(n) if keeps[k] is not None})
    return rc, d, {}, []


def run_fanin(L, c, inp):
    B, Cc, H, W = c.shape
    n, G = len(c.modes), c.groups
    gs = [Buf(g.shape, 0, g) for g in inp["g"]]
    keeps, idx, bad = [], {}, []
    for k, m in enumerate(c.modes):
        if m == 4 and W % 8 == 0:                   # the index bytes the max-pool kernel wrote
            px, po, pi = Buf(c.shape, 0, inp["poolx"][k]), Buf((B, Cc, H // 2, W // 2)), Buf((B, Cc, H // 2, W // 2), dtype=torch.uint8)
            assert L.uaps_maxpool2x2_fwd(px.ptr, B, Cc, H, W, po.ptr, pi.ptr, _stream()) == OK
            torch.cuda.synchronize()
            idx[k] = pi.fetch()[0]
            if R.bits_differ(idx[k], R.maxpool2x2(inp["poolx"][k])[1]):
                bad.append(f"max-pool index bytes of position {k} differ from the host reference")
            keeps.append(pi)
        elif m == 4:                                # W % 8 != 0: the max-pool kernel has no form, the host reference's bytes
            keeps.append(Buf((B, Cc, H // 2, W // 2), 0, R.maxpool2x2(inp["poolx"][k])[1], torch.uint8))
        else:
            keeps.append(Buf((B, H * W), 0, inp["keep"][k], torch.uint8) if m == 3 else None)
    out = Buf(c.shape)
    offs = (C.c_uint64 * (n * G))(*[o for row in R.fan_offsets(c) for o in row])
    with _State(L, c.state):
        rc = L.uaps_fanin_perturbed(_ptrs(gs), (C.c_int * n)(*c.modes), _ptrs(keeps), offs, n, G, c.seed, c.range, c.p, B, Cc, H, W,
                                    out.ptr, _stream())
    return rc, dict(out=out), dict(aux=dict(idx=idx)), bad


def run_maxpool(L, c, inp):
    B, Cc, H, W = c.shape
    x, out, idx = Buf(c.shape, 0, inp["x"]), Buf((B, Cc, H // 2, W // 2)), Buf((B, Cc, H // 2, W // 2), dtype=torch.uint8)
    rc = L.uaps_maxpool2x2_fwd(x.ptr, B, Cc, H, W, out.ptr, idx.ptr, _stream())
    bad = []
    if rc == OK:                                    # torch on the CPU: the flat index of the plane -> dy * 2 + dx
        torch.cuda.synchronize()
        to, ti = F.max_pool2d(torch.from_numpy(inp["x"]), 2, return_indices=True)
        ti = ((ti // W) % 2 * 2 + (ti % W) % 2).to(torch.uint8).numpy()
        if R.bits_differ(out.fetch()[0], to.numpy()) or R.bits_differ(idx.fetch()[0], ti):
            bad.append("differs from torch.nn.functional.max_pool2d(return_indices=True)")
    return rc, dict(out=out, idx=idx), {}, bad


def _off(c, i):
    return c.offs_in[i] if i < len(c.offs_in) else 0


def run_sum(L, c, inp):
    ins = [Buf(c.count, _off(c, i), t) for i, t in enumerate(inp["ins"])]
    out = ins[0] if c.alias else Buf(c.count, c.offo)
    rc = L.uaps_sum_tensors(_ptrs(ins), c.n, out.ptr, c.count, _stream())
    return rc, dict(out=out), {}, []


def run_confusion(L, c, inp):
    B, Cc, H, W = c.shape
    z, y = Buf(c.shape, 0, inp["z"]), Buf((B, H, W), 0, inp["y"], torch.int64)
    counts = Buf((Cc, Cc), dtype=torch.int64)
    return L.uaps_seg_confusion(z.ptr, y.ptr, B, Cc, H, W, counts.ptr, _stream()), dict(counts=counts), {}, []


def run_up_fwd(L, c, inp, amax_any=False):
    H, W = 2 * c.h, 2 * c.w
    skip = Buf((c.B, c.Cs, H, W), c.offs, inp["skip"]) if c.Cs else Buf(4, c.offs)
    low, out = Buf(inp["low"].shape, 0, inp["low"]), Buf((c.B, c.Cs + c.Cl, H, W), c.offo)
    amax = _bound(L, c.amax) if c.amax is not None else None
    rc = L.uaps_up_cat_fwd_h(_hints(out_amax=amax) if amax is not None else None, skip.ptr, low.ptr, out.ptr, c.B, c.Cs, c.Cl, c.h, c.w,
                             _stream())
    torch.cuda.synchronize()
    o, bad = out.fetch()[0], []
    if rc == OK and amax is not None and _bval(amax) != max(c.amax, float(np.abs(o).max())):
        bad.append(f"out_amax {_bval(amax)} != max(start {c.amax}, max|out| {float(np.abs(o).max())})")
    if rc != OK and amax is not None and _bval(amax) != c.amax:
        bad.append("a refused call raised out_amax")
    return rc, dict(out=out), dict(skip_part=o[:, :c.Cs], up_part=o[:, c.Cs:]), bad


def run_up_bwd(L, c, inp):
    H, W = 2 * c.h, 2 * c.w
    dout = Buf(inp["dout"].shape, c.offd, inp["dout"])
    dskip = Buf((c.B, c.Cs, H, W), c.offs) if c.dskip and c.Cs else None
    dlow = Buf((c.B, c.Cl, c.h, c.w))
    rc = L.uaps_up_cat_bwd(dout.ptr, _p(dskip), dlow.ptr, c.B, c.Cs, c.Cl, c.h, c.w, _stream())
    return rc, (dict(dlow=dlow, dskip=dskip) if dskip is not None else dict(dlow=dlow)), {}, []


def run_join(L, c, inp):
    e, n = c.entry, c.n
    amax = _bound(L, c.amax) if c.amax is not None else None
    h = _hints(out_amax=amax) if amax is not None else None
    if e == "add_relu":
        a, b, out = Buf(n, _off(c, 0), inp["a"]), Buf(n, _off(c, 1), inp["b"]), Buf(n, _off(c, 2))
        rc, d = L.uaps_add_relu_h(h, a.ptr, b.ptr, out.ptr, n, _stream()), dict(out=out)
    elif e == "cat2":
        a, b, out = Buf(n, _off(c, 0), inp["a"]), Buf(n, _off(c, 1), inp["b"]), Buf(2 * n, _off(c, 2))
        rc, d = L.uaps_cat2_h(h, a.ptr, b.ptr, out.ptr, n, _stream()), dict(out=out)
    elif e == "relu_bwd":
        g, o, dx = Buf(n, _off(c, 0), inp["a"]), Buf(n, _off(c, 1), inp["b"]), Buf(n, _off(c, 2))
        rc, d = L.uaps_relu_bwd(g.ptr, o.ptr, dx.ptr, n, _stream()), dict(dx=dx)
    else:
        gs = [Buf(n, _off(c, i), t) for i, t in enumerate(inp["gs"])]
        o, dx = Buf(n, _off(c, 4), inp["b"]), Buf(n, _off(c, 5))
        rc, d = L.uaps_relu_bwd_sum(_ptrs(gs), c.k, o.ptr, dx.ptr, n, _stream()), dict(dx=dx)
    torch.cuda.synchronize()
    return rc, d, (dict(amax=_bval(amax)) if amax is not None else {}), []


def run_adam(L, c, inp, step=None, null_at=None):
    ts = inp["t"]
    bufs = [{k: Buf(t[k].size, 1 if i in c.offs_in else 0, t[k]) for k in ("p", "g", "m", "v")} for i, t in enumerate(ts)]
    arr = {k: _ptrs([b[k] for b in bufs]) for k in ("p", "g", "m", "v")}
    if null_at is not None:
        arr["g"][null_at] = None
    numel = (C.c_long * len(ts))(*[t["p"].size for t in ts])
    h = R.ADAM_HYPER
    with _State(L, c.state):
        rc = L.uaps_adam_step(arr["p"], arr["g"], arr["m"], arr["v"], numel, len(ts), h["lr"], h["b1"], h["b2"], h["eps"], c.wd,
                              c.step if step is None else step, _stream())
        torch.cuda.synchronize()
    outs = {f"{k}{i}": b[k] for i, b in enumerate(bufs) for k in ("p", "m", "v")}
    got, guards = [], True
    for b in bufs:
        t = {}
        for k in ("p", "m", "v"):
            t[k], ok = b[k].fetch()
            guards = guards and ok
        got.append(t)
    extra = dict(adam=got)
    if c.special == "zero":
        extra["p0"] = got[0]["p"]
    return rc, outs, extra, ([] if guards else ["a guard float around an Adam tensor was written"])


RUN = dict(noise=run_noise, noise_apply=run_noise, bernoulli=run_bernoulli, mask_apply=run_mask_apply, fdrop=run_fdrop,
           fdrop_stats=run_fdrop_stats, fanout=run_fanout, fanin=run_fanin, maxpool=run_maxpool, sum=run_sum, confusion=run_confusion,
           up_fwd=run_up_fwd, up_bwd=run_up_bwd, add_relu=run_join, relu_bwd=run_join, relu_bwd_sum=run_join, cat2=run_join,
           adam=run_adam)


def _launch(L, c, inp):
    """One launch on fresh buffers: (outputs on the host, aux for the reference, failed checks)."""
    rc, outs, extra, bad = RUN[c.entry](L, c, inp)
    assert rc == OK, rc
    torch.cuda.synchronize()
    got = {}
    if c.entry != "adam":                          # (run_adam fetched its 3 x n tensors and their guards itself)
        for k, b in outs.items():
            got[k], ok = b.fetch()
            if not ok:
                bad.append(f"the sentinels around {k} were written")
    aux = extra.pop("aux", None)
    got.update(extra)
    if "out" in got and c.entry == "up_fwd":
        del got["out"]
    return got, aux, bad


def _same(a, b) -> bool:
    if isinstance(a, list):
        return all(_same(x[k], y[k]) for x, y in zip(a, b) for k in x)
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def run_case(L, c):
    """(the ratio of every float64-compared quantity to its bar, the failed checks) of one case."""
    inp = R.inputs(c)
    got, aux, bad = _launch(L, c, inp)
    ratios, bad2 = R.compare(R.reference(c, inp, aux=aux), got)
    again, _, _ = _launch(L, c, inp)
    bad3 = [f"second launch differs in {k}" for k in got if not _same(got[k], again[k])]
    return ratios, bad + bad2 + bad3


def _ids(entry):
    return [c.id for c in R.CASES if c.entry in entry]


def _check(L, cid):
    try:
        ratios, bad = run_case(L, R.BY_ID[cid])
    except RuntimeError as e:                      # a HIP error is sticky: launch nothing more on a device that has faulted
        if "hip" in str(e).lower():
            pytest.exit(f"{cid}: {e}", returncode=3)
        raise
    print(cid, " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())) or "bit-exact")
    assert not bad, bad


@pytest.mark.parametrize("cid", _ids(("noise", "noise_apply")))
def test_feature_noise(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("bernoulli", "mask_apply")))
def test_dropout(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("fdrop",)))
def test_feature_dropout(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("fdrop_stats",)))
def test_feature_dropout_stats(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("fanout",)))
def test_fanout_perturbed(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("fanin",)))
def test_fanin_perturbed(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("maxpool",)))
def test_maxpool2x2(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("sum",)))
def test_sum_tensors(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("confusion",)))
def test_seg_confusion(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("up_fwd",)))
def test_up_cat_fwd(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("up_bwd",)))
def test_up_cat_bwd(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("add_relu", "relu_bwd", "relu_bwd_sum", "cat2")))
def test_joins(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", _ids(("adam",)))
def test_adam_step(L, cid):
    _check(L, cid)


# ---- refusals: nothing launched, nothing written -----------------------------------------------------------------------------------
def _refused(rc, outs, want):
    torch.cuda.synchronize()
    assert rc == want, rc
    wrote = [k for k, b in outs.items() if b is not None and not b.untouched()]
    assert not wrote, f"a refused call wrote {wrote}"


@pytest.mark.parametrize("p", [-0.1, 1.0, float("nan")])
def test_dropout_refuses_p(L, p):
    c = R.Case("refuse-bern", "bernoulli", n=9)
    rc, outs, _, _ = run_bernoulli(L, c, R.inputs(c), p=p)
    _refused(rc, outs, EINVAL)


def _fan_refusal_case(kind, **kw):
    p = dict(shape=(4, 3, 4, 4), modes=(1, 2, 3) if kind == "fanout" else (1, 2, 3, 4), groups=2, u=(0.8, 0.8))
    p.update(kw)
    return R.Case("refuse-" + kind, kind, **p)


@pytest.mark.parametrize("kw", [dict(shape=(4, 3, 3, 3)), dict(groups=5, shape=(5, 3, 4, 4), u=(0.8,) * 5), dict(modes=(1,) * 9),
                                dict(groups=3, u=(0.8,) * 3)])
def test_fanout_refuses(L, kw):
    c = _fan_refusal_case("fanout", **kw)
    rc, outs, _, _ = run_fanout(L, c, R.inputs(c))
    _refused(rc, outs, EINVAL)


@pytest.mark.parametrize("which", ["f", "out", "keep", "ws"])
def test_fanout_refuses_misaligned(L, which):
    """f, an output, a keep mask (4 bytes) or the statistics workspace (16 bytes: the attention map is read as float4)."""
    c = _fan_refusal_case("fanout")
    B, Cc, H, W = c.shape
    inp = R.inputs(c)
    x = Buf(c.shape, int(which == "f"), inp["x"])
    outs = [Buf(c.shape, int(which == "out" and k == 1)) for k in range(3)]
    keep = Buf((B, H * W), int(which == "keep"), dtype=torch.uint8)
    ws = _fdrop_ws(L, c.shape)
    xa = Buf(c.shape, 0, inp["x"])
    assert L.uaps_feat_dropout_stats(xa.ptr, B, Cc, H, W, ws.data_ptr(), ws.numel(), _stream()) == OK
    big = torch.empty(ws.numel() + 16, dtype=torch.uint8, device=DEV)
    wsp = big[4:].data_ptr() if which == "ws" else ws.data_ptr()
    offs = (C.c_uint64 * 6)(*range(6))
    rc = L.uaps_fanout_perturbed(x.ptr, _ptrs(outs), (C.c_int * 3)(1, 2, 3), _ptrs([None, None, keep]), offs, (C.c_float * 2)(0.8, 0.8),
                                 wsp, 3, 2, 1, 0.3, 0.3, B, Cc, H, W, _stream())
    _refused(rc, dict(out0=outs[0], out1=outs[1], out2=outs[2], keep=keep), EINVAL)


@pytest.mark.parametrize("entry", ["fwd", "stats"])
@pytest.mark.parametrize("how,want", [("misaligned", EINVAL), ("short", EWORKSPACE)])
def test_feature_dropout_refuses_workspace(L, entry, how, want):
    """A workspace that is not 16-byte aligned (include/uaps_hip.h) or too small: nothing is written, the workspace included."""
    shape = (2, 3, 4, 8)
    B, Cc, H, W = shape
    x, y, keep = Buf(shape, 0, np.ones(shape, np.float32)), Buf(shape), Buf((B, H * W), dtype=torch.uint8)
    ws = Buf(_fdrop_ws(L, shape).numel(), 4 if how == "misaligned" else 0, dtype=torch.uint8)
    nbytes = ws.n - (1 if how == "short" else 0)
    if entry == "fwd":
        rc = L.uaps_feat_dropout_fwd(x.ptr, y.ptr, B, Cc, H, W, 0.8, keep.ptr, ws.ptr, nbytes, _stream())
    else:
        rc = L.uaps_feat_dropout_stats(x.ptr, B, Cc, H, W, ws.ptr, nbytes, _stream())
    _refused(rc, dict(y=y, keep=keep, ws=ws), want)


@pytest.mark.parametrize("kw", [dict(shape=(4, 3, 3, 4), modes=(0, 4)), dict(shape=(4, 3, 4, 6), modes=(0, 4)), dict(shape=(4, 3, 3, 3), modes=(0,)),
                                dict(groups=5, shape=(5, 3, 4, 4), modes=(0, 1)), dict(modes=(0,) * 9), dict(groups=3, modes=(0, 1))])
def test_fanin_refuses(L, kw):
    """Mode 4 with H odd or W % 4, H * W % 4, groups = 5, n = 9, B % groups."""
    c = _fan_refusal_case("fanin", **kw)
    B, Cc, H, W = c.shape
    n = len(c.modes)
    gs = [Buf(c.shape, 0, np.ones(c.shape, np.float32)) for _ in range(n)]
    keeps = [Buf(B * Cc * H * W, dtype=torch.uint8) if m >= 3 else None for m in c.modes]
    out = Buf(c.shape)
    offs = (C.c_uint64 * (n * c.groups))()
    rc = L.uaps_fanin_perturbed(_ptrs(gs), (C.c_int * n)(*c.modes), _ptrs(keeps), offs, n, c.groups, 1, 0.3, 0.3, B, Cc, H, W, out.ptr, _stream())
    _refused(rc, dict(out=out), EINVAL)


@pytest.mark.parametrize("which", ["g", "out", "keep"])
def test_fanin_refuses_misaligned(L, which):
    shape = (2, 3, 4, 4)
    gs = [Buf(shape, int(which == "g" and k == 1), np.ones(shape, np.float32)) for k in range(2)]
    keep = Buf((2, 16), int(which == "keep"), np.ones((2, 16), np.uint8), torch.uint8)
    out = Buf(shape, int(which == "out"))
    rc = L.uaps_fanin_perturbed(_ptrs(gs), (C.c_int * 2)(0, 3), _ptrs([None, keep]), (C.c_uint64 * 2)(), 2, 1, 1, 0.3, 0.3, 2, 3, 4, 4, out.ptr,
                                _stream())
    _refused(rc, dict(out=out), EINVAL)


@pytest.mark.parametrize("shape,offs", [((1, 2, 3, 8), (0, 0, 0)), ((1, 2, 4, 12), (0, 0, 0)), ((1, 2, 4, 8), (1, 0, 0)), ((1, 2, 4, 8), (0, 1, 0)),
                                        ((1, 2, 4, 8), (0, 0, 1))])
def test_maxpool_refuses(L, shape, offs):
    """H odd, W % 8, a misaligned x / out (16 bytes) / idx (4 bytes)."""
    B, Cc, H, W = shape
    x = Buf(shape, offs[0], np.ones(shape, np.float32))
    out, idx = Buf((B, Cc, H // 2, W // 2), offs[1]), Buf((B, Cc, H // 2, W // 2), offs[2], dtype=torch.uint8)
    _refused(L.uaps_maxpool2x2_fwd(x.ptr, B, Cc, H, W, out.ptr, idx.ptr, _stream()), dict(out=out, idx=idx), EINVAL)


@pytest.mark.parametrize("n", [0, 5])
def test_sum_refuses(L, n):
    ins = [Buf(8, 0, np.ones(8, np.float32)) for _ in range(5)]
    out = Buf(8)
    _refused(L.uaps_sum_tensors(_ptrs(ins), n, out.ptr, 8, _stream()), dict(out=out), EINVAL)


@pytest.mark.parametrize("Cc", [0, R.MAX_CLASSES + 1])
def test_confusion_refuses(L, Cc):
    z, y = Buf((1, 9, 2, 2), 0, np.ones((1, 9, 2, 2), np.float32)), Buf((1, 2, 2), 0, np.zeros((1, 2, 2), np.int64), torch.int64)
    counts = Buf((9, 9), dtype=torch.int64)
    _refused(L.uaps_seg_confusion(z.ptr, y.ptr, 1, Cc, 2, 2, counts.ptr, _stream()), dict(counts=counts), ERANGE)


@pytest.mark.parametrize("kw", [dict(Cs=2, Cl=2, h=4, w=4), dict(Cs=0, Cl=2, h=4, w=3), dict(Cs=0, Cl=2, h=4, w=4, offo=1)])
def test_up_cat_fwd_refuses_amax_outside_the_tiled_form(L, kw):
    """out_amax is tracked by the plain up-sampling (Cs = 0, W % 4 == 0, aligned out) alone: UAPS_ERANGE elsewhere."""
    c = R.Case("refuse-up", "up_fwd", B=1, amax=0.5, **kw)
    rc, outs, _, bad = run_up_fwd(L, c, R.inputs(c))
    _refused(rc, outs, ERANGE)
    assert not bad, bad


def test_adam_refuses_step_below_one_without_state(L):
    c = R.Case("refuse-adam", "adam", numels=(5, 7))
    rc, outs, _, _ = run_adam(L, c, R.inputs(c), step=0)
    assert rc == EINVAL, rc
    wrote = [k for k, b in outs.items() if R.bits_differ(b.fetch()[0], R.inputs(c)["t"][int(k[1:])][k[0]])]
    assert not wrote, wrote


def test_adam_refuses_before_the_first_launch(L):
    """A NULL gradient in the second batch of 48: no tensor of the first batch may have been stepped."""
    c = R.Case("refuse-adam-50", "adam", numels=(3,) * 50)
    inp = R.inputs(c)
    rc, outs, _, _ = run_adam(L, c, inp, null_at=49)
    assert rc == EINVAL, rc
    wrote = [k for k, b in outs.items() if R.bits_differ(b.fetch()[0], inp["t"][int(k[1:])][k[0]])]
    assert not wrote, wrote

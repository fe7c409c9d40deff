"""The loss block (uaps_amd/csrc/loss_kernels.hpp and its launchers): the case table, a float64 reference, the conditioning of every
compared quantity and the bars (tests/test_loss_form_table.py on the CPU, tests/test_gpu_loss_forms.py on the GPU).

Reference: oracle.uaps_oracle (loss_sums -> loss_from_sums, unsupervised_terms) on float64 tensors with autograd.  The reductions and
gradients are taken with the pseudo-labels the caller passes (the kernel's own on the GPU), so a pixel whose two best mixed
probabilities tie within fp32 cannot pollute them; the pseudo-labels themselves are held exactly wherever the float64 margin is
at least MARGIN.

Every case names the kernel form it must take, from a restatement of the launchers' rules (loss_dispatch.hpp: pair_vec_ok, vec_ok,
unsup_vec): the pair kernels run <VS = 4, VU = unsup_vec(D, C)> when H*W % 4 == 0 and every pointer is 16-byte aligned and <1, 1>
otherwise; the two-branch kernels run V = unsup_vec(D, C) (unsupervised) / 4 (supervised) pixels wide under the same kind of
condition and one pixel wide otherwise.

Conditioning: an fp32 probability p = exp(z - max) / sum carries a relative error of about (1 + |log p|) ulp, so the magnitude that
stands for p in every bound below is pt = p (1 + |log p|).  A gradient element's conditioning is the sum of the magnitudes of its
terms in the closed form the kernels evaluate, restated here as closed_form_grads(); a scalar's is the same
arithmetic as its value with every difference replaced by a sum of magnitudes.
"""
from __future__ import annotations

import contextlib
import math
import zlib
from dataclasses import dataclass, replace

import numpy as np
import torch

from oracle import uaps_oracle as O

THREADS = 256                # kThreads
EPS = float(np.float32(1e-7))
MARGIN = 1e-5                # pseudo-labels are held exactly where the float64 top-two margin of the mixed probabilities is >= this
TIE_SHARE = 1e-3             # at most this share of a case's pixels may fall below MARGIN (planted ties apart)
BOUND_SLOTS, BOUND_STRIDE = 16, 64
BOUND_FLOATS = BOUND_SLOTS * BOUND_STRIDE
PAIR, TWO_BRANCH, SUMS = "pair", "two_branch", "sums"
VEC_SHAPE, SCALAR_SHAPE, V2_SHAPE = (3, 20, 36), (3, 13, 17), (5, 9, 14)
ALL_DC = [(D, C) for D in range(1, 9) for C in range(2, 9)]
EXTRA_DC = [(4, 4), (6, 2), (3, 5), (8, 8), (1, 2)]


def unsup_vec(D: int, C: int) -> int:
    return 4 if D * C <= 16 else (2 if D * C <= 32 else 1)


# ---- scalar block layouts (include/uaps_hip.h) ---------------------------------------------------------------------------------
def u_layout(D, C):
    b = 4 * D + 4
    return dict(ce=(0, D), dice=(D, D), s=(2 * D, D), E=(3 * D, D), ps_loss=(4 * D, 1), l_uncert=(4 * D + 1, 1), loss=(4 * D + 2, 1),
                total=(4 * D + 3, 1), a1=(b, D * C), a2=(b + D * C, D * C), I=(b + 2 * D * C, D * C), card=(b + 3 * D * C, D * C),
                cnt=(b + 4 * D * C, C), n=b + 4 * D * C + C)


def s_layout(D, C):
    b = 2 * D + 2
    return dict(ce=(0, D), dice=(D, D), sup=(2 * D, 1), bad=(2 * D + 1, 1), a1=(b, D * C), a2=(b + D * C, D * C), I=(b + 2 * D * C, D * C),
                card=(b + 3 * D * C, D * C), cnt=(b + 4 * D * C, C), n=b + 4 * D * C + C)


def n_sums(D, C):
    """(supervised, unsupervised) raw sums of sums_out: CE[D] | I[D*C] | P[D*C] | cnt[C] | bad, then the same | E[D] | V[D]."""
    return D + 2 * D * C + C + 1, D + 2 * D * C + C + 2 * D


def slot(block, layout, name):
    o, n = layout[name]
    return np.asarray(block)[o:o + n]


# ---- the case table -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    entry: str                   # PAIR, TWO_BRANCH or SUMS (the pair forward with sums_out, uaps_pairloss_finalize_sums, the pair backward)
    D: int
    B: int
    C: int
    H: int
    W: int
    off: int = 0                 # floats by which head 0's logits and gradient outputs are moved off 16-byte alignment
    lab_off: int = 0             # int64 elements by which labels / pseudo are moved
    cfg: int = 0                 # (supervised block cap << 16) | unsupervised block cap
    track: bool = False          # uaps_call_hints::out_amax on the pair backward
    gscale: object = 1.0         # the upstream gradient (a device scalar); None: a NULL pointer
    nloss_mult: int = 1          # SUMS: the sums are multiplied by this (as many equal ranks), finalised and differentiated with mult * N
    state: bool = False          # mixing weights and cw1 / cw2 from the step state (w_host = NULL, cw passed as NaN)
    want_var: bool = True
    logit_scale: float = 1.0
    planted: str = ""            # "zero": pixels whose fp32 probabilities underflow to 0; "ties": exact two-class ties
    bad_labels: bool = False     # labels of -1, C, 255 and five values no int holds on a few pixels (the supervised half is then not compared, only finite)
    seed_id: str = ""            # cases that must agree bit for bit share their data: seeded from this instead of the id

    @property
    def HW(self):
        return self.H * self.W

    @property
    def N(self):
        return self.B * self.HW

    @property
    def aligned(self) -> bool:
        return self.off % 4 == 0 and self.lab_off % 2 == 0

    @property
    def form_sup(self) -> str:
        if self.entry == TWO_BRANCH:
            return "vec4" if self.HW % 4 == 0 and self.aligned else "scalar"
        return "vec4" if self.HW % 4 == 0 and self.aligned else "scalar"

    @property
    def form(self) -> str:
        """The unsupervised half (the pair kernels' VU; the two-branch kernels' V)."""
        V = unsup_vec(self.D, self.C)
        if self.entry == TWO_BRANCH:
            return f"vec{V}" if V > 1 and self.HW % V == 0 and self.aligned else "scalar"
        if self.form_sup == "scalar":
            return "scalar"
        return f"vec{V}" if V > 1 else "scalar"

    @property
    def kernels(self) -> tuple:
        """The instantiations the launchers pick, as a demangler prints them."""
        D, C = self.D, self.C
        vs = 4 if self.form_sup == "vec4" else 1
        vu = 1 if self.form == "scalar" else int(self.form[3:])
        if self.entry == TWO_BRANCH:
            return (f"unsup_fwd_kernel<{D}, {C}, {vu}>", f"unsup_bwd_kernel<{D}, {C}, {vu}>", f"sup_fwd_kernel<{D}, {C}, {vs}>",
                    f"sup_bwd_kernel<{D}, {C}, {vs}>")
        return (f"pair_fwd_kernel<{D}, {C}, {vs}, {vu}, false, false, 2>",
                f"pair_bwd_kernel<{D}, {C}, {vs}, {vu}, true>")           # one instantiation, with and without out_amax

    def blocks(self, v: int) -> int:
        return -(-(self.N // v) // THREADS)


def _pair_group(D, C):
    """Vector and scalar shape, each with and without out_amax; the two runs of a shape share their data."""
    i = ALL_DC.index((D, C))
    out = []
    for j, (name, (B, H, W)) in enumerate((("vec", VEC_SHAPE), ("scalar", SCALAR_SHAPE))):
        base = f"pair-{D}x{C}-{name}"
        for track in (True, False):
            out.append(Case(f"{base}-{'track' if track else 'plain'}", PAIR, D, B, C, H, W, track=track, want_var=(i + j) % 2 == 0, seed_id=base))
    return out


def _two_branch_group(D, C):
    out = [Case(f"two-{D}x{C}-vec", TWO_BRANCH, D, *VEC_SHAPE[:1], C, *VEC_SHAPE[1:]),
           Case(f"two-{D}x{C}-scalar", TWO_BRANCH, D, *SCALAR_SHAPE[:1], C, *SCALAR_SHAPE[1:])]
    if 16 < D * C <= 32:
        out.append(Case(f"two-{D}x{C}-v2", TWO_BRANCH, D, *V2_SHAPE[:1], C, *V2_SHAPE[1:]))
    return out


def _extras(D, C):
    B, H, W = VEC_SHAPE
    n = f"x-{D}x{C}"
    base = Case(f"{n}-base", PAIR, D, B, C, H, W, track=True, seed_id=f"{n}-base")
    cs = [base,
          replace(base, id=f"{n}-cfg1x1", cfg=(1 << 16) | 1),
          replace(base, id=f"{n}-cfg2x3", cfg=(2 << 16) | 3),
          replace(base, id=f"{n}-gscale-null", gscale=None),
          replace(base, id=f"{n}-state", state=True),
          Case(f"{n}-off1", PAIR, D, B, C, H, W, off=1, track=True),
          Case(f"{n}-laboff1", PAIR, D, B, C, H, W, lab_off=1),
          Case(f"{n}-gscale0.37", PAIR, D, B, C, H, W, gscale=0.37, track=True),
          Case(f"{n}-gscale-2", PAIR, D, B, C, H, W, gscale=-2.0),
          Case(f"{n}-nloss2", SUMS, D, B, C, H, W, nloss_mult=2),
          Case(f"{n}-sums", SUMS, D, *SCALAR_SHAPE[:1], C, *SCALAR_SHAPE[1:]),
          Case(f"{n}-scale30", PAIR, D, B, C, H, W, logit_scale=30.0, planted="zero", track=True),
          Case(f"{n}-scale30-scalar", PAIR, D, *SCALAR_SHAPE[:1], C, *SCALAR_SHAPE[1:], logit_scale=30.0, planted="zero"),
          Case(f"{n}-ties", PAIR, D, B, C, H, W, planted="ties"),
          Case(f"{n}-ties-scalar", PAIR, D, *SCALAR_SHAPE[:1], C, *SCALAR_SHAPE[1:], planted="ties", want_var=False),
          Case(f"{n}-badlabels", PAIR, D, B, C, H, W, bad_labels=True),
          Case(f"{n}-badlabels-scalar", PAIR, D, *SCALAR_SHAPE[:1], C, *SCALAR_SHAPE[1:], bad_labels=True, track=True),
          Case(f"{n}-tiny-2x1x1", PAIR, D, 2, C, 1, 1, track=True),
          Case(f"{n}-tiny-1x1x4", PAIR, D, 1, C, 1, 4, track=True),
          Case(f"{n}-b1", PAIR, D, 1, C, H, W)]
    return cs


PAIR_GROUPS = {dc: _pair_group(*dc) for dc in ALL_DC}
TWO_GROUPS = {dc: _two_branch_group(*dc) for dc in ALL_DC}
EXTRA_GROUPS = {dc: _extras(*dc) for dc in EXTRA_DC}
CASES = [c for g in (PAIR_GROUPS, TWO_GROUPS, EXTRA_GROUPS) for cs in g.values() for c in cs]
BY_ID = {c.id: c for c in CASES}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def rng_for(case_id: str, salt: int = 0) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(case_id.encode()) * 1009 + salt)          # the same data in every process


def inputs(case: Case) -> dict:
    """Host data: lab / un logits [D][B, C, H, W] fp32, labels [B, H, W] int64, the Dirichlet mixing weights w (float64), cw1 / cw2
    (fp32 values), the planted pixels (flat indices into B*H*W) and, for planted ties, the lower of the two tied classes."""
    rng = rng_for(case.seed_id or case.id)
    D, B, C, H, W = case.D, case.B, case.C, case.H, case.W
    sc = 2.0 * case.logit_scale
    lab = [(rng.standard_normal((B, C, H, W)) * sc).astype(np.float32) for _ in range(D)]
    un = [(rng.standard_normal((B, C, H, W)) * sc).astype(np.float32) for _ in range(D)]
    labels = rng.integers(0, C, (B, H, W)).astype(np.int64)
    w = rng.dirichlet(np.ones(D))
    cw1, cw2 = (float(np.float32(v)) for v in rng.uniform(0.03, 0.2, 2))
    d = dict(lab=lab, un=un, labels=labels, w=w, cw1=cw1, cw2=cw2, planted=np.zeros(0, np.int64), tie_class=np.zeros(0, np.int64), n_bad=0)
    N, HW = case.N, case.HW

    def put(arrs, pix, vals):                       # vals [D, npix, C] -> the logits of pixel pix of every head
        b, hw = pix // HW, pix % HW
        for k, a in enumerate(arrs):
            a.reshape(B, C, HW)[b, :, hw] = vals[k]

    if case.planted == "zero":
        # one class ahead of all others by 200 (fp32 probabilities exactly 0) or by 95 (denormal) in every head
        pix = rng.choice(N, size=min(N, 32), replace=False)
        win = rng.integers(0, C, pix.size)
        half = np.where(np.arange(pix.size) % 2 == 0, 100.0, 47.5)
        vals = -half[None, :, None] * np.ones((D, pix.size, C))
        vals[:, np.arange(pix.size), win] = half[None]
        put(lab, pix, vals.astype(np.float32))
        put(un, pix, vals.astype(np.float32))
        d["planted"] = np.sort(pix)
    elif case.planted == "ties":
        # two classes with identical logits in every head, the rest at least 6 below
        pix = np.sort(rng.choice(N, size=min(N, 24), replace=False))
        ab = np.stack([np.sort(rng.choice(C, 2, replace=False)) for _ in range(pix.size)])
        top = rng.uniform(1.0, 4.0, (D, pix.size)).astype(np.float32)
        vals = top[..., None] - 6.0 - np.abs(rng.standard_normal((D, pix.size, C)))
        for j in range(pix.size):
            vals[:, j, ab[j, 0]] = top[:, j]
            vals[:, j, ab[j, 1]] = top[:, j]
        put(un, pix, vals.astype(np.float32))
        d["planted"], d["tie_class"] = pix, ab[:, 0].astype(np.int64)
    # no chance ties: a pixel whose float64 top-two margin of the mixed probabilities is below 10 MARGIN gets new logits
    for _ in range(8):
        _, margin = margin_and_argmax(d)
        close = margin.reshape(-1) < 10 * MARGIN
        if case.planted == "ties":
            close[d["planted"]] = False
        if not close.any():
            break
        pix = np.nonzero(close)[0]
        put(un, pix, (rng.standard_normal((D, pix.size, C)) * sc).astype(np.float32))
    if case.bad_labels:
        pix = rng.choice(N, size=min(N, 16), replace=False)     # the last five fit no int: narrowed, three of them would be classes 1, 1, 0
        labels.reshape(-1)[pix] = np.resize(np.array([-1, C, 255, 2 ** 31, 2 ** 32 + 1, -2 ** 32 + 1, -2 ** 63, 2 ** 63 - 1], np.int64), pix.size)
        d["n_bad"] = int(pix.size)
    return d


# ---- the float64 reference ------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _fixed_pseudo(pseudo):
    """Inside: the oracle's pseudo-label is `pseudo` (the mixed probabilities stay its own)."""
    if pseudo is None:
        yield
        return
    real = O.mix_pseudo_label

    def fixed(probs, w):
        r = real(probs, w)
        r["pseudo"] = torch.as_tensor(np.asarray(pseudo), dtype=torch.long)
        return r
    O.mix_pseudo_label = fixed
    try:
        yield
    finally:
        O.mix_pseudo_label = real


def _softmax64(z):
    z = np.asarray(z, np.float64)
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(1, keepdims=True)
    lse = mx + np.log(s)
    return e / s, z - lse, lse[:, 0]


def _xlogx(m):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > 0, m * np.log(np.where(m > 0, m, 1.0)), 0.0)


def margin_and_argmax(inp: dict):
    """float64: the arg-max of the mixed probabilities (first maximum wins) and the gap between its two largest values."""
    w32 = [float(np.float32(x)) for x in inp["w"]]
    mixed = sum(w32[k] * _softmax64(z)[0] for k, z in enumerate(inp["un"]))
    top = np.sort(mixed, axis=1)
    return np.argmax(mixed, axis=1), top[:, -1] - top[:, -2]


def reference(case: Case, inp: dict, pseudo=None, dtype=torch.float64) -> dict:
    """The oracle on `dtype` tensors with autograd: var [D, B, H, W], the raw sums (times nloss_mult), both scalar blocks, dlab /
    dun [D, B, C, H, W].  pseudo: the labels the reductions and gradients use (None: the oracle's own arg-max)."""
    D, C, N, mult = case.D, case.C, case.N, case.nloss_mult
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
    un, lab = [t(a) for a in inp["un"]], [t(a) for a in inp["lab"]]
    y = torch.tensor(inp["labels"])
    valid = (y >= 0) & (y < C)
    w32 = [float(np.float32(x)) for x in inp["w"]]
    gs = 1.0 if case.gscale is None else float(np.float32(case.gscale))
    with _fixed_pseudo(pseudo):
        T = O.loss_sums(un, lab, torch.where(valid, y, torch.zeros_like(y)), w32)
        with torch.no_grad():
            u = O.unsupervised_terms([z.detach() for z in un], w32)
    ps = T.pop("pseudo")
    tot = {k: v + (mult - 1) * v.detach() for k, v in T.items()}
    L = O.loss_from_sums(tot, N * mult, inp["cw1"], inp["cw2"], eps=EPS)
    (gs * L["loss"]).backward()
    S = {k: v.detach().double().numpy() for k, v in tot.items()}
    r = dict(pseudo=ps.numpy(), var=torch.stack(u["var"]).double().numpy(), S=S,
             dlab=torch.stack([z.grad for z in lab]).double().numpy(), dun=torch.stack([z.grad for z in un]).double().numpy(),
             **{k: float(L[k].detach()) for k in ("loss", "sup", "ps_loss", "l_uncert")})
    return r


def details(case: Case, inp: dict, pseudo) -> dict:
    """float64 numpy intermediates of both branches from the inputs alone (for the conditioning and the closed form)."""
    D, B, C, HW = case.D, case.B, case.C, case.HW
    q = {}
    for name, zs, y in (("u", inp["un"], pseudo), ("s", inp["lab"], inp["labels"])):
        sm = [_softmax64(z.reshape(B, C, HW)) for z in zs]
        p, lp, lse = (np.stack([s[i] for s in sm]) for i in range(3))                 # [D, B, C, HW] x 2, [D, B, HW]
        oh = (np.asarray(y).reshape(B, 1, HW) == np.arange(C)[None, :, None]).astype(np.float64)
        z = np.stack([np.asarray(a, np.float64).reshape(B, C, HW) for a in zs])
        q[name] = dict(p=p, lp=lp, lse=lse, oh=oh, z=z, pt=p * (1 + np.abs(lp)))
    u = q["u"]
    m = u["p"].mean(0)
    mt = u["pt"].mean(0)
    xm = _xlogx(m)
    u["m"], u["mt"] = m, mt
    u["v"] = xm.sum(1)[None] - (m[None] * u["lp"]).sum(2)                           # [D, B, HW]
    with np.errstate(divide="ignore"):
        lm = np.where(m > 0, np.log(np.where(m > 0, m, 1.0)), 0.0)
    u["lm1"] = np.where(m > 0, lm + 1.0, 0.0)
    u["cv"] = (mt * (np.abs(lm) + 1.0)).sum(1)[None] + (mt[None] * (np.abs(u["z"]) + np.abs(u["lse"])[:, :, None])).sum(2)
    return q


def cond_sums(case: Case, q: dict) -> dict:
    """Magnitude sums that go with the raw sums: CE as sum(|z_y| + |lse|), V as sum(cond of var), E as sum(exp(-v) (1 + cond of var))."""
    c = {}
    for n in ("u", "s"):
        b = q[n]
        c[n + "_ce"] = ((np.abs(b["z"]) * b["oh"][None]).sum(2) + np.abs(b["lse"]) * b["oh"].sum(1)[None]).sum((1, 2))
    c["u_V"] = q["u"]["cv"].sum((1, 2))
    c["u_E"] = (np.exp(-q["u"]["v"]) * (1 + q["u"]["cv"])).sum((1, 2))
    return c


def slots(case: Case, inp: dict, S: dict, cS: dict) -> dict:
    """Both scalar blocks from the raw sums S (already times nloss_mult) in float64, with the conditioning of every slot: (sup values,
    sup conditioning, unsup values, unsup conditioning), laid out as include/uaps_hip.h says.  cS: cond_sums (local, times nloss_mult
    inside)."""
    D, C, mult = case.D, case.C, case.nloss_mult
    Nl = float(case.N * mult)
    cw1, cw2, coef = inp["cw1"], inp["cw2"], 0.5 / D
    su, cu, ss, cs_ = np.zeros(u_layout(D, C)["n"]), np.zeros(u_layout(D, C)["n"]), np.zeros(s_layout(D, C)["n"]), np.zeros(s_layout(D, C)["n"])

    def common(pre, val, cnd, lay):
        I, P, cnt = S[pre + "_I"], S[pre + "_P"], S[pre + "_cnt"]
        den = P + cnt[None] + EPS
        dt = 2.0 * I / den
        dice, cdice = 1.0 - dt.mean(1), 1.0 + dt.mean(1)
        ce, cce = S[pre + "_ce"] / Nl, cS[pre + "_ce"] * mult / Nl
        a1, a2 = -(2.0 / C) / den, (2.0 / C) * I / (den * den)
        for name, v, c in (("ce", ce, cce), ("dice", dice, cdice), ("a1", a1, np.abs(a1)), ("a2", a2, np.abs(a2)), ("I", I, I),
                           ("card", P + cnt[None], P + cnt[None]), ("cnt", cnt, cnt)):
            o, n = lay[name]
            val[o:o + n], cnd[o:o + n] = np.ravel(v), np.ravel(c)
        return ce, cce, dice, cdice

    ul, sl = u_layout(D, C), s_layout(D, C)
    ce, cce, dice, cdice = common("u", su, cu, ul)
    s, c_s = 0.5 * (ce + dice), 0.5 * (cce + cdice)
    E, cE = S["u_E"] / Nl, cS["u_E"] * mult / Nl
    ps, cps = (s * E).mean(), (c_s * E + s * cE).mean()
    lu, clu = S["u_V"].sum() / (Nl * D), cS["u_V"].sum() * mult / (Nl * D)
    loss, closs = cw1 * ps + cw2 * lu, abs(cw1) * cps + abs(cw2) * clu
    for name, v, c in (("s", s, c_s), ("E", E, cE), ("ps_loss", ps, cps), ("l_uncert", lu, clu), ("loss", loss, closs)):
        o, n = ul[name]
        su[o:o + n], cu[o:o + n] = v, c
    ce, cce, dice, cdice = common("s", ss, cs_, sl)
    sup, csup = (coef * (ce + dice)).sum(), (coef * (cce + cdice)).sum()
    ss[sl["sup"][0]], cs_[sl["sup"][0]] = sup, csup
    ss[sl["bad"][0]] = inp["n_bad"] * mult
    su[ul["total"][0]], cu[ul["total"][0]] = sup + loss, csup + closs
    return dict(s=ss, cs=cs_, u=su, cu=cu)


def closed_form_grads(case: Case, inp: dict, q: dict, sl: dict, *, mags: bool = False, n_ce: float = None, head_w=None, extra_div: bool = False):
    """d(gscale * loss) / d logits in the form the kernels evaluate (loss_kernels.hpp sup_bwd_body / unsup_bwd_body), in float64 from
    the float64 scalars: (dlab, dun) [D, B, C, H, W].  mags: every term's magnitude instead (the conditioning).  The other arguments
    plant mistakes for the checker's self-test: n_ce = the pixel count the per-pixel terms divide by (the kernels': nloss_mult * N);
    head_w[k] multiplies head k's share of the pseudo-supervision term; extra_div divides the unsupervised gradients by D again."""
    D, B, C, HW = case.D, case.B, case.C, case.HW
    Nl = float(case.N * case.nloss_mult) if n_ce is None else float(n_ce)
    gs = 1.0 if case.gscale is None else float(np.float32(case.gscale))
    ul, sly = u_layout(D, C), s_layout(D, C)
    cw1, cw2, coef = inp["cw1"], inp["cw2"], 0.5 / D
    A = np.abs if mags else (lambda x: x)
    sg = -1.0 if mags else 1.0                       # a - sg * b: a - b, or |a| + |b| for the magnitudes

    def dice_part(b, a1, a2):
        p = b["pt"] if mags else b["p"]
        a = A(b["oh"][None] * a1[:, None, :, None]) + A(a2[:, None, :, None])
        return p, a, (p * a).sum(2, keepdims=True)

    # supervised: gce (p - oh) + gdc p (a - pa)
    b = q["s"]
    a1, a2 = slot(sl["s"], sly, "a1").reshape(D, C), slot(sl["s"], sly, "a2").reshape(D, C)
    p, a, pa = dice_part(b, a1, a2)
    gce, gdc = gs * coef / Nl, gs * coef
    dlab = A(gce) * (p - sg * b["oh"][None]) + A(gdc) * p * (a - sg * pa)
    # unsupervised
    b = q["u"]
    a1, a2 = slot(sl["u"], ul, "a1").reshape(D, C), slot(sl["u"], ul, "a2").reshape(D, C)
    p, a, pa = dice_part(b, a1, a2)
    hw_ = np.ones(D) if head_w is None else np.asarray(head_w, np.float64)
    s_k, E_k = slot(sl["u"], ul, "s"), slot(sl["u"], ul, "E")
    gu = gs * cw2 / (Nl * D)
    ge = gs * (cw1 / D) * s_k * hw_ / Nl
    cs = gs * (cw1 / D) * E_k * hw_ * 0.5
    ev = np.exp(-b["v"])
    if mags:
        gk = abs(gu) + np.abs(ge)[:, None, None] * ev * (1 + b["cv"])
        h = (gk[:, :, None] * (np.abs(b["lm1"])[None] + np.abs(b["lp"]))).mean(0)
        ph = (p * h[None]).sum(2, keepdims=True)
        dun = np.abs(cs)[:, None, None, None] * ((p + b["oh"][None]) / Nl + p * (a + pa)) + gk[:, :, None] * (b["mt"][None] + p) + p * (h[None] + ph)
    else:
        gk = gu - ge[:, None, None] * ev
        h = (gk[:, :, None] * (b["lm1"][None] - b["lp"])).mean(0)
        ph = (p * h[None]).sum(2, keepdims=True)
        dun = cs[:, None, None, None] * ((p - b["oh"][None]) / Nl + p * (a - pa)) - gk[:, :, None] * (b["m"][None] - p) + p * (h[None] - ph)
    if extra_div:
        dun = dun / D
    shape = (D, B, C, case.H, case.W)
    return dlab.reshape(shape), dun.reshape(shape)


def full_reference(case: Case, inp: dict, pseudo=None) -> dict:
    """reference() plus the scalar blocks, every conditioning and the pseudo-label margins."""
    am, margin = margin_and_argmax(inp)
    ref = reference(case, inp, pseudo)
    q = details(case, inp, ref["pseudo"])
    ref["argmax64"], ref["margin"] = am, margin
    ref["slots"] = slots(case, inp, ref["S"], cond_sums(case, q))
    ref["c_var"] = q["u"]["cv"].reshape(case.D, case.B, case.H, case.W)
    ref["c_dlab"], ref["c_dun"] = closed_form_grads(case, inp, q, ref["slots"], mags=True)
    ref["cS"] = cond_sums(case, q)
    ref["q"] = q
    return ref


def raw_sums(case: Case, S: dict, cS: dict = None) -> np.ndarray:
    """The sums_out vector of the pair forward (float64) from the reference's sums of ONE rank -- or its conditioning."""
    D, C = case.D, case.C
    if cS is None:
        return np.concatenate([S["s_ce"], S["s_I"].ravel(), S["s_P"].ravel(), S["s_cnt"], [0.0],
                               S["u_ce"], S["u_I"].ravel(), S["u_P"].ravel(), S["u_cnt"], S["u_E"], S["u_V"]])
    return np.concatenate([cS["s_ce"], S["s_I"].ravel(), S["s_P"].ravel(), S["s_cnt"], [0.0],
                           cS["u_ce"], S["u_I"].ravel(), S["u_P"].ravel(), S["u_cnt"], cS["u_E"], cS["u_V"]])


# ---- the bars -------------------------------------------------------------------------------------------------------------------
# Each value is about 3x the largest ratio the kernels reach on an MI355X over the whole table, and 3x to 6x the fp32 floor (the same
# oracle in torch.float32 on the CPU, fp32_floor below): profiles/loss_forms_tau.txt.  LEGACY: what tests/test_gpu_parity.py asserts for
# the same quantities (scalars relative, var absolute, gradients against max|g|), asserted beside the bars at logit_scale = 1.
TAU = dict(var=4.5e-7, scal=3.5e-7, coef=2e-6, isum=2e-6, dlab=9e-7, dun=8e-7)
LEGACY = dict(scal_rel=2e-5, var_abs=2e-5, grad_of_max=2e-5)
FLOOR = 1e-30               # added to every conditioning: an fp32 result below FLT_MIN = 1.2e-38 may be flushed to zero (TAU x FLOOR ~ 1e-36)


def ratio(got, ref, cond) -> float:
    got, ref, cond = (np.asarray(a, np.float64) for a in (got, ref, cond))
    if not np.all(np.isfinite(got)):
        return math.inf
    return float((np.abs(got - ref) / (cond + FLOOR)).max()) if got.size else 0.0


SCAL_U, SCAL_S = ("ce", "dice", "s", "E", "ps_loss", "l_uncert", "loss"), ("ce", "dice", "sup")


def compare(case: Case, inp: dict, ref: dict, got: dict):
    """(ratios per TAU key, failed exact conditions).  got: pseudo [B, H, W]; var [D, B, H, W] or None; sscal / uscal (fp32 blocks);
    dlab / dun [D, B, C, H, W]; optionally sums (float64 raw sums as the forward wrote them, ONE rank's) and amax (the bound's value).
    ref: full_reference(case, inp, got['pseudo'])."""
    D, C, N, mult = case.D, case.C, case.N, case.nloss_mult
    ul, sl = u_layout(D, C), s_layout(D, C)
    r, bad = {}, []
    sup_ok = not case.bad_labels                       # the reference has no out-of-range labels: that half is only held finite
    # exact: pseudo-labels, counts
    ps = np.asarray(got["pseudo"]).reshape(-1)
    clear = ref["margin"].reshape(-1) >= MARGIN
    planted = np.zeros(N, bool)
    if case.planted == "ties":
        planted[inp["planted"]] = True
        if not np.array_equal(ps[inp["planted"]], inp["tie_class"]):
            bad.append("a planted tie did not resolve to the lower class index")
    if ((~clear) & (~planted)).sum() > TIE_SHARE * N:
        bad.append(f"{int(((~clear) & (~planted)).sum())} of {N} pixels have a float64 margin below {MARGIN}")
    if not np.array_equal(ps[clear], ref["argmax64"].reshape(-1)[clear]):
        bad.append(f"pseudo-label differs from the float64 arg-max at {int((ps[clear] != ref['argmax64'].reshape(-1)[clear]).sum())} clear pixels")
    if ps.min() < 0 or ps.max() >= C:
        bad.append("pseudo-label outside [0, C)")
        return r, bad
    ucnt, scnt = slot(got["uscal"], ul, "cnt"), slot(got["sscal"], sl, "cnt")
    if not np.array_equal(ucnt, mult * np.bincount(ps, minlength=C)) or ucnt.sum() != mult * N:
        bad.append(f"unsupervised cnt {ucnt} is not {mult} x bincount(pseudo)")
    y = inp["labels"].reshape(-1)
    if not np.array_equal(scnt, mult * np.bincount(y[(y >= 0) & (y < C)], minlength=C)):
        bad.append(f"supervised cnt {scnt} is not {mult} x bincount(labels)")
    if float(slot(got["sscal"], sl, "bad")[0]) != mult * inp["n_bad"]:
        bad.append(f"UAPS_S_BAD {float(slot(got['sscal'], sl, 'bad')[0])} != {mult * inp['n_bad']}")
    for k in ("sscal", "uscal", "dlab", "dun"):
        if not np.all(np.isfinite(got[k])):
            bad.append(f"{k} is not finite")
    # bars
    S = ref["slots"]
    if got.get("var") is not None:
        r["var"] = ratio(got["var"], ref["var"], ref["c_var"])
        if case.logit_scale == 1.0 and not np.abs(got["var"] - ref["var"]).max() <= LEGACY["var_abs"]:
            bad.append(f"var off by {np.abs(got['var'] - ref['var']).max()} (absolute bar {LEGACY['var_abs']})")
    names_u = SCAL_U + (("total",) if case.entry != TWO_BRANCH and sup_ok else ())
    scal = [ratio(slot(got["uscal"], ul, n), slot(S["u"], ul, n), slot(S["cu"], ul, n)) for n in names_u]
    coef = [ratio(slot(got["uscal"], ul, n), slot(S["u"], ul, n), slot(S["cu"], ul, n)) for n in ("a1", "a2")]
    isum = [ratio(slot(got["uscal"], ul, n), slot(S["u"], ul, n), slot(S["cu"], ul, n)) for n in ("I", "card")]
    rel = [np.abs(slot(got["uscal"], ul, n) - slot(S["u"], ul, n)) / (np.abs(slot(S["u"], ul, n)) + FLOOR) for n in ("ce", "dice", "s", "E", "ps_loss", "loss")]
    if sup_ok:
        scal += [ratio(slot(got["sscal"], sl, n), slot(S["s"], sl, n), slot(S["cs"], sl, n)) for n in SCAL_S]
        coef += [ratio(slot(got["sscal"], sl, n), slot(S["s"], sl, n), slot(S["cs"], sl, n)) for n in ("a1", "a2")]
        isum += [ratio(slot(got["sscal"], sl, n), slot(S["s"], sl, n), slot(S["cs"], sl, n)) for n in ("I", "card")]
        rel += [np.abs(slot(got["sscal"], sl, n) - slot(S["s"], sl, n)) / (np.abs(slot(S["s"], sl, n)) + FLOOR) for n in SCAL_S]
    if case.entry == TWO_BRANCH and float(slot(got["uscal"], ul, "total")[0]) != 0.0:
        bad.append("the two-branch forward left UAPS_U_TOTAL non-zero")
    if got.get("sums") is not None:
        one = {k: v / mult for k, v in ref["S"].items()}
        gs_, rs_, cs_ = np.asarray(got["sums"], np.float64), raw_sums(case, one), raw_sums(case, one, ref["cS"])
        ns = n_sums(D, C)[0]
        keep = np.ones(gs_.size, bool)
        keep[ns - 1] = False                            # the out-of-range count: exact, below
        if not sup_ok:
            keep[:ns] = False
        isum.append(ratio(gs_[keep], rs_[keep], cs_[keep]))
        if gs_[ns - 1] != inp["n_bad"]:
            bad.append(f"raw out-of-range count {gs_[ns - 1]} != {inp['n_bad']}")
    r["scal"], r["coef"], r["isum"] = max(scal), max(coef), max(isum)
    if case.logit_scale == 1.0 and max(float(np.max(x)) for x in rel) > LEGACY["scal_rel"]:
        bad.append(f"a scalar is off by more than {LEGACY['scal_rel']} relative")
    for k in ("dlab", "dun"):
        if k == "dlab" and not sup_ok:
            continue
        r[k] = ratio(got[k], ref[k], ref["c_" + k])
        if case.logit_scale == 1.0 and not np.abs(got[k] - ref[k]).max() <= LEGACY["grad_of_max"] * np.abs(ref[k]).max():
            bad.append(f"{k} off by {np.abs(got[k] - ref[k]).max()} > {LEGACY['grad_of_max']} max|g| = {LEGACY['grad_of_max'] * np.abs(ref[k]).max()}")
    if got.get("amax") is not None:
        want = float(max(np.abs(np.asarray(got["dlab"], np.float32)).max(), np.abs(np.asarray(got["dun"], np.float32)).max()))
        if float(got["amax"]) != want:
            bad.append(f"out_amax {got['amax']!r} != max|d logits| {want!r}")
    return r, bad


def over_bars(ratios: dict) -> dict:
    return {k: (v, TAU[k]) for k, v in ratios.items() if not v <= TAU[k]}


def as_got(case: Case, inp: dict, ref: dict, dtype=np.float32) -> dict:
    """The reference's own outputs in the shape of a kernel's (rounded to fp32): what the checker's self-test plants mistakes in."""
    D, C = case.D, case.C
    one = {k: v / case.nloss_mult for k, v in ref["S"].items()}
    g = dict(pseudo=ref["pseudo"].copy(), var=ref["var"].astype(dtype) if case.want_var else None, sscal=ref["slots"]["s"].astype(dtype),
             uscal=ref["slots"]["u"].astype(dtype), dlab=ref["dlab"].astype(dtype), dun=ref["dun"].astype(dtype))
    if case.entry == SUMS:
        g["sums"] = raw_sums(case, one)
    if case.entry == TWO_BRANCH:
        g["uscal"][u_layout(D, C)["total"][0]] = 0.0
    if case.track:
        g["amax"] = float(max(np.abs(g["dlab"]).max(), np.abs(g["dun"]).max()))
    return g


def fp32_floor(case: Case) -> dict:
    """The same oracle in torch.float32 on the CPU against the float64 reference: each quantity's ratio.  Independent of the kernels."""
    inp = inputs(case)
    ref = full_reference(case, inp)
    lo = reference(case, inp, ref["pseudo"], dtype=torch.float32)
    q = details(case, inp, ref["pseudo"])
    sl = slots(case, inp, {k: np.asarray(v, np.float64) for k, v in lo["S"].items()}, cond_sums(case, q))
    got = dict(pseudo=ref["pseudo"], var=lo["var"].astype(np.float32), sscal=sl["s"].astype(np.float32), uscal=sl["u"].astype(np.float32),
               dlab=lo["dlab"].astype(np.float32), dun=lo["dun"].astype(np.float32))
    if case.entry == TWO_BRANCH:
        got["uscal"][u_layout(case.D, case.C)["total"][0]] = 0.0
    return compare(case, inp, ref, got)[0]

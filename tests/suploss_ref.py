"""The dense-label loss kernels that share uaps_amd/csrc/loss_common.hpp -- CPS (loss_cps.hip), UCC with its cut-mix (loss_ucc.hip) and
the class counts and guarded launches tests/test_gpu_seglosses.py lacks (loss_seg.hip): one case per entry point, class count, form,
reason for the form and set of optional outputs; references in plain numpy; the comparison code (tests/test_suploss_ref.py,
tests/test_gpu_suploss_forms.py).  The machinery is tests/consistency_ref.py's: class E (a float64 value of the exact formula with
a running bound of what float32 can have lost), its operations, Ref, compare.

Held exactly (Ref.exact): the pseudo-label bytes (the arg-max of the same float32 logits, the lowest index among equal values), the
count of labels outside [0, C), the reserved scalars, the cut-mix outputs, mixed labels and max|.| (numpy `where`), and the variance
maps of two identical heads (every operation of kl_pair is x - x or q * 0 there: +0).

Held against bars (Ref.f64): the float64 reference walks the kernels' own operation sequence.  The three files are built without
fast-math, so the IEEE figures of consistency_ref apply (expf 3 ulp, logf 3 ulp, `/` 1 ulp, U = 2^-24 per other operation).  A sum over
pixels gets (n + 2) U sum|term| beside the terms' own bounds, n = the float32 additions a term can pass through: trips x V in the
lane's loop, six shuffles, the LDS round (n_adds below: never less than consistency_ref.lane_adds with the family's block cap).  The
block partials are added and the finalize formulas evaluated in double, then rounded once; the reference bounds that by treating every
finalize operation as a float32 one, which is more than it needs.  The class counts enter the cardinalities as integers.  The backward
reference reads the forward REFERENCE's scalars with their bounds, so nothing a kernel returns enters a bar.

A bar that swallows its quantity proves nothing: swallowed(ref) lists the compared tensors whose largest bar is not below 2^-10 of
their largest |reference value|; it must be empty for every case, and the tests assert that before a device is asked.

Every case names the kernel instantiations it must reach, from a restatement of the launchers' rules: UAPS_BY_C, each entry point's
`vec` expression (they differ: forward and backward decide separately, from different pointer sets), split_for / grid_for with the
caps 512 per row set (CPS), 1024 (UCC, seg) and 4096 (cut-mix), the trip count and the workspace bytes.  A mutant is a switch on a
reference (`mut`); the CPU test proves with them that the comparisons bite.
"""
from __future__ import annotations

import numpy as np

import consistency_ref as CR
from bn_ref import rng_for
from consistency_ref import E, F32, F64, TINY, U, add, as_got, compare, const32, csum, div, exp_, log_, mul, scale2, softmax_E, sub, total
from ops_ref import Ref, amax_after

THREADS, MAX_CLASSES, UCC_MAX_BATCH = 256, 8, 64
CAP = dict(cps=512, ucc=1024, seg=1024, cutmix=4096)                     # kMaxBlocks of the three files (CPS: per row set)
COLS = dict(cps=80, ucc=100, seg=40)                                      # kCols: floats of a block's partial row
CLASSES = tuple(range(2, MAX_CLASSES + 1))
EPS = float(F32(1e-7))
SWALLOW = 2.0 ** -10
# labels outside [0, C): the last five do not fit an int, and three of them narrow to class 1, 1 and 0
EDGE_LABELS = (-1, None, 255, 2 ** 31, 2 ** 32 + 1, -2 ** 32 + 1, -2 ** 63, 2 ** 63 - 1)        # None: C


def edge_labels(C: int) -> np.ndarray:
    return np.array([C if v is None else v for v in EDGE_LABELS], np.int64)


# ---- the launchers' rules ---------------------------------------------------------------------------------------------------------
def grid_for(items: int, cap: int) -> int:
    return max(1, min(cap, (items + THREADS - 1) // THREADS))


def trips(items: int, cap: int) -> int:
    return -(-items // (grid_for(items, cap) * THREADS))


def n_adds(items: int, cap: int, V: int) -> int:
    """float32 additions a term can pass through on its way into a block partial."""
    return max(trips(items, cap) * V + 8, CR.lane_adds(items, cap, V))


def workspace_bytes(entry: str) -> int:
    return (2 if entry == "cps" else 1) * CAP[entry] * COLS[entry] * 4


ALIGN = dict(z1=4, z2=4, labels=2, pseudo1=4, pseudo2=4, var1=4, var2=4, dz1=4, dz2=4, z=4, dz=4, x_l=4, x_wk=4, x_st=4, out=4)   # elements
VEC_SETS = {("cps", "fwd"): ("z1", "z2", "labels", "pseudo1", "pseudo2"), ("cps", "bwd"): ("z1", "z2", "labels", "dz1", "dz2"),
            ("ucc", "fwd"): ("z1", "z2", "labels", "pseudo1", "pseudo2", "var1", "var2"), ("ucc", "bwd"): ("z1", "z2", "labels", "dz1", "dz2"),
            ("seg", "fwd"): ("z", "labels"), ("seg", "bwd"): ("z", "labels", "dz"), ("cutmix", "fwd"): ("x_l", "x_wk", "x_st", "out")}


class Case:
    """id, entry (cps / ucc / seg run forward and backward; cutmix), parameters (absent ones read as the defaults)."""
    DEFAULTS = dict(regime="randn2", offs={}, outs=("pseudo1", "pseudo2", "var1", "var2"), g=(0.83, 0.31, 0.57), gnull=False, eps=EPS,
                    edges=False, B_lab=1, Cin=3, rects="mixed", hinted=False, heavy=False, ignore=None)

    def __init__(self, id: str, entry: str, **p):
        self.id, self.entry, self.params = id, entry, p

    def __getattr__(self, k):
        p = self.__dict__.get("params", {})
        if k in p:
            return p[k]
        if k in Case.DEFAULTS:
            return Case.DEFAULTS[k]
        raise AttributeError(k)

    def off(self, name: str) -> int:
        return self.offs.get(name, 0)

    @property
    def C(self):
        return self.shape[1]

    @property
    def HW(self):
        return self.shape[2] * self.shape[3]

    def has(self, name: str) -> bool:
        """Whether the optional output is passed (CPS has no variance maps)."""
        return name in self.outs and not (self.entry == "cps" and name.startswith("var"))

    def vec(self, d: str = "fwd") -> bool:
        """The `vec` expression of the entry point: H W % 4 == 0 and every pointer of its own set aligned (a NULL output passes)."""
        names = [n for n in VEC_SETS[(self.entry, d)] if not (n.startswith(("pseudo", "var")) and not self.has(n))]
        return self.HW % 4 == 0 and all(self.off(n) % ALIGN[n] == 0 for n in names)

    def V(self, d: str = "fwd") -> int:
        return 4 if self.vec(d) else 1

    def row_sets(self, d: str = "fwd"):
        """[(first row, rows, items, grid, cap)] of the launch: CPS splits the grid into a labelled and an unlabelled part."""
        N, V = self.shape[0], self.V(d)
        if self.entry == "cps":
            sets = [(0, self.B_lab), (self.B_lab, N - self.B_lab)]
        elif self.entry == "cutmix":
            sets = [(0, N * self.Cin)]
        else:
            sets = [(0, N)]
        cap = CAP[self.entry]
        return [(r0, n, n * self.HW // V, grid_for(n * self.HW // V, cap), cap) for r0, n in sets]

    def trips(self, d: str = "fwd") -> int:
        return max(trips(items, cap) for _, _, items, _, cap in self.row_sets(d))

    @property
    def kernels(self) -> frozenset:
        e, C = self.entry, self.C
        if e == "cutmix":
            return frozenset({f"ucc_cutmix_kernel<{self.V()}>"})
        return frozenset({f"{e}_fwd_kernel<{C}, {self.V('fwd')}>", f"{e}_finalize<{C}>", f"{e}_bwd_kernel<{C}, {self.V('bwd')}>"})

    @property
    def workspace_bytes(self) -> int:
        return workspace_bytes(self.entry)


KERNEL_NAMES = ("cps_fwd_kernel", "cps_finalize", "cps_bwd_kernel", "ucc_cutmix_kernel", "ucc_fwd_kernel", "ucc_finalize", "ucc_bwd_kernel",
                "seg_fwd_kernel", "seg_finalize", "seg_bwd_kernel")


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
REGIMES = ("randn2", "sat", "same", "one_class", "absent")


def logits(rng, shape, regime: str) -> np.ndarray:
    """randn2: consistency_ref's.  sat: |z| up to 60, softmaxes whose small probabilities underflow.  one_class: class 1 wins every
    pixel.  absent: class 0 never wins (and the labels never name it).  (same: see inputs().)"""
    B, C, H, W = shape
    if regime in ("randn2", "same"):
        z = CR.logits(rng, shape, "randn2")
        flat = z.reshape(B, C, H * W)                    # the planted ties of the existing sweeps
        flat[:, C - 1, 0] = flat[:, :, 0].max(axis=1)    # the top value repeated at class C - 1
        flat[:, :, H * W - 1] = 0.25                     # all classes equal
        return z
    if regime == "sat":
        return np.clip(rng.standard_normal(shape) * 30, -60, 60).astype(F32)
    z = CR.logits(rng, shape, "randn2")
    if regime == "one_class":
        z[:, 1] = np.abs(z).max(axis=1) + F32(0.5)
    elif regime == "absent":
        z[:, 0] = z[:, 1:].min(axis=1) - F32(0.5)
    else:
        raise ValueError(regime)
    return z


def rect_lists(rng, B, H, W, kind: str):
    """(rects_l, rects_u) int32 [B, 5]: flag, y0, y1, x0, x1."""
    def some():
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        return (1, y0, int(rng.integers(y0 + 1, H + 1)), x0, int(rng.integers(x0 + 1, W + 1)))       # never empty
    rows = {"mixed": lambda i: some() if i % 3 != 2 else (0,) + some()[1:], "full": lambda i: (1, 0, H, 0, W), "off": lambda i: (0,) + some()[1:],
            "empty": lambda i: (1, H // 2, H // 2, 0, W), "column": lambda i: (1, 0, H, W // 2, min(W, W // 2 + 1))}[kind]
    return np.array([rows(i) for i in range(B)], np.int32), np.array([rows(i + 1) for i in range(B)], np.int32)


def inputs(c: Case) -> dict:
    rng = rng_for(c.id)
    N, C, H, W = c.shape
    if c.entry == "cutmix":
        sh = (N, c.Cin, H, W)
        d = dict(x_l=rng.standard_normal(sh).astype(F32), x_wk=(rng.standard_normal(sh) * 3).astype(F32), x_st=(rng.standard_normal(sh) * 5).astype(F32),
                 y_l=rng.integers(0, 4, (N, H, W)).astype(np.int64))
        d["x_l"].reshape(-1)[0] = F32(-0.0)
        d["rl"], d["ru"] = rect_lists(rng, N, H, W, c.rects)
        return d
    rows = {"cps": N, "ucc": 3 * N, "seg": N}[c.entry]
    nlab = {"cps": c.B_lab, "ucc": N, "seg": N}[c.entry]
    z1 = logits(rng, (rows, C, H, W), c.regime)
    z2 = logits(rng, (rows, C, H, W), c.regime)
    if c.regime == "same":                               # two identical heads: every KL pair of UCC compares a tensor with itself
        z2 = z1.copy()
        if c.entry == "ucc":
            z2[N:2 * N], z2[2 * N:] = z1[2 * N:], z1[N:2 * N]
    lo = 1 if c.regime == "absent" else 0
    y = rng.integers(lo, C, (nlab, H, W)).astype(np.int64)
    if c.regime == "one_class":
        y[:] = 1
    n_planted = 0
    if c.edges:
        pix = rng.choice(y.size, size=min(y.size, 2 * len(EDGE_LABELS)), replace=False)
        y.reshape(-1)[pix] = np.resize(edge_labels(C), pix.size)
        n_planted = int(pix.size)
    if c.ignore is not None:
        y.reshape(-1)[::7] = c.ignore
    if c.entry == "seg":
        return dict(z=z1, labels=y, n_planted=n_planted, class_weight=(0.5 + 1.5 * rng.random(C)).astype(F32))
    return dict(z1=z1, z2=z2, labels=y, n_planted=n_planted)


# ---- shared pieces of the walks ---------------------------------------------------------------------------------------------------
def argmax(z, mut: str = "") -> np.ndarray:
    z = np.asarray(z, F32)
    C = z.shape[1]
    return (C - 1 - np.argmax(z[:, ::-1], axis=1)) if mut == "tie_high" else np.argmax(z, axis=1)


def in_range(y, C):
    """(labels with everything outside [0, C) as -1, how many were outside): decided in 64 bits."""
    y = np.asarray(y, np.int64)
    ok = (y >= 0) & (y < C)
    return np.where(ok, y, -1), int((~ok).sum())


def _soft(z):
    """(p, lse, mx) as softmax_inplace leaves them."""
    p, s, mx, _ = softmax_E(z)
    return p, log_(s), mx


def _nll(z, soft, t) -> E:
    """-(z[t] - mx - lse) where t >= 0, 0 elsewhere."""
    _, lse, mx = soft
    ok = t >= 0
    zt = np.take_along_axis(np.asarray(z, F64), np.where(ok, t, 0)[:, None], 1)[:, 0]
    lp = sub(sub(E(zt), E(mx)), lse)
    return E(np.where(ok, -lp.v, 0.0), np.where(ok, lp.e, 0.0))


def _where(m, x: E) -> E:
    return E(np.where(m, x.v, 0.0), np.where(m, x.e, 0.0))


def _tot(x: E, n: int) -> E:
    v, bar = total(x, n)
    return E(v, bar)


def _class_sums(p: E, t, n: int):
    """(A[c] = sum p_c, I[c] = sum p_c [t = c]) as E arrays [C], N[c] = #[t = c] as integers."""
    C = p.shape[1]
    A = [_tot(p[:, c], n) for c in range(C)]
    I = [_tot(_where(t == c, p[:, c]), n) for c in range(C)]
    return _stack(A), _stack(I), np.array([int((t == c).sum()) for c in range(C)], F64)


def _stack(xs) -> E:
    return E(np.array([float(x.v) for x in xs]), np.array([float(x.e) for x in xs]))


def _esum(a: E, b: E) -> E:
    """A sum formed in double: the values and the bounds add."""
    return E(a.v + b.v, a.e + b.e)


def _dice_rows(A: E, I: E, cnt, eps: float, C: int, mut: str = ""):
    """The finalize of one term: (card, A1 = 2 / (C den), A2 = 2 I / (C den^2), dice = 1 - mean_c 2 I / den), den = card + eps."""
    card = E(A.v + cnt, A.e)
    den = card if mut == "no_eps" else E(card.v + eps, card.e)
    cden = mul(E(float(C)), den)
    a1 = div(E(2.0), cden)
    a2 = div(scale2(I, 2.0), mul(cden, den))
    part = div(scale2(I, 2.0), den)
    dice = sub(E(1.0), div(E(part.v.sum(), part.e.sum() + C * U * np.abs(part.v).sum()), E(float(C))))
    return card, a1, a2, dice


def _bc(r: E) -> E:
    return E(r.v[None, :, None, None], r.e[None, :, None, None])


def _onehot(t, C):
    return t[:, None] == np.arange(C)[None, :, None, None]


def _f32(x: E) -> E:
    """The one rounding of a double to the float the kernel stores."""
    return E(x.v, x.e + U * np.abs(x.v) + TINY)


def _pair(x: E):
    return (x.v, x.e)


# ---- CPS ----------------------------------------------------------------------------------------------------------------------------
def cps_fwd(c: Case, inp: dict, mut: str = "") -> Ref:
    z = (np.asarray(inp["z1"], F32), np.asarray(inp["z2"], F32))
    N, C, H, W = z[0].shape
    b = c.B_lab
    y, bad = in_range(inp["labels"], C)
    am = [argmax(z[0], mut), argmax(z[1], mut)]
    soft = [_soft(z[0]), _soft(z[1])]
    sets = c.row_sets("fwd")
    V = c.V("fwd")
    rows = (slice(0, b), slice(b, N))
    n_pix = (float(b * H * W), float((N - b) * H * W))
    ce, dice, A1, A2, Is, CARD = [None] * 6, [None] * 6, [None] * 6, [None] * 6, [None] * 6, [None] * 6
    for m in range(2):
        other = am[m] if mut == "own_argmax" else am[1 - m]
        p = soft[m][0]
        part = []                                        # per row set: A, IX, NP of the target, the CE sum against the target
        for h in range(2):
            n = n_adds(sets[h][2], sets[h][4], V)
            sl = rows[h]
            sub_soft = (p[sl], soft[m][1][sl], soft[m][2][sl])
            A, IX, NP = _class_sums(p[sl], other[sl], n)
            part.append((A, IX, NP, _tot(_nll(z[m][sl], sub_soft, other[sl]), n)))
            if h == 0:
                _, IY, NY = _class_sums(p[sl], y, n)
                cey = _tot(_nll(z[m][sl], sub_soft, y), n)
        A_gt = _esum(part[0][0], part[1][0]) if mut == "unl_in_gt" else part[0][0]
        CARD[m], A1[m], A2[m], dice[m] = _dice_rows(A_gt, IY, NY, c.eps, C, mut)
        Is[m], ce[m] = IY, div(cey, E(n_pix[0]))
        for h in range(2):
            t = 2 + 2 * h + m
            A, IX, NP, cex = part[h]
            CARD[t], A1[t], A2[t], dice[t] = _dice_rows(A, IX, NP, c.eps, C, mut)
            Is[t], ce[t] = IX, div(cex, E(n_pix[h]))
    half = lambda t: scale2(add(ce[t], dice[t]), 0.5)
    head = [ce[t] for t in range(6)] + [dice[t] for t in range(6)] + [add(half(0), half(1)), add(half(2), half(3)), add(half(4), half(5))]
    ref = Ref(exact=dict(bad=F32(bad)))
    if c.has("pseudo1"):
        ref.exact["pseudo1"] = am[0].astype(np.uint8)
    if c.has("pseudo2"):
        ref.exact["pseudo2"] = am[1].astype(np.uint8)
    cat = lambda rows_: E(np.concatenate([r.v for r in rows_]), np.concatenate([r.e for r in rows_]))
    ref.f64 = dict(head=_pair(_f32(_stack(head))), A1=_pair(_f32(cat(A1))), A2=_pair(_f32(cat(A2))), I=_pair(_f32(cat(Is))), CARD=_pair(_f32(cat(CARD))))
    ref.parts = dict(am=am, y=y, soft=soft)
    return ref


def _term_grad(p: E, t, w: E, inv_n: E, a1: E, a2: E, mut: str = "") -> E:
    """term_grad_add / bwd_one for one term: p (d - <p, d>) + [t >= 0] w inv_n (p - onehot(t)), d = w a2 - [t = c] w a1."""
    C = p.shape[1]
    oh = _onehot(t, C)
    d = sub(_bc(mul(w, a2)), _where(oh, _bc(mul(w, a1))))
    dot = csum(mul(p, d))
    inner = d if mut == "no_projection" else sub(d, E(dot.v[:, None], dot.e[:, None]))
    ok = np.ones_like(t, bool) if mut == "ce_on_minus1" else t >= 0
    cepart = _where(ok[:, None], mul(mul(w, inv_n), sub(p, E(oh.astype(F64)))))
    return add(mul(p, inner), cepart)


def cps_bwd(c: Case, inp: dict, fwd: Ref, mut: str = "") -> Ref:
    """d(g_sup sup + g_lcps lcps) / dz on the labelled rows, d(g_cps cps) / dz on the unlabelled, from the forward REFERENCE's rows."""
    N, C, H, W = np.asarray(inp["z1"]).shape
    b = c.B_lab
    am, y, soft = fwd.parts["am"], fwd.parts["y"], fwd.parts["soft"]
    a1 = E(*fwd.f64["A1"]).v.reshape(6, C), E(*fwd.f64["A1"]).e.reshape(6, C)
    a2 = E(*fwd.f64["A2"]).v.reshape(6, C), E(*fwd.f64["A2"]).e.reshape(6, C)
    row = lambda a, t: E(a[0][t], a[1][t])
    g = (1.0, 1.0, 1.0) if c.gnull else tuple(float(F32(x)) for x in c.g)
    inv = [const32(1.0 / (b * H * W)), const32(1.0 / ((N - b) * H * W))]
    if mut == "inv_n_other":
        inv = inv[::-1]
    rows = (slice(0, b), slice(b, N))
    out = []
    for m in range(2):
        parts = []
        for h in range(2):                               # bwd_one: both terms' Dice rows are added before the projection
            sl = rows[h]
            p, other = soft[m][0][sl], am[1 - m][sl]
            yy = y if h == 0 else np.full(other.shape, -1)
            tx = 2 + 2 * h + m
            wy, wx = E(0.5 * g[0] if h == 0 else 0.0), E(0.5 * (g[1] if h == 0 else g[2]))
            oy, ox = _onehot(yy, C), _onehot(other, C)
            gy = sub(_bc(mul(wy, row(a2, m))), _where(oy, _bc(mul(wy, row(a1, m)))))
            gx = sub(_bc(mul(wx, row(a2, tx))), _where(ox, _bc(mul(wx, row(a1, tx)))))
            gg = add(gy, gx)
            dot = csum(mul(p, gg))
            inner = gg if mut == "no_projection" else sub(gg, E(dot.v[:, None], dot.e[:, None]))
            y_ok = np.ones_like(yy, bool) if (mut == "ce_on_minus1" and h == 0) else yy >= 0
            cey = _where(y_ok[:, None], mul(mul(wy, inv[h]), sub(p, E(oy.astype(F64)))))
            cex = mul(mul(wx, inv[h]), sub(p, E(ox.astype(F64))))
            parts.append(add(mul(p, inner), add(cey, cex)))
        out.append(E(np.concatenate([q.v for q in parts]), np.concatenate([q.e for q in parts])))
    return Ref(f64=dict(dz1=_pair(out[0]), dz2=_pair(out[1])))


# ---- UCC ----------------------------------------------------------------------------------------------------------------------------
def _kl_pair(za, zb):
    """kl_pair: (p, q, l = log q - log p from the logits, var = sum_c q l, both softmaxes' parts)."""
    sa, sb = _soft(za), _soft(zb)
    l = sub(E(np.asarray(zb, F64)), E(np.asarray(za, F64)))
    shift = add(sub(E(sa[2]), E(sb[2])), sub(sa[1], sb[1]))
    l = add(l, E(shift.v[:, None], shift.e[:, None]))
    var = csum(mul(sb[0], l))
    return sa, sb, l, var


def ucc_fwd(c: Case, inp: dict, mut: str = "") -> Ref:
    z1, z2 = np.asarray(inp["z1"], F32), np.asarray(inp["z2"], F32)
    B, C, H, W = c.shape
    lab, wk, st = slice(0, B), slice(B, 2 * B), slice(2 * B, 3 * B)
    y, bad = in_range(inp["labels"], C)
    (_, _, items, _, cap), = c.row_sets("fwd")
    n = n_adds(items, cap, c.V("fwd"))
    n_pix = float(B * H * W)
    pseudo2 = argmax(z1[wk], mut)
    pseudo1 = argmax(z1[wk] if mut == "pseudo1_from_z1" else z2[wk], mut)
    # pair 1 = (z1_wk, z2_st): variance_1, term 3; pair 2 = (z1_st, z2_wk): variance_2, term 2
    pa = _kl_pair(z1[wk], z2[st])
    pb = _kl_pair(z1[st], z2[wk])
    if mut == "var_swapped":
        pa, pb = (pa[0], pa[1], pb[2], pb[3]), (pb[0], pb[1], pa[2], pa[3])
    same1, same2 = np.array_equal(z1[wk], z2[st]), np.array_equal(z1[st], z2[wk])
    terms = [(z1[lab], _soft(z1[lab]), y), (z2[lab], _soft(z2[lab]), y), (z1[st], pb[0], pseudo1), (z2[st], pa[1], pseudo2)]
    ce, dice, A1, A2, Is, CARD = [], [], [], [], [], []
    for zt, soft, t in terms:
        A, I, cnt = _class_sums(soft[0], t, n)
        card, a1, a2, d = _dice_rows(A, I, cnt, c.eps, C, mut)
        ce.append(div(_tot(_nll(zt, soft, t), n), E(n_pix)))
        dice.append(d); A1.append(a1); A2.append(a2); Is.append(I); CARD.append(card)
    means = []
    for var in (pa[3], pb[3]):
        neg = scale2(var, -1.0)
        means += [div(_tot(var, n), E(n_pix)), div(_tot(exp_(neg), n), E(n_pix))]
    V1, E1, V2, E2 = means
    S = [scale2(add(ce[t], dice[t]), 0.5) for t in range(4)]
    ps1 = add(S[2] if mut == "no_exp" else mul(S[2], E1), V1)
    ps2 = add(S[3] if mut == "no_exp" else mul(S[3], E2), V2)
    head = ce + dice + [add(S[0], S[1]), add(ps1, ps2), ps1, ps2, V1, E1, V2, E2]
    ref = Ref(exact=dict(bad=F32(bad), reserved=np.zeros(3, F32)))
    for name, v in (("pseudo1", pseudo1), ("pseudo2", pseudo2)):
        if c.has(name):
            ref.exact[name] = v.astype(np.uint8)
    cat = lambda rows_: E(np.concatenate([r.v for r in rows_]), np.concatenate([r.e for r in rows_]))
    ref.f64 = dict(head=_pair(_f32(_stack(head))), A1=_pair(_f32(cat(A1))), A2=_pair(_f32(cat(A2))), I=_pair(_f32(cat(Is))), CARD=_pair(_f32(cat(CARD))))
    for name, var, same in (("var1", pa[3], same1), ("var2", pb[3], same2)):
        if c.has(name):
            if same and not mut:
                ref.exact[name] = np.zeros(var.shape, F32)
            else:
                ref.f64[name] = _pair(var)
    ref.parts = dict(y=y, pseudo1=pseudo1, pseudo2=pseudo2, pa=pa, pb=pb, lab=(terms[0][1], terms[1][1]), S=S, E=(E1, E2))
    return ref


def ucc_bwd(c: Case, inp: dict, fwd: Ref, mut: str = "") -> Ref:
    B, C, H, W = c.shape
    P = fwd.parts
    a1 = E(*fwd.f64["A1"]).v.reshape(4, C), E(*fwd.f64["A1"]).e.reshape(4, C)
    a2 = E(*fwd.f64["A2"]).v.reshape(4, C), E(*fwd.f64["A2"]).e.reshape(4, C)
    row = lambda a, t: E(a[0][t], a[1][t])
    head = E(*fwd.f64["head"])
    S1 = scale2(add(head[2], head[6]), 0.5)               # from the stored CE and Dice of terms 2, 3
    S2 = scale2(add(head[3], head[7]), 0.5)
    E1, E2 = head[13], head[15]
    gs, gp = (1.0, 1.0) if c.gnull else (float(F32(c.g[0])), float(F32(c.g[2])))
    inv = const32(1.0 / (B * H * W))
    w_sup, w1, w2 = E(0.5 * gs), mul(E(0.5 * gp), E1), mul(E(0.5 * gp), E2)
    y = P["y"]
    g_lab = [_term_grad(P["lab"][m][0], y, w_sup, inv, row(a1, m), row(a2, m), mut) for m in range(2)]

    def pair(parts, S):
        sa, sb, l, var = parts
        ev = exp_(scale2(var, -1.0))
        one = add(E(1.0), mul(S, ev)) if mut == "k_sign" else sub(E(1.0), mul(S, ev))
        k = mul(mul(E(gp), one), inv)
        kb = E(k.v[:, None], k.e[:, None])
        ga = mul(kb, sub(sa[0], sb[0]))
        gb = mul(mul(kb, sb[0]), sub(l, E(var.v[:, None], var.e[:, None])))
        return ga, gb
    ga1, gb1 = pair(P["pa"], S1)                         # (z1_wk, z2_st): k1 carries S1
    ga2, gb2 = pair(P["pb"], S2)                         # (z1_st, z2_wk)
    gb1 = add(gb1, _term_grad(P["pa"][1][0], P["pseudo2"], w2, inv, row(a1, 3), row(a2, 3), mut))      # z2_st: term 3
    ga2 = add(ga2, _term_grad(P["pb"][0][0], P["pseudo1"], w1, inv, row(a1, 2), row(a2, 2), mut))      # z1_st: term 2
    cat = lambda xs: E(np.concatenate([x.v for x in xs]), np.concatenate([x.e for x in xs]))
    return Ref(f64=dict(dz1=_pair(cat([g_lab[0], ga1, ga2])), dz2=_pair(cat([g_lab[1], gb2, gb1]))))


# ---- cut-mix: numpy `where`, bit for bit ----------------------------------------------------------------------------------------------
def _inside(r, H, W, mut: str = ""):
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    inc = 1 if mut == "end_inclusive" else 0
    return (yy >= r[1]) & (yy < r[2] + inc) & (xx >= r[3]) & (xx < r[4] + inc) & bool(r[0])


def cutmix(c: Case, inp: dict, mut: str = "") -> Ref:
    x_l, x_wk, x_st, y_l = inp["x_l"], inp["x_wk"], inp["x_st"], inp["y_l"]
    B, _, H, W = x_l.shape
    o_l, o_y, o_wk, o_st = [], [], [], []
    for i in range(B):
        nb = (i - 1) % B if mut == "neighbour_back" else (i + 1) % B
        m1, m2 = _inside(inp["rl"][i], H, W, mut), _inside(inp["ru"][i], H, W, mut)
        o_l.append(np.where(m1, x_l[nb], x_l[i]))
        o_y.append(y_l[i] if mut == "labels_not_mixed" else np.where(m1, y_l[nb], y_l[i]))
        paste = x_l[i] if mut == "paste_raw" else o_l[i]
        o_wk.append(np.where(m2, paste, x_wk[i]))
        o_st.append(np.where(m2, paste, x_st[i]))
    out = np.stack(o_l + o_wk + o_st).astype(F32)
    return Ref(exact=dict(out=out, y_out=np.stack(o_y).astype(np.int64), amax=amax_after(0.0, out, True)))


# ---- the supervised family: CE (class weights), Dice, Jaccard and Tversky at once ----------------------------------------------------
SEG_TERMS = 1 | 4 | 8 | 16                              # UAPS_SEG_CE | DICE | JACCARD | TVERSKY
SEG_COEF = (0.83, 0.0, 0.57, 1.3, 0.44, 0.0)
SEG_TVERSKY = (0.3, 0.7)


def seg_fwd(c: Case, inp: dict, mut: str = "") -> Ref:
    z = np.asarray(inp["z"], F32)
    B, C, H, W = z.shape
    raw = np.asarray(inp["labels"], np.int64)
    ign = raw == c.ignore if c.ignore is not None else np.zeros(raw.shape, bool)
    y, _ = in_range(raw, C)
    bad = int(((y < 0) & ~ign).sum())
    y = np.where(ign, -1, y)
    ok = y >= 0
    (_, _, items, _, cap), = c.row_sets("fwd")
    n = n_adds(items, cap, c.V("fwd"))
    soft = _soft(z)
    w = np.asarray(inp["class_weight"], F32).astype(F64)
    wy = np.where(ok, w[np.where(ok, y, 0)], 0.0)
    ce_sum, w_sum = _tot(mul(E(wy), _nll(z, soft, y)), n), _tot(E(wy), n)
    p = _where(ok[:, None], soft[0])
    A, I, N = _class_sums(p, y, n)
    eps, (al, be) = float(F32(c.eps)), (float(F32(SEG_TVERSKY[0])), float(F32(SEG_TVERSKY[1])))
    coef = [float(F32(x)) for x in SEG_COEF]
    inv_c = 1.0 / C
    AN = E(A.v + N, A.e)
    d_d = E(AN.v + eps, AN.e)
    d_j = sub(d_d, I)
    d_t = E(I.v + al * (A.v - I.v) + be * (N - I.v) + eps, I.e * (1 + al + be) + al * A.e + 8 * U * (np.abs(I.v) + al * np.abs(A.v) + be * N))
    f = [div(scale2(I, 2.0), d_d), div(I, d_j), div(I, d_t)]
    sq = lambda d: mul(d, d)
    gI = scale2(mul(E(coef[2] * inv_c), div(E(2.0), d_d)), -1.0)
    gA = mul(E(coef[2] * inv_c), div(scale2(I, 2.0), sq(d_d)))
    gI = sub(gI, mul(E(coef[3] * inv_c), div(add(d_j, I), sq(d_j))))
    gA = add(gA, mul(E(coef[3] * inv_c), div(I, sq(d_j))))
    gI = sub(gI, mul(E(coef[4] * inv_c), div(sub(d_t, mul(I, E(1.0 - al - be))), sq(d_t))))
    gA = add(gA, mul(E(coef[4] * inv_c), div(mul(E(al), I), sq(d_t))))
    mean = lambda x: div(E(x.v.sum(), x.e.sum() + C * U * np.abs(x.v).sum()), E(float(C)))
    term = [div(ce_sum, w_sum)] + [sub(E(1.0), mean(x)) for x in f]
    loss = term[0]
    loss = mul(E(coef[0]), loss)
    for k, t in zip((2, 3, 4), term[1:]):
        loss = add(loss, mul(E(coef[k]), t))
    kce = div(E(coef[0]), w_sum)
    ref = Ref(exact=dict(bad=F32(bad), n_valid=F32(ok.sum()), N=N.astype(F32)))
    ref.f64 = dict(terms=_pair(_f32(_stack(term + [loss]))), wsum=_pair(_f32(w_sum)), kce=_pair(_f32(kce)), A=_pair(_f32(A)), I=_pair(_f32(I)),
                   GA=_pair(_f32(gA)), GI=_pair(_f32(gI)))
    ref.parts = dict(y=y, p=soft[0], wy=wy)
    return ref


def seg_bwd(c: Case, inp: dict, fwd: Ref, mut: str = "") -> Ref:
    y, p, wy = fwd.parts["y"], fwd.parts["p"], fwd.parts["wy"]
    C = p.shape[1]
    gs = E(1.0 if c.gnull else float(F32(c.g[0])))
    GA, GI, kce = mul(gs, E(*fwd.f64["GA"])), mul(gs, E(*fwd.f64["GI"])), mul(gs, E(*fwd.f64["kce"]))
    oh = _onehot(y, C)
    d = add(_bc(GA), _where(oh, _bc(GI)))
    dot = csum(mul(p, d))
    inner = d if mut == "no_projection" else sub(d, E(dot.v[:, None], dot.e[:, None]))
    pw = mul(kce, E(wy))
    dz = add(mul(p, inner), mul(E(pw.v[:, None], pw.e[:, None]), sub(p, E(oh.astype(F64)))))
    ok = (y >= 0)[:, None]
    return Ref(f64=dict(dz=(np.where(ok, dz.v, 0.0), np.where(ok, dz.e, 0.0))))


# ---- one reference per case -----------------------------------------------------------------------------------------------------------
FWD = dict(cps=cps_fwd, ucc=ucc_fwd, seg=seg_fwd)
BWD = dict(cps=cps_bwd, ucc=ucc_bwd, seg=seg_bwd)
BWD_MUTS = {"no_projection", "inv_n_other", "ce_on_minus1", "k_sign"}


def reference(c: Case, inp: dict, mut: str = "") -> Ref:
    """Forward and backward of a case as one Ref (cut-mix: its outputs)."""
    if c.entry == "cutmix":
        return cutmix(c, inp, mut)
    fwd = FWD[c.entry](c, inp, "" if mut in BWD_MUTS else mut)
    bwd = BWD[c.entry](c, inp, fwd, mut if mut in BWD_MUTS else "")
    fwd.f64.update(bwd.f64)
    return fwd


def swallowed(ref: Ref) -> list:
    """The compared tensors whose largest bar is not below 2^-10 of their largest |reference value|."""
    out = []
    for k, (val, bar) in ref.f64.items():
        top = float(np.max(np.abs(val)))
        if not float(np.max(bar)) < SWALLOW * top:
            out.append((k, float(np.max(bar)), top))
    return out


# ---- the case table -------------------------------------------------------------------------------------------------------------------
V4, V1A, V1B = (16, 24), (5, 7), (37, 53)
OUT4 = ("pseudo1", "pseudo2", "var1", "var2")
PTR_REASONS = {"cps": (("z1",), ("pseudo1",), ("dz2",), ("labels",)), "ucc": (("z2",), ("pseudo1",), ("var2",), ("dz2",), ("labels",)),
               "seg": (("z",), ("dz",), ("labels",))}


def _combos(names):
    return [tuple(n for j, n in enumerate(names) if (i >> j) & 1) for i in range(1 << len(names))]


def _cases():
    cs = []

    def add_(id, entry, **p):
        cs.append(Case(id, entry, **p))
    for i, C in enumerate(CLASSES):
        N = 3 + i % 2
        blab = (1, N - 1)[i % 2]
        # CPS: every C in both forms, by shape and by each pointer of either launch; B_lab = 1 and N - 1
        add_(f"cps-c{C}-v4", "cps", shape=(N, C) + V4, B_lab=blab)
        add_(f"cps-c{C}-v1", "cps", shape=(N, C) + (V1A, V1B)[i % 2], B_lab=(N - 1, 1)[i % 2], gnull=i % 3 == 0)
        who = PTR_REASONS["cps"][i % 4]
        add_(f"cps-c{C}-ptr-{who[0]}", "cps", shape=(N, C) + V4, B_lab=blab, offs={who[0]: 1})
        # UCC
        add_(f"ucc-c{C}-v4", "ucc", shape=(1 + i % 3, C) + V4)
        add_(f"ucc-c{C}-v1", "ucc", shape=(1 + (i + 1) % 3, C) + (V1A, V1B)[i % 2], gnull=i % 3 == 1)
        who = PTR_REASONS["ucc"][i % 5]
        add_(f"ucc-c{C}-ptr-{who[0]}", "ucc", shape=(2, C) + V4, offs={who[0]: 1})
    # every pointer reason once per family (the sweep over C above rotates through them; these make each explicit at one C)
    for e in ("cps", "ucc"):
        for who in PTR_REASONS[e]:
            add_(f"{e}-ptr-{who[0]}", e, shape=(3 if e == "cps" else 2, 3) + V4, offs={who[0]: 1}, B_lab=2)
    # optional outputs: each NULL / non-NULL combination once in either form
    for j, outs in enumerate(_combos(OUT4[:2])):
        add_(f"cps-outs{j}-v4", "cps", shape=(3, 4) + V4, outs=outs, B_lab=2)
        add_(f"cps-outs{j}-v1", "cps", shape=(3, 4) + V1A, outs=outs, B_lab=1)
    for j, outs in enumerate(_combos(OUT4)):
        add_(f"ucc-outs{j}-v4", "ucc", shape=(2, 2 + j % 7) + V4, outs=outs)
        add_(f"ucc-outs{j}-v1", "ucc", shape=(1, 2 + (j + 3) % 7) + V1A, outs=outs)
    # input regimes, degenerate maps, label edges
    for j, r in enumerate(REGIMES[1:]):
        add_(f"cps-{r}-v4", "cps", shape=(4, 3 + j) + V4, B_lab=2, regime=r)
        add_(f"cps-{r}-v1", "cps", shape=(3, 6 - j) + V1B, B_lab=1, regime=r)
        add_(f"ucc-{r}-v4", "ucc", shape=(2, 3 + j) + V4, regime=r)
        add_(f"ucc-{r}-v1", "ucc", shape=(1, 6 - j) + V1B, regime=r)
    for e in ("cps", "ucc"):
        add_(f"{e}-1x40", e, shape=(2, 5, 1, 40), B_lab=1)
        add_(f"{e}-1x1", e, shape=(2, 3, 1, 1), B_lab=1, eps=1e-3)
        add_(f"{e}-edges-v4", e, shape=(3, 4) + V4, B_lab=2, edges=True)
        add_(f"{e}-edges-v1", e, shape=(3, 6) + V1B, B_lab=2, edges=True)
    # the second trip of the grid-stride loops (one coefficient set, every tensor below 30 MB)
    add_("cps-trip-v1", "cps", shape=(2, 2, 363, 363), B_lab=1, heavy=True)
    add_("ucc-trip-v1", "ucc", shape=(1, 2, 513, 513), heavy=True)
    add_("ucc-trip-v4", "ucc", shape=(1, 2, 1026, 1024), heavy=True)
    # cut-mix: the row wrap of the four-pixel form (H W % 4 == 0, W % 4 != 0), each pointer off, Cin = 1, the largest batch, two trips
    for j, (H, W) in enumerate(((4, 6), (6, 10), V4, V1A, V1B, (1, 40), (1, 1))):
        for kind in ("mixed", "full", "off", "empty", "column"):
            add_(f"cutmix-{H}x{W}-{kind}", "cutmix", shape=(1 + (j + len(kind)) % 3, 2, H, W), rects=kind, Cin=1 + (j + len(kind)) % 3, hinted=j % 2 == 1)
    for who in VEC_SETS[("cutmix", "fwd")]:
        add_(f"cutmix-ptr-{who}", "cutmix", shape=(2, 2, 6, 10), offs={who: 1})
    add_("cutmix-b64", "cutmix", shape=(UCC_MAX_BATCH, 2, 4, 6), Cin=1)
    add_("cutmix-trip-v1", "cutmix", shape=(2, 2, 725, 725), Cin=1, heavy=True)
    add_("cutmix-trip-v4", "cutmix", shape=(2, 2, 840, 840), Cin=3, heavy=True)
    # seg: what tests/test_gpu_seglosses.py lacks -- C = 5 and 6 in both forms, by shape and by pointer, in guarded buffers
    for C in (5, 6):
        add_(f"seg-c{C}-v4", "seg", shape=(2, C) + V4, ignore=255 if C == 5 else None)
        add_(f"seg-c{C}-v1", "seg", shape=(3, C) + V1B, ignore=255 if C == 6 else None, gnull=C == 6)
        for who in PTR_REASONS["seg"]:
            add_(f"seg-c{C}-ptr-{who[0]}", "seg", shape=(2, C) + V4, offs={who[0]: 1})
    add_("seg-edges-v4", "seg", shape=(2, 5) + V4, edges=True, ignore=255)
    add_("seg-edges-v1", "seg", shape=(2, 6) + V1A, edges=True)
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def seg_sweep_kernels() -> frozenset:
    """What the float64 sweep of tests/test_gpu_seglosses.py launches, by the same restatement: it goes through the Python surface, whose
    gradient buffer is aligned, so only H W % 4 and the `misaligned` logits decide the form, for forward and backward alike."""
    from test_gpu_seglosses import _SWEEP
    out = set()
    for B, C, H, W, _, misaligned in _SWEEP:
        out |= Case("sweep", "seg", shape=(B, C, H, W), offs=dict(z=1, dz=1) if misaligned else {}).kernels
    return frozenset(out)

# mutant -> a case on which it must be rejected (the 1x1 map with eps = 1e-3 for the dropped eps; a label-edge case for the CE
# gradient of a y = -1 pixel; a case whose two row sets differ in size for inv_n)
MUTANTS = {"own_argmax": "cps-c4-v4", "unl_in_gt": "cps-c3-v1", "tie_high": "cps-c5-v4", "no_eps": "cps-1x1", "no_projection": "cps-c6-v4",
           "inv_n_other": "cps-c2-v4", "ce_on_minus1": "cps-edges-v4", "var_swapped": "ucc-c4-v4", "pseudo1_from_z1": "ucc-c3-v1",
           "no_exp": "ucc-c5-v4", "k_sign": "ucc-c6-v4", "neighbour_back": "cutmix-4x6-mixed", "end_inclusive": "cutmix-6x10-mixed",
           "labels_not_mixed": "cutmix-4x6-full", "paste_raw": "cutmix-37x53-full"}
MUTANTS_ALSO = [("tie_high", "ucc-c4-v1"), ("no_eps", "ucc-1x1"), ("no_projection", "ucc-c7-v4"), ("ce_on_minus1", "ucc-edges-v1"),
                ("no_projection", "seg-c5-v4")]

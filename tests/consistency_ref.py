"""The teacher and consistency kernels -- Mean Teacher / UAMT (uaps_amd/csrc/loss_mean_teacher.hip), CCT / DCT (loss_cct_dct.hip) and
the two-tensor softmax terms of the first half of pair_ops.hip: references in plain numpy, the comparison code, and one case per entry
point, class count, layout and launch rule (tests/test_consistency_ref.py, tests/test_gpu_consistency_forms.py).

Two kinds of reference, as in tests/ops_ref.py.

Bit-exact float32 restatements (Ref.exact): the EMA update fma(1 - a, p, rn(e a)), formed without double rounding (the exact product
and sum in float64, rounded to odd, then once to float32); teacher_noise_apply (one multiply, a clamp, one add); rot90_batch (a copy,
a permutation, max|.|); sum m of the masked forward (a count); and the mask byte wherever the float64 uncertainty is further from the
threshold than its bar.

float64 values with a bar per quantity (Ref.f64; |got - value| / bar must stay <= 1).  The bar is a running error bound: the float64
reference walks the kernel's own operation sequence and carries, beside every value, a bound of what float32 can have lost so far
(class E below).  Each float32 operation adds U |result| (U = 2^-24, half an ulp: one correctly rounded operation) and propagates its
operands' bounds to first order; a product that the compiler contracts into an fma rounds once less, so the bound holds either way.
The function calls add, with 1 ulp = 2 U relative:
    loss_mean_teacher.hip, loss_cct_dct.hip, philox.hpp (IEEE forms): expf 3 ulp, logf 3 ulp, sincospif 4 ulp (the OpenCL full-profile
        limits the device library is built to), `/` and sqrtf 1 ulp (correctly rounded by default: 0.5 ulp would do)
    pair_ops.hip (fast forms), from what the instructions give: __expf(d) is v_exp_f32(rn(d log2e)): the product's rounding and the
        rounded constant move the exponent by 2 U |d| log2e, i.e. the result by 2 U |d| relative, and v_exp_f32 adds 1 ulp;
        __logf is v_log_f32 (1 ulp of log2 x) times ln 2 in extended precision: 2 ulp relative, plus an ABSOLUTE 2 U, because a
        relative bound cannot be relied on where log2 x crosses zero (the sums of a saturated softmax are 1 + tiny);
        __builtin_amdgcn_rcpf is v_rcp_f32: 1 ulp.
    results below 2^-126 may be flushed: every operation adds TINY = 2^-126 absolute.
A sum over pixels gets (n + 2) U sum |term| for the n float32 additions an element can pass through (the lane's strided loop, the six
shuffles, the LDS round) beside the terms' own bounds; the block partials are added in double.  No bar is fitted to what a kernel returns.

A UAMT pixel whose float64 uncertainty lies within its bar of the threshold may get either mask bit: the reference takes the kernel's
bit there (Ref.finish) and such pixels may be at most AMBIG_CAP of the case, asserted on the reference before the device is asked.  A
teacher-noise draw within its bar of the clamp edge may be clamped or not (the clamp is continuous, so its value bar holds either
way); such draws are counted and held to EDGE_CAP.

Every case names the kernel instantiations it must reach, derived from the launchers' own rules (UAPS_BY_C, the `vec` rule of
uaps_cct_consistency_*, grid_for); the CPU test checks that the cases together name every kernel of the three sources found in the
built code object.  A mutant is a switch on a reference (`mut`): the CPU test proves with them that the comparisons bite.
"""
from __future__ import annotations

import math

import numpy as np

from bn_ref import rng_for
from ops_ref import Ref, amax_after, bits_differ, words

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
ULP_EXP, ULP_LOG, ULP_SINCOS, ULP_DIV, ULP_SQRT, ULP_RCP = 3, 3, 4, 1, 1, 1
MAX_CLASSES, MAX_T, MAX_HEADS = 8, 16, 8            # UAPS_MAX_CLASSES, UAPS_MC_MAX_T, UAPS_CCT_MAX_HEADS
THREADS, MAX_BLOCKS, NOISE_BLOCKS = 256, 1024, 4096
EMA_BATCH, EMA_CHUNK, TILE = 128, 1024, 32
AMBIG_CAP, EDGE_CAP = 0.01, 0.001
EPS6 = float(F32(1e-6))
M64 = (1 << 64) - 1


def grid_for(items: int, cap: int = MAX_BLOCKS) -> int:
    return max(1, min(cap, (items + THREADS - 1) // THREADS))


def lane_adds(items: int, cap: int = MAX_BLOCKS, inner: int = 1) -> int:
    """float32 additions a term can pass through on its way into a block partial."""
    return -(-items // (grid_for(items, cap) * THREADS)) + inner + 8


# ---- values with running error bounds -----------------------------------------------------------------------------------------
class E:
    """v: float64 values of the exact formula; e: a bound of |float32 kernel value - v|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, F64)
        self.e = np.zeros_like(self.v) + e

    def __getitem__(self, i):
        return E(self.v[i], self.e[i])

    @property
    def shape(self):
        return self.v.shape


def _E(x) -> E:
    return x if isinstance(x, E) else E(x)


def _rnd(v, e, ulps=0.5) -> E:
    return E(v, e + 2 * ulps * U * np.abs(v) + TINY)


def const32(x: float) -> E:
    """A constant the launcher rounds to float32: the exact value of the plain formula, the rounding as its bound."""
    return E(x, abs(x - float(F32(x))))


def add(a, b) -> E:
    a, b = _E(a), _E(b)
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b) -> E:
    a, b = _E(a), _E(b)
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b) -> E:
    a, b = _E(a), _E(b)
    return _rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def scale2(a, k) -> E:
    """a power of two times a: exact."""
    a = _E(a)
    return E(a.v * k, a.e * abs(k))


def div(a, b) -> E:
    a, b = _E(a), _E(b)
    q = a.v / b.v
    return _rnd(q, (a.e + np.abs(q) * b.e) / np.maximum(np.abs(b.v) - b.e, TINY), ULP_DIV)


def rcp(b) -> E:
    b = _E(b)
    q = 1.0 / b.v
    return _rnd(q, np.abs(q) * b.e / np.maximum(np.abs(b.v) - b.e, TINY), ULP_RCP)


def exp_(a: E, fast: bool = False) -> E:
    v = np.exp(a.v)
    if fast:
        return _rnd(v, v * np.expm1(a.e + 2 * U * np.abs(a.v)), 1)
    return _rnd(v, v * np.expm1(a.e), ULP_EXP)


def log_(a: E, fast: bool = False) -> E:
    """log of a positive value (the callers keep a.v > 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(a.v)
        r = np.minimum(a.e / np.maximum(a.v, TINY), 0.5)
    r = -np.log1p(-r)
    if fast:
        return _rnd(v, r + 2 * U, 2)
    return _rnd(v, r, ULP_LOG)


def sqrt_(a: E) -> E:
    v = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a.e > 0, np.minimum(a.e / np.maximum(v + np.sqrt(np.maximum(a.v - a.e, 0.0)), TINY), v + np.sqrt(a.e)), 0.0)
    return _rnd(v, r, ULP_SQRT)


def xlogx(t: E, fast: bool) -> E:
    """t > 0 ? t log t : 0, the bound taken over the whole interval of t (t log t has an infinite slope at 0)."""
    f = lambda x: np.where(x > 0, x * np.log(np.where(x > 0, x, 1.0)), 0.0)
    v, hi, lo = f(t.v), f(t.v + t.e), f(np.maximum(t.v - t.e, 0.0))
    inner = np.maximum(np.abs(hi - v), np.abs(lo - v)) + np.where((t.v - t.e < math.exp(-1)) & (t.v + t.e > math.exp(-1)), 3 * t.e * t.e, 0.0)
    logerr = (2 * (2 if fast else ULP_LOG) * U) * np.abs(v) + (2 * U * np.abs(t.v) if fast else 0.0)
    return _rnd(v, inner + logerr)


def csum(x: E) -> E:
    """The sequential float32 sum over axis 1 (the classes), c = 0, 1, ... (a kernel that starts from acc = 0 adds the first term
    exactly)."""
    acc = x[:, 0]
    for c in range(1, x.shape[1]):
        acc = add(acc, x[:, c])
    return acc


def total(x: E, n_adds: int):
    """(float64 sum, bar) of the float32 terms x summed by a block-partial reduction of n_adds float32 additions per term."""
    return float(x.v.sum()), float(x.e.sum() + (n_adds + 2) * U * np.abs(x.v).sum())


def softmax_E(z, fast: bool = False):
    """(p, s, mx, z) over axis 1 as softmax_p / softmax_inplace (IEEE) or softmax_c of pair_ops.hip (fast) form it."""
    z = _E(np.asarray(z, F64))
    mx = z.v.max(axis=1, keepdims=True)
    e = exp_(sub(z, E(mx)), fast)
    s = csum(e)
    sb = E(s.v[:, None], s.e[:, None])
    p = mul(e, rcp(sb)) if fast else div(e, sb)
    return p, s, mx[:, 0], z


def log_softmax_fast(z: E, s: E, mx) -> E:
    """lp[c] = z[c] - (mx + __logf(s)): pair_ops.hip's softmax_c.  The bar follows the kernel's own association, so it grows with
    U |z|: under the +1e4 shift it is about 5000 times what (z - mx) - log s would need, and the shift regime therefore cannot flag
    that conditioning loss (the pair_ops paragraph, records it)."""
    lse = add(E(mx), log_(s, fast=True))
    return sub(z, E(lse.v[:, None], lse.e[:, None]))


# ---- EMA --------------------------------------------------------------------------------------------------------------------
def _rn32_sum(a, b) -> np.ndarray:
    """rn_float32(a + b) of float64 arrays, rounded ONCE: TwoSum gives the exact remainder, the float64 sum is rounded to odd."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return odd.astype(F32)


def ema(e, p, alpha, oma, mut: str = "") -> np.ndarray:
    """fma(oma, p, rn(e alpha)) in float32, exactly: the products of two float32 are exact in float64."""
    e64, p64, a, o = np.asarray(e, F32).astype(F64), np.asarray(p, F32).astype(F64), float(F32(alpha)), float(F32(oma))
    if mut == "round_once":
        return _rn32_sum(e64 * a, p64 * o)
    return _rn32_sum((e64 * a).astype(F32).astype(F64), p64 * o)


def ema_alpha(alpha: float, step: int):
    """uaps_amd.mean_teacher.ema_alpha (update_ema_variables): step 0 gives (0, 1), a bit copy of the student."""
    a = min(1 - 1 / (step + 1), alpha)
    return a, 1.0 - a


# ---- teacher noise ----------------------------------------------------------------------------------------------------------
C01, C02 = F32(0.1), F32(0.2)


def noise_apply(x, noise, B: int, T: int) -> np.ndarray:
    """out[r] = x[r % B] + clamp(rn(0.1 n), -0.2, 0.2), (1 + T) B rows, in float32."""
    x = np.asarray(x, F32)
    nz = np.clip((np.asarray(noise, F32).reshape(-1) * C01).astype(F32), -C02, C02)
    return (np.tile(x.reshape(-1), 1 + T) + nz).astype(F32).reshape(((1 + T) * B,) + x.shape[1:])


def gauss_E(seed: int, offset: int, n: int, mut: str = "") -> E:
    """Element i of the draw: counter offset + i / 4, words (0, 1) -> elements 0, 1 and words (2, 3) -> elements 2, 3 of the
    counter, Box-Muller as gauss2 of csrc/philox.hpp."""
    n4 = (n + 3) // 4
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset & M64) + np.arange(n4, dtype=np.uint64)
    w = words(seed, ctr, mut).astype(np.uint64)                         # [n4, 4]
    out_v, out_e = np.empty((n4, 4)), np.empty((n4, 4))
    for h in range(2):
        a, b = w[:, 2 * h], w[:, 2 * h + 1]
        u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(F64) * U      # exact in float32
        u2 = (b >> np.uint64(8)).astype(F64) * U
        rad = sqrt_(scale2(log_(E(u1)), -2.0))
        ang = 2.0 * u2                                                  # exact
        for q, tr in enumerate((np.cos(np.pi * ang), np.sin(np.pi * ang))):
            t = E(tr, 2 * ULP_SINCOS * U * np.abs(tr) + TINY)
            r = mul(rad, t)
            out_v[:, 2 * h + q], out_e[:, 2 * h + q] = r.v, r.e
    return E(out_v.reshape(-1)[:n], out_e.reshape(-1)[:n])


def noise_draw(x, B: int, T: int, seed: int, offset: int, mut: str = ""):
    """(value, bar, draws within their bar of the clamp edge) of uaps_teacher_noise."""
    x = np.asarray(x, F32)
    total_n = (1 + T) * x.size
    g = mul(gauss_E(seed, offset, total_n, mut), E(float(C01)))
    edge = int((np.abs(np.abs(g.v) - float(C02)) <= g.e).sum())
    nz = E(np.clip(g.v, -float(C02), float(C02)), g.e)
    out = add(E(np.tile(x.reshape(-1).astype(F64), 1 + T)), nz)
    shape = ((1 + T) * B,) + x.shape[1:]
    return out.v.reshape(shape), out.e.reshape(shape), edge


# ---- Mean Teacher / UAMT consistency -------------------------------------------------------------------------------------------
def _sq_dist(p: E, q: E) -> E:
    t = sub(p, q)
    return csum(mul(t, t))


def mc_uncertainty(mc, T: int, mut: str = "") -> E:
    """u = -sum_c pb log(pb + 1e-6), pb = (1/T) sum_t softmax(mc_t) (T > 0) or mc itself (T = 0)."""
    if T > 0:
        mc = np.asarray(mc, F32)
        pb = softmax_E(mc[0])[0]
        for t in range(1, T):
            pb = add(pb, softmax_E(mc[t])[0])
        if mut != "t_sum":
            pb = mul(pb, const32(1.0 / T))
    else:
        pb = E(np.asarray(mc, F64))
    lg = log_(pb if mut == "no_eps" else add(pb, E(EPS6)))
    term = mul(pb, lg)
    u = scale2(term[:, 0], -1.0)
    for c in range(1, term.shape[1]):
        u = sub(u, term[:, c])
    return u


def mc_fwd(s, e, mc=None, T: int = 0, thr: float = 0.0, want_unc: bool = True, mut: str = "") -> Ref:
    """uaps_mc_consistency_fwd: MT mode (mc None) or masked.  Ref.finish(got) completes the masked loss with the kernel's bits on
    the ambiguous pixels; Ref.info holds their count."""
    s = np.asarray(s, F32)
    B, C, H, W = s.shape
    N = B * H * W
    d = _sq_dist(softmax_E(s)[0], softmax_E(e)[0])
    n_adds = lane_adds(N, inner=C)
    ref = Ref()
    ref.info = dict(ambiguous=0, pixels=N)
    if mc is None:
        S, bar = total(d, n_adds)
        norm = N if mut == "nc_vs_n" else N * C
        ref.f64 = dict(loss=(S / norm, bar / norm + 4 * U * abs(S / norm) + TINY), sum_md=(S, bar + 2 * U * abs(S)))
        ref.exact = dict(sum_m=F32(N))
        ref.finish = None
        return ref
    u = mc_uncertainty(mc, T, mut)
    t = float(F32(thr))
    m_ref = u.v < t
    amb = np.abs(u.v - t) <= u.e
    ref.info["ambiguous"] = int(amb.sum())
    if want_unc:
        ref.f64["unc"] = (u.v, u.e)

    def finish(got):
        gm = np.asarray(got["mask"]).reshape(m_ref.shape) != 0
        m = np.where(amb, gm, m_ref)
        ref.exact["mask"] = m.astype(np.uint8)                        # the kernel's bit on the ambiguous pixels, 0 / 1 bytes everywhere
        S, bar = total(E(np.where(m, d.v, 0.0), np.where(m, d.e, 0.0)), n_adds)
        sm = float(m.sum())
        den = (sm if mut == "denom_m" else 2.0 * sm) + 1e-16
        ref.exact["sum_m"] = F32(sm)
        ref.f64["loss"] = (S / den, bar / den + 6 * U * abs(S / den) + TINY)
        ref.f64["sum_md"] = (S, bar + 2 * U * abs(S))
        ref.finish = None
        return ref
    ref.finish = finish
    ref.mask_ref = m_ref
    return ref


def mc_bwd(s, e, mask, g: float, sum_m, mut: str = "") -> Ref:
    """ds_c = k 2 p_c [(p_c - q_c) - sum_k p_k (p_k - q_k)], k = g m / (2 sum m + 1e-16) (masked) or g / (B C H W) (MT)."""
    s = np.asarray(s, F32)
    B, C, H, W = s.shape
    N = B * H * W
    p, q = softmax_E(s)[0], softmax_E(e)[0]
    if mask is None:
        scale = mul(E(float(F32(g))), const32(1.0 / (N if mut == "nc_vs_n" else N * C)))
        k = E(np.full((B, 1, H, W), scale.v), scale.e)
    else:
        den = add(scale2(E(float(F32(sum_m))), 1.0 if mut == "denom_m" else 2.0), E(1e-16))
        scale = div(E(float(F32(g))), den)
        m = (np.asarray(mask).reshape(B, 1, H, W) != 0)
        k = E(np.where(m, scale.v, 0.0), np.where(m, scale.e, 0.0))
    diff = sub(p, q)
    dot = csum(mul(p, diff))
    inner = sub(diff, E(dot.v[:, None], dot.e[:, None]))
    ds = mul(k, mul(scale2(p, 2.0), inner))
    ref = Ref(f64=dict(ds=(ds.v, ds.e)))
    return ref


# ---- CCT ----------------------------------------------------------------------------------------------------------------------
def _win(x, b0, B):
    return np.asarray(x)[b0:b0 + B]


def cct_fwd(heads, b0: int, B: int, vec: bool, mut: str = "") -> Ref:
    """out[0] = (1 / (D - 1)) sum_k mean((softmax(z0) - softmax(zk))^2), out[k] = the k-th sum, over rows [b0, b0 + B)."""
    if mut == "window_ignored":
        b0 = 0
    D = len(heads)
    _, C, H, W = np.asarray(heads[0]).shape
    npix = B * H * W
    V = 4 if vec else 1
    n_adds = lane_adds(npix // V, inner=C * V)
    p0 = softmax_E(_win(heads[0], b0, B))[0]
    sums, bars = [], []
    for k in range(1, D):
        S, bar = total(_sq_dist(p0, softmax_E(_win(heads[k], b0, B))[0]), n_adds)
        sums.append(S)
        bars.append(bar)
    div_ = (D if mut == "d_vs_dm1" else D - 1) * npix * C
    loss = sum(sums) / div_
    ref = Ref(f64=dict(loss=(loss, sum(bars) / div_ + 2 * U * abs(loss) + TINY)))
    ref.f64["sums"] = (np.array(sums), np.array(bars) + 2 * U * np.abs(np.array(sums)))
    return ref


def cct_bwd(heads, b0: int, B: int, g: float, mut: str = "") -> Ref:
    """dz of every head inside the window: a = g 2 / ((D - 1) n), head k: -a pk (diff_k - <pk, diff_k>), head 0: a p0 (s - <p0, s>),
    s = sum_k diff_k, diff_k = p0 - pk.  Ref.f64["dz<k>"] covers the window's rows only."""
    if mut == "window_ignored":
        b0 = 0
    D = len(heads)
    _, C, H, W = np.asarray(heads[0]).shape
    npix = B * H * W
    a = mul(E(float(F32(g))), const32(2.0 / ((D if mut == "d_vs_dm1" else D - 1) * float(npix) * C)))
    p0 = softmax_E(_win(heads[0], b0, B))[0]
    ref, s = Ref(), None
    for k in range(1, D):
        pk = softmax_E(_win(heads[k], b0, B))[0]
        diff = sub(p0, pk)
        dot = csum(mul(pk, diff))
        dz = mul(scale2(a, -1.0), mul(pk, sub(diff, E(dot.v[:, None], dot.e[:, None]))))
        ref.f64[f"dz{k}"] = (dz.v, dz.e)
        if s is None:
            s = diff                                     # 0 + diff is exact
        elif mut != "head0_no_sum":
            s = add(s, diff)
    dot = csum(mul(p0, s))
    dz = mul(a, mul(p0, sub(s, E(dot.v[:, None], dot.e[:, None]))))
    ref.f64["dz0"] = (dz.v, dz.e)
    return ref


# ---- DCT: the rotated batch and the rotation consistency ------------------------------------------------------------------------
def rot90(x, k: int, mut: str = ""):
    if mut == "k_swap" and k in (1, 3):
        k = 4 - k
    return np.ascontiguousarray(np.rot90(x, k, axes=(2, 3)))


def rot90_batch(xl, xu, k: int, start: float = None, mut: str = "") -> Ref:
    xl, xu = np.asarray(xl, F32), np.asarray(xu, F32)
    ref = Ref(exact=dict(cat=np.concatenate([xl.reshape(-1), xu.reshape(-1)]), rot=rot90(xu, k, mut)))
    if start is not None:
        ref.exact["amax"] = amax_after(start, np.concatenate([xl.reshape(-1), xu.reshape(-1)]), True)
    return ref


def _apply_E(x: E, f) -> E:
    return E(f(x.v), f(x.e))


def rot_fwd(r, r_b0, u, u_b0, B: int, k: int, mut: str = "") -> Ref:
    """out2 = [mean((softmax(r) - rot90(softmax(u), k))^2), the sum]."""
    if mut == "window_ignored":
        r_b0 = u_b0 = 0
    pr = softmax_E(_win(r, r_b0, B))[0]
    pu = _apply_E(softmax_E(_win(u, u_b0, B))[0], lambda a: rot90(a, k, mut))
    _, C, Ho, Wo = pr.shape
    tiles = B * (-(-Ho // TILE)) * (-(-Wo // TILE))
    n_adds = 4 * C * (-(-tiles // min(tiles, MAX_BLOCKS))) + 8          # a lane adds 4 rows x C classes per tile
    t = sub(pr, pu)
    S, bar = total(mul(t, t), n_adds)
    n = B * C * Ho * Wo
    return Ref(f64=dict(loss=(S / n, bar / n + 2 * U * abs(S / n) + TINY), sum=(S, bar + 2 * U * abs(S))))


def rot_bwd(r, r_b0, u, u_b0, B: int, k: int, g: float, mut: str = "") -> Ref:
    """dr = a pr (d - <pr, d>), du = -a pu (d - <pu, d>) rotated back, d = pr - rot90(pu), a = g 2 / n; the windows' rows only."""
    if mut == "window_ignored":
        r_b0 = u_b0 = 0
    pr = softmax_E(_win(r, r_b0, B))[0]
    pu = _apply_E(softmax_E(_win(u, u_b0, B))[0], lambda a: rot90(a, k, mut))
    _, C, Ho, Wo = pr.shape
    a = mul(E(float(F32(g))), const32(2.0 / (float(B * Ho * Wo) * C)))
    d = sub(pr, pu)
    dotr, dotu = csum(mul(pr, d)), csum(mul(pu, d))
    dr = mul(a, mul(pr, sub(d, E(dotr.v[:, None], dotr.e[:, None]))))
    du = mul(scale2(a, -1.0), mul(pu, sub(d, E(dotu.v[:, None], dotu.e[:, None]))))
    if mut == "du_detached":
        du = E(np.zeros_like(du.v), du.e)
    du = _apply_E(du, lambda x: rot90(x, (4 - (4 - k if mut == "k_swap" and k in (1, 3) else k)) % 4))
    return Ref(f64=dict(dr=(dr.v, dr.e), du=(du.v, du.e)))


# ---- pair_ops.hip: the two-tensor softmax terms --------------------------------------------------------------------------------
def pair_fwd(a, b, probs: bool, mut: str = "") -> Ref:
    """mse_map = (softmax(a) - softmax(b))^2, kl_map = sum_c KLDivLoss('none')(log_softmax(a), softmax(b)), kl_mean = its mean over
    all B C H W elements; probs: a, b are probabilities and the input is log(a).  Ref.nonfinite: the per-pixel kind of kl_map
    (0 finite, 1 +inf, 2 -inf, 3 NaN) that the output must show exactly."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    B, C, H, W = a.shape
    N = B * H * W
    ref = Ref()
    if probs:
        a64, b64 = a.astype(F64), b.astype(F64)
        with np.errstate(divide="ignore", invalid="ignore"):
            plain = (np.where(b64 > 0, b64 * np.log(np.where(b64 > 0, b64, 1.0)), 0.0) - b64 * np.log(a64)).sum(axis=1)
        kind = np.where(np.isnan(plain), 3, np.where(plain == np.inf, 1, np.where(plain == -np.inf, 2, 0)))
        ok = (kind == 0)[:, None] & np.ones_like(a64, bool)
        p, t = E(np.where(ok, a64, 1.0)), E(b64)
        lp = log_(p, fast=True)
    else:
        kind = np.zeros((B, H, W), int)
        p, s, mx, z = softmax_E(a, fast=True)
        lp = log_softmax_fast(z, s, mx)
        t = softmax_E(b, fast=True)[0]
    d = sub(p, t) if not probs else sub(E(a.astype(F64)), t)
    mse = mul(d, d)
    term = sub(xlogx(t, True), mul(t, lp))
    kl = term[:, 0]                                                   # 0 + term is exact
    for c in range(1, C):
        kl = add(kl, term[:, c])
    fin = kind == 0
    ref.nonfinite = kind
    ref.f64["mse_map"] = (mse.v, mse.e)
    ref.f64["kl_map"] = (np.where(fin, kl.v, 0.0), np.where(fin, kl.e, 0.0))
    if fin.all():                                                     # the mean is compared on all-finite cases only
        S, bar = total(kl, lane_adds(N))
        den = N if mut == "nc_vs_n" else N * C
        ref.f64["kl_mean"] = (S / den, bar / den + 2 * U * abs(S / den) + TINY)
    return ref


def mse_bwd(a, b, gmap) -> Ref:
    """da_j = 2 p_j [G_j (p_j - t_j) - sum_c G_c (p_c - t_c) p_c]."""
    p, t = softmax_E(a, fast=True)[0], softmax_E(b, fast=True)[0]
    G = mul(E(np.asarray(gmap, F64)), sub(p, t))
    dot = csum(mul(G, p))
    da = mul(scale2(p, 2.0), sub(G, E(dot.v[:, None], dot.e[:, None])))
    return Ref(f64=dict(da=(da.v, da.e)))


def _klmap_db(p_parts, q_parts, G: E) -> E:
    (p, sp, mp, za), (q, sq, mq, zb) = p_parts, q_parts
    dl = sub(log_softmax_fast(zb, sq, mq), log_softmax_fast(za, sp, mp))
    v = csum(mul(q, dl))
    return mul(mul(G, q), sub(dl, E(v.v[:, None], v.e[:, None])))


def kl_bwd(a, b, g, mut: str = "") -> Ref:
    """da_j = g (p_j - t_j) / numel (g = 1 when no upstream scalar is given); the target gets no gradient."""
    a = np.asarray(a, F32)
    pa, pb = softmax_E(a, fast=True), softmax_E(b, fast=True)
    gs = mul(E(float(F32(1.0 if g is None else g))), const32(1.0 / a.size))
    da = mul(gs, sub(pa[0], pb[0]))
    if mut == "target_grad":                              # as if b were the same tensor and received its own gradient too
        da = add(da, _klmap_db(pa, pb, E(np.full((a.shape[0], 1) + a.shape[2:], gs.v))))
    return Ref(f64=dict(da=(da.v, da.e)))


def klmap_bwd(a, b, gmap, mut: str = "") -> Ref:
    """da_j = G (p_j - q_j), db_j = G q_j ((log q_j - log p_j) - v), v = the pixel's KL."""
    a = np.asarray(a, F32)
    pa, pb = softmax_E(a, fast=True), softmax_E(b, fast=True)
    G = E(np.asarray(gmap, F64).reshape(a.shape[0], 1, a.shape[2], a.shape[3]))
    da = mul(G, sub(pa[0], pb[0]))
    db = _klmap_db(pa, pb, G)
    if mut == "target_detached":
        db = E(np.zeros_like(db.v), db.e)
    return Ref(f64=dict(da=(da.v, da.e), db=(db.v, db.e)))


def entropy(p, mut: str = "") -> Ref:
    """ent = -sum_c p log(p + 1e-6), and its mean over the pixels."""
    p = E(np.asarray(p, F32).astype(F64))
    term = mul(p, log_(p if mut == "no_eps" else add(p, E(EPS6)), fast=True))
    ent = scale2(term[:, 0], -1.0)
    for c in range(1, term.shape[1]):
        ent = sub(ent, term[:, c])
    N = ent.v.size
    S, bar = total(ent, lane_adds(N))
    return Ref(f64=dict(ent_map=(ent.v, ent.e), ent_mean=(S / N, bar / N + 2 * U * abs(S / N) + TINY)))


# ---- the comparison both test files use ----------------------------------------------------------------------------------------
def bar_ratio(got, val, bar) -> float:
    got, val, bar = np.asarray(got, F64), np.asarray(val, F64), np.asarray(bar, F64)
    if got.shape != val.shape or not np.all(np.isfinite(got)):
        return math.inf
    d = np.abs(got - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bar)
    return float(np.max(q)) if q.size else 0.0


def kinds(x) -> np.ndarray:
    x = np.asarray(x)
    return np.where(np.isnan(x), 3, np.where(x == np.inf, 1, np.where(x == -np.inf, 2, 0)))


def compare(ref: Ref, got: dict):
    """(ratios: name -> max error / bar, bad: the failed checks).  Only the quantities present in `got` are compared (an optional
    output that the case leaves NULL is absent from it); every quantity of `got` must have a reference."""
    bad, ratios = [], {}
    if getattr(ref, "finish", None):
        ref.finish(got)
    nf = getattr(ref, "nonfinite", None)
    for k in got:
        if k not in ref.exact and k not in ref.f64 and not (k == "kl_mean" and nf is not None and nf.any()):
            bad.append(f"{k}: no reference")             # (the mean over pixels that are not all numbers is not compared)
    for k, v in ref.exact.items():
        if k not in got:
            continue
        if np.ndim(v) == 0:
            if not F32(got[k]) == F32(v):
                bad.append(f"{k}: {got[k]!r} != {v!r}")
            continue
        n = bits_differ(got[k], v)
        if n:
            bad.append(f"{k}: {n} of {np.size(v)} elements differ in their bits")
    for k, (val, bar) in ref.f64.items():
        if k not in got:
            continue
        g = got[k]
        if k == "kl_map" and nf is not None and nf.any():
            if not np.array_equal(kinds(g), nf):
                bad.append(f"{k}: {int((kinds(g) != nf).sum())} pixels are not of the reference's kind (finite, +inf, -inf, NaN)")
                continue
            g = np.where(nf == 0, g, 0.0)
        ratios[k] = bar_ratio(g, val, bar)
        if not ratios[k] <= 1.0:
            bad.append(f"{k}: error {ratios[k]:.3g} x its bar")
    return ratios, bad


def as_got(ref: Ref, keys=None) -> dict:
    """A reference as a kernel would return it: the float64 values rounded to float32 (the CPU test's stand-in for the device)."""
    if getattr(ref, "finish", None):
        ref.finish(dict(mask=ref.mask_ref.astype(np.uint8)))
    got = {k: (np.asarray(v).copy() if np.ndim(v) else v) for k, v in ref.exact.items()}
    for k, (val, _) in ref.f64.items():
        got[k] = np.asarray(val, F64).astype(F32)
    nf = getattr(ref, "nonfinite", None)
    if nf is not None and nf.any():
        got["kl_map"] = np.where(nf == 1, np.inf, np.where(nf == 2, -np.inf, np.where(nf == 3, np.nan, got["kl_map"]))).astype(F32)
    return got if keys is None else {k: got[k] for k in keys}


# ---- the case table -----------------------------------------------------------------------------------------------------------
class Case:
    """id, entry point family, parameters (attribute access; absent ones read as the defaults below)."""
    DEFAULTS = dict(regime="randn2", T=0, mode="mt", unc=True, thr_q=0.5, thr=None, offs=(), D=2, b0=0, Btot=None, k=0, r_b0=0, u_b0=0,
                    r_tot=None, u_tot=None, probs=False, outs=("mse_map", "kl_map", "kl_mean"), g=0.75, gnull=False, seed=0x9E3779B97F4A7C15,
                    offset=0, step=5, amax=None, rot_out=True, hinted=False, offe=(0,), offp=(0,))

    def __init__(self, id: str, entry: str, **p):
        self.id, self.entry, self.params = id, entry, p

    def __getattr__(self, k):
        p = self.__dict__.get("params", {})
        if k in p:
            return p[k]
        if k in Case.DEFAULTS:
            return Case.DEFAULTS[k]
        raise AttributeError(k)

    def off(self, i: int) -> int:
        """The offset (in elements) of the case's i-th tensor inside its guarded buffer."""
        return self.offs[i] if i < len(self.offs) else 0

    @property
    def kernels(self) -> frozenset:
        return frozenset(_kernels(self))


def _b(x: bool) -> str:
    return "true" if x else "false"


def cct_vec(c: Case) -> bool:
    """The `vec` rule of uaps_cct_consistency_*: H W % 4 == 0 and every head (and gradient) pointer 16-byte aligned; tensors
    0..D-1 are the heads, D..2D-1 the gradients."""
    n = c.D * (2 if c.entry == "cct_bwd" else 1)
    return (c.shape[2] * c.shape[3]) % 4 == 0 and all(c.off(i) % 4 == 0 for i in range(n))


def _kernels(c: Case):
    e = c.entry
    if e == "ema":
        return {"ema_kernel"}
    if e == "noise":
        return {"teacher_noise_kernel<true>"}
    if e == "noise_apply":
        return {"teacher_noise_kernel<false>"}
    C = c.shape[1] if hasattr(c, "shape") else 0
    if e == "mc_fwd":
        return {f"mc_fwd_kernel<{C}>", "mc_finalize"}
    if e == "mc_bwd":
        return {f"mc_bwd_kernel<{C}>"}
    if e == "cct_fwd":
        return {f"cct_fwd_kernel<{C}, {4 if cct_vec(c) else 1}>", "cct_finalize"}
    if e == "cct_bwd":
        return {f"cct_bwd_kernel<{C}, {4 if cct_vec(c) else 1}>"}
    if e == "rot90":
        return {"rot90_batch_kernel"}
    if e == "rot_fwd":
        return {f"rot_cons_kernel<{C}, false>", "cct_finalize"}
    if e == "rot_bwd":
        return {f"rot_cons_kernel<{C}, true>"}
    if e == "pair_fwd":
        return {f"pair_fwd_kernel<{C}, {_b(c.probs)}>"} | ({"pair_finalize"} if "kl_mean" in c.outs else set())
    if e == "mse_bwd":
        return {f"pair_bwd_kernel<{C}, true>"}
    if e == "kl_bwd":
        return {f"pair_bwd_kernel<{C}, false>"}
    if e == "klmap_bwd":
        return {f"pair_klmap_bwd_kernel<{C}>"}
    if e == "entropy":
        return {f"entropy_kernel<{C}>"} | ({"pair_finalize"} if "ent_mean" in c.outs else set())
    raise ValueError(e)


KERNEL_NAMES = ("ema_kernel", "teacher_noise_kernel", "mc_fwd_kernel", "mc_bwd_kernel", "mc_finalize", "cct_fwd_kernel", "cct_bwd_kernel",
                "cct_finalize", "rot90_batch_kernel", "rot_cons_kernel", "pair_fwd_kernel", "pair_bwd_kernel", "pair_klmap_bwd_kernel",
                "entropy_kernel", "pair_finalize")
CLASSES = tuple(range(2, MAX_CLASSES + 1))
RAGGED = ((1, 1, 1), (1, 1, 40), (3, 33, 45), (2, 16, 24))            # (B, H, W): degenerate, one row, odd, H W % 4 == 0
V1_SHAPES = ((1, 1, 1), (1, 1, 41), (3, 33, 45), (2, 15, 25))         # H W % 4 != 0: the one-pixel CCT form whatever the alignment
V4_SHAPES = ((2, 16, 24), (1, 1, 40))                                 # H W % 4 == 0
CAP_PIX = (1, 517, 509)                                                # 263,153 pixels > 1024 x 256
REGIMES = ("randn2", "sat", "equal", "shift")
EMA_SIZES = (1, 3, 1023, 1024, 1025, 2049, 70000)


def _cases():
    cs = []

    def add_(id, entry, **p):
        cs.append(Case(id, entry, **p))

    def shp(C, i):
        B, H, W = RAGGED[i % len(RAGGED)]
        return (B, C, H, W)

    # EMA: tensor counts around the 128-tensor launch table, every size class, step 0, views off 16 bytes on either side
    for n in (1, 128, 129, 257):
        add_(f"ema-n{n}", "ema", numels=tuple(EMA_SIZES[i % 6] for i in range(n)), offe=(0, 1, 0, 1, 0), offp=(0, 0, 1, 1))
    add_("ema-sizes", "ema", numels=EMA_SIZES)
    add_("ema-sizes-offe", "ema", numels=EMA_SIZES, offe=(1,))
    add_("ema-sizes-offp", "ema", numels=EMA_SIZES, offp=(3,))
    add_("ema-sizes-offboth", "ema", numels=EMA_SIZES, offe=(1,), offp=(2,))
    add_("ema-step0", "ema", numels=(1, 1025, 2049), step=0, offe=(0, 1), offp=(0,))
    add_("ema-step1", "ema", numels=(3, 1024, 1025), step=1)
    add_("ema-late", "ema", numels=(1023, 2049), step=10 ** 6)
    # teacher noise: T, the vec rule (chw % 4, alignment of x / out / noise), the 4096-block cap
    for i, T in enumerate((0, 1, 3, 16)):
        add_(f"noise-T{T}", "noise", shape=(2, 3, 5, 7) if i % 2 else (2, 3, 4, 8), T=T, seed=0xFEDCBA9876543210 + i, offset=(2 ** 32 - 3) * (i % 2))
        add_(f"apply-T{T}", "noise_apply", shape=(2, 3, 5, 7) if i % 2 else (2, 3, 4, 8), T=T)
    for j, offs in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        add_(f"apply-off{j}", "noise_apply", shape=(2, 3, 4, 8), T=3, offs=offs)
    add_("noise-offx", "noise", shape=(2, 3, 4, 8), T=3, offs=(1, 0))
    add_("noise-offo", "noise", shape=(1, 1, 1, 1), T=1, offs=(0, 1))
    add_("noise-cap", "noise", shape=(1, 3, 300, 300), T=16)
    add_("apply-cap", "noise_apply", shape=(1, 3, 300, 300), T=16)
    add_("noise-cap-scalar", "noise", shape=(1, 3, 299, 301), T=16, offset=2 ** 32 - 5)
    # Mean Teacher / UAMT: every C x mode, every ragged shape, T in {0, 1, 3, 16}, uncertainty NULL, thresholds at three quantiles
    for i, C in enumerate(CLASSES):
        add_(f"mt-c{C}", "mc_fwd", shape=shp(C, i), mode="mt")
        add_(f"mtb-c{C}", "mc_bwd", shape=shp(C, i), mode="mt")
        T = (0, 1, 3, 16)[i % 4]
        add_(f"uamt-c{C}-T{T}", "mc_fwd", shape=shp(C, i + 2), mode="mask", T=T, thr_q=(0.25, 0.5, 0.9)[i % 3], unc=i % 2 == 0)
        add_(f"uamt-c{C}-T{(0, 1, 3, 16)[(i + 1) % 4]}-off", "mc_fwd", shape=shp(C, i + 3), mode="mask",
             T=(0, 1, 3, 16)[(i + 1) % 4], thr_q=(0.25, 0.5, 0.9)[(i + 1) % 3], unc=i % 2 == 1, offs=(1, 0, 2, 1, 3))
        add_(f"uamtb-c{C}", "mc_bwd", shape=shp(C, i + 1), mode="mask", offs=(0, 1, 3, 0))
    for i, (B, H, W) in enumerate(RAGGED):
        for T in (0, 1, 3, 16):
            add_(f"uamt-{B}x{H}x{W}-T{T}", "mc_fwd", shape=(B, 2 + (3 * i + T) % 7, H, W), mode="mask", T=T, thr_q=(0.25, 0.5, 0.9)[(i + T) % 3])
    for r in REGIMES[1:]:
        add_(f"mt-{r}", "mc_fwd", shape=(2, 3, 16, 24), mode="mt", regime=r)
        add_(f"mtb-{r}", "mc_bwd", shape=(2, 5, 16, 24), mode="mt", regime=r)
        # (all-equal Monte-Carlo logits give u = ln C on every pixel: no threshold splits them, the mask is whole)
        add_(f"uamt-{r}", "mc_fwd", shape=(2, 4, 16, 24), mode="mask", T=3, regime=r, thr=2.0 if r == "equal" else None)
        add_(f"uamtb-{r}", "mc_bwd", shape=(2, 6, 16, 24), mode="mask", regime=r)
    add_("mt-cap", "mc_fwd", shape=(1, 3) + CAP_PIX[1:], mode="mt", offs=(1, 0))
    add_("uamt-cap", "mc_fwd", shape=(1, 2) + CAP_PIX[1:], mode="mask", T=1, offs=(0, 1, 1))
    add_("mtb-cap", "mc_bwd", shape=(1, 2) + CAP_PIX[1:], mode="mt", offs=(0, 0, 0, 1))
    add_("uamtb-cap", "mc_bwd", shape=(1, 5) + CAP_PIX[1:], mode="mask")
    # CCT: every C x V, D in {2, 3, 8}, windows, one misaligned pointer with H W % 4 == 0, both caps
    for i, C in enumerate(CLASSES):
        D = (2, 3, 8)[i % 3]
        v1, v4 = V1_SHAPES[i % 4], V4_SHAPES[i % 2]
        add_(f"cct-c{C}-v4", "cct_fwd", shape=(v4[0], C) + v4[1:], D=D, b0=1 + i % 2, Btot=4)
        add_(f"cct-c{C}-v1", "cct_fwd", shape=(v1[0], C) + v1[1:], D=(3, 8, 2)[i % 3], b0=1, Btot=4)
        add_(f"cct-c{C}-forced", "cct_fwd", shape=(2, C, 16, 24), D=D, offs=tuple(int(j == i % D) for j in range(D)))
        add_(f"cctb-c{C}-v4", "cct_bwd", shape=(v4[0], C) + v4[1:], D=D, b0=1, Btot=3)
        add_(f"cctb-c{C}-v1", "cct_bwd", shape=(v1[0], C) + v1[1:], D=(3, 8, 2)[i % 3], b0=1, Btot=4)
        add_(f"cctb-c{C}-forced", "cct_bwd", shape=(2, C, 16, 24), D=D, offs=tuple(int(j == (i % (2 * D))) for j in range(2 * D)))
    for r in REGIMES[1:]:
        add_(f"cct-{r}", "cct_fwd", shape=(2, 4, 16, 24), D=3, regime=r)
        add_(f"cctb-{r}", "cct_bwd", shape=(2, 3, 33, 45), D=3, regime=r)
    add_("cct-cap-v1", "cct_fwd", shape=(1, 2) + CAP_PIX[1:], D=2)
    add_("cctb-cap-v1", "cct_bwd", shape=(1, 2) + CAP_PIX[1:], D=2)
    add_("cct-cap-v4", "cct_fwd", shape=(1, 2, 1026, 1024), D=2)
    add_("cctb-cap-v4", "cct_bwd", shape=(1, 2, 1026, 1024), D=2)
    # rot90_batch: every k on non-square images (odd k needs rot_out), the shared buffer on squares, the concatenation cap
    for k in range(4):
        add_(f"rot90-k{k}", "rot90", shape=(2, 3, 33, 45), k=k, amax=0.0, hinted=k % 2 == 1)
        add_(f"rot90-k{k}-sq", "rot90", shape=(1, 2, 40, 40), k=k, rot_out=False, amax=2.5 if k < 2 else None)
    add_("rot90-1x1", "rot90", shape=(1, 1, 1, 1), k=3, amax=0.0)
    add_("rot90-off", "rot90", shape=(2, 3, 16, 24), k=1, offs=(1, 0, 0, 0), amax=0.0)
    add_("rot90-cap", "rot90", shape=(1, 1, 724, 728), k=2, amax=0.0)               # n = 527,072 > 524,288, aligned
    add_("rot90-cap-off", "rot90", shape=(1, 1, 724, 728), k=1, offs=(0, 0, 1, 0), amax=0.0)
    add_("rot90-cap-n3", "rot90", shape=(1, 1, 723, 727), k=3, amax=0.0)            # n % 4 == 1: the scalar form, the tail included
    # rotation consistency: every C x direction, every k on non-square images, differing windows, the tile cap
    for i, C in enumerate(CLASSES):
        add_(f"rot-c{C}", "rot_fwd", shape=(2, C, 33, 45), k=i % 4, r_b0=1 + i % 2, r_tot=4, u_b0=2 - 2 * (i % 2), u_tot=4)
        add_(f"rotb-c{C}", "rot_bwd", shape=(2, C, 33, 45), k=(i + 1) % 4, r_b0=1 + (i + 1) % 2, r_tot=4, u_b0=2 * (i % 2), u_tot=4)
    for k in range(4):
        add_(f"rot-k{k}", "rot_fwd", shape=(1, 3, 40, 70), k=k)
        add_(f"rotb-k{k}", "rot_bwd", shape=(1, 2, 70, 40), k=k)
        add_(f"rot-k{k}-1x40", "rot_fwd", shape=(1, 4, 1, 40), k=k)
        add_(f"rotb-k{k}-1x1", "rot_bwd", shape=(1, 5, 1, 1), k=k)
    for r in REGIMES[1:]:
        add_(f"rot-{r}", "rot_fwd", shape=(2, 4, 16, 24), k=1, regime=r)
        add_(f"rotb-{r}", "rot_bwd", shape=(2, 3, 16, 24), k=3, regime=r)
    for k in (1, 2):
        add_(f"rot-cap-k{k}", "rot_fwd", shape=(1, 2, 1, 32805), k=k)                # 1026 tiles along one axis, the last 5 wide
        add_(f"rotb-cap-k{k}", "rot_bwd", shape=(1, 2, 1, 32805), k=k)
    # pair_ops: every C x kernel, every regime, every combination of optional outputs, the cap
    combos = [o for o in ((("mse_map",), ("kl_map",), ("kl_mean",), ("mse_map", "kl_map"), ("mse_map", "kl_mean"), ("kl_map", "kl_mean"),
                           ("mse_map", "kl_map", "kl_mean")))]
    for i, C in enumerate(CLASSES):
        add_(f"pair-c{C}", "pair_fwd", shape=shp(C, i), outs=combos[i % 7], offs=(i % 2, 0, 1))
        add_(f"pairp-c{C}", "pair_fwd", shape=shp(C, i + 1), probs=True, regime="probs", outs=combos[(i + 3) % 7])
        add_(f"mseb-c{C}", "mse_bwd", shape=shp(C, i + 2), offs=(0, 1))
        add_(f"klb-c{C}", "kl_bwd", shape=shp(C, i + 3), gnull=i % 3 == 0)
        add_(f"klmapb-c{C}", "klmap_bwd", shape=shp(C, i), outs=(("da", "db"), ("da",), ("db",))[i % 3])
        add_(f"ent-c{C}", "entropy", shape=shp(C, i + 1), regime="probs", outs=(("ent_map", "ent_mean"), ("ent_map",), ("ent_mean",))[i % 3])
    for r in REGIMES:
        add_(f"pair-{r}", "pair_fwd", shape=(2, 4, 16, 24), regime=r)
        add_(f"mseb-{r}", "mse_bwd", shape=(2, 3, 16, 24), regime=r)
        add_(f"klb-{r}", "kl_bwd", shape=(2, 5, 16, 24), regime=r)
        add_(f"klmapb-{r}", "klmap_bwd", shape=(2, 6, 16, 24), regime=r, outs=("da", "db"))
    for j, o in enumerate(combos):
        add_(f"pair-outs{j}", "pair_fwd", shape=(3, 3, 33, 45), outs=o)
    add_("pairp-01", "pair_fwd", shape=(2, 4, 16, 24), probs=True, regime="probs01")
    add_("pairp-01-map", "pair_fwd", shape=(2, 3, 16, 24), probs=True, regime="probs01", outs=("kl_map",))
    add_("ent-01", "entropy", shape=(2, 4, 16, 24), regime="probs01", outs=("ent_map", "ent_mean"))
    add_("pair-cap", "pair_fwd", shape=(1, 2) + CAP_PIX[1:])
    add_("pairp-cap", "pair_fwd", shape=(1, 3) + CAP_PIX[1:], probs=True, regime="probs", outs=("kl_mean",))
    add_("mseb-cap", "mse_bwd", shape=(1, 2) + CAP_PIX[1:])
    add_("klb-cap", "kl_bwd", shape=(1, 3) + CAP_PIX[1:])
    add_("klmapb-cap", "klmap_bwd", shape=(1, 2) + CAP_PIX[1:], outs=("da", "db"))
    add_("ent-cap", "entropy", shape=(1, 2) + CAP_PIX[1:], regime="probs", outs=("ent_map", "ent_mean"))
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
ENTRIES = sorted({c.entry for c in CASES})


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def logits(rng, shape, regime: str) -> np.ndarray:
    B, C, H, W = shape
    if regime == "randn2":
        z = rng.standard_normal(shape) * 2
    elif regime == "recipe":                                          # the recipe of tests/test_gpu_mean_teacher.py
        z = rng.standard_normal(shape) * 2 + rng.standard_normal((1, C, H, W)) * 3
    elif regime == "sat":
        z = rng.standard_normal(shape) * 40
    elif regime == "equal":
        z = np.repeat(rng.standard_normal((B, 1, H, W)) * 3, C, axis=1)
    elif regime == "shift":
        z = rng.standard_normal(shape) * 2 + 1e4
    else:
        raise ValueError(regime)
    return z.astype(F32)


def probabilities(rng, shape, regime: str) -> np.ndarray:
    """float32 probabilities over axis 1; probs01: a third of the pixels hold an exact 1 and exact 0s, a third one exact 0."""
    z = rng.standard_normal(shape) * 2
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(F32)
    if regime == "probs01":
        B, C, H, W = shape
        kind = rng.integers(0, 3, (B, H, W))
        hot = rng.integers(0, C, (B, H, W))
        onehot = (np.arange(C)[None, :, None, None] == hot[:, None]).astype(F32)
        p = np.where((kind == 0)[:, None], onehot, p)
        p = np.where((kind == 1)[:, None] & (onehot != 0), F32(0), p).astype(F32)
    return p


def inputs(c: Case) -> dict:
    rng = rng_for(c.id)
    e = c.entry
    if e == "ema":
        a, oma = ema_alpha(0.99, c.step)
        return dict(t=[dict(e=rng.standard_normal(n).astype(F32), p=rng.standard_normal(n).astype(F32)) for n in c.numels],
                    alpha=float(F32(a)), oma=float(F32(oma)))
    if e in ("noise", "noise_apply"):
        d = dict(x=rng.standard_normal(c.shape).astype(F32))
        if e == "noise_apply":
            d["noise"] = (rng.standard_normal((1 + c.T) * int(np.prod(c.shape))) * 1.5).astype(F32)
        return d
    sh = c.shape
    B, C, H, W = sh
    if e in ("mc_fwd", "mc_bwd"):
        se = "randn2" if c.mode == "mask" and c.regime == "equal" else c.regime   # (equal student and teacher: every distance 0)
        d = dict(s=logits(rng, sh, se), e=logits(rng, sh, se))
        if c.mode == "mask" and e == "mc_fwd":
            reg = "recipe" if c.regime == "randn2" else c.regime
            d["mc"] = logits(rng, (c.T * B, C, H, W), reg).reshape(c.T, B, C, H, W) if c.T > 0 else probabilities(rng, sh, "probs")
            if c.thr is not None:
                d["thr"] = float(F32(c.thr))
            else:                                                     # a quantile of the float64 uncertainty (no device value involved)
                u = np.sort(mc_uncertainty(d["mc"], c.T).v.reshape(-1))
                k = min(int(c.thr_q * (u.size - 1)), u.size - 2)       # half way between two neighbours: on no pixel's own value
                d["thr"] = float(F32(0.5 * (u[k] + u[k + 1]) if u.size > 1 else 1.25 * u[0]))          # one pixel: inside the mask
        if c.mode == "mask" and e == "mc_bwd":
            d["mask"] = (rng.random((B, H, W)) < 0.6).astype(np.uint8) if B * H * W > 1 else np.ones((B, H, W), np.uint8)
            d["sum_m"] = float(d["mask"].sum())
        return d
    if e in ("cct_fwd", "cct_bwd"):
        Bt = c.Btot or c.b0 + B
        return dict(heads=[logits(rng, (Bt, C, H, W), c.regime) for _ in range(c.D)])
    if e == "rot90":
        return dict(xl=rng.standard_normal(sh).astype(F32), xu=(rng.standard_normal(sh) * 1.7).astype(F32))
    if e in ("rot_fwd", "rot_bwd"):
        Ho, Wo = (W, H) if c.k & 1 else (H, W)
        return dict(r=logits(rng, (c.r_tot or c.r_b0 + B, C, Ho, Wo), c.regime), u=logits(rng, (c.u_tot or c.u_b0 + B, C, H, W), c.regime))
    if e == "entropy":
        return dict(p=probabilities(rng, sh, c.regime))
    if e == "pair_fwd" and c.probs:
        return dict(a=probabilities(rng, sh, c.regime), b=probabilities(rng, sh, c.regime))
    d = dict(a=logits(rng, sh, c.regime), b=logits(rng, sh, c.regime))
    if e == "mse_bwd":
        d["gmap"] = rng.standard_normal(sh).astype(F32)
    if e == "klmap_bwd":
        d["gmap"] = rng.standard_normal((B, H, W)).astype(F32)
    return d


def reference(c: Case, inp: dict, mut: str = "") -> Ref:
    e = c.entry
    if e == "ema":
        ref = Ref(exact={f"e{i}": ema(t["e"], t["p"], inp["alpha"], inp["oma"], mut) for i, t in enumerate(inp["t"])})
    elif e == "noise_apply":
        ref = Ref(exact=dict(out=noise_apply(inp["x"], inp["noise"], c.shape[0], c.T)))
    elif e == "noise":
        val, bar, edge = noise_draw(inp["x"], c.shape[0], c.T, c.seed, c.offset, mut)
        ref = Ref(f64=dict(out=(val, bar)))
        ref.info = dict(edge=edge, draws=val.size)
    elif e == "mc_fwd":
        ref = mc_fwd(inp["s"], inp["e"], inp.get("mc"), c.T, inp.get("thr", 0.0), c.unc, mut)
    elif e == "mc_bwd":
        ref = mc_bwd(inp["s"], inp["e"], inp.get("mask"), c.g, inp.get("sum_m"), mut)
    elif e == "cct_fwd":
        ref = cct_fwd(inp["heads"], c.b0, c.shape[0], cct_vec(c), mut)
    elif e == "cct_bwd":
        ref = cct_bwd(inp["heads"], c.b0, c.shape[0], c.g, mut)
        ref.window = {k: (0 if mut == "window_ignored" else c.b0, c.shape[0]) for k in ref.f64}
    elif e == "rot90":
        ref = rot90_batch(inp["xl"], inp["xu"], c.k, c.amax, mut)
    elif e == "rot_fwd":
        ref = rot_fwd(inp["r"], c.r_b0, inp["u"], c.u_b0, c.shape[0], c.k, mut)
    elif e == "rot_bwd":
        ref = rot_bwd(inp["r"], c.r_b0, inp["u"], c.u_b0, c.shape[0], c.k, c.g, mut)
        z = mut == "window_ignored"
        ref.window = dict(dr=(0 if z else c.r_b0, c.shape[0]), du=(0 if z else c.u_b0, c.shape[0]))
    elif e == "pair_fwd":
        ref = pair_fwd(inp["a"], inp["b"], c.probs, mut)
    elif e == "mse_bwd":
        ref = mse_bwd(inp["a"], inp["b"], inp["gmap"])
    elif e == "kl_bwd":
        ref = kl_bwd(inp["a"], inp["b"], None if c.gnull else c.g, mut)
    elif e == "klmap_bwd":
        ref = klmap_bwd(inp["a"], inp["b"], inp["gmap"], mut)
    elif e == "entropy":
        ref = entropy(inp["p"], mut)
    else:
        raise ValueError(e)
    if not hasattr(ref, "info"):
        ref.info = {}
    check_caps(c, ref)
    return ref


def check_caps(c: Case, ref: Ref):
    """The two caps, asserted on the reference before any device value is looked at."""
    i = ref.info
    assert i.get("ambiguous", 0) <= AMBIG_CAP * i.get("pixels", 0), (c.id, i)
    assert i.get("edge", 0) <= EDGE_CAP * i.get("draws", 0), (c.id, i)


def window_split(ref: Ref, got: dict):
    """For the windowed gradients: `got` holds whole tensors.  Returns (got restricted to the windows' rows, the failed checks):
    every row outside a window must still hold the NaN it was filled with."""
    bad, out = [], dict(got)
    for k, (b0, B) in getattr(ref, "window", {}).items():
        if k not in got:
            continue
        g = got[k]
        outside = np.ones(g.shape[0], bool)
        outside[b0:b0 + B] = False
        if not np.isnan(g[outside]).all():
            bad.append(f"{k}: rows outside the window [{b0}, {b0 + B}) were written")
        out[k] = g[b0:b0 + B]
    return out, bad


def as_full(ref: Ref, c: Case, inp: dict) -> dict:
    """as_got for the windowed gradients: whole tensors, NaN outside the window the (possibly mutated) reference believes in."""
    got = as_got(ref)
    for k, (b0, B) in getattr(ref, "window", {}).items():
        tot = (inp["heads"][0].shape[0] if c.entry == "cct_bwd" else inp["r" if k == "dr" else "u"].shape[0])
        full = np.full((tot,) + got[k].shape[1:], np.nan, F32)
        full[b0:b0 + B] = got[k]
        got[k] = full
    return got

"""The kernels between the convolutions -- the feature perturbations and the confusion counts (uaps_amd/csrc/perturb.hip), the
up-sampling glue (resample.hip), the multi-tensor Adam step (adam.hip) and the residual joins at the end of pair_ops.hip: references in
plain numpy, the comparison code, and one case per entry point and layout (tests/test_ops_ref.py, tests/test_gpu_ops_forms.py).

Two kinds of reference.  Where a kernel pins its arithmetic (add_rn / mul_rn), does one operation per element or only adds, the
reference is a float32 restatement and the kernel must match it to the bit (Ref.exact).  Where the compiler may contract a product into
an fma or the kernel interpolates, the reference is float64 and the bar is derived from the number of roundings (Ref.f64: value, bar;
the ratio |got - ref| / bar must stay <= 1).  Adam alone is held against measured bars (TAU_ADAM, profiles/ops_forms_tau.txt).

Every case names the kernel instantiations it must reach, derived from the launchers' own rules; the CPU test checks that the cases
together name every kernel of the four sources found in the built code object.  The one branch no case reaches is the 64-bit division
of fan_divmod: it needs a tensor of 2^32 float4 (64 GiB).

A mutant is a switch on a reference (`mut`): the CPU test proves with them that the comparisons of the GPU test bite.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from bn_ref import UAPS_WORD, _U32, keep_mask, philox4x32_10, rng_for

F32 = np.float32
EPS24 = 2.0 ** -24
MAX_CLASSES = 8              # UAPS_MAX_CLASSES
THREADS, MAX_BLOCKS = 256, 2048
ADAM_BATCH = 48              # tensors per launch (kAdamBatch)
STEP_WORDS, STEP_ADAM = 16, 12
M64 = (1 << 64) - 1

# Adam: 3x the largest ratio |got - float64| / (2^-24 cond) measured on an MI355X over the adam cases (profiles/ops_forms_tau.txt)
TAU_ADAM = dict(p=13.2, m=2.3, v=3.5)


# ---- Philox draws -------------------------------------------------------------------------------------------------------------
def words(seed: int, ctr, mut: str = "") -> np.ndarray:
    """uint32 [..., 4]: the four words of counter `ctr` (uint64, wrapping) under key `seed`."""
    with np.errstate(over="ignore"):
        ctr = np.asarray(ctr, dtype=np.uint64) + np.uint64(1 if mut == "ctr_shift" else 0)
    hi = np.zeros_like(ctr) if mut == "no_hi" else ctr >> np.uint64(32)
    w = np.stack(philox4x32_10(ctr & _U32, hi, UAPS_WORD, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), axis=-1)
    return np.roll(w, 1, axis=-1) if mut == "word_rot" else w


def u01(w) -> np.ndarray:
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(F32) * F32(EPS24)


def _ctr(offset: int, n: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.uint64(offset & M64) + np.arange(n, dtype=np.uint64)


def element_u01(seed: int, offset: int, n: int, mut: str = "") -> np.ndarray:
    """u01 of elements 0..n-1: element e draws word e & 3 of counter offset + (e >> 2)."""
    return u01(words(seed, _ctr(offset, (n + 3) // 4), mut)).reshape(-1)[:n]


def noise_of(seed: int, offset: int, n: int, rng: float, mut: str = "") -> np.ndarray:
    """FeatureNoise draw: (2 u01 - 1) range in float32 (2 u01 - 1 is exact, so one rounding whatever the compiler fuses)."""
    return (F32(2) * element_u01(seed, offset, n, mut) - F32(1)) * F32(rng)


def noise_apply(x, n) -> np.ndarray:
    """y = rn(rn(x n) + x), the noise [chw] shared by the batch."""
    x = np.asarray(x, F32)
    nb = np.asarray(n, F32).reshape((1,) + x.shape[1:])
    return (x * nb).astype(F32) + x


def drop_scale(p: float) -> np.float32:
    return F32(1) / (F32(1) - F32(p))


def bernoulli(x, p, seed, offset, mut: str = ""):
    x = np.asarray(x, F32)
    u = element_u01(seed, offset, x.size, mut)
    keep = (u > F32(p)) if mut == "gt" else (u >= F32(p))
    return mask_apply(x, keep, drop_scale(p)), keep.astype(np.uint8)


def mask_apply(x, keep, scale) -> np.ndarray:
    x = np.asarray(x, F32)
    return np.where(np.asarray(keep).reshape(x.shape) != 0, x * F32(scale), F32(0)).astype(F32)


# ---- FeatureDropout -----------------------------------------------------------------------------------------------------------
def fkey(a) -> np.ndarray:
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def fkey_inv(k) -> np.ndarray:
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def attention(x, split: bool, mut: str = "") -> np.ndarray:
    """[B, HW] float32: the channel sum in the kernel's order (plain: c = 0..C-1; split: four quarter sums, ((q0+q1)+q2)+q3),
    then one correctly rounded division by C."""
    x = np.asarray(x, F32)
    B, C = x.shape[:2]
    x = x.reshape(B, C, -1)
    if mut == "other_order":
        split = not split
    if split and C % 4 == 0:
        q = []
        for w in range(4):
            s = x[:, w * (C // 4)].copy()
            for c in range(w * (C // 4) + 1, (w + 1) * (C // 4)):
                s = s + x[:, c]
            q.append(s)
        s = ((q[0] + q[1]) + q[2]) + q[3]
    else:
        s = x[:, 0].copy()
        for c in range(1, C):
            s = s + x[:, c]
    return (s / F32(C)).astype(F32)


def att_max(att) -> np.ndarray:
    """[B] float32: the per-image maximum, decoded from the largest order-preserving key (-0.0 < +0.0)."""
    return fkey_inv(fkey(att).max(axis=1))


def fdrop_keep(att, mx, u, mut: str = "") -> np.ndarray:
    """uint8 [B, HW]: att < rn(max u), u float32 per image."""
    thr = (np.asarray(mx, F32) * np.asarray(u, F32)).astype(F32)[:, None]
    return ((att <= thr) if mut == "le" else (att < thr)).astype(np.uint8)


def fdrop_apply(x, keep) -> np.ndarray:
    x = np.asarray(x, F32)
    B, C = x.shape[:2]
    return np.where(keep.reshape(B, 1, -1) != 0, x.reshape(B, C, -1), F32(0)).reshape(x.shape).astype(F32)


def device_u(seed: int, offset: int, fused: bool = True) -> np.float32:
    """The threshold factor the fan-out kernel draws itself: 0.7f + 0.2f u01(word 0 of counter `offset`).  The build may contract it
    into one fma (fused) or round the product first; tests/test_ops_ref.py checks that no case's masks depend on which."""
    u = float(u01(words(seed, np.uint64(offset & M64))[0]))
    prod = float(F32(0.2)) * u
    return F32(float(F32(0.7)) + prod) if fused else F32(F32(0.7) + F32(prod))


# ---- the fan kernels ----------------------------------------------------------------------------------------------------------
def _group_of(b: int, Bg: int, groups: int, B: int, mut: str) -> int:
    return ((b + Bg) % B) // Bg if mut == "wrong_group" else b // Bg


def fan_factors(shape, modes, groups, offs, seed, rng, p, keeps, mut: str = ""):
    """Per fan position k: ("id",) | ("noise", n [B, chw] f32) | ("keep", mask [B, chw] bool, scale f32) | ("pool",)."""
    B, C, H, W = shape
    chw, Bg = C * H * W, B // groups
    out = []
    for k, m in enumerate(modes):
        if m == 1:
            per = [noise_of(seed, offs[k][g], chw, rng, mut) for g in range(groups)]
            out.append(("noise", np.stack([per[_group_of(b, Bg, groups, B, mut)] for b in range(B)])))
        elif m == 2:
            u = element_u01(seed, offs[k][0], B * chw, mut).reshape(B, chw)
            out.append(("keep", (u > F32(p)) if mut == "gt" else (u >= F32(p)), drop_scale(p)))
        elif m == 3:
            kp = np.asarray(keeps[k]).reshape(B, 1, H * W) != 0
            out.append(("keep", np.broadcast_to(kp, (B, C, H * W)).reshape(B, chw), F32(1)))
        elif m == 4:
            out.append(("pool",))
        else:
            out.append(("id",))
    return out


def fanout(x, modes, groups, offs, u, seed, rng, p, att=None, mx=None, mut: str = ""):
    """(copies [n][B,C,H,W] float32, keep masks [n] uint8 [B,HW] or None): all bit-exact.  u [groups] float32 (host or device_u)."""
    x = np.asarray(x, F32)
    B, C, H, W = x.shape
    keeps = [None] * len(modes)
    for k, m in enumerate(modes):
        if m == 3:
            ub = np.array([u[_group_of(b, B // groups, groups, B, mut)] for b in range(B)], F32)
            keeps[k] = fdrop_keep(att, mx, ub, mut)
    outs = []
    xf = x.reshape(B, -1)
    for f in fan_factors(x.shape, modes, groups, offs, seed, rng, p, keeps, mut):
        if f[0] == "noise":
            outs.append(((xf * f[1]).astype(F32) + xf).reshape(x.shape))
        else:
            outs.append(np.where(f[1], xf * f[2] if f[2] != 1 else xf, F32(0)).astype(F32).reshape(x.shape))
    return outs, keeps


def unpool(g, idx) -> np.ndarray:
    """[B,C,H/2,W/2] routed to the arg-max position dy*2+dx of each 2x2 window: [B,C,H,W]."""
    g, idx = np.asarray(g), np.asarray(idx)
    B, C, Ho, Wo = g.shape
    out = np.zeros((B, C, 2 * Ho, 2 * Wo), g.dtype)
    for w in range(4):
        out[:, :, w // 2::2, w % 2::2] = np.where(idx == w, g, 0)
    return out


def fanin(gs, modes, groups, offs, seed, rng, p, keeps, shape, mut: str = ""):
    """(float64 sum of the float64 terms built from the exact float32 draws, bar = (n + 2) 2^-24 sum_k |term_k|)."""
    B = shape[0]
    total, mag = np.zeros((B, int(np.prod(shape[1:])))), np.zeros((B, int(np.prod(shape[1:]))))
    fac = fan_factors(shape, modes, groups, offs, seed, rng, p, keeps, mut)
    for k, f in enumerate(fac):
        if mut == "drop_term" and k == len(fac) - 1:
            continue
        g = np.asarray(gs[k], np.float64)
        if f[0] == "pool":
            t = unpool(g, keeps[k]).reshape(B, -1)
        elif f[0] == "noise":
            g = g.reshape(B, -1)
            t = g * f[1].astype(np.float64) + g
        elif f[0] == "keep":
            t = np.where(f[1], g.reshape(B, -1) * float(f[2]), 0.0)
        else:
            t = g.reshape(B, -1)
        total += t
        mag += np.abs(t)
    return total.reshape(shape), ((len(modes) + 2) * EPS24 * mag).reshape(shape)


# ---- max-pool, sums, joins, confusion -------------------------------------------------------------------------------------------
def maxpool2x2(x, mut: str = ""):
    """(out, idx uint8): first maximum in scan order wins, a NaN replaces whatever is held (torch.nn.MaxPool2d)."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        m = x[..., 0::2, 0::2].copy()
        idx = np.zeros(m.shape, np.uint8)
        for w in (1, 2, 3):
            t = x[..., w // 2::2, w % 2::2]
            take = ((t >= m) if mut == "last_wins" else (t > m)) | np.isnan(t)
            m = np.where(take, t, m)
            idx = np.where(take, np.uint8(w), idx)
    return m.astype(F32), idx


def sum_tensors(ins) -> np.ndarray:
    s = np.asarray(ins[0], F32).copy()
    for t in ins[1:]:
        s = s + np.asarray(t, F32)
    return s


def add_relu(a, b, mut: str = "") -> np.ndarray:
    """relu(a + b) as torch.relu: NaN stays NaN, everything else not above 0 is +0."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(a, F32) + np.asarray(b, F32)
        keep = (s > 0) if mut == "nan_to_zero" else ((s > 0) | np.isnan(s))
    return np.where(keep, s, F32(0)).astype(F32)


def relu_bwd(douts, out) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.asarray(out, F32) > 0, sum_tensors(douts), F32(0)).astype(F32)


def amax_after(start: float, values, absolute: bool) -> float:
    """A bound holding `start` raised by a kernel's output: the maximum over the outputs that are numbers."""
    v = np.asarray(values, np.float64).reshape(-1)
    v = np.abs(v) if absolute else v
    v = v[~np.isnan(v)]
    return float(max(start, v.max() if v.size else 0.0))


def confusion(z, labels, mut: str = "") -> np.ndarray:
    """int64 [C, C]: counts[label, argmax], the lowest index winning a tie, labels outside [0, C) ignored."""
    z = np.asarray(z, F32)
    B, C = z.shape[:2]
    arg = (C - 1 - np.argmax(z[:, ::-1], axis=1)) if mut == "last_wins" else np.argmax(z, axis=1)
    y = np.asarray(labels).reshape(-1)
    ok = (y >= 0) & (y < C)
    out = np.zeros((C, C), np.int64)
    np.add.at(out, (y[ok], arg.reshape(-1)[ok]), 1)
    return out


# ---- bilinear x2, align_corners=True -------------------------------------------------------------------------------------------
def taps(n_in: int, mut: str = ""):
    """(i0, i1, l0, l1) of the 2 n_in outputs, the index and fraction formed in float32 as the kernel and ATen form them."""
    n_out = 2 * n_in
    o = np.arange(n_out, dtype=F32)
    if mut == "half_pixel":                                      # align_corners=False
        sx = np.maximum((o + F32(0.5)) * F32(0.5) - F32(0.5), F32(0))
    else:
        r = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
        sx = (r * o).astype(F32)
    i0 = sx.astype(np.int32)
    i1 = i0 + 1 if mut == "no_clamp" else i0 + (i0 < n_in - 1)
    l1 = (sx - i0.astype(F32)).astype(F32)
    return i0, i1, (F32(1) - l1).astype(F32), l1


def _tap_matrix(n_in: int, mut: str = "") -> np.ndarray:
    """float64 [2 n_in, n_in + 1] (the extra column: what an unclamped i1 reads, dropped by the callers that clamp)."""
    i0, i1, l0, l1 = taps(n_in, mut)
    A = np.zeros((2 * n_in, n_in + 1))
    np.add.at(A, (np.arange(2 * n_in), i0), l0.astype(np.float64))
    np.add.at(A, (np.arange(2 * n_in), i1), l1.astype(np.float64))
    return A


def _touch_matrix(n_in: int, mut: str = "") -> np.ndarray:
    """1 where an output reads an input at all, whatever its weight (0 inf = NaN: a read with weight 0 is not harmless)."""
    i0, i1, _, _ = taps(n_in, mut)
    T = np.zeros((2 * n_in, n_in + 1))
    T[np.arange(2 * n_in), i0] = 1
    T[np.arange(2 * n_in), i1] = 1
    return T


def up2x(low, mut: str = ""):
    """(float64 [.., 2h, 2w], bar = 4 2^-24 sum_corners |w| |v|): three lerp2 deep, each one rounded product and one fma.
    A +inf input makes every output +inf that reads it with a weight above 0, and none NaN: the clamped second tap of the last row and
    column has weight 0 and stays inside the plane.  (The last output of every size lands exactly on the last input, so a missing
    clamp changes no finite result: it reads the next plane's memory with weight 0, which only an inf there turns into a NaN.)"""
    low = np.asarray(low, np.float64)
    h, w = low.shape[-2:]
    Ay, Ax = _tap_matrix(h, mut), _tap_matrix(w, mut)
    planes = low.reshape(-1, h, w)
    pad = np.zeros((len(planes), h + 1, w + 1))
    pad[:, :h, :w] = planes
    if mut == "no_clamp":                                        # what lies behind a plane's rows and its last row: the memory that follows
        nxt = np.concatenate([planes.reshape(-1), np.zeros(h * w + w + 1)])
        base = (np.arange(len(planes)) * h * w)[:, None]
        pad[:, h, :] = nxt[base + h * w + np.arange(w + 1)]
        pad[:, :h, w] = nxt[base + np.arange(h) * w + w]
    inf = np.isinf(pad)
    fin = np.where(inf, 0.0, pad)
    val = np.einsum("yi,pij,xj->pyx", Ay, fin, Ax)
    mag = np.einsum("yi,pij,xj->pyx", np.abs(Ay), np.abs(fin), np.abs(Ax))
    hit = np.einsum("yi,pij,xj->pyx", np.abs(Ay), inf.astype(np.float64), np.abs(Ax)) > 0
    val[hit] = np.inf
    touched = np.einsum("yi,pij,xj->pyx", _touch_matrix(h, mut), inf.astype(np.float64), _touch_matrix(w, mut)) > 0
    val[touched & ~hit] = np.nan
    shape = low.shape[:-2] + (2 * h, 2 * w)
    return val.reshape(shape), (4 * EPS24 * mag).reshape(shape)


def up2x_adjoint(dout, mut: str = ""):
    """(float64 [.., h, w], bar = 16 2^-24 sum |wy| |wx| |dout|): the transpose of up2x, two 7-tap sums."""
    dout = np.asarray(dout, np.float64)
    h, w = dout.shape[-2] // 2, dout.shape[-1] // 2
    Ay, Ax = _tap_matrix(h, mut)[:, :h], _tap_matrix(w, mut)[:, :w]
    val = np.einsum("yi,...yx,xj->...ij", Ay, dout, Ax)
    mag = np.einsum("yi,...yx,xj->...ij", np.abs(Ay), np.abs(dout), np.abs(Ax))
    return val, 16 * EPS24 * mag


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, b1, b2, step: int):
    """(lr / bias-correction1, 1 / sqrt(bias-correction2)) as float32: what the launcher passes, or the step state holds."""
    return F32(lr / (1.0 - b1 ** step)), F32(1.0 / math.sqrt(1.0 - b2 ** step))


def adam(p, g, m, v, *, lr, b1, b2, eps, wd, step: int = 0, scalars=None, mut: str = "", dtype=np.float64):
    """One step from the float32 state.  float64 (the reference: torch.optim.Adam's formula with the hyper-parameters as doubles) or
    float32 (the kernel's operation order, what the unmutated restatement of the CPU test is).  scalars: (step_size, inv_sqrt_bc2)
    float32 values read from a step state instead of derived from `step`."""
    T = dtype
    p, g, m, v = (np.asarray(a, F32).astype(T) for a in (p, g, m, v))
    if scalars is not None:
        step_size, inv = T(scalars[0]), T(scalars[1])
    elif T is np.float64:
        step_size, inv = lr / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step)
    else:
        step_size, inv = adam_scalars(lr, b1, b2, step)
    if mut == "no_bias_correction":
        step_size, inv = T(lr), T(1.0)
    G = g if mut == "decoupled_wd" else g + T(wd) * p
    M = m + (G - m) * T(1.0 - b1)
    V = v * T(b2) + T(1.0 - b2) * G * G
    den = np.sqrt(V * inv * inv + T(eps)) if mut == "eps_inside" else np.sqrt(V) * inv + T(eps)
    upd = step_size * (M / den)
    P = p - upd
    if mut == "decoupled_wd":
        P = P - T(lr) * T(wd) * p
    return dict(p=P.astype(T), m=M.astype(T), v=V.astype(T),
                cond=dict(p=np.abs(p) + np.abs(upd), m=np.abs(m) + np.abs(g), v=np.abs(v) + g * g))


def adam_ratios(got: dict, ref: dict) -> dict:
    """max |got - ref| / (2^-24 cond) per quantity (0 / 0 = 0: an untouched zero state)."""
    r = {}
    for k in ("p", "m", "v"):
        d = np.abs(np.asarray(got[k], np.float64) - ref[k])
        c = EPS24 * np.asarray(ref["cond"][k], np.float64)
        if not np.all(np.isfinite(d)):
            r[k] = math.inf
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(d == 0, 0.0, d / c)
        r[k] = float(q.max()) if q.size else 0.0
    return r


# ---- the comparisons both test files use -----------------------------------------------------------------------------------------
@dataclass
class Ref:
    exact: dict = field(default_factory=dict)          # name -> array: bit for bit
    f64: dict = field(default_factory=dict)            # name -> (float64 value, bar): |got - value| <= bar
    adam: list = field(default_factory=list)           # per tensor: the dict of adam()


def bits_differ(got, ref) -> int:
    """How many elements differ in their bits (float32 / uint8 / int64); a shape or dtype mismatch counts as everything.  Two NaNs
    are equal whatever their sign and payload: inf - inf is 0x7FC00000 on the GPU and 0xFFC00000 on an x86 host."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return max(got.size, ref.size, 1)
    if got.dtype == F32:
        both_nan = np.isnan(got) & np.isnan(ref)
        return int(((got.view(np.uint32) != ref.view(np.uint32)) & ~both_nan).sum())
    return int((got != ref).sum())


def bar_ratio(got, val, bar) -> float:
    """max |got - val| / bar, 0 where both vanish; inf when got holds a value that is not a number."""
    got, val = np.asarray(got, np.float64), np.asarray(val, np.float64)
    if got.shape != val.shape:
        return math.inf
    inf = np.isinf(val)                                          # an infinite reference value must be met exactly
    if not np.array_equal(got[inf], val[inf]) or not np.all(np.isfinite(got[~inf])):
        return math.inf
    got, val = np.where(inf, 0.0, got), np.where(inf, 0.0, val)
    d = np.abs(got - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bar)
    return float(q.max()) if q.size else 0.0


def compare(ref: Ref, got: dict):
    """(ratios: name -> max error / bar, bad: the failed checks).  got: name -> host array, for adam a list of p / m / v dicts."""
    bad, ratios = [], {}
    for k, v in ref.exact.items():
        if isinstance(v, float):
            if not got[k] == v:
                bad.append(f"{k}: {got[k]!r} != {v!r}")
            continue
        n = bits_differ(got[k], v)
        if n:
            bad.append(f"{k}: {n} of {np.size(v)} elements differ in their bits")
    for k, (val, bar) in ref.f64.items():
        ratios[k] = bar_ratio(got[k], val, bar)
        if not ratios[k] <= 1.0:
            bad.append(f"{k}: error {ratios[k]:.3g} x its bar")
    if ref.adam:
        worst = dict(p=0.0, m=0.0, v=0.0)
        for i, (r, g) in enumerate(zip(ref.adam, got["adam"])):
            for k, q in adam_ratios(g, r).items():
                worst[k] = max(worst[k], q)
                if not q <= TAU_ADAM[k]:
                    bad.append(f"adam tensor {i} {k}: {q:.3g} roundings > {TAU_ADAM[k]}")
        ratios.update({"adam_" + k: q for k, q in worst.items()})
    return ratios, bad


# ---- the case table -----------------------------------------------------------------------------------------------------------
class Case:
    """id, entry point family, parameters (attribute access; absent ones read as the family's defaults below)."""
    DEFAULTS = dict(seed=0x9E3779B97F4A7C15, offset=0, offx=0, offy=0, offn=0, offk=0, offo=0, offs=0, offd=0, noise_out=True, range=0.3,
                    p=0.3, keep=True, u=0.8, special="", groups=1, state=False, amax=None, dskip=True, alias=False, offs_in=(),
                    wd=0.0, step=1, k=1)

    def __init__(self, id: str, entry: str, **p):
        self.id, self.entry, self.params = id, entry, p

    def __getattr__(self, k):
        p = self.__dict__.get("params", {})
        if k in p:
            return p[k]
        if k in Case.DEFAULTS:
            return Case.DEFAULTS[k]
        raise AttributeError(k)

    @property
    def kernels(self) -> frozenset:
        return frozenset(_kernels(self))


def _al(*offs) -> bool:
    return all(o % 4 == 0 for o in offs)


def stats_kernel(C, HW, offx) -> str:
    vec = HW % 4 == 0 and _al(offx)
    if vec and C >= 64 and C % 4 == 0 and HW <= 4096:
        return "fdrop_attention_split"
    return "fdrop_attention<4>" if vec else "fdrop_attention<1>"


def _kernels(c: Case):
    """The launchers' rules restated (perturb.hip, resample.hip, adam.hip, pair_ops.hip)."""
    e = c.entry
    if e in ("noise", "noise_apply"):
        B, C, H, W = c.shape
        vec = (C * H * W) % 4 == 0 and _al(c.offx, c.offy) and (_al(c.offn) if (e == "noise_apply" or c.noise_out) else True)
        return {("noise_rng_" if e == "noise" else "noise_apply_") + ("vec4" if vec else "scalar")}
    if e == "bernoulli":
        vec = _al(c.offx, c.offy) and (not c.keep or c.offk % 4 == 0) and c.n >= 4
        return ({"bernoulli_vec4"} if vec else set()) | ({"bernoulli_scalar"} if not vec or c.n % 4 else set())
    if e == "mask_apply":
        return {"mask_apply_kernel"}
    if e == "fdrop":
        B, C, H, W = c.shape
        v = "4" if (H * W) % 4 == 0 and _al(c.offx, c.offy) and c.offk % 4 == 0 else "1"
        return {"zero_words_kernel", f"fdrop_attention<{v}>", f"fdrop_apply<{v}>", f"fdrop_bwd<{v}>"}
    if e == "fdrop_stats":
        B, C, H, W = c.shape
        return {"zero_words_kernel", stats_kernel(C, H * W, c.offx)}
    if e == "fanout":
        B, C, H, W = c.shape
        return {"fanout_perturbed_kernel"} | ({"zero_words_kernel", stats_kernel(C, H * W, 0)} if 3 in c.modes else set())
    if e == "fanin":
        return {"fanin_perturbed_kernel"} | ({"maxpool2x2_fwd_kernel"} if 4 in c.modes and c.shape[3] % 8 == 0 else set())
    if e == "maxpool":
        return {"maxpool2x2_fwd_kernel"}
    if e == "sum":
        return {"sum_n_kernel"}
    if e == "confusion":
        return {"zero_words_kernel", "confusion_kernel"}
    if e == "up_fwd":
        H, W = 2 * c.h, 2 * c.w
        if c.Cs == 0 and W % 4 == 0 and _al(c.offo):
            return {"up2x_tiled_kernel<64, 4>" if W >= 64 and H >= 64 else "up2x_tiled_kernel<64, 1>" if W >= 64 else "up2x_tiled_kernel<32, 1>"}
        return {"up_cat_fwd_kernel<true>" if W % 4 == 0 and _al(c.offs, c.offo) else "up_cat_fwd_kernel<false>"}
    if e == "up_bwd":
        ks = {"up_cat_bwd_low_kernel<32>" if c.h >= 32 else "up_cat_bwd_low_kernel<8>"}
        if c.dskip and c.Cs > 0:
            ks.add("slice_channels_kernel<true>" if (4 * c.h * c.w) % 4 == 0 and _al(c.offd, c.offs) else "slice_channels_kernel<false>")
        return ks
    if e in ("add_relu", "relu_bwd", "relu_bwd_sum"):
        return {e + "_kernel"}
    if e == "cat2":
        return {"cat2_amax_kernel"}
    if e == "adam":
        return {"adam_kernel"}
    raise ValueError(e)


def _cases():
    cs = []

    def add(id, entry, **p):
        cs.append(Case(id, entry, **p))

    # FeatureNoise: vec, scalar by size (chw % 4 == 3: the last counter partly used), scalar by each pointer, no noise_out, a
    # counter carrying into the high word, a seed with its high half set, the grid-stride loop run twice
    add("noise-vec", "noise", shape=(3, 2, 2, 4))
    add("noise-size", "noise", shape=(2, 3, 3, 3))
    add("noise-offx", "noise", shape=(3, 2, 2, 4), offx=1)
    add("noise-offy", "noise", shape=(3, 2, 2, 4), offy=1)
    add("noise-offn", "noise", shape=(3, 2, 2, 4), offn=1)
    add("noise-offn-unused", "noise", shape=(3, 2, 2, 4), noise_out=False)
    add("noise-size-nonoise", "noise", shape=(2, 3, 3, 3), noise_out=False)
    add("noise-carry", "noise", shape=(2, 5, 4, 4), offset=2 ** 32 - 3)
    add("noise-carry-scalar", "noise", shape=(2, 5, 3, 3), offset=2 ** 32 - 3, offx=1)
    add("noise-seed-hi", "noise", shape=(3, 2, 2, 4), seed=0xFEDCBA9800000001, offset=7)
    add("noise-two-trips", "noise", shape=(1, 33, 256, 256), offset=2 ** 32 - 300000)
    add("napply-vec", "noise_apply", shape=(3, 2, 2, 4))
    add("napply-size", "noise_apply", shape=(2, 3, 3, 3))
    add("napply-offx", "noise_apply", shape=(3, 2, 2, 4), offx=1)
    add("napply-offy", "noise_apply", shape=(3, 2, 2, 4), offy=1)
    add("napply-offn", "noise_apply", shape=(3, 2, 2, 4), offn=1)
    # Dropout: n < 4 scalar only, else vec + a tail of 0..3
    for n in (1, 3, 4, 7, 4101):
        add(f"bern-n{n}", "bernoulli", n=n, offset=2 ** 32 - 1)
    # a draw exactly at p (element 5 of 8): u01 >= p keeps it, u01 > p would drop it
    add("bern-tie", "bernoulli", n=8, offset=11, p=float(element_u01(Case.DEFAULTS["seed"], 11, 8)[5]))
    add("bern-offx", "bernoulli", n=4101, offx=1)
    add("bern-offy", "bernoulli", n=8, offy=1)
    add("bern-keep-byte", "bernoulli", n=4101, offk=1)
    add("bern-nokeep", "bernoulli", n=7, keep=False)
    add("bern-p0", "bernoulli", n=4101, p=0.0)
    add("bern-p999", "bernoulli", n=4101, p=0.999, seed=0xFEDCBA9800000001)
    add("mask-odd", "mask_apply", n=4099)
    # FeatureDropout forward + backward
    for C in (1, 3, 16, 20, 35):
        add(f"fdrop-c{C}", "fdrop", shape=(2, C, 4, 8))
    add("fdrop-3x3", "fdrop", shape=(2, 5, 3, 3))
    add("fdrop-offx", "fdrop", shape=(2, 3, 4, 8), offx=1)
    add("fdrop-offy", "fdrop", shape=(2, 3, 4, 8), offy=1)
    add("fdrop-offk", "fdrop", shape=(2, 3, 4, 8), offk=1)
    add("fdrop-tie", "fdrop", shape=(2, 4, 4, 8), special="tie", u=0.75)
    add("fdrop-negative", "fdrop", shape=(2, 3, 4, 8), special="neg", u=0.75)
    add("fdrop-zero", "fdrop", shape=(2, 3, 4, 8), special="zero")
    add("fdrop-grid-cap", "fdrop", shape=(2048, 1, 64, 64))
    # FeatureDropout statistics: the split form, and the plain form just outside each of its conditions
    add("stats-split-2x2", "fdrop_stats", shape=(2, 64, 2, 2))
    add("stats-split-68", "fdrop_stats", shape=(1, 68, 4, 72))
    add("stats-split-hw4096", "fdrop_stats", shape=(1, 64, 64, 64))
    add("stats-split-256", "fdrop_stats", shape=(3, 256, 16, 16))
    add("stats-plain-c66", "fdrop_stats", shape=(2, 66, 4, 8))
    add("stats-plain-c60", "fdrop_stats", shape=(2, 60, 4, 8))
    add("stats-plain-hw4100", "fdrop_stats", shape=(1, 64, 41, 100))
    add("stats-scalar-offx", "fdrop_stats", shape=(2, 64, 4, 8), offx=1)
    add("stats-scalar-hw9", "fdrop_stats", shape=(2, 64, 3, 3))
    # fan-out: modes 1..3 in every position, n = 1 and 8, groups 1..4, the three reachable fan_divmod combinations (both powers of
    # two / hw4 only / neither; the 64-bit division needs 2^32 float4 and stays uncovered), host and device u, a step state
    add("fanout-pow2", "fanout", shape=(4, 16, 8, 8), modes=(1, 2, 3), groups=2, u=(0.8, 0.72))
    add("fanout-hw-pow2", "fanout", shape=(2, 3, 8, 8), modes=(3, 1, 2), groups=1, u=(0.85,))
    add("fanout-neither", "fanout", shape=(2, 5, 6, 6), modes=(2, 3, 1), groups=2, u=(0.7, 0.9))
    add("fanout-n1", "fanout", shape=(2, 3, 4, 4), modes=(1,), groups=1, u=(0.8,))
    add("fanout-n8", "fanout", shape=(6, 4, 4, 6), modes=(1, 2, 3, 3, 2, 1, 1, 3), groups=3, u=(0.8, 0.75, 0.88))
    add("fanout-g4", "fanout", shape=(4, 64, 4, 8), modes=(1, 3), groups=4, u=(0.8, 0.71, 0.9, 0.77), offset=2 ** 32 - 5)
    add("fanout-device-u", "fanout", shape=(4, 8, 8, 8), modes=(3, 2, 3), groups=2, u=(-1.0, 0.8))
    add("fanout-state", "fanout", shape=(4, 5, 6, 6), modes=(1, 2, 3), groups=2, u=(-1.0, -1.0), state=True, seed=0xFFFFFFFFFFFFFFF0)
    # fan-in: the same shapes with modes 0..4 mixed; mode 4 at W = 8 (shift) and W = 12 (32-bit division of the row index)
    add("fanin-pow2", "fanin", shape=(4, 16, 8, 8), modes=(0, 1, 2, 3, 4), groups=2)
    add("fanin-hw-pow2", "fanin", shape=(2, 3, 8, 8), modes=(4, 3, 0, 1), groups=1)
    add("fanin-neither", "fanin", shape=(2, 5, 6, 12), modes=(1, 4, 2, 0), groups=2)
    add("fanin-neither-6x6", "fanin", shape=(2, 5, 6, 6), modes=(2, 0, 3, 1), groups=2)
    add("fanin-n1", "fanin", shape=(2, 3, 4, 4), modes=(2,), groups=1)
    add("fanin-n8", "fanin", shape=(6, 4, 4, 8), modes=(1, 0, 2, 3, 4, 1, 2, 3), groups=3, offset=2 ** 32 - 5)
    add("fanin-g4", "fanin", shape=(4, 4, 2, 4), modes=(1, 4, 1), groups=4)
    add("fanin-state", "fanin", shape=(4, 5, 6, 6), modes=(1, 2, 0), groups=2, state=True, seed=0xFFFFFFFFFFFFFFF0)
    # max-pool
    add("pool-1x1x2x8", "maxpool", shape=(1, 1, 2, 8))
    add("pool-3x5x6x24", "maxpool", shape=(3, 5, 6, 24))
    add("pool-special", "maxpool", shape=(1, 1, 2 * 26, 8), special="special")
    # sums
    for n in (1, 2, 3, 4):
        for count in (1, 3, 4, 5, 1027):
            add(f"sum-n{n}-c{count}", "sum", n=n, count=count)
    for i in range(4):
        add(f"sum-off-in{i}", "sum", n=4, count=1027, offs_in=tuple(int(j == i) for j in range(4)))
    add("sum-off-out", "sum", n=3, count=1027, offo=1)
    add("sum-alias", "sum", n=3, count=1027, alias=True)
    add("sum-alias-scalar", "sum", n=2, count=5, alias=True, offs_in=(1, 0))
    # confusion counts
    add("conf-c1", "confusion", shape=(2, 1, 5, 7))
    add("conf-c4", "confusion", shape=(3, 4, 9, 11))
    add("conf-c8", "confusion", shape=(2, MAX_CLASSES, 16, 16))
    add("conf-loop", "confusion", shape=(3, 4, 211, 211))
    # up-sampling forward
    for h, w in ((1, 2), (5, 16), (33, 18), (3, 32), (9, 34), (32, 32), (35, 34)):
        add(f"up-tiled-{h}x{w}", "up_fwd", B=2, Cs=0, Cl=3, h=h, w=w, amax=(0.25 if (h + w) % 2 else 1e3))
    add("up-cat-2x2", "up_fwd", B=2, Cs=3, Cl=2, h=2, w=2)
    add("up-cat-5x6", "up_fwd", B=2, Cs=3, Cl=2, h=5, w=6)
    add("up-scalar-w3", "up_fwd", B=2, Cs=2, Cl=2, h=4, w=3)
    add("up-scalar-w1", "up_fwd", B=2, Cs=1, Cl=2, h=3, w=1)
    add("up-scalar-1x1", "up_fwd", B=2, Cs=1, Cl=2, h=1, w=1)
    add("up-scalar-offo", "up_fwd", B=2, Cs=3, Cl=2, h=5, w=6, offo=1)
    add("up-scalar-offs", "up_fwd", B=2, Cs=3, Cl=2, h=5, w=6, offs=1)
    add("up-scalar-cs0-offo", "up_fwd", B=2, Cs=0, Cl=3, h=5, w=16, offo=1)
    # +inf in the first element of every plane but the first: a second tap that is not clamped at the last row or column reads it
    # with weight 0 and turns the output into a NaN
    add("up-clamp-cat", "up_fwd", B=2, Cs=1, Cl=3, h=3, w=6, special="inf")
    add("up-clamp-scalar", "up_fwd", B=2, Cs=1, Cl=3, h=4, w=5, special="inf")
    add("up-clamp-tiled", "up_fwd", B=2, Cs=0, Cl=3, h=5, w=16, special="inf")
    add("up-clamp-tiled-64", "up_fwd", B=1, Cs=0, Cl=2, h=32, w=32, special="inf")
    # up-sampling backward
    for h, w in ((1, 1), (5, 6), (9, 33), (2, 3), (32, 32), (33, 34), (40, 36)):
        add(f"upb-{h}x{w}", "up_bwd", B=2, Cs=2, Cl=3, h=h, w=w)
    add("upb-cs0", "up_bwd", B=2, Cs=0, Cl=3, h=5, w=6, dskip=False)
    add("upb-nodskip", "up_bwd", B=2, Cs=2, Cl=3, h=5, w=6, dskip=False)
    add("upb-offs", "up_bwd", B=2, Cs=2, Cl=3, h=5, w=6, offs=1)
    add("upb-offd", "up_bwd", B=2, Cs=2, Cl=3, h=5, w=6, offd=1)              # W % 4 == 0 and a misaligned dout
    add("upb-offd-32", "up_bwd", B=1, Cs=1, Cl=2, h=32, w=34, offd=3)
    # joins
    for e in ("add_relu", "relu_bwd", "cat2"):
        for n in (1, 3, 4, 5, 1031):
            add(f"{e}-n{n}", e, n=n, amax=(None if e == "relu_bwd" else (0.125 if n % 2 else 64.0)))
        for i in range(3):
            add(f"{e}-off{i}", e, n=1032, offs_in=tuple(int(j == i) for j in range(3)))
        add(f"{e}-special", e, n=1031, special="special", amax=(None if e == "relu_bwd" else 0.5))
    for k in (1, 2, 3, 4):
        for n in (1, 3, 4, 5, 1031):
            add(f"relu_bwd_sum-k{k}-n{n}", "relu_bwd_sum", k=k, n=n)
    for i in range(6):
        add(f"relu_bwd_sum-off{i}", "relu_bwd_sum", k=4, n=1032, offs_in=tuple(int(j == i) for j in range(6)))
    add("relu_bwd_sum-special", "relu_bwd_sum", k=3, n=1031, special="special")
    # Adam: 1 / 48 / 49 / 97 tensors (one, one, two, three launches), every tail length, the grid cap, a misaligned tensor
    sizes = (1, 3, 4, 5, 1023)
    add("adam-1", "adam", numels=(1023,), wd=0.0, step=1)
    add("adam-48", "adam", numels=tuple(sizes[i % 5] for i in range(48)), wd=0.01, step=1000)
    add("adam-49", "adam", numels=tuple(sizes[(i * 3) % 5] for i in range(49)), wd=0.0, step=1000, offs_in=(7,))
    add("adam-97", "adam", numels=tuple(sizes[(i * 2) % 5] for i in range(97)), wd=0.01, step=1, offs_in=(50, 96))
    add("adam-grid-cap", "adam", numels=(262144 * 4 + 7, 1, 40000), wd=0.01, step=3)
    add("adam-grid-cap-misaligned", "adam", numels=(5, 262144 * 4 + 7), wd=0.0, step=2, offs_in=(1,))
    add("adam-zero-state", "adam", numels=(1023, 5), wd=0.0, step=5, special="zero")
    add("adam-tiny", "adam", numels=(1023, 5), wd=0.0, step=10, special="tiny")          # sqrt(v) ~ eps: where eps sits matters
    add("adam-state", "adam", numels=(1023, 4, 3), wd=0.01, step=0, state=True)
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
ENTRIES = sorted({c.entry for c in CASES})
# every kernel of perturb.hip, resample.hip, adam.hip and the joins of pair_ops.hip (the filter of tests/test_ops_ref.py)
KERNEL_NAMES = ("zero_words_kernel", "noise_rng_vec4", "noise_rng_scalar", "noise_apply_vec4", "noise_apply_scalar", "bernoulli_vec4",
                "bernoulli_scalar", "mask_apply_kernel", "fdrop_attention", "fdrop_attention_split", "fdrop_apply", "fdrop_bwd",
                "sum_n_kernel", "maxpool2x2_fwd_kernel", "fanin_perturbed_kernel", "fanout_perturbed_kernel", "confusion_kernel",
                "up_cat_fwd_kernel", "up2x_tiled_kernel", "up_cat_bwd_low_kernel", "slice_channels_kernel", "adam_kernel",
                "add_relu_kernel", "relu_bwd_kernel", "relu_bwd_sum_kernel", "cat2_amax_kernel")
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
STATE_KEY = 0x0123456789ABCDEF        # words 0-1 of the step state of the `state` cases


def seed_eff(c: Case) -> int:
    return (c.seed + STATE_KEY) & M64 if c.state else c.seed


def fan_offsets(c: Case):
    """offsets [n][groups]: distinct, the first one from c.offset (so a carry case carries in position 0)."""
    n = len(c.modes)
    return [[(c.offset + 1000003 * (k * c.groups + g)) & M64 for g in range(c.groups)] for k in range(n)]


SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 3.5], F32)


# ---- inputs and references per case ---------------------------------------------------------------------------------------------
def inputs(c: Case) -> dict:
    """The case's host data, seeded from a CRC of its id."""
    rng = rng_for(c.id)
    nrm = lambda *s: rng.standard_normal(s, dtype=F32)
    e = c.entry
    if e in ("noise", "noise_apply"):
        d = dict(x=nrm(*c.shape))
        if e == "noise_apply":
            d["noise"] = (rng.uniform(-0.3, 0.3, int(np.prod(c.shape[1:])))).astype(F32)
        return d
    if e == "bernoulli":
        return dict(x=nrm(c.n))
    if e == "mask_apply":
        return dict(x=nrm(c.n), keep=rng.choice(np.array([0, 1, 2, 255, 0, 1], np.uint8), c.n), scale=F32(1.0 / 0.7))
    if e in ("fdrop", "fdrop_stats"):
        B, C, H, W = c.shape
        x = nrm(*c.shape) + F32(0.5)
        if c.special == "tie":                 # every channel equal and C a power of two: the attention is the channel value exactly
            a = rng.uniform(0.0, 3.9, (B, 1, H, W)).astype(F32)
            a[:, 0, 0, 0], a[:, 0, 1, 1], a[:, 0, 2, 2] = 4.0, 3.0, np.nextafter(F32(3), F32(0))
            x = np.broadcast_to(a, c.shape).copy()
        elif c.special == "neg":
            x = -np.abs(x) - F32(0.25)
        elif c.special == "zero":
            x = np.zeros(c.shape, F32)
        return dict(x=x, dy=nrm(*c.shape))
    if e == "fanout":
        B, C, H, W = c.shape
        return dict(x=nrm(*c.shape) + F32(0.5))
    if e == "fanin":
        B, C, H, W = c.shape
        d = dict(g=[], keep=[], poolx=[])
        for m in c.modes:
            d["g"].append(nrm(B, C, H // 2, W // 2) if m == 4 else nrm(*c.shape))
            d["keep"].append((rng.random((B, H * W)) < 0.6).astype(np.uint8) if m == 3 else None)
            d["poolx"].append(nrm(*c.shape) if m == 4 else None)
        return d
    if e == "maxpool":
        x = nrm(*c.shape)
        if c.special:
            x = pool_special()
        return dict(x=x)
    if e == "sum":
        return dict(ins=[nrm(c.count) for _ in range(c.n)])
    if e == "confusion":
        B, C, H, W = c.shape
        z = np.round(nrm(*c.shape) * 2) / 2                      # a coarse grid: many exact ties between classes
        y = rng.integers(-1, C + 1, (B, H, W)).astype(np.int64)   # -1 and C are ignored
        return dict(z=z.astype(F32), y=y)
    if e == "up_fwd":
        H, W = 2 * c.h, 2 * c.w
        low = nrm(c.B, c.Cl, c.h, c.w)
        if c.special == "inf":
            low.reshape(-1, c.h * c.w)[1:, 0] = np.inf
        return dict(skip=nrm(c.B, max(c.Cs, 1), H, W)[:, :c.Cs], low=low)
    if e == "up_bwd":
        return dict(dout=nrm(c.B, c.Cs + c.Cl, 2 * c.h, 2 * c.w))
    if e in ("add_relu", "relu_bwd", "cat2", "relu_bwd_sum"):
        k = c.k if e == "relu_bwd_sum" else 1
        d = dict(a=nrm(c.n), b=nrm(c.n), gs=[nrm(c.n) for _ in range(k)])
        if c.special:
            for i, t in enumerate([d["a"], d["b"]] + d["gs"]):
                t[:64] = np.roll(np.repeat(SPECIAL, 8), i * 3)             # every pair of special values meets somewhere
            d["b"][64:72] = -d["a"][64:72]                                 # sums of exactly +0
        return d
    if e == "adam":
        ts = []
        for i, n in enumerate(c.numels):
            # |g| >= half its scale and weight_decay |p| <= 0.05 <= |g|: the conditioning |m| + |g|, |v| + g^2 of the bars (which
            # names the gradient, not the decayed gradient g + weight_decay p) then is within a factor two of the decayed one's
            gn = nrm(n)
            p, g = nrm(n) * F32(10.0 ** rng.uniform(-2, 0)), np.copysign(F32(0.5) + np.abs(gn), gn) * F32(10.0 ** rng.uniform(-1, 1))
            # m carries g's sign: 0.9 m + 0.1 g does not cancel, so the update's error stays a few roundings of |update| (with mixed
            # signs it is 2^-24 (|m| + |g|) / |M| of it, which the conditioning |p| + |update| of the bar does not model)
            m, v = np.copysign(nrm(n), gn) * F32(10.0 ** rng.uniform(-3, 0)), (nrm(n) * F32(10.0 ** rng.uniform(-3, 0))) ** 2
            if c.special == "tiny":
                g, m, v = g * F32(1e-8), m * F32(1e-8), v * F32(1e-16)
            if c.special == "zero" and i == 0:
                g, m, v = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
            ts.append(dict(p=p, g=g, m=m, v=v))
        return dict(t=ts)
    raise ValueError(e)


def pool_special() -> np.ndarray:
    """[1, 1, 52, 8]: one 2x2 window per case -- every pair of positions equal and largest (6), all four equal, -0.0 against +0.0
    in both orders (2 x 6 placements collapse to 12 windows), all -inf, NaN at each position (4), two NaNs in every pair (6)."""
    wins = []
    for i in range(4):
        for j in range(i + 1, 4):
            w = np.array([-1.0, -2.0, -3.0, -4.0], F32)
            w[[i, j]] = 5.0
            wins.append(w)
    wins.append(np.full(4, 2.0, F32))
    for i in range(4):
        for j in range(4):
            if i != j:
                w = np.full(4, -1.0, F32)
                w[i], w[j] = -0.0, 0.0
                wins.append(w)
    wins.append(np.full(4, -np.inf, F32))
    for i in range(4):
        w = np.array([1.0, 9.0, -3.0, np.inf], F32)
        w[i] = np.nan
        wins.append(w)
    for i in range(4):
        for j in range(i + 1, 4):
            w = np.array([1.0, 9.0, -3.0, np.inf], F32)
            w[[i, j]] = np.nan
            wins.append(w)
    wins = wins + [wins[0]] * (104 - len(wins))
    x = np.zeros((1, 1, 52, 8), F32)
    for n, w in enumerate(wins[:104]):
        r, q = divmod(n, 4)
        x[0, 0, 2 * r:2 * r + 2, 2 * q:2 * q + 2] = w.reshape(2, 2)
    return x


def reference(c: Case, inp: dict, mut: str = "", aux: dict = None) -> Ref:
    """The expected outputs of the case.  aux: what the GPU test hands over from an earlier launch (the arg-max bytes of the max-pool
    kernel for the fan-in's mode 4); absent, the host reference of the same is used."""
    e, r = c.entry, Ref()
    if e == "noise":
        chw = int(np.prod(c.shape[1:]))
        n = noise_of(c.seed, c.offset, chw, c.range, mut)
        r.exact["y"] = noise_apply(inp["x"], n)
        if c.noise_out:
            r.exact["noise"] = n
    elif e == "noise_apply":
        r.exact["y"] = noise_apply(inp["x"], inp["noise"])
    elif e == "bernoulli":
        y, k = bernoulli(inp["x"], c.p, c.seed, c.offset, mut)
        r.exact["y"] = y
        if c.keep:
            r.exact["keep"] = k
    elif e == "mask_apply":
        r.exact["y"] = mask_apply(inp["x"], inp["keep"], inp["scale"])
    elif e in ("fdrop", "fdrop_stats"):
        B, C, H, W = c.shape
        split = e == "fdrop_stats" and stats_kernel(C, H * W, c.offx) == "fdrop_attention_split"
        att = attention(inp["x"], split, mut)
        r.exact["att"], r.exact["max"] = att, att_max(att)
        if e == "fdrop":
            keep = fdrop_keep(att, r.exact["max"], np.full(B, c.u, F32), mut)
            r.exact.update(keep=keep, y=fdrop_apply(inp["x"], keep), dx=fdrop_apply(inp["dy"], keep))
        else:
            x64 = inp["x"].astype(np.float64).reshape(B, C, -1)
            r.f64["att64"] = (x64.mean(1), C * EPS24 * np.abs(x64).mean(1))
    elif e == "fanout":
        B, C, H, W = c.shape
        seed, offs = seed_eff(c), fan_offsets(c)
        att = mx = None
        if 3 in c.modes:
            att = attention(inp["x"], stats_kernel(C, H * W, 0) == "fdrop_attention_split", "other_order" if mut == "other_order" else "")
            mx = att_max(att)
        outs, keeps = [], []
        for k, m in enumerate(c.modes):            # position by position: a device-drawn u belongs to (position, group)
            u = [F32(v) if v >= 0 else device_u(seed, offs[k][g], fused=mut != "unfused") for g, v in enumerate(c.u)]
            o, kp = fanout(inp["x"], (m,), c.groups, [offs[k]], u, seed, c.range, c.p, att, mx, mut)
            outs.append(o[0])
            keeps.append(kp[0])
        for k in range(len(c.modes)):
            r.exact[f"out{k}"] = outs[k]
            if keeps[k] is not None:
                r.exact[f"keep{k}"] = keeps[k]
    elif e == "fanin":
        keeps = list(inp["keep"])
        for k, m in enumerate(c.modes):
            if m == 4:
                keeps[k] = aux["idx"][k] if aux and aux.get("idx", {}).get(k) is not None else maxpool2x2(inp["poolx"][k])[1]
        r.f64["out"] = fanin(inp["g"], c.modes, c.groups, fan_offsets(c), seed_eff(c), c.range, c.p, keeps, c.shape, mut)
    elif e == "maxpool":
        r.exact["out"], r.exact["idx"] = maxpool2x2(inp["x"], mut)
    elif e == "sum":
        r.exact["out"] = sum_tensors(inp["ins"])
    elif e == "confusion":
        r.exact["counts"] = confusion(inp["z"], inp["y"], mut)
    elif e == "up_fwd":
        val, bar = up2x(inp["low"], mut)
        r.exact["skip_part"] = np.ascontiguousarray(inp["skip"])
        r.f64["up_part"] = (val, bar)
    elif e == "up_bwd":
        r.f64["dlow"] = up2x_adjoint(inp["dout"][:, c.Cs:], mut)
        if c.dskip and c.Cs > 0:
            r.exact["dskip"] = np.ascontiguousarray(inp["dout"][:, :c.Cs])
    elif e == "add_relu":
        r.exact["out"] = add_relu(inp["a"], inp["b"], mut)
        if c.amax is not None:
            r.exact["amax"] = amax_after(c.amax, r.exact["out"], absolute=False)
    elif e == "relu_bwd":
        r.exact["dx"] = relu_bwd([inp["a"]], inp["b"])
    elif e == "relu_bwd_sum":
        r.exact["dx"] = relu_bwd(inp["gs"], inp["b"])
    elif e == "cat2":
        r.exact["out"] = np.concatenate([inp["a"], inp["b"]])
        if c.amax is not None:
            r.exact["amax"] = amax_after(c.amax, r.exact["out"], absolute=True)
    elif e == "adam":
        sc = adam_scalars(ADAM_HYPER["lr"], ADAM_HYPER["b1"], ADAM_HYPER["b2"], 7) if c.state else None
        r.adam = [adam(t["p"], t["g"], t["m"], t["v"], wd=c.wd, step=c.step, scalars=sc, mut=mut, **ADAM_HYPER) for t in inp["t"]]
        if c.special == "zero":
            r.exact["p0"] = inp["t"][0]["p"]
    else:
        raise ValueError(e)
    return r


def as_got(ref: Ref) -> dict:
    """A reference turned into what a correct (or, from a mutated reference, a wrong) kernel would hand back: float32 outputs."""
    got = dict(ref.exact)
    got.update({k: np.asarray(v[0]).astype(F32) for k, v in ref.f64.items()})
    if ref.adam:
        got["adam"] = [{k: t[k].astype(F32) for k in ("p", "m", "v")} for t in ref.adam]
    return got

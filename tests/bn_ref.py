"""Train-mode BatchNorm + LeakyReLU + Dropout (uaps_amd/csrc/norm_act.hip): a float64 reference in plain numpy, a host Philox4x32-10,
inputs with no pixel near the LeakyReLU kink, the bars, and one case per entry point and layout (tests/test_bn_ref.py,
tests/test_gpu_bn_forms.py).

Every case names the kernel instantiations it must reach, derived from the launchers' own rules: VEC = H*W % 4 == 0 and every
streamed pointer 16-byte aligned, DROP = drop_p > 0.  The CPU test checks that the cases together name every norm_act kernel of the
built code object; the GPU test runs every case through the C ABI and holds every output against the reference.

The inputs keep every z = gamma * x_hat + beta at least DELTA / 2 away from 0 (the kink), so the reference and the kernel choose the
same slope at every pixel and no pixel or channel is left out of a comparison.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

CHUNK = 4096                 # floats per block of the streaming kernels (kChunk)
MAX_GROUPS = 8               # kMaxGroups
DELTA = 1e-3                 # the band around the kink no input z falls into (|z| >= DELTA / 2 is asserted)
BOUND_SLOTS, BOUND_STRIDE = 16, 64
BOUND_FLOATS = BOUND_SLOTS * BOUND_STRIDE
EPS = 1e-5

# ---- Philox4x32-10 (csrc/philox.hpp) ------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
UAPS_WORD = 0x55415053       # counter word 2 of every draw ("UAPS")
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The ten rounds on uint32 arrays (broadcast): the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _U32 for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(_M0) * c0
        p1 = np.uint64(_M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _U32, n2, p0 & _U32
        k0 = (k0 + np.uint64(_W0)) & _U32
        k1 = (k1 + np.uint64(_W1)) & _U32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def keep_mask(n: int, p: float, seed: int, offset: int, ctr_shift: int = 0, word_shift: int = 0) -> np.ndarray:
    """The dropout keep mask of an n-element tensor: element e uses counter offset + (e >> 2), word e & 3, and is kept when
    (r >> 8) * 2^-24 >= p (p as the fp32 the kernel is passed).  ctr_shift / word_shift move the draw (mutants of the tests)."""
    e = np.arange(n, dtype=np.uint64)
    ncnt = (n + 3) // 4 + 1
    ctr = np.uint64(offset + ctr_shift) + np.arange(ncnt, dtype=np.uint64)
    w = philox4x32_10(ctr & _U32, ctr >> np.uint64(32), UAPS_WORD, 0, seed, seed >> 32)
    words = np.stack(w, axis=1).reshape(-1)                 # words[4 * j + k] = word k of counter offset + j
    r = words[(e >> np.uint64(2)) * np.uint64(4) + ((e + np.uint64(word_shift)) & np.uint64(3))]
    return (r >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 >= float(np.float32(p))


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def _grouped(a, G):
    """[B, C, H, W] -> [G, C, Bg * H * W] (a view where possible)."""
    B, C = a.shape[:2]
    return a.reshape(G, B // G, C, -1).transpose(0, 2, 1, 3).reshape(G, C, -1)


def _ungrouped(a, shape):
    B, C, H, W = shape
    G = a.shape[0]
    return a.reshape(G, C, B // G, H * W).transpose(0, 2, 1, 3).reshape(shape)


def batch_stats(y, G: int, mut: str = ""):
    """Per statistics group: mean [G, C], biased var [G, C] (float64)."""
    yg = _grouped(np.asarray(y, dtype=np.float64), G)
    if mut == "drop_chunk":                                # one 4096-float chunk of image 0, channel 0 left out of the sums
        B, C, H, W = y.shape
        m = np.ones(yg.shape[-1], dtype=bool)
        m[:CHUNK] = False
        mean = yg.mean(-1)
        var = yg.var(-1)
        mean[0, 0] = yg[0, 0, m].mean()
        var[0, 0] = yg[0, 0, m].var()
        return mean, var
    return yg.mean(-1), yg.var(-1)


def forward(y, gamma, beta, *, groups: int, slope: float, p: float = 0.0, mask=None, conv_bias=None, rm=None, rv=None,
            nbt: Optional[int] = None, momentum: float = 0.1, eps: float = EPS, res=None, mut: str = "") -> dict:
    """The train-mode forward in float64.  y [B, C, H, W]; mask: the keep mask (flat, y's element order) when p > 0; res: the
    residual join, out = relu(bn(y) + res).  Running statistics update group after group; None leaves them out."""
    y = np.asarray(y, dtype=np.float64)
    shape, G = y.shape, groups
    B, C, H, W = shape
    eps = float(np.float32(eps))
    M = (B // G) * H * W
    gamma = np.asarray(gamma, np.float64)
    beta = np.asarray(beta, np.float64)
    mean, var = batch_stats(y, G, mut)
    invstd = 1.0 / (np.sqrt(var) + eps) if mut == "eps_outside" else 1.0 / np.sqrt(var + eps)
    if mut == "group0_stats" and G > 1:
        mean[1], invstd[1] = mean[0], invstd[0]
    xhat = (_grouped(y, G) - mean[..., None]) * invstd[..., None]
    z = _ungrouped(gamma[None, :, None] * xhat + beta[None, :, None], shape)
    if res is not None:
        out = np.maximum(z + np.asarray(res, np.float64), 0.0)
    else:
        out = np.where(z > 0, z, z * slope)
        if p > 0:
            scale = 1.0 if mut == "no_drop_scale" else 1.0 / (1.0 - float(np.float32(p)))
            out = np.where(mask.reshape(shape), out * scale, 0.0)
    sc = gamma[None] * invstd
    r = dict(out=out, z=z, mean=mean, var=var, invstd=invstd, xhat=xhat, xf=np.stack([sc, beta[None] - mean * sc], -1))
    if rm is not None:
        rm, rv = np.asarray(rm, np.float64).copy(), np.asarray(rv, np.float64).copy()
        bias = np.zeros(C) if conv_bias is None or mut == "rm_no_bias" else np.asarray(conv_bias, np.float64)
        mom = float(np.float32(momentum))
        for g in range(G):
            unb = var[g] if mut == "rv_biased" else (var[g] * M / (M - 1) if M > 1 else var[g])
            rm = (1 - mom) * rm + mom * (mean[g] + bias)
            rv = (1 - mom) * rv + mom * unb
        r["rm"], r["rv"] = rm, rv
    if nbt is not None:
        r["nbt"] = nbt + G
    return r


def eval_forward(y, gamma, beta, rm, rv, *, slope: float, conv_bias=None, eps: float = EPS) -> dict:
    """Eval mode: coef = gamma / sqrt(rv + eps), mean_eff = rm - conv bias, out = leaky_relu((y - mean_eff) coef + beta)."""
    y = np.asarray(y, np.float64)
    eps = float(np.float32(eps))
    mean_eff = np.asarray(rm, np.float64) - (0.0 if conv_bias is None else np.asarray(conv_bias, np.float64))
    sc = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(rv, np.float64) + eps)
    z = (y - mean_eff[None, :, None, None]) * sc[None, :, None, None] + np.asarray(beta, np.float64)[None, :, None, None]
    return dict(out=np.where(z > 0, z, z * slope), z=z, sc=sc, mean_eff=mean_eff)


def eval_backward(dout, z, sc, slope: float) -> np.ndarray:
    return np.where(z > 0, dout, dout * slope) * np.asarray(sc)[None, :, None, None]


def backward(dout, y, gamma, beta, mean, invstd, *, groups: int, slope: float, p: float = 0.0, mask=None, mut: str = "") -> dict:
    """The train-mode backward in float64 from the saved statistics mean / invstd [G, C] (the values the kernel is given)."""
    y, dout = np.asarray(y, np.float64), np.asarray(dout, np.float64)
    shape, G = y.shape, groups
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean, invstd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    xhat = (_grouped(y, G) - mean[..., None]) * invstd[..., None]
    z = gamma[None, :, None] * xhat + beta[None, :, None]
    g = _grouped(dout, G)
    if p > 0:
        scale = 1.0 if mut == "no_drop_scale" else 1.0 / (1.0 - float(np.float32(p)))
        g = np.where(_grouped(mask.reshape(shape), G), g * scale, 0.0)
    d = np.where(z < 0, g, g * slope) if mut == "slope_pos" else np.where(z > 0, g, g * slope)
    k2, k3 = d.mean(-1), (d * xhat).mean(-1)
    k2u = np.zeros_like(k2) if mut == "no_k2" else k2
    k3u = np.zeros_like(k3) if mut == "no_k3" else k3
    sc = gamma[None] * invstd
    dy = sc[..., None] * (d - k2u[..., None] - xhat * k3u[..., None])
    sd, sdx = d.sum(-1), (d * xhat).sum(-1)
    upto = 1 if mut == "first_group" else G
    return dict(dy=_ungrouped(dy, shape), d=d, xhat=xhat, z=z, k2=k2, k3=k3, dgamma=sdx[:upto].sum(0), dbeta=sd[:upto].sum(0),
                abs_dgamma=np.abs(d * xhat).sum(-1).sum(0), abs_dbeta=np.abs(d).sum(-1).sum(0),
                rms_d=np.sqrt((d * d).mean(-1)), sc=sc)


def two_halves_coef(bwd: dict, mean, invstd, gamma, beta) -> np.ndarray:
    """coef [G][C][8] of uaps_bn_act_bwd_prepare / _finalize: (mean, invstd, gamma invstd, beta, k2, k3, 0, 0)."""
    mean, invstd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    G, C = mean.shape
    q = np.zeros((G, C, 8))
    q[..., 0], q[..., 1] = mean, invstd
    q[..., 2] = np.float32(gamma)[None] * np.float32(invstd)          # the fp32 product the kernel stores
    q[..., 3] = np.asarray(beta, np.float64)[None]
    q[..., 4], q[..., 5] = bwd["k2"], bwd["k3"]
    return q


def dy_bound(bwd: dict) -> float:
    """bn_bwd_finalize_kernel: max over groups and channels of |gamma invstd| (max|d| + |k2| + max|x_hat| |k3|), the maxima over the
    whole tensor."""
    Gm, Xm = float(np.abs(bwd["d"]).max()), float(np.abs(bwd["xhat"]).max())
    return float((np.abs(bwd["sc"]) * (Gm + np.abs(bwd["k2"]) + Xm * np.abs(bwd["k3"]))).max())


def host_partials(y, B: int, C: int, ppi: int, shift=None, dout=None, mean=None, invstd=None, gamma=None, beta=None, slope=0.0,
                  G: int = 1) -> np.ndarray:
    """float2 [C][B][ppi] in float64 -> fp32: per image, the plane cut into ppi contiguous runs (empty runs hold 0).
    Forward: (sum(y - shift), sum((y - shift)^2)); backward (dout given): (sum d, sum d x_hat)."""
    y = np.asarray(y, np.float64).reshape(B, C, -1)
    HW = y.shape[-1]
    if dout is None:
        v1 = y - (0.0 if shift is None else np.asarray(shift, np.float64)[None, :, None])
        v2 = v1 * v1
    else:
        Bg = B // G
        gi = np.arange(B) // Bg
        mu, inv = np.asarray(mean, np.float64)[gi], np.asarray(invstd, np.float64)[gi]          # [B, C]
        xh = (y - mu[..., None]) * inv[..., None]
        z = np.asarray(gamma, np.float64)[None, :, None] * xh + np.asarray(beta, np.float64)[None, :, None]
        g = np.asarray(dout, np.float64).reshape(B, C, -1)
        v1 = np.where(z > 0, g, g * slope)
        v2 = v1 * xh
    edges = (np.arange(ppi + 1) * HW) // ppi
    out = np.zeros((C, B, ppi, 2))
    c1 = np.concatenate([np.zeros((B, C, 1)), np.cumsum(v1, -1)], -1)
    c2 = np.concatenate([np.zeros((B, C, 1)), np.cumsum(v2, -1)], -1)
    out[..., 0] = (c1[..., edges[1:]] - c1[..., edges[:-1]]).transpose(1, 0, 2)
    out[..., 1] = (c2[..., edges[1:]] - c2[..., edges[:-1]]).transpose(1, 0, 2)
    return out.astype(np.float32)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def rng_for(case_id: str, salt: int = 0) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(case_id.encode()) * 1009 + salt)          # the same data in every process


def kinkfree(rng, B, C, H, W, G, gamma, beta, mean_gc, std_gc, delta: float = DELTA):
    """y [B, C, H, W] fp32 with every statistics group's and channel's standardised values x_hat pushed out of the band
    |gamma x_hat + beta| < delta, re-standardised exactly in float64, then y = mean + std x_hat ([G, C] each) rounded to fp32.
    beta is returned too: where a group has one or two values per channel (x_hat fixed at 0 or +-1), beta is moved instead."""
    M = (B // G) * H * W
    std = np.broadcast_to(np.asarray(std_gc, np.float64), (G, C))
    # the kernel's x_hat divides by sqrt(var + eps): z = gamma f x + beta with f = std / sqrt(std^2 + eps)
    ga = (np.asarray(gamma, np.float64)[None] * std / np.sqrt(std * std + float(np.float32(EPS))))[..., None]
    beta = np.asarray(beta, np.float64).copy()
    be = beta[None, :, None]
    x = rng.standard_normal((G, C, M), dtype=np.float32).astype(np.float64)
    for _ in range(2):
        x -= x.mean(-1, keepdims=True)
        s = x.std(-1, keepdims=True)
        x /= np.where(s > 0, s, 1.0)
        g_, c_, m_ = np.nonzero(np.abs(ga * x + be) < delta)
        zi = ga[g_, c_, 0] * x[g_, c_, m_] + be[0, c_, 0]
        x[g_, c_, m_] = (np.where(zi >= 0, 3 * delta, -3 * delta) - be[0, c_, 0]) / ga[g_, c_, 0]
    x -= x.mean(-1, keepdims=True)
    s = x.std(-1, keepdims=True)
    x /= np.where(s > 0, s, 1.0)
    for _ in range(8 if M <= 2 else 0):                     # x_hat is pinned (M <= 2): move beta out of the band
        bad = (np.abs(ga * x + beta[None, :, None]) < 2 * delta).any(-1).any(0)
        if not bad.any():
            break
        beta[bad] += 5 * delta
    yg = np.broadcast_to(np.asarray(mean_gc, np.float64), (G, C))[..., None] + std[..., None] * x
    y = _ungrouped(yg, (B, C, H, W)).astype(np.float32)
    return y, beta


def min_abs_z(y, gamma, beta, G: int, eps: float = EPS) -> float:
    """min |z| of the exact float64 batch statistics of the fp32 y."""
    r = forward(y, gamma, beta, groups=G, slope=1.0, eps=eps)
    return float(np.abs(r["z"]).min())


# ---- the case table -----------------------------------------------------------------------------------------------------------
FWD, FWD_PARTIALS, FINALIZE, BWD, HALVES, BWD_FINALIZE, EVAL = "fwd", "fwd_partials", "finalize", "bwd", "halves", "bwd_finalize", "eval"


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                   # one of the names above
    B: int
    C: int
    H: int
    W: int
    groups: int = 1
    slope: float = 0.01
    p: float = 0.0
    bias: bool = True            # a conv bias in front (forward: shifts running_mean; backward: d(conv bias) = 0 is written)
    shift: bool = True           # given partials: formed about stats_mean - stats_bias (hints); the own pass always shifts (shift_of)
    running: bool = True         # running_mean / running_var / num_batches_tracked (False: NULL, track_running_stats=False)
    residual: bool = False
    amax: bool = False           # uaps_call_hints::out_amax
    off: int = 0                 # the streamed tensors are views this many floats into their buffers (1: misaligned)
    ppi: int = 0                 # host partials: parts per image (FWD_PARTIALS, FINALIZE, BWD_FINALIZE)
    large_mean: bool = False     # channels whose mean is > 1e3 standard deviations (with the shift near the mean)
    seed: int = 0x9E3779B97F4A7C15
    offset: int = 0

    @property
    def HW(self):
        return self.H * self.W

    @property
    def M(self):
        return self.B // self.groups * self.HW

    @property
    def vec(self) -> bool:
        return self.HW % 4 == 0 and self.off % 4 == 0

    @property
    def kernels(self) -> frozenset:
        """The instantiations the launchers pick for this case (norm_act.hip: vec = HW % 4 == 0 and 16-byte aligned streamed
        pointers; D = drop_p > 0); every forward case also runs uaps_bn_param_bounds."""
        v, d = ("true" if self.vec else "false"), ("true" if self.p > 0 else "false")
        e = self.entry
        if e == FWD:
            return frozenset({f"bn_stats_kernel<{v}>", "bn_finalize_fwd", f"bn_apply_kernel<{v}, {d}>", "bn_param_bounds_kernel"})
        if e == FWD_PARTIALS:
            return frozenset({"bn_finalize_fwd", f"bn_apply_kernel<{v}, {d}>", "bn_param_bounds_kernel"})
        if e == FINALIZE:
            return frozenset({"bn_finalize_fwd"})
        if e == BWD:
            return frozenset({f"bn_bwd_sums_kernel<{v}, {d}>", f"bn_bwd_dx_kernel<{v}, {d}>"})
        if e == HALVES:
            return frozenset({f"bn_bwd_sums_max_kernel<{v}>", "bn_bwd_finalize_kernel", f"bn_bwd_dx_coef_kernel<{v}>"})
        if e == BWD_FINALIZE:
            return frozenset({"bn_bwd_finalize_kernel", f"bn_bwd_dx_coef_kernel<{v}>"})
        if e == EVAL:
            return frozenset({"bn_coef_eval", f"bn_apply_kernel<{v}, false>", f"bn_bwd_eval_kernel<{v}>"})
        raise ValueError(e)


def _cases():
    cs = []
    add = cs.append
    # the step's layers: B = 32 in two statistics groups (labelled / unlabelled), the U-Net's channel / size pairs
    for C_, H_, p in ((16, 256, 0.0), (32, 128, 0.1), (64, 64, 0.0), (128, 32, 0.3), (256, 16, 0.5)):
        add(Case(f"fwd-step-{C_}x{H_}", FWD, 32, C_, H_, H_, 2, p=p, amax=C_ == 64))
        add(Case(f"bwd-step-{C_}x{H_}", BWD, 32, C_, H_, H_, 2, p=p, amax=C_ == 128, offset=2 ** 32 - 3))
    add(Case("halves-step-16x256", HALVES, 32, 16, 256, 256, 2, amax=True))
    add(Case("halves-step-64x64", HALVES, 32, 64, 64, 64, 2, slope=0.2))
    # ragged shapes, odd B, tiny planes, a tail chunk, scalar paths
    add(Case("fwd-odd-hw1", FWD, 5, 24, 1, 1, 1, p=0.2, offset=2 ** 32 - 1))
    add(Case("fwd-hw2-bg1", FWD, 3, 8, 1, 2, 3))                          # Bg = 1, M = 2: torch's M / (M - 1) = 2
    add(Case("fwd-hw3-bg1", FWD, 4, 7, 3, 1, 4, slope=0.0))
    add(Case("fwd-hw63", FWD, 3, 5, 7, 9, 1, p=0.5, amax=True))
    add(Case("fwd-hw4097-g5", FWD, 5, 3, 17, 241, 5, slope=0.2))          # H*W = 4097: a one-float tail chunk; 5 groups (two rounds)
    add(Case("fwd-65x65-g8", FWD, 8, 6, 65, 65, 8, p=0.25, large_mean=True))
    add(Case("fwd-misaligned", FWD, 4, 16, 32, 32, 2, off=1, p=0.3, amax=True))            # HW % 4 == 0, scalar path
    add(Case("fwd-misaligned-nodrop", FWD, 2, 8, 16, 20, 1, off=1))
    add(Case("fwd-bc65535", FWD, 257, 255, 1, 1, 1, bias=False))          # B * C = 65535 planes, the gridDim.y limit
    add(Case("fwd-stem-2x64x320", FWD, 2, 64, 320, 320, 2, large_mean=True, amax=True))
    add(Case("fwd-norunning", FWD, 6, 12, 9, 12, 3, running=False, p=0.1))
    add(Case("fwd-nobias-slope1", FWD, 4, 10, 12, 12, 4, bias=False, slope=1.0))
    add(Case("fwd-residual", FWD, 4, 16, 24, 24, 2, residual=True, amax=True))
    add(Case("fwd-residual-scalar", FWD, 3, 5, 5, 7, 1, residual=True))
    add(Case("fwd-large-mean-g4", FWD, 8, 16, 40, 40, 4, large_mean=True, p=0.1))
    # the statistics from host partials: parts per image 1, 7, 4096 and 2333 (not a multiple of 8 * 256: the clamped tail)
    add(Case("fwdp-ppi1-g2", FWD_PARTIALS, 4, 16, 32, 32, 2, ppi=1, large_mean=True, amax=True))
    add(Case("fwdp-ppi7-g3", FWD_PARTIALS, 6, 9, 13, 11, 3, ppi=7, p=0.2))
    add(Case("fwdp-ppi4096-g1", FWD_PARTIALS, 2, 4, 64, 64, 1, ppi=4096, shift=False))
    add(Case("fwdp-ppi2333-g8-misaligned", FWD_PARTIALS, 8, 5, 48, 48, 8, ppi=2333, off=1, p=0.4))
    add(Case("fin-ppi7-g5", FINALIZE, 10, 11, 8, 8, 5, ppi=7, large_mean=True))
    add(Case("fin-ppi4096-g4", FINALIZE, 4, 3, 64, 64, 4, ppi=4096))
    add(Case("fin-ppi2333-g1-bg1", FINALIZE, 1, 6, 50, 50, 1, ppi=2333, running=False))
    add(Case("fin-ppi1-g8-bg1", FINALIZE, 8, 7, 1, 3, 8, ppi=1))
    # backward
    add(Case("bwd-odd-hw3-g3", BWD, 3, 7, 3, 1, 3, p=0.3))
    add(Case("bwd-hw4097-g5", BWD, 5, 3, 17, 241, 5, slope=0.2, amax=True))
    add(Case("bwd-misaligned-drop", BWD, 4, 16, 32, 32, 2, off=1, p=0.3))
    add(Case("bwd-misaligned", BWD, 2, 8, 16, 20, 2, off=1, bias=False))
    add(Case("bwd-bc65535", BWD, 257, 255, 1, 1, 1, bias=False))
    add(Case("bwd-65x65-g8", BWD, 8, 6, 65, 65, 8, p=0.25))
    add(Case("bwd-stem", BWD, 2, 64, 320, 320, 2, slope=0.1))
    add(Case("halves-hw63", HALVES, 3, 5, 7, 9, 1))
    add(Case("halves-misaligned-g4", HALVES, 8, 6, 20, 20, 4, off=1, amax=True))
    add(Case("halves-hw4097-g5", HALVES, 5, 3, 17, 241, 5, slope=0.0))
    add(Case("bfin-ppi1-g2", BWD_FINALIZE, 4, 16, 32, 32, 2, ppi=1))
    add(Case("bfin-ppi2333-g8", BWD_FINALIZE, 8, 5, 48, 48, 8, ppi=2333, off=1))
    add(Case("bfin-ppi7-g3", BWD_FINALIZE, 6, 9, 13, 11, 3, ppi=7, bias=False))
    # eval forward + backward
    add(Case("eval", EVAL, 3, 16, 24, 24, 1))
    add(Case("eval-misaligned", EVAL, 2, 5, 7, 9, 1, off=1, slope=0.2))
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def inputs(case: Case) -> dict:
    """The case's host data (float32 numpy), seeded from a CRC of its id."""
    rng = rng_for(case.id)
    B, C, H, W, G = case.B, case.C, case.H, case.W, case.groups
    gamma = rng.uniform(0.3, 2.0, C) * np.where(rng.random(C) < 0.2, -1.0, 1.0)
    beta = rng.standard_normal(C)
    std_c = 10.0 ** rng.uniform(-1.5, 1.5, C)
    ratio = rng.standard_normal(C) * 10.0 ** rng.uniform(-1.0, 1.2, C)            # mean / std up to ~50
    if case.large_mean:
        ratio[::3] = np.where(rng.random(len(ratio[::3])) < 0.5, -1, 1) * rng.uniform(1.2e3, 3e3, len(ratio[::3]))
    mean_c = ratio * std_c
    gamma, beta = gamma.astype(np.float32), beta.astype(np.float32)
    # the statistics groups differ: group g's mean and std move around the channel's
    mean_gc = mean_c[None] + std_c[None] * rng.standard_normal((G, C)) * 0.5
    std_gc = std_c[None] * rng.uniform(0.7, 1.4, (G, C))
    y, beta64 = kinkfree(rng, B, C, H, W, G, gamma, beta, mean_gc, std_gc)
    beta = beta64.astype(np.float32)
    d = dict(y=y, gamma=gamma, beta=beta)
    d["conv_bias"] = (rng.standard_normal(C) * 0.5).astype(np.float32) if case.bias else None
    b = np.zeros(C) if d["conv_bias"] is None else d["conv_bias"].astype(np.float64)
    # running_mean tracks the channel's mean (+ conv bias) within a few std: the shift of the statistics pass; without a shift the
    # large means are absent, so the shift-free sums stay conditioned
    d["rm"] = (mean_c + b + std_c * rng.standard_normal(C) * 2.0).astype(np.float32)
    d["rv"] = (std_c ** 2 * rng.uniform(0.5, 2.0, C)).astype(np.float32)
    d["nbt"] = 7
    mag = 10.0 ** rng.uniform(-1, 1, C)
    dout = rng.standard_normal((B, C, H, W))
    d["dout"] = (np.sign(dout) * (0.5 + np.abs(dout)) * mag[None, :, None, None]).astype(np.float32)   # |dout| >= 0.5 mag
    if case.residual:
        d["res"] = rng.standard_normal((B, C, H, W)).astype(np.float32)
        d["res"][np.abs(d["res"]) < 4 * DELTA] = 0.5               # the join's relu kink: z + res away from 0 as well
    d["mask"] = keep_mask(B * C * H * W, case.p, case.seed, case.offset) if case.p > 0 else None
    if case.entry in (BWD, HALVES, BWD_FINALIZE):
        r = forward(y, gamma, beta, groups=G, slope=case.slope)
        d["save_mean"] = r["mean"].astype(np.float32)
        d["save_invstd"] = r["invstd"].astype(np.float32)
    if case.entry == EVAL:                                           # running statistics = the batch's: z stays out of the band
        r = forward(y, gamma, beta, groups=1, slope=case.slope)
        d["rm"] = (r["mean"][0] + b).astype(np.float32)
        d["rv"] = r["var"][0].astype(np.float32)
    return d


def shift_of(case: Case, inp: dict):
    """The per-channel value the partial sums are formed about (float64): running_mean - conv bias for the own statistics pass
    (0 - conv bias without running statistics), stats_mean - stats_bias (= running_mean - conv bias) for given partials with the
    shift named, else 0."""
    b = np.zeros(case.C) if inp["conv_bias"] is None else inp["conv_bias"].astype(np.float64)
    if case.entry == FWD:
        return (inp["rm"].astype(np.float64) if case.running else 0.0) - b
    return inp["rm"].astype(np.float64) - b if case.shift else np.zeros(case.C)


# ---- the bars: each pointwise error over a bound scaled by its own conditioning ----------------------------------------------
# TAU values: 4x (at most) the largest ratio measured on an MI355X over all cases (profiles/bn_forms_tau.txt)
TAU = dict(out=5e-7, mean=2.5e-7, invstd=4e-7, running=1.5e-7, xf=4e-7, dy=6e-7, dgamma=1.2e-7, dbeta=1.8e-7, k=1e-7)


def ratio(got, ref, cond) -> float:
    got, ref, cond = (np.asarray(a, np.float64) for a in (got, ref, cond))
    if not np.all(np.isfinite(got)):
        return math.inf
    return float((np.abs(got - ref) / cond).max()) if got.size else 0.0


def fwd_conds(case: Case, inp: dict, ref: dict) -> dict:
    """Conditioning of each forward output.  r = |mean - shift| / sigma: the variance from sums formed about `shift` loses
    ~r^2 ulps; |mean| / sigma: save_mean is an fp32 value."""
    G = case.groups
    gamma, beta = inp["gamma"].astype(np.float64), inp["beta"].astype(np.float64)
    sigma = 1.0 / ref["invstd"]
    r = np.abs(ref["mean"] - shift_of(case, inp)[None]) / sigma
    am = np.abs(ref["mean"]) / sigma
    ga = np.abs(gamma)[None]
    xa = np.abs(ref["xhat"])
    scale = 1.0 / (1.0 - float(np.float32(case.p))) if case.p > 0 else 1.0
    y_cond = (ga[..., None] * ((xa + 1) * (1 + r * r)[..., None] + am[..., None]) + np.abs(beta)[None, :, None]) * scale
    out = _ungrouped(y_cond, (case.B, case.C, case.H, case.W))
    if case.residual:
        out = out + np.abs(inp["res"])
    c = dict(out=out, mean=np.abs(ref["mean"]) + sigma * (1 + r), invstd=ref["invstd"] * (1 + r * r))
    sc = ga * ref["invstd"]
    c["xf0"] = sc * (1 + r * r)
    c["xf1"] = np.abs(beta)[None] + sc * (np.abs(ref["mean"]) * (1 + r * r) + sigma * (1 + r))
    if "rm" in ref:
        b = np.zeros(case.C) if inp["conv_bias"] is None else np.abs(inp["conv_bias"].astype(np.float64))
        c["rm"] = np.abs(inp["rm"].astype(np.float64)) + b + (np.abs(ref["mean"]) + sigma * (1 + r)).max(0)
        c["rv"] = inp["rv"].astype(np.float64) + (ref["var"] * (1 + r * r)).max(0) * (case.M / max(case.M - 1, 1))
    return c


def fwd_ratios(case: Case, inp: dict, ref: dict, got: dict) -> dict:
    """got: out [B,C,H,W], mean / invstd [G,C], rm / rv [C], xf [G,C,2] (any subset)."""
    c = fwd_conds(case, inp, ref)
    r = {}
    if "out" in got:
        r["out"] = ratio(got["out"], ref["out"], c["out"])
    if "mean" in got:
        r["mean"] = ratio(got["mean"], ref["mean"], c["mean"])
        r["invstd"] = ratio(got["invstd"], ref["invstd"], c["invstd"])
    if "rm" in got:
        r["running"] = max(ratio(got["rm"], ref["rm"], c["rm"]), ratio(got["rv"], ref["rv"], c["rv"]))
    if "xf" in got:
        r["xf"] = max(ratio(got["xf"][..., 0], ref["xf"][..., 0], c["xf0"]), ratio(got["xf"][..., 1], ref["xf"][..., 1], c["xf1"]))
    return r


def bwd_ratios(case: Case, ref: dict, got: dict) -> dict:
    """got: dy [B,C,H,W], dgamma / dbeta [C], coef [G,C,8] (k2, k3 held against their bars)."""
    shape = (case.B, case.C, case.H, case.W)
    r = {}
    if "dy" in got:
        cond = np.abs(ref["sc"])[..., None] * (np.abs(ref["d"]) + np.abs(ref["k2"])[..., None] + np.abs(ref["xhat"]) *
                                             np.abs(ref["k3"])[..., None] + ref["rms_d"][..., None])
        r["dy"] = ratio(got["dy"], ref["dy"], _ungrouped(cond, shape))
    if "dgamma" in got:
        r["dgamma"] = ratio(got["dgamma"], ref["dgamma"], ref["abs_dgamma"])
        r["dbeta"] = ratio(got["dbeta"], ref["dbeta"], ref["abs_dbeta"])
    if "coef" in got:
        r["k"] = max(ratio(got["coef"][..., 4], ref["k2"], np.abs(ref["d"]).mean(-1)),
                     ratio(got["coef"][..., 5], ref["k3"], np.abs(ref["d"] * ref["xhat"]).mean(-1)))
    return r


def param_bound(gamma, beta) -> np.float32:
    """uaps_bn_param_bounds of one layer: max_c(|gamma_c| + |beta_c|) in fp32."""
    return np.float32((np.abs(np.float32(gamma)) + np.abs(np.float32(beta))).max())


def output_bound_factor(case: Case) -> float:
    """bounds.bn_output_bound's factor: sqrt(elements per channel and statistics group) x 1 / (1 - p) of the dropout."""
    return math.sqrt(max(1, case.M)) * (1.0 / (1.0 - case.p) if case.p > 0 else 1.0)

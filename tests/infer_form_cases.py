"""The kernel forms of the inference side, one small record per case (tests/test_infer_form_table.py, tests/test_gpu_infer_forms.py,
tools/infer_tau.py): csrc/tta.hip (uaps_tta_views, uaps_tta_fold), csrc/tiled.hip (uaps_tile_cut, uaps_tile_fold) and csrc/curves.hip
(uaps_score_curves, uaps_plane_curves).

A case names the entry point, the element offset of every tensor view, the pattern, the call's arguments and the forms it is there to
reach; Case.kernels gives the demangled kernel instantiations it must launch, from the launch rules of the three files restated here:
  folds    V = 4 when W % 4 == 0 and every output that is not NULL (probs, mask, conf, each map_out) is 16-byte aligned, else V = 1;
           C by UAPS_BY_C (2 .. 8; the tiled fold also 0: maps alone)
  curves   V = 4 when H W % 4 == 0 and scores, target, (plane: pred,) (regions: region_labels) are 16-byte aligned; a workgroup spans
           512 V 2 pixels of one image and stops at the first round of 512 V pixels that starts at or behind H W;
           units per group = clamp(65536 // (bins * (12 with qsum, else 4)), 1, 2 R), groups = ceil(2 R / that); zero_kernel always,
           pro_kernel with regions and n_classes > 0

The references.
  curves   tests/curves_ref.py: integers, exact; pro_sum bit for bit (IEEE double divisions added in ascending region order on both sides).
           One exception, the existing sweep's: with from_logits qsum adds the fixed point of the DEVICE's fp32 probabilities, which a
           float64 softmax does not reproduce to the last bit; a cell may differ by Q_LOGITS per pixel it counts (hist stays exact).
           walk() is a second restatement with switches for the mutants of tests/test_infer_form_table.py.
  folds    a float64 walk of the operation sequence of include/uaps_hip.h with the fp32-exact parts formed in numpy float32 exactly as
           the kernels form them -- TTA: r, src = r * d rounded on its own, i0, i1, l1 = src - i0, l0 = 1 - l1; tiled: w = wy * wx rounded
           on its own and the running weight sum in the kernel's order -- so that only the softmax and the order of the fp32 mixes differ.
           Beside every value runs a bound of what an fp32 evaluation can have lost, per element:
             softmax     d = z - max: U |d| relative on e = exp(d); expf 3 ulp and `/` 1 ulp, the IEEE figures of
                         tests/consistency_ref.py (the build has no fast-math; U = 2^-24, one ulp = 2 U relative); the largest class
                         has d = 0 exactly and expf(0) is 1 exactly, so its term carries no error; the sum: the terms' bounds and U
                         per partial sum.
             TTA mix     the weights are exact; l0h (l0w a + l1w b) + l1h (l0w c + l1w d) is four levels of fp32 operations on
                         non-negative numbers (fused or not): 4 U of the value beside the weighted corner bounds; every running add U.
             tiled       each weighted add is one fma: U of the accumulator behind it; the final division DIV_ULP ulp.
           The bar of an output element is that bound, times SLACK = 1.01 for the second-order terms, plus 2^-126 for a flushed
           denormal.  Nothing a kernel returns enters a bar.  tests/test_infer_form_table.py asserts that no bar exceeds the bars of
           the existing sweeps (tta_ref.TAU_SUM / TAU_VIEWS, tiled_ref.TAU).
  exact    uaps_tile_cut is a copy; the flipped half of uaps_tta_views is the plain half mirrored; mask is the lowest-index arg-max of
           the kernel's own probs; tiled conf is that value, TTA conf float32(max) / float32(views), one IEEE division.
  masks    equal to the float64 arg-max wherever the float64 top-2 margin exceeds twice the case's largest bar; at most MAX_EXCLUDED of a
           case's pixels under it (asserted on the CPU from the reference alone).  The `ties` case is exempt: its two largest classes are
           bit-identical everywhere and its mask must name the lower one."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

import curves_ref as CR
import instances_ref as IR
import tiled_ref as TR

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EXPF_ULP, DIV_ULP = 3, 1
SLACK, TINY = 1.01, 2.0 ** -126
MAX_EXCLUDED = 0.01
U8, I32, I64 = 1, 4, 8                        # UAPS_LABEL_*
NP_OF = {U8: np.uint8, I32: np.int32, I64: np.int64}
ELEM = dict(probs=4, mask=8, conf=4, map0=4, map1=4, scores=4, rl=4, out=4, x=4)
KERNEL_NAMES = ("tta_views_kernel", "tta_fold_kernel", "tile_cut_kernel", "tile_fold_kernel", "curves_kernel", "zero_kernel", "pro_kernel")
UNREACHABLE = {}                              # kernel -> why no call can launch it
Q_LOGITS = 7.2e-7 * 2 ** 24 + 1                # fixed-point units a pixel's q(s) may differ by under from_logits (tests/curves_ref.py: the
                                              # device's expf, adds and division move a probability by less than 7.2e-7; one for rintf)
CT, ITER, LDS, PEEL = 512, 2, 65536, 4        # curves.hip: threads of a workgroup, rounds, bytes of LDS, broadcast rounds of wave_add


def al16(off, size):
    return off * size % 16 == 0


def units_per_group(R, bins, q):
    return min(max(LDS // (bins * (12 if q else 4)), 1), 2 * R)


def groups(R, bins, q):
    return -(-2 * R // units_per_group(R, bins, q))


def span(V):
    return CT * ITER * V


def wpi(HW, V):
    return -(-HW // span(V))


def rounds_run(HW, V):
    """The rounds of 512 V pixels the last workgroup of an image runs."""
    first = (wpi(HW, V) - 1) * span(V)
    return sum(1 for it in range(ITER) if first + it * CT * V < HW)


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                  # "tta_fold", "tta_views", "tile_cut", "tile_fold", "score", "plane"
    pattern: str
    offs: tuple = ()            # ((tensor, elements the view is moved by from a 256-byte boundary), ...); 0 where not named
    args: tuple = ()            # ((argument, value), ...)
    forms: tuple = ()           # the forms the case is there to reach

    def off(self, name):
        return dict(self.offs).get(name, 0)

    def arg(self, name, default=None):
        return dict(self.args).get(name, default)

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def outs(self):
        if self.entry == "tta_fold":
            return self.arg("outs", ("probs", "mask", "conf"))
        if self.entry == "tile_fold":
            return (self.arg("outs", ("probs", "mask", "conf")) if self.arg("C") else ()) + tuple(f"map{m}" for m in range(self.arg("n_maps", 0)))
        return ()

    @property
    def V(self):
        a = self.arg
        if self.entry in ("tta_fold", "tile_fold"):
            return 4 if a("W") % 4 == 0 and all(al16(self.off(k), ELEM[k]) for k in self.outs) else 1
        if self.entry == "score":
            ok = a("H") * a("W") % 4 == 0 and al16(self.off("scores"), 4) and al16(self.off("target"), a("tdt", I64))
            return 4 if ok and (not a("regions") or al16(self.off("rl"), 4)) else 1
        if self.entry == "plane":
            ok = a("H") * a("W") % 4 == 0 and al16(self.off("scores"), 4)
            return 4 if ok and al16(self.off("target"), a("tdt", I64)) and al16(self.off("pred"), a("pdt", I64)) else 1
        return None

    @property
    def R(self):
        return 1 if self.entry == "plane" else len(self.arg("classes", ())) + self.arg("top", 1)

    @property
    def kernels(self):
        e, a = self.entry, self.arg
        if e == "tta_views":
            return frozenset({"tta_views_kernel"})
        if e == "tile_cut":
            return frozenset({"tile_cut_kernel"})
        if e == "tta_fold":
            return frozenset({f"tta_fold_kernel<{a('C')}, {self.V}>"})
        if e == "tile_fold":
            return frozenset({f"tile_fold_kernel<{a('C')}, {self.V}>"})
        q = "true" if a("qsum", 0) else "false"
        k = {"zero_kernel", f"curves_kernel<{a('C') if e == 'score' else 0}, {self.V}, {q}>"}
        if e == "score" and a("regions") and len(a("classes", ())) > 0:
            k.add("pro_kernel")
        return frozenset(k)


CASES: list = []


def add(cid, entry, pattern="randn", offs=None, forms=(), **args):
    CASES.append(Case(cid, entry, pattern, tuple(sorted((offs or {}).items())), tuple(sorted(args.items())), tuple(forms)))


def ids(entry):
    return [c.id for c in CASES if c.entry == entry]


def _rng(c, salt=0):
    return np.random.default_rng(c.seed + salt)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ the softmax and its bound
def softmax_b(z):
    """(float64 softmax over axis 1 of the fp32 logits z, the bound of an fp32 evaluation of it)."""
    z = z.astype(F64)
    d = z - z.max(axis=1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=1, keepdims=True)
    rel = np.where(d == 0, 0.0, 2 * EXPF_ULP * U + U * np.abs(d))          # expf(0) is 1
    partial = np.cumsum(e, axis=1)[:, 1:].sum(axis=1, keepdims=True)          # every fp32 add rounds its partial sum
    err_s = (e * rel).sum(axis=1, keepdims=True) + U * partial
    p = e / s
    return p, p * (rel + err_s / s + 2 * DIV_ULP * U)


def _bar(b):
    return b * SLACK + TINY


# ------------------------------------------------------------------------------------------------ test-time augmentation
def corners(n_in, n_out, mut=""):
    """(i0, i1, l0, l1) of every destination index, formed in fp32 as csrc/tta.hip forms them."""
    if mut == "ratio_inverse":
        r = F32(n_out - 1) / F32(n_in - 1) if n_in > 1 else F32(0)
    else:
        r = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = (F32(r) * np.arange(n_out, dtype=F32)).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 if mut == "i1_is_i0" else i0 + (i0 < n_in - 1)
    l1 = (src - (i1 if mut == "l1_from_i1" else i0).astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0.astype(F64), l1.astype(F64)


def _mix(v, h_in, w_in, H, W, cols=None, mut=""):
    """The bilinear mix of v [..., h, w] (float64) at every output pixel; cols maps the two source columns (the un-flip)."""
    y0, y1, my, ly = corners(h_in, H, mut)
    x0, x1, mx, lx = corners(w_in, W, mut)
    if cols is not None:
        x0, x1 = cols(x0), cols(x1)
    my, ly = my[:, None], ly[:, None]
    g = lambda ys, xs: v[..., ys, :][..., xs]
    return my * (mx * g(y0, x0) + lx * g(y0, x1)) + ly * (mx * g(y1, x0) + lx * g(y1, x1))


def tta_fold_inputs(c):
    a, rng = c.arg, _rng(c)
    n = (2 if a("flip", 1) else 1) * a("B", 2)
    zs = [(rng.standard_normal((n, a("C"), h, w)) * a("gain", 2.0)).astype(F32) for h, w in a("sizes")]
    if c.pattern == "ties":                        # classes 1 and 3 bit-identical and the largest everywhere
        for z in zs:
            z[:, 1] = np.abs(z[:, 1]) + F32(20)
            z[:, 3] = z[:, 1]
    return {f"z{s}": _ro(z) for s, z in enumerate(zs)}


def tta_fold_walk(c, inp, mut=""):
    """(the float64 sum [B,C,H,W], its bound)."""
    a = c.arg
    B, H, W, flip = a("B", 2), a("H"), a("W"), a("flip", 1)
    acc = bnd = None
    for s, (h, w) in enumerate(a("sizes")):
        p, pb = softmax_b(inp[f"z{s}"])
        for half in range(2 if flip else 1):
            img = slice(0, B) if (half == 0 or mut == "flip_same_image") else slice(B, 2 * B)
            cols = (lambda x, w=w: w - 1 - x) if (half == 1 and mut != "no_unflip") else None
            t = _mix(p[img], h, w, H, W, cols, mut)
            tb = _mix(pb[img], h, w, H, W, cols, mut) + 4 * U * np.abs(t)
            if acc is None:
                acc, bnd = t, tb
            else:
                acc = acc + t
                bnd = bnd + tb + U * np.abs(acc)
    return acc, bnd


def tta_views_inputs(c):
    a = c.arg
    return dict(x=_ro(_rng(c).standard_normal((a("B", 2), a("Cin"), a("H"), a("W"))).astype(F32)))


def tta_views_walk(c, inp, mut=""):
    a = c.arg
    x = inp["x"].astype(F64)
    v = _mix(x, a("H"), a("W"), a("h"), a("w"), None, mut)
    return v, _mix(np.abs(x), a("H"), a("W"), a("h"), a("w"), None, mut) * 4 * U


# ------------------------------------------------------------------------------------------------ tiled inference
def axis_tiles(n, t, o, mut=""):
    """(origins, cover [tiles, n] bool) of one axis, from the header's formula."""
    s = t - o
    if n <= t:
        orig = [0]
    else:
        cnt = -(-(n - t) // s) + 1
        orig = [i * s for i in range(cnt - 1)] + [(cnt - 1) * s if mut == "last_is_regular" else n - t]
    p = np.arange(n)
    cover = np.array([(p >= y0) & (p < y0 + t) for y0 in orig])
    if mut == "drop_third":
        cover[-1] &= cover.sum(axis=0) < 3
    return orig, cover


def mirror(i, n, mut=""):
    if n == 1:
        return 0
    if mut == "mirror_repeats_edge":
        j = i % (2 * n)
        return j if j < n else 2 * n - 1 - j
    j = i % (2 * (n - 1))
    return j if j < n else 2 * (n - 1) - j


def tile_geometry(c, mut=""):
    a = c.arg
    (th, tw), (oy, ox) = a("tile"), a("overlap")
    return axis_tiles(a("H"), th, oy, mut), axis_tiles(a("W"), tw, ox, mut)


def n_tiles(c):
    (ys, _), (xs, _) = tile_geometry(c)
    return c.arg("B", 2) * len(ys) * len(xs)


def tile_cut_inputs(c):
    a = c.arg
    return dict(x=_ro(_rng(c).standard_normal((a("B", 2), a("Cin"), a("H"), a("W"))).astype(F32)))


def tile_cut_walk(c, inp, mut=""):
    """The tiles [g0, g1) of x, element by element from the header's rule."""
    a, x = c.arg, inp["x"]
    B, Cin, H, W = x.shape
    th, tw = a("tile")
    (ys, _), (xs, _) = tile_geometry(c)
    g0, g1 = a("g0", 0), a("g1", None) or n_tiles(c)
    out = np.empty((g1 - g0, Cin, th, tw), dtype=F32)
    T, nx = len(ys) * len(xs), len(xs)
    for g in range(g0, g1):
        b, q = divmod(g, T)
        iy, ix = divmod(q, nx)
        sy = [mirror(ys[iy] + r, H, mut) if H < th else ys[iy] + r for r in range(th)]
        sx = [mirror(xs[ix] + r, W, mut) if W < tw else xs[ix] + r for r in range(tw)]
        out[g - g0] = x[b][:, sy][:, :, sx]
    return out


def tile_fold_inputs(c):
    a, rng = c.arg, _rng(c)
    G, (th, tw) = n_tiles(c), a("tile")
    inp = {}
    if a("C"):
        inp["z"] = _ro((rng.standard_normal((G, a("C"), th, tw)) * a("gain", 2.0)).astype(F32))
    for m in range(a("n_maps", 0)):
        inp[f"m{m}"] = _ro((rng.random((G, th, tw)) * 2 - 0.5).astype(F32))          # uncertainty-like maps, some values negative
    kind = a("window", "asym")
    if kind == "asym":                             # independent values: no symmetry hides a mirrored or swapped index
        inp["wy"], inp["wx"] = _ro(rng.uniform(0.1, 1.0, th).astype(F32)), _ro(rng.uniform(0.1, 1.0, tw).astype(F32))
    else:
        inp["wy"], inp["wx"] = _ro(TR.window(th, kind).astype(F32)), _ro(TR.window(tw, kind).astype(F32))
    return inp


def source_tile(g, b, T, tpc, mut=""):
    """The tile whose data tile g reads: g, unless locate() takes the chunk from the image's own first tile on."""
    if mut != "locate_per_image" or tpc is None:
        return g
    ch = (b * T) // tpc + (g - b * T) // tpc
    return ch * tpc + min(g - ch * tpc, tpc - 1)


def tile_fold_walk(c, inp, mut=""):
    """dict name -> (float64 value, bound) of probs and the blended maps; the scatter loop visits a pixel's tiles in ascending (iy, ix)."""
    a = c.arg
    B, C, H, W, n_maps = a("B", 2), a("C"), a("H"), a("W"), a("n_maps", 0)
    (ys, cy), (xs, cx) = tile_geometry(c, mut)
    wy, wx = inp["wy"], inp["wx"]
    if mut == "swap_windows":
        assert len(wy) == len(wx)
        wy, wx = wx, wy
    if mut == "mirror_weight_index":
        wy, wx = wy[::-1], wx[::-1]
    w2 = (wy[:, None] * wx[None, :]).astype(F32)                    # rounded on its own
    T, nx = len(ys) * len(xs), len(xs)
    names = (["probs"] if C else []) + [f"map{m}" for m in range(n_maps)]
    src, sb = {}, {}
    if C:
        src["probs"], sb["probs"] = softmax_b(inp["z"])
    for m in range(n_maps):
        src[f"map{m}"] = inp[f"m{m}"].astype(F64)[:, None]
        sb[f"map{m}"] = np.zeros_like(src[f"map{m}"])
    acc = {k: np.zeros((B, src[k].shape[1], H, W)) for k in names}
    bnd = {k: np.zeros((B, src[k].shape[1], H, W)) for k in names}
    ws = np.zeros((B, H, W), dtype=F32)
    cnt = np.zeros((B, H, W))
    for b in range(B):
        for iy, y0 in enumerate(ys):
            py = np.nonzero(cy[iy])[0]
            for ix, x0 in enumerate(xs):
                px = np.nonzero(cx[ix])[0]
                if not len(py) or not len(px):
                    continue
                g = source_tile(b * T + iy * nx + ix, b, T, a("tpc"), mut)
                at, tl = np.ix_(py, px), np.ix_(py - y0, px - x0)
                w = w2[tl]
                ws[b][at] = (ws[b][at] + w).astype(F32)             # the kernel's own order: exact
                cnt[b][at] += 1
                for k in names:
                    acc[k][b][(slice(None),) + at] += w.astype(F64) * src[k][g][(slice(None),) + tl]
                    bnd[k][b][(slice(None),) + at] += w.astype(F64) * sb[k][g][(slice(None),) + tl] + U * np.abs(acc[k][b][(slice(None),) + at])
    den = (cnt if mut == "divide_by_count" else ws.astype(F64))[:, None]
    out = {}
    for k in names:
        v = acc[k] / den
        b_ = bnd[k] / den + 2 * DIV_ULP * U * np.abs(v)
        out[k] = (v, b_) if k == "probs" else (v[:, 0], b_[:, 0])
    return out


# ------------------------------------------------------------------------------------------------ curves
def crafted_regions(c, t):
    """(labels int32 [B,H,W], count int32 [B], table int64 [B,Mg,9]): horizontal bands as regions, with every oddity of the contract --
    labels 0, negative, above count[b] but <= max_regions, above max_regions; count[b] of 0, negative and above max_regions (B = 4);
    rows of a class outside the scored ones and rows with area <= 0 between the counted ones."""
    a, rng = c.arg, _rng(c, 7)
    B, C, H, W, Mg = a("B", 2), a("C"), a("H"), a("W"), a("max_regions", 6)
    n, scored = Mg - 1, a("classes")
    labels = np.zeros((B, H, W), dtype=np.int32)
    table = np.zeros((B, Mg, 9), dtype=np.int64)
    band = max(H // (n + 1), 1)
    for b in range(B):
        for r in range(Mg):
            cls = scored[(r + b) % len(scored)] if r % 4 != 1 else C + 1            # every fourth row: a class that is not scored
            if r < n and r * band < H:
                x0 = (3 * r + b) % max(W // 2, 1)
                labels[b, r * band:(r + 1) * band, x0:x0 + max(W // 2, 1)] = r + 1
            area = int((labels[b] == r + 1).sum())
            table[b, r] = (cls, area if r % 5 != 2 else (0, -3)[b % 2], 0, 0, 0, 0, 0, 0, 0)
            if area == 0 and r % 5 != 2:
                table[b, r, 1] = 7                                                   # a counted row without pixels
        free = np.argwhere(labels[b] == 0)
        pick = free[rng.permutation(len(free))[:8]] if len(free) >= 8 else free
        for (y, x), v in zip(pick, (-2, Mg, Mg + 5, 2 ** 30, -2 ** 31, Mg, Mg + 1, -1)):
            labels[b, y, x] = v
    count = np.array([n, 0, -1, Mg + 3][:B] if B == 4 else [n] * B, dtype=np.int32)
    return _ro(labels), _ro(count), _ro(table)


def _key_scores(c, shape, V):
    """Probabilities whose bins form exactly `keys` distinct keys among the 64 lanes of a wave: pixel i of a lane's V takes bin
    (i // V) % keys (spread over the bins), in [lo, hi)."""
    a = c.arg
    B, C, H, W = shape
    keys, bins, lo, hi = a("keys"), a("bins", 64), a("lo", 0.0), a("hi", 1.0)
    i = np.arange(H * W)
    b = ((i // V) % keys) * (bins // keys)
    s = (lo + (b + 0.5) / bins * (hi - lo)).astype(F32)
    assert np.array_equal(CR.bins_of(s, bins, lo, hi), b)
    return np.broadcast_to(s.reshape(1, 1, H, W), shape)


def score_inputs(c):
    a, rng = c.arg, _rng(c)
    B, C, H, W, tdt = a("B", 2), a("C"), a("H"), a("W"), a("tdt", I64)
    shape, p = (B, C, H, W), c.pattern
    nlab = max(C, 2)
    t = rng.integers(0, nlab, (B, H, W)).astype(np.int64)
    if p == "logits":
        S = CR.logits((B, H, W), C, (a("bins", 64),), seed=c.seed % 1000)
    elif p == "logit_ties":                        # the two largest logits differ, their fp32 probabilities do not
        S = (rng.standard_normal(shape) * 2 - 12).astype(F32)
        hi_c = rng.integers(0, C, (B, H, W))
        lo_c = (hi_c + 1 + rng.integers(0, C - 1, (B, H, W))) % C
        np.put_along_axis(S, hi_c[:, None], F32(1e-9), axis=1)
        np.put_along_axis(S, lo_c[:, None], F32(0), axis=1)
        t = np.where(rng.random((B, H, W)) < 0.5, hi_c, lo_c).astype(np.int64)
    elif p == "keys":
        S = _key_scores(c, shape, c.V)
        t = np.full((B, H, W), nlab - 1, dtype=np.int64)
    elif p in ("uniform", "ignored"):
        S = rng.random(shape, dtype=F32)
    elif p == "nans":
        S = rng.random(shape, dtype=F32)
        S[rng.random(shape) < 0.06] = np.nan
        S[:, :, 0, 0] = np.nan                      # every row of every image sees one
        S[:, 1:, -1, -1] = F32(0.25)                # the last pixel of every image: a NaN for the top row (C = 1: for every row),
        S[:, 0, -1, -1] = np.nan                    # a counted score for the rows of the classes above 0
    elif p == "edges":
        e = CR.edge_values((15, a("bins", 64)))
        S = e[rng.integers(0, len(e), shape)]
        S.reshape(-1)[:min(len(e), S.size)] = e[:S.size]
    else:
        raise KeyError(p)
    if p == "ignored" or a("ignored", 0):
        m = rng.random((B, H, W))
        t = np.where(m < 0.05, -1, np.where(m < 0.10, 255, np.where(m < 0.15, nlab, t)))
    if tdt == U8:
        t = np.where(t < 0, 255, t)                # what a byte can say
    inp = dict(scores=_ro(np.asarray(S, dtype=F32)), target=_ro(t.astype(NP_OF[tdt])))
    if a("regions"):
        inp["rl"], inp["rcount"], inp["rtable"] = crafted_regions(c, t)
    return inp


def fma_sensitive(bins, lo, hi):
    """Scores beside the bin edges that (s - lo) * inv rounded twice and rounded once put into different bins."""
    inv = F32(F32(bins) / F32(F32(hi) - F32(lo)))
    out = []
    for k in range(1, bins):
        v = F32(F64(lo) + k / F64(inv))
        for _ in range(4):
            v = np.nextafter(v, F32(-np.inf))
        for _ in range(9):
            if _bins_mut([v], bins, lo, hi, "")[0] != _bins_mut([v], bins, lo, hi, "bin_one_fma")[0]:
                out.append(v)
            v = np.nextafter(v, F32(np.inf))
    return np.array(out, dtype=F32)


def plane_inputs(c):
    a, rng = c.arg, _rng(c)
    B, H, W = a("B", 2), a("H"), a("W")
    lo, hi = a("lo", 0.0), a("hi", 1.0)
    s = (lo - 1 + rng.random((B, H, W)) * (hi - lo + 2)).astype(F32)             # beyond both bounds
    s.reshape(-1)[:6] = (np.inf, -np.inf, np.nan, lo, hi, np.nextafter(F32(hi), F32(lo)))
    s[rng.random((B, H, W)) < 0.03] = np.nan
    pred, target = rng.integers(0, 3, (B, H, W)), rng.integers(0, 3, (B, H, W))
    target = np.where(rng.random((B, H, W)) < 0.1, -1, target)
    pdt, tdt = a("pdt", I64), a("tdt", I64)
    e = fma_sensitive(a("bins", 64), lo, hi)[:40]                                # where one fma would change the bin
    s.reshape(-1)[8:8 + len(e)] = e
    target.reshape(-1)[8:8 + len(e)] = 0
    if tdt == U8:
        target = np.where(target < 0, 255, target)
    return dict(scores=_ro(s), pred=_ro(pred.astype(NP_OF[pdt])), target=_ro(target.astype(NP_OF[tdt])))


def _bins_mut(s, bins, lo, hi, mut):
    s = np.asarray(s, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        inv = F32(F32(bins) / F32(F32(hi) - F32(lo)))
        if mut == "bin_one_fma":                   # s * inv - lo * inv, rounded once
            x = (s.astype(F64) * F64(inv) - F64(F32(lo)) * F64(inv)).astype(F32)
        else:
            x = ((s - F32(lo)).astype(F32) * inv).astype(F32)
        t = np.rint(x) if mut == "bin_rint" else np.floor(x)
        if mut == "clamp_after_int":               # the conversion saturates at the int range first; out-of-range floats wrap to INT_MIN
            t = np.where(np.abs(t) >= 2.0 ** 31, -2.0 ** 31, t)
    return np.clip(t, 0, bins - 1).astype(np.int64)


def score_walk(c, inp, mut=""):
    """A second restatement of uaps_score_curves (and of uaps_plane_curves) with the mutants as switches."""
    a = c.arg
    bins, lo, hi, q = a("bins", 64), a("lo", 0.0), a("hi", 1.0), a("qsum", 0)
    S = inp["scores"]
    t = inp["target"].astype(np.int64)
    if c.entry == "plane":
        rows = [(S, inp["pred"].astype(np.int64) == t, t >= 0, np.isnan(S))]
        C, classes = 0, ()
    else:
        C, classes, from_logits = a("C"), list(a("classes", ())), a("from_logits", 0)
        if mut == "u8_255_counted" and a("tdt", I64) == U8:
            t = np.where(t == 255, C - 1, t)
        rows = CR.rows_of(S, t, classes, a("top", 1), from_logits)
        if a("top", 1) and C >= 2 and mut == "argmax_of_probabilities":
            P = CR.probabilities(S, from_logits)
            s_, ev, ok, bad = rows[-1]
            rows[-1] = (s_, P.argmax(axis=1) == t, ok, bad)
        if a("top", 1) and C == 1 and mut == "no_max_at_c1":
            s_, ev, ok, bad = rows[-1]
            rows[-1] = (CR.probabilities(S, from_logits)[:, 0], ev, ok, bad)
    B, Rn = S.shape[0], len(rows)
    hist = np.zeros((B, Rn, 2, bins), dtype=np.int64)
    qsum = np.zeros((B, Rn, 2, bins), dtype=np.int64) if q else None
    nan = np.zeros((B, Rn), dtype=np.int64)
    upg = units_per_group(Rn, bins, q)
    for b in range(B):
        for r, (s, ev, ok, bad) in enumerate(rows):
            split = (2 * r) // upg != (2 * r + 1) // upg
            nan[b, r] = np.count_nonzero(ok[b] & bad[b]) * (2 if split and mut == "nan_by_both_groups" else 1)
            for e in (0, 1):
                sel = ok[b] & ~bad[b] & (ev[b] == bool(e))
                idx = _bins_mut(s[b][sel], bins, lo, hi, mut)
                hist[b, r, e] = np.bincount(idx, minlength=bins)
                if q:
                    np.add.at(qsum[b, r, e], idx, IR.fixed_point(s[b][sel]))
    out = dict(hist=hist, nan=nan)
    if q:
        out["qsum"] = qsum
    if c.entry == "score" and a("regions"):
        labels, count, table = inp["rl"], inp["rcount"], inp["rtable"]
        Mg = table.shape[1]
        P = CR.probabilities(S, a("from_logits", 0))
        pro = np.zeros((B, len(classes), bins), dtype=F64)
        n_reg = np.zeros((B, len(classes)), dtype=np.int64)
        times = groups(Rn, bins, q) if mut == "region_hist_by_every_group" else 1
        for b in range(B):
            for r in range(max(min(int(count[b]), Mg), 0)):
                cls, area = int(table[b, r, 0]), int(table[b, r, 1])
                if cls not in classes or area <= 0:
                    continue
                s = P[b, 0 if C == 1 else cls][labels[b] == r + 1]
                h = np.bincount(_bins_mut(s[~np.isnan(s)], bins, lo, hi, mut), minlength=bins) * times
                run = np.cumsum(h) if mut == "prefix_sums" else np.cumsum(h[::-1])[::-1]
                for k, ck in enumerate(classes):
                    if ck == cls:
                        n_reg[b, k] += 1
                        pro[b, k] += run.astype(F64) / F64(area)
        out.update(pro_sum=pro, n_regions=n_reg)
    return out


def score_reference(c, inp):
    """tests/curves_ref.py as it stands."""
    a = c.arg
    if c.entry == "plane":
        ref = CR.plane(inp["scores"], inp["pred"], inp["target"], a("bins", 64), a("lo", 0.0), a("hi", 1.0), bool(a("qsum", 0)))
    else:
        reg = (inp["rl"], inp["rcount"], inp["rtable"]) if a("regions") else None
        ref = CR.curves(inp["scores"], inp["target"], list(a("classes", ())), a("bins", 64), bool(a("top", 1)), bool(a("from_logits", 0)), reg,
                        bool(a("qsum", 0)), a("lo", 0.0), a("hi", 1.0))
    return {k: ref[k] for k in ("hist", "qsum", "nan", "pro_sum", "n_regions") if ref[k] is not None}


# ------------------------------------------------------------------------------------------------ one door for every entry point
INPUTS = dict(tta_fold=tta_fold_inputs, tta_views=tta_views_inputs, tile_cut=tile_cut_inputs, tile_fold=tile_fold_inputs, score=score_inputs,
              plane=plane_inputs)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The host arrays of a case: computed once, shared, read-only."""
    return INPUTS[c.entry](c)


def walk(c, mut=""):
    """The reference walk of a case, with a mutant switched on or none: exact outputs as arrays, float outputs as (value, bound)."""
    inp = inputs(c)
    if c.entry == "tta_fold":
        return dict(probs=tta_fold_walk(c, inp, mut))
    if c.entry == "tta_views":
        return dict(out=tta_views_walk(c, inp, mut))
    if c.entry == "tile_cut":
        return dict(out=tile_cut_walk(c, inp, mut))
    if c.entry == "tile_fold":
        return tile_fold_walk(c, inp, mut)
    return score_walk(c, inp, mut)


@functools.lru_cache(maxsize=None)
def reference(c):
    """What the GPU test compares with: computed once, shared, never written."""
    if c.entry in ("score", "plane"):
        return score_reference(c, inputs(c))
    return walk(c)


def bars(c):
    """name -> the per-element bar of every float64-compared output of a case."""
    return {k: _bar(v[1]) for k, v in reference(c).items() if isinstance(v, tuple)}


def margin(c):
    """Twice the largest bar of the class map: above it the arg-max must agree with float64."""
    return 2 * float(bars(c)["probs"].max())


def excluded(c):
    """The share of a case's pixels whose float64 top-2 margin is at or under margin(c)."""
    v = np.sort(reference(c)["probs"][0], axis=1)
    return float(((v[:, -1] - v[:, -2]) <= margin(c)).mean())


def as_got(c, w):
    """What a device that computed `w` (a walk) would hand back: fp32 values, the mask and conf derived from them, the views' mirror."""
    got = {}
    for k, v in w.items():
        got[k] = v[0].astype(F32) if isinstance(v, tuple) else v
    if c.entry == "tta_views":
        if c.arg("flip", 1):
            got["out"] = np.concatenate([got["out"], got["out"][..., ::-1]])
        elif c.arg("buf2"):
            got["out"] = np.concatenate([got["out"], np.full_like(got["out"], np.frombuffer(b"\xee" * 4, dtype=F32)[0])])
    if "probs" in got and c.entry in ("tta_fold", "tile_fold"):
        p = got["probs"]
        got["mask"] = p.argmax(axis=1).astype(np.int64)
        got["conf"] = p.max(axis=1) / F32(views(c)) if c.entry == "tta_fold" else p.max(axis=1)
        got = {k: v for k, v in got.items() if k in c.outs}
    return got


def views(c):
    return len(c.arg("sizes")) * (2 if c.arg("flip", 1) else 1)


def compare(c, got, own_probs=None):
    """(failed checks, name -> largest |got - reference| / bar) of one launch's outputs.  own_probs: the class map a launch of the same
    data with every output gave, for a case that asks for no probs itself (the mask and conf are functions of it)."""
    ref, bad, ratios = reference(c), [], {}
    want = set(c.outs) if c.outs else set(ref)
    if set(got) != want:
        return [f"outputs {sorted(got)} for {sorted(want)}"], ratios
    for k, r in ref.items():
        if k not in got:
            continue
        g = got[k]
        if isinstance(r, tuple):
            v, bar = r[0], _bar(r[1])
            if c.entry == "tta_views":
                B = v.shape[0]
                if c.arg("flip", 1):
                    if g.shape[0] != 2 * B or g[B:].tobytes() != np.ascontiguousarray(g[:B][..., ::-1]).tobytes():
                        bad.append("the flipped half is not the plain half mirrored")
                elif c.arg("buf2") and (g.shape[0] != 2 * B or set(g[B:].tobytes()) != {0xEE}):
                    bad.append("flip == 0 wrote images B .. 2B-1")
                g = g[:B]
            if g.dtype != F32 or g.shape != v.shape:
                bad.append(f"{k}: {g.dtype} {g.shape}")
                continue
            err = np.abs(g.astype(F64) - v)
            ratios[k] = float((err / bar).max())
            if not (err <= bar).all():                                       # (a NaN fails)
                i = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err / bar)), err.shape)
                bad.append(f"{k}{list(i)}: {g[i]!r} for {v[i]!r}, {err[i] / bar[i]:.2f} of the bar {bar[i]:.3e}")
        else:
            r = np.asarray(r)
            if g.dtype != r.dtype or g.shape != r.shape:
                bad.append(f"{k}: {g.dtype} {g.shape} for {r.dtype} {r.shape}")
            elif k == "qsum" and c.arg("from_logits"):                         # sums of the DEVICE's fp32 probabilities: Q_LOGITS a pixel
                over = np.abs(g - r) > ref["hist"] * Q_LOGITS
                if over.any():
                    i = tuple(np.argwhere(over)[0])
                    bad.append(f"qsum{list(i)}: {g[i]} for {r[i]} over {ref['hist'][i]} pixels")
            elif g.tobytes() != r.tobytes():
                i = tuple(np.argwhere(g != r)[0]) if (g != r).any() else ()
                bad.append(f"{k}{list(i)}: {g[i] if i else g!r} for {r[i] if i else r!r}")
    if c.entry in ("tta_fold", "tile_fold") and c.arg("C"):
        p = got.get("probs", own_probs)
        if p is None:
            return bad + ["no class map to derive the mask from"], ratios
        am = p.argmax(axis=1).astype(np.int64)                                # numpy: the lowest index among equal values
        if "mask" in got:
            if got["mask"].dtype != np.int64 or not np.array_equal(got["mask"], am):
                bad.append("mask is not the lowest-index arg-max of probs")
            v64 = ref["probs"][0]
            if c.pattern == "ties":
                if not (got["mask"] == 1).all():
                    bad.append("bit-identical classes 1 and 3: the mask must name 1")
            else:
                top2 = np.sort(v64, axis=1)
                clear = (top2[:, -1] - top2[:, -2]) > margin(c)
                if not np.array_equal(got["mask"][clear], v64.argmax(axis=1)[clear]):
                    bad.append("mask differs from the float64 arg-max above the margin")
        if "conf" in got:
            cf = p.max(axis=1) / F32(views(c)) if c.entry == "tta_fold" else p.max(axis=1)
            if got["conf"].dtype != F32 or got["conf"].tobytes() != cf.astype(F32).tobytes():
                bad.append("conf is not the picked value" + (" / views" if c.entry == "tta_fold" else ""))
    return bad, ratios


# ================================================================================================ the table
# ---- uaps_tta_fold: output 8 x 12, three scales, flip, B = 2 unless a case says otherwise
SIZES = ((4, 6), (8, 12), (12, 18))
TF = dict(H=8, W=12, sizes=SIZES)
for C_ in range(2, 9):
    add(f"tta-c{C_}-v4", "tta_fold", C=C_, forms=(f"tta-C{C_}-V4",), **TF)
    add(f"tta-c{C_}-v1", "tta_fold", C=C_, offs=dict(probs=1, z0=1, z1=3), forms=(f"tta-C{C_}-V1",), **TF)
add("tta-v1-w6", "tta_fold", C=4, H=8, W=6, sizes=SIZES, forms=("tta-V1-by-W",))
add("tta-v1-probs", "tta_fold", C=4, offs=dict(probs=1), forms=("tta-V1-by-probs",), **TF)
add("tta-v1-mask", "tta_fold", C=4, offs=dict(mask=1), forms=("tta-V1-by-mask",), **TF)
add("tta-v1-conf", "tta_fold", C=4, offs=dict(conf=1), forms=("tta-V1-by-conf",), **TF)
add("tta-only-mask", "tta_fold", C=4, outs=("mask",), forms=("tta-V4-null-outputs",), **TF)
add("tta-only-conf", "tta_fold", C=4, outs=("conf",), forms=("tta-V4-null-outputs",), **TF)
add("tta-only-probs", "tta_fold", C=4, outs=("probs",), forms=("tta-V4-null-outputs",), **TF)
add("tta-s1", "tta_fold", C=3, H=8, W=12, sizes=((5, 7),), forms=("tta-S1",))
add("tta-s8", "tta_fold", C=3, H=8, W=12, sizes=((4, 6), (8, 12), (12, 18), (3, 5), (16, 24), (7, 11), (9, 13), (2, 2)), forms=("tta-S8",))
add("tta-thin-scales", "tta_fold", C=4, H=8, W=12, sizes=((1, 6), (4, 1), (8, 12), (1, 1)), forms=("tta-h1", "tta-w1", "tta-identity"))
add("tta-out-h1", "tta_fold", C=4, H=1, W=12, sizes=SIZES, forms=("tta-H1",))
add("tta-out-w1", "tta_fold", C=4, H=8, W=1, sizes=SIZES, forms=("tta-W1",))
add("tta-up-only", "tta_fold", C=5, H=8, W=12, sizes=((3, 5), (4, 6)), forms=("tta-upscale-only",))
add("tta-down-only", "tta_fold", C=5, H=8, W=12, sizes=((16, 24), (13, 17)), forms=("tta-downscale-only",))
add("tta-noflip", "tta_fold", C=4, flip=0, forms=("tta-flip0",), **TF)
add("tta-b1", "tta_fold", C=6, B=1, offs=dict(mask=1, conf=3, probs=2), forms=("tta-B1",), **TF)
add("tta-ties", "tta_fold", "ties", C=5, forms=("tta-ties",), **TF)
add("tta-saturated", "tta_fold", C=4, gain=60.0, H=16, W=24, sizes=((8, 12), (16, 24), (24, 36)), forms=("tta-saturated",))

# ---- uaps_tta_views
for Cin_ in (1, 3):
    add(f"views-down-cin{Cin_}", "tta_views", Cin=Cin_, H=16, W=24, h=8, w=12, offs=dict(x=1, out=3), forms=("views-down", f"views-cin{Cin_}"))
add("views-up", "tta_views", Cin=3, H=5, W=7, h=9, w=13, offs=dict(x=3, out=1), forms=("views-up",))
add("views-identity", "tta_views", Cin=1, H=7, W=9, h=7, w=9, offs=dict(out=1), forms=("views-identity",))
add("views-h1", "tta_views", Cin=3, H=6, W=9, h=1, w=5, offs=dict(x=1), forms=("views-h1",))
add("views-w1", "tta_views", Cin=1, H=6, W=9, h=4, w=1, offs=dict(x=1, out=1), forms=("views-w1",))
add("views-noflip", "tta_views", Cin=3, H=6, W=9, h=8, w=5, flip=0, buf2=1, offs=dict(x=1, out=1), forms=("views-flip0",))

# ---- uaps_tile_cut
add("cut-h1", "tile_cut", Cin=1, H=1, W=20, tile=(16, 16), overlap=(4, 4), offs=dict(x=1, out=1), forms=("cut-H1",))
add("cut-h5", "tile_cut", Cin=3, H=5, W=20, tile=(16, 16), overlap=(4, 4), offs=dict(x=1, out=3), forms=("cut-mirror-periods",))
add("cut-w1", "tile_cut", Cin=1, H=20, W=1, tile=(16, 16), overlap=(4, 4), offs=dict(out=1), forms=("cut-W1",))
add("cut-w5", "tile_cut", Cin=3, H=20, W=5, tile=(16, 16), overlap=(4, 4), offs=dict(x=3), forms=("cut-mirror-periods",))
add("cut-equal", "tile_cut", Cin=3, H=16, W=16, tile=(16, 16), overlap=(4, 4), offs=dict(x=1, out=1), forms=("cut-tile-is-image",))
add("cut-clamp", "tile_cut", Cin=3, H=41, W=50, tile=(16, 16), overlap=(4, 4), offs=dict(x=1, out=1), forms=("cut-clamped-last",))
add("cut-window", "tile_cut", Cin=1, H=41, W=50, tile=(16, 16), overlap=(4, 4), g0=13, g1=19, offs=dict(x=3, out=1), forms=("cut-window",))

# ---- uaps_tile_fold: 12 x 20 images, 8 x 8 tiles, overlap 3, 5 tiles a chunk (16 tiles: 5, 5, 5, 1) unless a case says otherwise
FD = dict(H=12, W=20, tile=(8, 8), overlap=(3, 3), tpc=5)
for n_ in (1, 2):
    add(f"fold-maps{n_}-v4", "tile_fold", C=0, n_maps=n_, forms=(f"fold-C0-maps{n_}-V4",), **FD)
    add(f"fold-maps{n_}-v1", "tile_fold", C=0, n_maps=n_, offs=dict(map0=1, map1=1), forms=(f"fold-C0-maps{n_}-V1",), **FD)
for C_ in range(2, 9):
    add(f"fold-c{C_}-v4", "tile_fold", C=C_, forms=(f"fold-C{C_}-V4",), **FD)
    add(f"fold-c{C_}-v1", "tile_fold", C=C_, offs=dict(probs=1, z=1, wy=1, wx=3), forms=(f"fold-C{C_}-V1",), **FD)
add("fold-c4-maps2", "tile_fold", C=4, n_maps=2, forms=("fold-C4-maps2",), **FD)
add("fold-v1-w18", "tile_fold", C=4, H=12, W=18, tile=(8, 8), overlap=(3, 3), tpc=5, forms=("fold-V1-by-W",))
add("fold-v1-probs", "tile_fold", C=4, n_maps=1, offs=dict(probs=1), forms=("fold-V1-by-probs",), **FD)
add("fold-v1-mask", "tile_fold", C=4, n_maps=1, offs=dict(mask=1), forms=("fold-V1-by-mask",), **FD)
add("fold-v1-conf", "tile_fold", C=4, n_maps=1, offs=dict(conf=1), forms=("fold-V1-by-conf",), **FD)
add("fold-v1-map1", "tile_fold", C=4, n_maps=2, offs=dict(map1=2), forms=("fold-V1-by-map",), **FD)
add("fold-overlap0", "tile_fold", C=3, H=16, W=24, tile=(8, 8), overlap=(0, 0), tpc=7, forms=("fold-overlap0",))
add("fold-odd-tile", "tile_fold", C=3, H=16, W=20, tile=(7, 7), overlap=(3, 3), tpc=7, forms=("fold-half-overlap-odd",))
add("fold-nine", "tile_fold", C=4, H=17, W=20, tile=(8, 8), overlap=(4, 3), tpc=9, forms=("fold-nine-tiles",))
add("fold-rect-tile", "tile_fold", C=3, H=14, W=28, tile=(8, 12), overlap=(2, 5), tpc=4, forms=("fold-th-ne-tw",))
add("fold-one-chunk", "tile_fold", C=4, H=12, W=20, tile=(8, 8), overlap=(3, 3), tpc=16, forms=("fold-one-chunk",))
add("fold-32-chunks", "tile_fold", C=2, H=16, W=16, tile=(4, 4), overlap=(0, 0), tpc=1, forms=("fold-32-chunks",))
add("fold-small-image", "tile_fold", C=3, H=5, W=4, tile=(8, 8), overlap=(3, 3), tpc=2, forms=("fold-image-below-tile",))
for kind_ in ("uniform", "triangle", "gauss"):
    add(f"fold-{kind_}", "tile_fold", C=4, window=kind_, forms=(f"fold-window-{kind_}",), **FD)
add("fold-saturated", "tile_fold", C=4, gain=60.0, forms=("fold-saturated",), **FD)

# ---- uaps_score_curves
SC = dict(H=10, W=12)                              # 120 pixels: two waves of V = 1, half a wave of V = 4
for C_ in range(1, 9):
    cls_ = (1,) if C_ == 1 else tuple(range(1, C_))
    for q_ in (0, 1):
        add(f"score-c{C_}-v4-q{q_}", "score", "uniform", C=C_, classes=cls_, qsum=q_, ignored=1, forms=(f"score-C{C_}-V4-q{q_}",), **SC)
        add(f"score-c{C_}-v1-q{q_}", "score", "uniform", C=C_, classes=cls_, qsum=q_, ignored=1, offs=dict(scores=1 + q_, hist=1),
            forms=(f"score-C{C_}-V1-q{q_}",), **SC)
for C_ in (1, 3, 8):
    for d_ in (U8, I32, I64):
        cls_ = (1,) if C_ == 1 else (C_ - 1, 0)
        add(f"score-c{C_}-d{d_}-v4", "score", "ignored", C=C_, classes=cls_, tdt=d_, qsum=1, forms=(f"score-dtype{d_}-V4",), **SC)
        add(f"score-c{C_}-d{d_}-v1", "score", "ignored", C=C_, classes=cls_, tdt=d_, offs=dict(target={U8: 3, I32: 1, I64: 1}[d_]),
            forms=(f"score-dtype{d_}-V1",), **SC)
add("score-v1-hw", "score", "uniform", C=4, classes=(1, 2, 3), H=9, W=13, forms=("score-V1-by-HW",))
add("score-v1-scores", "score", "uniform", C=4, classes=(1, 2, 3), offs=dict(scores=3), forms=("score-V1-by-scores",), **SC)
add("score-v1-target-u8", "score", "ignored", C=4, classes=(1, 2, 3), tdt=U8, offs=dict(target=1), forms=("score-V1-by-target",), **SC)
add("score-v1-target-i64", "score", "ignored", C=4, classes=(1, 2, 3), tdt=I64, offs=dict(target=1), forms=("score-V1-by-target",), **SC)
add("score-v1-rl", "score", "uniform", C=4, classes=(1, 2, 3), regions=1, offs=dict(rl=1), forms=("score-V1-by-region-labels",), **SC)
for hw_, B_ in ((512, 2), (513, 3), (1024, 2), (1025, 3)):
    add(f"score-span-v1-{hw_}", "score", "nans", C=2, classes=(1,), B=B_, H=1, W=hw_, offs=dict(scores=1), qsum=1, forms=("score-span-V1",))
for hw_, B_ in ((2048, 2), (2052, 3), (4096, 2), (4100, 3)):
    add(f"score-span-v4-{hw_}", "score", "nans", C=2, classes=(1,), B=B_, H=4, W=hw_ // 4, qsum=1, forms=("score-span-V4",))
KY = dict(C=2, classes=(1,), H=16, W=64, bins=64)  # 1024 pixels: four waves of V = 4
for k_ in (1, 4, 5, 64):
    add(f"score-keys{k_}-v4", "score", "keys", keys=k_, forms=(f"score-keys{k_}",), **KY)
    add(f"score-keys{k_}-v1", "score", "keys", keys=k_, offs=dict(scores=1), forms=(f"score-keys{k_}",), **KY)
for k_, f_ in ((64, "single-lane"), (1, "several-lanes")):
    add(f"score-q-{f_}-v4", "score", "keys", keys=k_, qsum=1, lo=-1.0, hi=1.0, forms=(f"score-qsum-{f_}",), **KY)
    add(f"score-q-{f_}-v1", "score", "keys", keys=k_, qsum=1, lo=-1.0, hi=1.0, offs=dict(target=1), forms=(f"score-qsum-{f_}",), **KY)
add("score-upg3", "score", "nans", C=3, classes=(2, 0), bins=1367, qsum=1, forms=("score-odd-upg",), **SC)
add("score-upg1", "score", "nans", C=3, classes=(2, 0), bins=4096, qsum=1, offs=dict(scores=1), forms=("score-odd-upg",), **SC)
for C_ in (1, 2, 5):
    add(f"score-logits-c{C_}", "score", "logits", C=C_, classes=(1,), from_logits=1, bins=15, qsum=1, ignored=1, forms=("score-from-logits",), **SC)
add("score-logit-ties", "score", "logit_ties", C=4, classes=(0, 2), from_logits=1, bins=15, forms=("score-logit-ties",), **SC)
add("score-top-alone", "score", "uniform", C=4, classes=(), top=1, forms=("score-top-alone",), **SC)
add("score-classes-alone", "score", "uniform", C=4, classes=(0, 1, 2, 3), top=0, forms=("score-classes-alone",), **SC)
add("score-partial", "score", "ignored", C=4, classes=(3, 1), top=1, offs=dict(nan=1, hist=1, qsum=1), qsum=1, forms=("score-unsorted-classes",), **SC)
for b_ in (2, 15, 255, 256, 257, 1024, 4096):
    add(f"score-bins{b_}", "score", "edges", C=2, classes=(0, 1), bins=b_, qsum=b_ % 2, forms=(f"score-bins{b_}",), **SC)
for C_ in (1, 4, 8):
    cls_ = (1,) if C_ == 1 else (C_ - 1, 1, 0)
    add(f"score-regions-c{C_}-v4", "score", "nans", C=C_, classes=cls_, regions=1, B=4, H=14, W=12, bins=15, forms=(f"regions-C{C_}", "regions-counts"))
    add(f"score-regions-c{C_}-v1", "score", "nans", C=C_, classes=cls_, regions=1, B=4, H=14, W=12, bins=15, offs=dict(rl=1, rcount=1, rtable=1, pro_sum=1, n_regions=1),
        forms=(f"regions-C{C_}", "regions-counts"))
add("score-regions-groups", "score", "uniform", C=4, classes=(1, 2, 3), regions=1, bins=4096, qsum=1, H=14, W=12, forms=("regions-many-groups",))
for b_ in (2, 255, 257, 1000, 4096):
    add(f"score-pro-bins{b_}", "score", "uniform", C=3, classes=(2, 1), regions=1, bins=b_, max_regions=9, H=14, W=12, top=0, forms=(f"pro-bins{b_}",))

# ---- uaps_plane_curves
PL = dict(H=10, W=12, bins=15, lo=-2.5, hi=7.0)
for p_ in (U8, I32, I64):
    for t_ in (U8, I32, I64):
        add(f"plane-d{p_}-d{t_}-v4", "plane", pdt=p_, tdt=t_, qsum=int(p_ == t_), forms=("plane-dtypes-V4", f"plane-q{int(p_ == t_)}-V4"), **PL)
        add(f"plane-d{p_}-d{t_}-v1", "plane", pdt=p_, tdt=t_, qsum=int(p_ != t_), offs=dict(pred={U8: 1, I32: 1, I64: 1}[p_]),
            forms=("plane-dtypes-V1", f"plane-q{int(p_ != t_)}-V1"), **PL)

BY_ID = {c.id: c for c in CASES}
FORMS = tuple(dict.fromkeys(f for c in CASES for f in c.forms))

# mutant -> (what it is, the entry points whose walk has the switch)
MUTANTS = {
    "no_unflip": ("the flipped columns not mirrored back", ("tta_fold",)),
    "flip_same_image": ("the flipped image read at b instead of B + b", ("tta_fold",)),
    "i1_is_i0": ("i1 = i0", ("tta_fold", "tta_views")),
    "ratio_inverse": ("the ratio formed as out / in", ("tta_fold", "tta_views")),
    "l1_from_i1": ("l1 formed against i1", ("tta_fold", "tta_views")),
    "last_is_regular": ("the last tile's origin taken as i * s", ("tile_fold",)),
    "drop_third": ("the third candidate tile dropped", ("tile_fold",)),
    "swap_windows": ("wy and wx swapped", ("tile_fold",)),
    "mirror_weight_index": ("the weight index mirrored", ("tile_fold",)),
    "mirror_repeats_edge": ("the mirror repeating the edge", ("tile_cut",)),
    "divide_by_count": ("division by the tile count instead of the weight sum", ("tile_fold",)),
    "locate_per_image": ("locate() with the wrong chunk at an image boundary", ("tile_fold",)),
    "bin_rint": ("rint instead of floor", ("score", "plane")),
    "bin_one_fma": ("the bin rule as one fma", ("score", "plane")),
    "clamp_after_int": ("the clamp applied after the int conversion", ("score", "plane")),
    "nan_by_both_groups": ("a NaN counted by both groups of a split row", ("score",)),
    "argmax_of_probabilities": ("the top row's event from the arg-max of the probabilities where they tie and the logits do not", ("score",)),
    "u8_255_counted": ("255 not ignored for uint8 targets", ("score",)),
    "region_hist_by_every_group": ("region_hist filled by every group", ("score",)),
    "prefix_sums": ("prefix sums instead of suffix sums", ("score",)),
    "no_max_at_c1": ("max(p, 1 - p) dropped at C = 1", ("score",)),
}

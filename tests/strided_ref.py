"""The kernels of uaps_amd/csrc/conv_strided.hip -- the general strided convolutions (forward, input gradient, weight gradient, the stem's
own weight gradient, the weight packing), the 3x3 / 2 / 1 max-pool, the 1x1 / 2 sampling and the four-phase rearrangement: references
in plain numpy, the host dispatch restated, the comparison code and one case per kernel form and edge (tests/test_strided_ref.py,
tests/test_gpu_strided_forms.py).

References.  Loops over the taps and einsum over explicitly padded float64 arrays, no torch.  With integer-valued inputs float64 is exact
(every sum stays far below 2^53), so the same code gives the int64 reference of the integer run.

Two kinds of input per convolution case.  Integer-valued (x, w, dy from {-3..3}): every product and every partial sum is an integer below
2^24 (9 K < 2^24 is asserted), so float32 holds each of them exactly in whatever order the kernel and the matrix instruction sum: the
output must EQUAL the reference, every element.  Real-valued (magnitudes uniform in [0.5, 1], random signs), against float64 under the
per-element bar (K + R) 2^-24 sum|terms|: K the contraction length of that output (valid taps x channels, or output pixels), R the
further additions (the three that join the four row-waves, and one per split of the reduction), sum|terms| the float64 sum of the
absolute products.  To first order in 2^-24 that bar holds for any summation order of K + R rounded additions (the second-order term
is K 2^-25 of it: below 1e-4 for the K of the real-valued set).  The real-valued run is there for what small integers cannot see -- an
operand passed through fp16, an xf32-style instruction -- and runs where the largest bar stays below 0.125, half the smallest single
term (0.5 * 0.5): there a dropped term shows too.

Every case names the kernel instantiations it must reach, from the launchers' rules restated in plan_wrw / _kernels; the CPU test checks
that the cases together name exactly the kernels of conv_strided.hip in the built code object.

A mutant is a switch (`mut`) on a reference: the CPU test proves with them that the comparisons of the GPU test bite.
"""
from __future__ import annotations

import math
import zlib
import numpy as np

from bn_ref import rng_for

F32 = np.float32
EPS24 = 2.0 ** -24
SENT = float(F32(-12345.678))           # the sentinel of the GPU test's buffers: no integer, so no integer-valued output can equal it
REAL_BAR_MAX = 0.125                    # half the smallest single term of the real-valued inputs
STEM_N = 160                            # kStemN: the slab columns of the stem form


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def out_size(H: int, ks: int, s: int, p: int) -> int:
    return (H + 2 * p - ks) // s + 1


def check_sconv(B, Cin, Cout, H, W, ks, s, p) -> int:
    """check_sconv of the source: 0, -1 (UAPS_EINVAL) or -2 (UAPS_ERANGE)."""
    if min(B, Cin, Cout, H, W) <= 0:
        return -1
    if ks < 1 or ks > 7 or ks % 2 == 0 or s not in (1, 2) or p < 0 or p > ks // 2 + 3:
        return -2
    if out_size(H, ks, s, p) <= 0 or out_size(W, ks, s, p) <= 0:
        return -1
    return 0


# ---- convolution references ------------------------------------------------------------------------------------------------------
def _padded(x, p):
    x = np.asarray(x, np.float64)
    out = np.zeros(x.shape[:-2] + (x.shape[-2] + 2 * p, x.shape[-1] + 2 * p))
    out[..., p:p + x.shape[-2], p:p + x.shape[-1]] = x
    return out


def _border(a, mut):
    """The border mutants: the first / last column or row of the operand a kernel gathers from treated as padding."""
    a = np.array(a, np.float64)
    if mut == "drop_left":
        a[..., :, 0] = 0
    elif mut == "drop_right":
        a[..., :, -1] = 0
    elif mut == "drop_top":
        a[..., 0, :] = 0
    elif mut == "drop_bottom":
        a[..., -1, :] = 0
    return a


def _fp16(a, mut):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64) if mut == "fp16" else np.asarray(a, np.float64)


def _zero_last_block(out, axis, mut):
    """zero_last_block: the last, partial block of 16 channels never stored."""
    C = out.shape[axis]
    if mut == "zero_last_block" and C % 16:
        sl = [slice(None)] * out.ndim
        sl[axis] = slice(C // 16 * 16, None)
        out[tuple(sl)] = 0
    return out


def conv_fwd(x, w, s, p, mut: str = ""):
    """float64 y [B, Cout, OH, OW] = conv2d(x [B, Cin, H, W], w [Cout, Cin, ks, ks], stride s, padding p)."""
    x, w = _border(_fp16(x, mut), mut), np.asarray(w, np.float64)
    B, Cin, H, W = x.shape
    Cout, _, ks, _ = w.shape
    OH, OW = out_size(H, ks, s, p), out_size(W, ks, s, p)
    xp = _padded(x, p)
    y = np.zeros((B, Cout, OH, OW))
    for ky in range(ks):
        for kx in range(ks):
            y += np.einsum("bchw,oc->bohw", xp[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s], w[:, :, ky, kx])
    return _zero_last_block(y, 1, mut)


def conv_dx(dy, w, s, p, H, W, mut: str = ""):
    """float64 dx [B, Cin, H, W], gathered as the kernel gathers it: input row iy and the columns ix = px + s j of one parity class see
    tap (ky, kx) iff ny = iy + p - ky and nx0 = px + p - kx are multiples of s; they then read dy[ny / s][nx0 / s + j]."""
    dy, w = _border(_fp16(dy, mut), mut), np.asarray(w, np.float64)
    B, Cout, OH, OW = dy.shape
    Cin, ks = w.shape[1], w.shape[2]
    if mut == "flip_taps":
        w = w[:, :, ::-1, ::-1]
    dx = np.zeros((B, Cin, H, W))
    for px in range(s):
        cols = np.arange(px, W, s)
        for kx in range(ks):
            nx0 = px + p - kx
            if nx0 % s:
                continue
            base = nx0 // s + (1 if mut == "neg_div" and nx0 < 0 else 0)
            ox = base + np.arange(len(cols))
            ok = (ox >= 0) & (ox < OW)
            if not ok.any():
                continue
            for iy in range(H):
                for ky in range(ks):
                    ny = iy + p - ky
                    if ny < 0 or ny % s or ny // s >= OH:
                        continue
                    dx[:, :, iy, cols[ok]] += np.einsum("bow,oc->bcw", dy[:, :, ny // s, ox[ok]], w[:, :, ky, kx])
    if mut == "swap_parity" and s == 2:
        n, sw = W // 2, dx.copy()
        sw[..., 0:2 * n:2], sw[..., 1:2 * n:2] = dx[..., 1:2 * n:2], dx[..., 0:2 * n:2]
        dx = sw
    return _zero_last_block(dx, 1, mut)


def conv_dx_adjoint(dy, w, s, p, H, W):
    """The same gradient as the transpose of conv_fwd (scattered into the padded input): what conv_dx is checked against."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    B, Cout, OH, OW = dy.shape
    Cin, ks = w.shape[1], w.shape[2]
    dxp = np.zeros((B, Cin, max(H + 2 * p, s * (OH - 1) + ks), max(W + 2 * p, s * (OW - 1) + ks)))
    for ky in range(ks):
        for kx in range(ks):
            dxp[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] += np.einsum("bohw,oc->bchw", dy, w[:, :, ky, kx])
    return dxp[:, :, p:p + H, p:p + W]


def tile_split(B, OH, OW, nsplit):
    """int [B, OH, OW]: the split that owns each output pixel (tiles of 4 rows x 32 columns in (image, tile row, tile column) order,
    split k owning tiles [ntiles k / nsplit, ntiles (k + 1) / nsplit))."""
    tx, ty = (OW + 31) // 32, (OH + 3) // 4
    ntiles = B * tx * ty
    owner = np.zeros(ntiles, np.int64)
    for k in range(nsplit):
        owner[ntiles * k // nsplit:ntiles * (k + 1) // nsplit] = k
    b, oy, ox = np.meshgrid(np.arange(B), np.arange(OH), np.arange(OW), indexing="ij")
    return owner[(b * ty + oy // 4) * tx + ox // 32]


def conv_dw(dy, x, ks, s, p, mut: str = "", plan: dict = None):
    """float64 dw [Cout, Cin, ks, ks] = sum over (b, oy, ox) of dy[b, co, oy, ox] x[b, ci, oy s + ky - p, ox s + kx - p]."""
    dy, x = _fp16(dy, mut), _border(x, mut)
    B, Cout, OH, OW = dy.shape
    Cin = x.shape[1]
    if mut == "drop_split":                                      # the last split's tiles never reach the sum
        dy = dy * (tile_split(B, OH, OW, plan["nsplit"]) != plan["nsplit"] - 1)[:, None]
    elif mut == "drop_wave":                                     # the wave of tile row 1 left out of the four-wave sum
        dy = dy * (np.arange(OH) % 4 != 1)[None, None, :, None]
    elif mut == "perm_group":                                    # pixels 1 and 2 of every group of four exchanged in dy alone
        perm = np.arange(OW)
        for g in range(0, OW - 3, 4):
            perm[g + 1], perm[g + 2] = g + 2, g + 1
        dy = dy[..., perm]
    xp = _padded(x, p)
    dw = np.zeros((Cout, Cin, ks, ks))
    for ky in range(ks):
        for kx in range(ks):
            dw[:, :, ky, kx] = np.einsum("bohw,bchw->oc", dy, xp[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s])
    if mut == "stem_ncob":                                       # the stem's count of 64-channel blocks taken for 16-channel blocks
        dw[16 * ((Cout + 63) // 64):] = 0
    elif mut == "leak_cols":                                     # dw indexed with the slab's 160 columns: the unused ones (which
        ncol = Cin * ks * ks                                     # repeat column 0) leak in
        full = np.zeros((Cout, STEM_N))
        full[:, :ncol] = dw.reshape(Cout, ncol)
        full[:, ncol:] = full[:, :1]
        dw = full.reshape(-1)[:Cout * ncol].reshape(dw.shape)
    return _zero_last_block(dw, 0, mut)


def pack_weights(w):
    """(wf [taps][CinP4][CoutP16], wb [taps][CoutP4][CinP16]) float32, flat, zero padded: taps row-major, not flipped."""
    w = np.asarray(w, F32)
    Cout, Cin, ks, _ = w.shape
    taps = ks * ks
    wt = w.reshape(Cout, Cin, taps)
    wf = np.zeros((taps, round_up(Cin, 4), round_up(Cout, 16)), F32)
    wb = np.zeros((taps, round_up(Cout, 4), round_up(Cin, 16)), F32)
    for t in range(taps):
        wf[t, :Cin, :Cout] = wt[:, :, t].T
        wb[t, :Cout, :Cin] = wt[:, :, t]
    return wf.reshape(-1), wb.reshape(-1)


# ---- pooling, sampling, phases ------------------------------------------------------------------------------------------------
def maxpool3(x, mut: str = ""):
    """(y float32, idx uint8) of the 3x3 / 2 / 1 max-pool over the last two axes: the window scanned row-major, a larger value or a NaN
    replaces what is held (torch.nn.MaxPool2d: the first maximum, of several NaNs the last), idx = ky * 3 + kx."""
    x = np.asarray(x, F32)
    H, W = x.shape[-2:]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = np.full(x.shape[:-2] + (OH, OW), -np.inf, F32)
    idx = np.zeros(best.shape, np.uint8)
    have = np.zeros(best.shape, bool)
    with np.errstate(invalid="ignore"):
        for ky in range(3):
            for kx in range(3):
                iy, ix = 2 * np.arange(OH) + ky - 1, 2 * np.arange(OW) + kx - 1
                valid = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
                v = x[..., np.clip(iy, 0, H - 1)[:, None], np.clip(ix, 0, W - 1)[None, :]]
                if mut == "pool_nonan":
                    take = valid & ~np.isnan(v) & (~have | (v > best))
                else:
                    take = valid & (~have | ((v >= best) if mut == "pool_last" else (v > best)) | np.isnan(v))
                best, idx, have = np.where(take, v, best), np.where(take, np.uint8(ky * 3 + kx), idx), have | take
    return best.astype(F32), idx.astype(np.uint8)


def maxpool3_bwd(dy, idx, H, W):
    """float64 dx [..., H, W]: every window's gradient routed to its arg-max position (windows overlap: sums of up to four)."""
    dy, idx = np.asarray(dy, np.float64), np.asarray(idx)
    OH, OW = dy.shape[-2:]
    dxp = np.zeros(dy.shape[:-2] + (2 * OH + 1, 2 * OW + 1))
    for ky in range(3):
        for kx in range(3):
            dxp[..., ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] += np.where(idx == ky * 3 + kx, dy, 0.0)
    return dxp[..., 1:1 + H, 1:1 + W]


def subsample2(x):
    return np.ascontiguousarray(np.asarray(x)[..., ::2, ::2])


def subsample2_adjoint(dy, H, W, mut: str = ""):
    dy = np.asarray(dy, F32)
    dx = np.zeros(dy.shape[:-2] + (H, W), F32)
    if mut == "sub_odd_rows":                                    # the odd rows never written: what the buffer held stays
        dx[..., 1::2, :] = F32(SENT)
    dx[..., ::2, ::2] = dy
    return dx


def space_to_depth2(x, mut: str = ""):
    """xs [B, 4, C, H/2, W/2] with xs[b][2 py + px][c][i][j] = x[b][c][2 i + py][2 j + px]."""
    x = np.asarray(x)
    B, C, H, W = x.shape
    xs = np.zeros((B, 4, C, H // 2, W // 2), x.dtype)
    for py in range(2):
        for px in range(2):
            xs[:, (2 * px + py) if mut == "phase_swap" else (2 * py + px)] = x[:, :, py::2, px::2]
    return xs


def depth_to_space2(xs, mut: str = ""):
    xs = np.asarray(xs)
    B, _, C, h, w = xs.shape
    x = np.zeros((B, C, 2 * h, 2 * w), xs.dtype)
    for py in range(2):
        for px in range(2):
            x[:, :, py::2, px::2] = xs[:, (2 * px + py) if mut == "phase_swap" else (2 * py + px)]
    return x


# ---- the host dispatch restated ----------------------------------------------------------------------------------------------------
def nw_of(CP16: int) -> int:
    """NW of convs_fwd_kernel (CP16 = round_up(Cout, 16)) and of convs_bwd_data_kernel (round_up(Cin, 16))."""
    return 4 if CP16 >= 64 else (2 if CP16 >= 32 else 1)


def stem_shape(Cin, OW, ks, s, p) -> bool:
    return ks == 7 and s == 2 and p == 3 and Cin <= 3 and OW % 4 == 0


def plan_wrw(B, Cin, Cout, H, W, ks, s, p, dy_aligned: bool = True) -> dict:
    """What uaps_convs_bwd_weight runs for this call -- the shape AND dy's 16-byte alignment decide the form, and the blocks, slab
    strides and workspace are that form's own -- and `query`, what uaps_convs_wrw_workspace_bytes (which cannot see dy) reports:
    the larger of the two forms' needs where the shape admits the stem form."""
    OH, OW = out_size(H, ks, s, p), out_size(W, ks, s, p)
    tx, ty = (OW + 31) // 32, (OH + 3) // 4
    tiles = B * tx * ty

    def general():
        ncob, ncib = (Cout + 15) // 16, (Cin + 15) // 16
        blocks = ncob * ncib * (7 if ks == 7 else 1)
        nsplit = max(1, min(1 if blocks >= 1024 else 1024 // blocks, tiles))
        n = ks * ks * ncob * 16 * ncib * 16
        gh, gw = (3, 3) if ks == 3 else (1, ks)
        return dict(stem=False, ncob=ncob, ncib=ncib, CoutS=ncob * 16, CinS=ncib * 16, nsplit=nsplit, tiles=tiles, ws_bytes=nsplit * n * 4,
                    reduce=16 if n < 32768 else 64, kernels=(f"convs_wrw_kernel<{gh}, {gw}, {s}>",))

    def stem():
        ncob = (Cout + 63) // 64
        nsplit = max(1, min(1024 // ncob, tiles))
        return dict(stem=True, ncob=ncob, ncib=1, CoutS=ncob * 64, CinS=STEM_N, nsplit=nsplit, tiles=tiles, ws_bytes=nsplit * ncob * 64 * STEM_N * 4,
                    reduce=0, kernels=("stem7_wrw_kernel", "stem7_reduce_kernel"))

    g = general()
    if stem_shape(Cin, OW, ks, s, p):
        st = stem()
        run = st if dy_aligned else g
        return dict(run, query=max(g["ws_bytes"], st["ws_bytes"]))
    return dict(g, query=g["ws_bytes"])


def sub_vec(W: int, *offs) -> bool:
    """The vec flag of subsample2_fwd_kernel / subsample2_bwd_kernel."""
    return W % 8 == 0 and all(o % 4 == 0 for o in offs)


# ---- the case table -----------------------------------------------------------------------------------------------------------
class Case:
    """id, family (conv / pool / sub / s2d), parameters by attribute.  conv: B Cin Cout H W ks s p, ops (of fwd, dx, dw), offdy (floats
    dy sits off 16-byte alignment: the one pointer the dispatch looks at).  The other views get 0..3 floats from a CRC of the id."""
    DEFAULTS = dict(ops=("fwd", "dx", "dw"), offdy=0, offx=0, offy=0, special="")

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
        """The view `name` of a conv case sits this many floats off alignment (every pointer but dy may: the kernels read scalars)."""
        if name == "dy":
            return self.offdy
        return zlib.crc32((self.id + "/" + name).encode()) % 4

    @property
    def geom(self):
        return (self.B, self.Cin, self.Cout, self.H, self.W, self.ks, self.s, self.p)

    @property
    def OH(self):
        return out_size(self.H, self.ks, self.s, self.p)

    @property
    def OW(self):
        return out_size(self.W, self.ks, self.s, self.p)

    @property
    def plan(self) -> dict:
        return plan_wrw(*self.geom, dy_aligned=self.offdy % 4 == 0)

    @property
    def kernels(self) -> frozenset:
        return frozenset(_kernels(self))


def _kernels(c: Case):
    e = c.entry
    if e == "conv":
        ks = {"convs_pack_kernel"} if set(c.ops) & {"fwd", "dx"} else set()
        if "fwd" in c.ops:
            ks.add(f"convs_fwd_kernel<{nw_of(round_up(c.Cout, 16))}>")
        if "dx" in c.ops:
            ks.add(f"convs_bwd_data_kernel<{nw_of(round_up(c.Cin, 16))}>")
        if "dw" in c.ops and c.ks != 5:
            ks |= set(c.plan["kernels"])
        return ks
    if e == "pool":
        return {"maxpool3s2_fwd_kernel", "maxpool3s2_bwd_kernel"}
    if e == "sub":
        return {"subsample2_fwd_kernel", "subsample2_bwd_kernel"}
    if e == "s2d":
        return {"space_depth2_kernel<false>", "space_depth2_kernel<true>"}
    raise ValueError(e)


def _cases():
    cs = []

    def conv(id, B, Cin, Cout, H, W, ks, s, p, **kw):
        cs.append(Case(id, "conv", B=B, Cin=Cin, Cout=Cout, H=H, W=W, ks=ks, s=s, p=p, **kw))

    # forward NW = 1, 2, 4 (and the input gradient's, with the channels swapped), a CoutP / CinP that is no multiple of 16 NW (40 -> 48
    # with NW = 2, 80 with NW = 4: the block past the end re-reads block 0), channels off 4 and off 16, OW < 16, OW = 16 k + 1, W = 1,
    # H = 1, B = 1 and 3.  The weight gradients ride along: <3,3,1>, <3,3,2>, <1,1,1>, <1,1,2>, one tile (nsplit = 1), OH off 4
    conv("c3s1-nw1", 1, 5, 7, 6, 9, 3, 1, 1)
    conv("c3s1-nw2x1", 3, 40, 13, 5, 17, 3, 1, 1)              # fwd NW 1, dx NW 2 with CinP 48; OW = 17
    conv("c3s2-nw2", 3, 6, 40, 9, 35, 3, 2, 1)                 # fwd NW 2 with CoutP 48; both parity classes, W odd: the odd class one short
    conv("c3s2-nw4", 1, 80, 66, 7, 33, 3, 2, 1)                # fwd NW 4 with CoutP 80, dx NW 4 with CinP 80; OW = 17
    conv("c1s1-nw4x2", 2, 34, 64, 5, 33, 1, 1, 0)              # <1,1,1>; dx NW 2
    conv("c1s2-odd-zero", 2, 9, 21, 7, 10, 1, 2, 0)            # <1,1,2>: the odd rows and columns of dx must be written as zero
    conv("c3s1-w1", 2, 4, 16, 5, 1, 3, 1, 1)
    conv("c3s2-h1", 3, 3, 5, 1, 37, 3, 2, 1)
    conv("c7s1-h1w1", 1, 2, 3, 1, 1, 7, 1, 3)                  # <1,7,1>: one pixel, 49 taps of which one is inside
    conv("c3s2-rem", 2, 5, 6, 8, 12, 3, 2, 1)                  # (H + 2 p - ks) % s != 0: the last input row and column meet fewer taps
    # padding other than ks / 2
    conv("c3s1-p0", 2, 5, 18, 6, 20, 3, 1, 0)
    conv("c3s2-p0", 2, 5, 18, 7, 21, 3, 2, 0)
    conv("c1s1-p1", 2, 6, 5, 4, 7, 1, 1, 1)                    # a ring of outputs that see no input at all
    conv("c1s2-p1", 1, 3, 4, 5, 6, 1, 2, 1)                    # only the odd rows and columns of dx are reached
    conv("c3s1-p4", 1, 3, 4, 3, 5, 3, 1, 4)                    # the limit ks / 2 + 3
    conv("c3s2-p4", 2, 3, 4, 4, 9, 3, 2, 4)
    conv("c5s2", 2, 6, 20, 9, 19, 5, 2, 2, ops=("fwd", "dx"))  # 5x5: no weight gradient (refused, see the GPU test)
    conv("c5s1-p0", 1, 3, 4, 7, 8, 5, 1, 0, ops=("fwd", "dx"))
    conv("c7s1", 2, 5, 18, 6, 40, 7, 1, 3)                     # <1,7,1>, OW off 32 over two tile columns
    conv("c7s2-general", 2, 5, 18, 11, 70, 7, 2, 3)            # <1,7,2> by Cin > 3
    # weight gradient, general: more than one tile per split and an uneven count (135 tiles over 113 splits), Cout and Cin off 16,
    # OH off 4, OW off 32
    conv("wrw-uneven-tiles", 3, 40, 36, 34, 131, 3, 1, 1, ops=("dw",))
    conv("wrw-blocks-1024", 1, 512, 512, 4, 4, 1, 1, 0)                        # nsplit = 1 by ncob ncib = 1024; reduce<64>; 2 x 262144 packed
                                                                               # floats: the pack kernel's 1024 blocks loop twice
    conv("wrw-reduce16-chains", 2, 3, 5, 20, 224, 1, 1, 0, ops=("dw",))        # reduce<16>: 70 splits = 64 + 6
    conv("wrw-reduce64-chains", 3, 20, 24, 28, 30, 7, 1, 3, ops=("dw",))       # reduce<64>: 21 splits = 16 + 5; <1,7,1>
    conv("wrw-s2-tiles", 2, 17, 16, 19, 80, 3, 2, 1, ops=("dw",))              # <3,3,2> over several tiles, Cin off 16
    conv("wrw-1x1s2-tiles", 2, 20, 33, 18, 70, 1, 2, 0, ops=("dw",))           # <1,1,2> over several tiles
    # the stem form: Cin 1, 2, 3; Cout 8, 64, 80 (a second, partial block of 64); OW % 4 == 0 below and above 32
    conv("stem-c1-o8", 1, 1, 8, 9, 24, 7, 2, 3)                                # OW 12
    conv("stem-c2-o64", 2, 2, 64, 10, 80, 7, 2, 3, ops=("dw",))                # OW 40
    conv("stem-c3-o80", 2, 3, 80, 17, 40, 7, 2, 3, ops=("dw",))                # OW 20
    conv("stem-c3-o80-ow21", 2, 3, 80, 17, 42, 7, 2, 3, ops=("dw",))           # OW % 4 != 0: general <1,7,2>
    conv("stem-c4-o80", 2, 4, 80, 17, 40, 7, 2, 3, ops=("dw",))                # Cin = 4: general
    conv("stem-c3-o80-dyoff", 2, 3, 80, 17, 40, 7, 2, 3, ops=("dw",), offdy=1)  # dy one float off: general, with the general plan

    def add(id, entry, **p):
        cs.append(Case(id, entry, **p))

    # max-pool: odd and even H and W, H or W = 1, the planted windows (ties, all -inf, NaNs)
    add("pool-6x8", "pool", shape=(2, 3, 6, 8))
    add("pool-7x9", "pool", shape=(3, 2, 7, 9))
    add("pool-1x9", "pool", shape=(2, 2, 1, 9))
    add("pool-8x1", "pool", shape=(2, 2, 8, 1))
    add("pool-1x1", "pool", shape=(5, 1, 1, 1))
    add("pool-special", "pool", shape=(1, 1, 4 * N_SPECIAL, 5), special="special")
    add("pool-grid", "pool", shape=(2, 260, 9, 30))                            # more than one workgroup
    # subsample2: 16-byte form, the scalar form by a pointer off alignment and by the width, odd sizes
    add("sub-vec", "sub", shape=(2, 3, 6, 16))
    add("sub-vec-oddh", "sub", shape=(2, 3, 5, 8))
    add("sub-offx", "sub", shape=(2, 3, 6, 16), offx=1)
    add("sub-offy", "sub", shape=(2, 3, 6, 16), offy=3)
    add("sub-w12", "sub", shape=(2, 3, 6, 12))
    add("sub-odd", "sub", shape=(3, 2, 7, 9))
    add("sub-1x1", "sub", shape=(2, 2, 1, 1))
    # space_to_depth2 and back: the smallest legal shape, and B, C > 1
    add("s2d-min", "s2d", shape=(1, 1, 2, 8))
    add("s2d-3x5", "s2d", shape=(3, 5, 6, 24))
    return cs


def _special_windows():
    """3x3 windows (row-major, 9 values): every pair of positions equal and largest, all equal, all -inf, a NaN first, last and in the
    middle, every pair of two NaNs among positions (0, 4, 8), -0.0 against +0.0."""
    wins = []
    for i in range(9):
        for j in range(i + 1, 9):
            w = -np.arange(1, 10, dtype=F32)
            w[[i, j]] = 5.0
            wins.append(w)
    wins.append(np.full(9, 2.0, F32))
    wins.append(np.full(9, -np.inf, F32))
    base = np.array([1.0, 9.0, -3.0, np.inf, 0.5, 9.0, -np.inf, 2.0, 4.0], F32)
    for i in (0, 4, 8):
        w = base.copy()
        w[i] = np.nan
        wins.append(w)
    for i, j in ((0, 4), (0, 8), (4, 8), (1, 2)):
        w = base.copy()
        w[[i, j]] = np.nan
        wins.append(w)
    for i, j in ((0, 8), (8, 0)):
        w = np.full(9, -1.0, F32)
        w[i], w[j] = -0.0, 0.0
        wins.append(w)
    return wins


N_SPECIAL = len(_special_windows())


def pool_special() -> np.ndarray:
    """[1, 1, 4 N, 5]: window n fills rows 4 n + 1 .. 4 n + 3, columns 1 .. 3 of a 5-wide plane: output (2 n + 1, 1) reads exactly it.
    Everything around is -2^100, below every finite planted value, so the outputs that straddle a window are decided by it too."""
    wins = _special_windows()
    x = np.full((1, 1, 4 * len(wins), 5), -2.0 ** 100, F32)
    for n, w in enumerate(wins):
        x[0, 0, 4 * n + 1:4 * n + 4, 1:4] = w.reshape(3, 3)
    return x


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
CONV = [c for c in CASES if c.entry == "conv"]
# every __global__ of conv_strided.hip (the filter of tests/test_strided_ref.py)
KERNEL_NAMES = ("convs_fwd_kernel", "convs_bwd_data_kernel", "convs_pack_kernel", "convs_wrw_kernel", "stem7_wrw_kernel", "stem7_reduce_kernel",
                "maxpool3s2_fwd_kernel", "maxpool3s2_bwd_kernel", "subsample2_fwd_kernel", "subsample2_bwd_kernel", "space_depth2_kernel")


# ---- inputs and references per case ---------------------------------------------------------------------------------------------
def conv_inputs(c: Case, kind: str) -> dict:
    """x, w, dy float32.  kind "int": integers from {-3..3}; "real": magnitudes uniform in [0.5, 1], random signs."""
    rng = rng_for(c.id, 1 if kind == "int" else 2)
    shapes = dict(x=(c.B, c.Cin, c.H, c.W), w=(c.Cout, c.Cin, c.ks, c.ks), dy=(c.B, c.Cout, c.OH, c.OW))
    if kind == "int":
        return {k: rng.integers(-3, 4, s).astype(F32) for k, s in shapes.items()}
    return {k: (rng.uniform(0.5, 1.0, s) * rng.choice([-1.0, 1.0], s)).astype(F32) for k, s in shapes.items()}


def contraction(c: Case, op: str) -> int:
    """At most this many terms meet in one output of `op`: taps x channels, or output pixels (fewer at a border or at stride 2)."""
    if op == "fwd":
        return c.ks * c.ks * c.Cin
    if op == "dx":
        return c.ks * c.ks * c.Cout
    return c.B * c.OH * c.OW


def extra_adds(c: Case, op: str) -> int:
    """R: the additions beyond the contraction -- none in the forward and the input gradient; in the weight gradient the three that
    join the four row-waves (general form) and one per split of the reduction."""
    if op != "dw":
        return 0
    return c.plan["nsplit"] + (0 if c.plan["stem"] else 3)


def conv_reference(c: Case, inp: dict, op: str, mut: str = "", bar: bool = True):
    """(float64 value, K per element, sum|terms| per element) of one of fwd / dx / dw; bar=False: the value alone (the integer run)."""
    a = {k: np.abs(v.astype(np.float64)) for k, v in inp.items()}
    one = {k: np.ones(v.shape) for k, v in inp.items()}
    if op == "fwd":
        f = lambda d, m="": conv_fwd(d["x"], d["w"], c.s, c.p, m)
    elif op == "dx":
        f = lambda d, m="": conv_dx(d["dy"], d["w"], c.s, c.p, c.H, c.W, m)
    else:
        f = lambda d, m="": conv_dw(d["dy"], d["x"], c.ks, c.s, c.p, m, c.plan)
    return (f(inp, mut), f(one), f(a)) if bar else (f(inp, mut), None, None)


def conv_bar(c: Case, op: str, K, mag):
    return (K + extra_adds(c, op)) * EPS24 * mag


_REAL_OPS = {}


def real_ops(c: Case):
    """The ops of a conv case whose real-valued run is held against its bar: those whose largest bar stays under REAL_BAR_MAX."""
    if c.id not in _REAL_OPS:
        inp, out = conv_inputs(c, "real"), []
        for op in c.ops:
            if op == "dw" and c.ks == 5:
                continue
            _, K, mag = conv_reference(c, inp, op)
            if conv_bar(c, op, K, mag).max() < REAL_BAR_MAX:
                out.append(op)
        _REAL_OPS[c.id] = tuple(out)
    return _REAL_OPS[c.id]


def pool_inputs(c: Case) -> dict:
    rng = rng_for(c.id)
    if c.special:
        x = pool_special()
    else:                                                        # a coarse grid: many exact ties inside a window
        x = (np.round(rng.standard_normal(c.shape) * 2) / 2).astype(F32)
    B, C_, H, W = x.shape
    return dict(x=x, dy=rng.integers(-3, 4, (B, C_, (H - 1) // 2 + 1, (W - 1) // 2 + 1)).astype(F32))


def plane_inputs(c: Case) -> dict:
    rng = rng_for(c.id)
    B, C_, H, W = c.shape
    d = dict(x=rng.standard_normal(c.shape).astype(F32))
    if c.entry == "sub":
        d["dy"] = rng.standard_normal((B, C_, (H - 1) // 2 + 1, (W - 1) // 2 + 1)).astype(F32)
    return d


def plane_reference(c: Case, inp: dict, mut: str = "") -> dict:
    """name -> array, all bit for bit (the pooled gradient sums at most four small integers)."""
    B, C_, H, W = inp["x"].shape
    if c.entry == "pool":
        y, idx = maxpool3(inp["x"], mut)
        return dict(y=y, idx=idx, dx=maxpool3_bwd(inp["dy"], idx, H, W).astype(F32))
    if c.entry == "sub":
        return dict(y=subsample2(inp["x"]), dx=subsample2_adjoint(inp["dy"], H, W, mut))
    xs = space_to_depth2(inp["x"], mut)
    return dict(xs=xs, back=depth_to_space2(xs, mut))


# ---- the comparisons both test files use -----------------------------------------------------------------------------------------
def bits_differ(got, ref) -> int:
    """How many elements differ in their bits; a shape or dtype mismatch counts as everything.  Two NaNs are equal."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return max(got.size, ref.size, 1)
    if got.dtype == F32:
        both_nan = np.isnan(got) & np.isnan(ref)
        return int(((got.view(np.uint32) != ref.view(np.uint32)) & ~both_nan).sum())
    return int((got != ref).sum())


def int_mismatch(got, ref64) -> int:
    """The integer run: how many elements of the float32 output differ from the int64 reference (which float64 holds exactly)."""
    got = np.asarray(got)
    if got.shape != ref64.shape or got.dtype != F32:
        return max(got.size, ref64.size, 1)
    ref = np.rint(ref64).astype(np.int64)
    assert np.array_equal(ref.astype(np.float64), ref64)
    g = got.astype(np.float64)
    return int((~(g == ref.astype(np.float64))).sum())


def bar_ratio(got, val, bar) -> float:
    """max |got - val| / bar over the elements (0 where both the error and the bar vanish); inf for a value that is no number."""
    got = np.asarray(got, np.float64)
    if got.shape != val.shape or not np.all(np.isfinite(got)):
        return math.inf
    d = np.abs(got - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bar)
    return float(q.max()) if q.size else 0.0


def unwritten(got) -> int:
    """Elements still holding the buffer's sentinel."""
    got = np.asarray(got)
    return int((got == F32(SENT)).sum()) if got.dtype == F32 else 0


def check_conv(c: Case, op: str, kind: str, got, inp: dict, mut_ref=None):
    """(ratio or None, failed checks) of one output.  mut_ref: a precomputed (value, K, mag), else the reference of the case."""
    val, K, mag = mut_ref if mut_ref is not None else conv_reference(c, inp, op)
    bad = []
    if unwritten(got):
        bad.append(f"{op}/{kind}: {unwritten(got)} elements were never written")
    if kind == "int":
        n = int_mismatch(got, val)
        if n:
            bad.append(f"{op}/int: {n} of {val.size} elements differ from the integer reference")
        return None, bad
    r = bar_ratio(got, val, conv_bar(c, op, K, mag))
    if not r <= 1.0:
        bad.append(f"{op}/real: error {r:.3g} x its bar")
    return r, bad

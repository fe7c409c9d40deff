"""Float64 restatement of tiled (sliding-window) inference for tests/test_tiled_host.py, tests/test_gpu_tiled.py and tools/tiled_tau.py:
the geometry of include/uaps_hip.h ("Tiled"), the blend in the SCATTER form (loop over the tiles, acc += w * softmax(tile), norm += w,
then divide -- the kernel gathers per output pixel instead, so the two share no index arithmetic), the numpy-indexed cut, the seeded case
table with its cached references, the raw entry-point callers, and the bars.

The bars.  probs, conf and blended maps: TAU = min(1e-4, max(3 x floor, 16 x 2^-24)).
    floor          the CPU's fp32 composition (uaps_amd.tiled on CPU tensors) against float64 over CASES x their windows, measured by
                   tools/tiled_tau.py (profiles/tiled_forms_tau.txt): 2.37e-7 at the largest (0.6e-7 .. 2.4e-7 over the table; there are
                   no resampling coordinates, only one softmax and up to nine weighted adds per pixel)   -> 3 x floor = 7.1e-7
    16 x 2^-24     = 9.54e-7, derived: a pixel sees one expf, one softmax division, up to nine multiply-adds and one final division, all
                   on values <= 1, so a different but valid rounding order (fused multiply-adds, another expf) may move it by about a
                   dozen half-ulps of 1
    TAU            = 9.54e-7: the derived term decides; the kernel's own error sets nothing.
mask: equal to the float64 arg-max wherever the float64 top-2 margin exceeds MARGIN = 1e-4, with at most 1 % of a case's pixels under
the margin.  The `saturated` case (logits N(0, 60^2): one-hot softmaxes, whose blend under integer weights gives exact 0.5 / 0.5 ties)
is exempt from that comparison only; on the device's own outputs every case must satisfy mask == probs.argmax(1) and
|conf - probs.max(1)| <= 2e-7."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

TAU = 16 * 2.0 ** -24    # = max(3 x 2.37e-7, 16 x 2^-24), below the 1e-4 cap
MARGIN = 1e-4            # the float64 top-2 margin above which the arg-max must agree
MAX_EXCLUDED = 0.01      # at most this share of a case's pixels may fall under MARGIN
SELF_CONF = 2e-7         # |conf - probs.max(1)| on the device's own outputs
DEV = "cuda:0"
TILES_PER_CHUNK = 3      # the chunked fold: a short last chunk, chunk boundaries inside an image

Case = namedtuple("Case", "name B C H W tile overlap gain windows")

CASES = (
    Case("small-5x7", 1, 3, 5, 7, (16, 16), (0, 0), 2.0, ("uniform", "triangle")),
    Case("row-1x40", 1, 2, 1, 40, (16, 16), (4, 4), 2.0, ("uniform", "triangle")),
    Case("exact-32x48", 2, 4, 32, 48, (16, 16), (0, 0), 2.0, ("uniform", "triangle")),
    Case("clamp-41x50", 2, 4, 41, 50, (16, 16), (4, 4), 2.0, ("uniform", "triangle")),
    Case("half-40x72", 1, 8, 40, 72, (16, 32), (8, 16), 2.0, ("uniform", "triangle", "gauss")),
    Case("c7-33x47", 2, 7, 33, 47, (16, 24), (5, 7), 2.0, ("uniform", "triangle")),
    Case("saturated", 2, 4, 41, 52, (16, 16), (4, 4), 60.0, ("uniform", "triangle")),
)
CASE_WINDOWS = tuple((c.name, w) for c in CASES for w in c.windows)
MASK_EXEMPT = ("saturated",)


def origins(n, t, o):
    """One axis: a single origin 0 when n <= t, else 0, s, 2s, ... while < n - t, then n - t."""
    if n <= t:
        return [0]
    out, s, k = [], t - o, 0
    while k * s < n - t:
        out.append(k * s)
        k += 1
    return out + [n - t]


def mirror(i, n):
    if n == 1:
        return 0
    j = i % (2 * (n - 1))
    return j if j < n else 2 * (n - 1) - j


def window(t, kind):
    """float64 numpy [t]: the named windows of the issue."""
    k = np.arange(t, dtype=np.float64)
    if kind == "uniform":
        return np.ones(t)
    if kind == "triangle":
        return np.minimum(k + 1, t - k)
    assert kind == "gauss"
    return np.exp(-0.5 * ((k - (t - 1) / 2) / (t / 8)) ** 2).astype(np.float32).astype(np.float64)


def cut(x, tile, overlap):
    """Every tile of x [B,Cin,H,W] (a torch tensor), numpy-indexed: [B * T, Cin, th, tw] in image-major order."""
    a = x.numpy()
    B, _, H, W = a.shape
    (th, tw), (oy, ox) = tile, overlap
    out = []
    for b in range(B):
        for y0 in origins(H, th, oy):
            sy = np.array([mirror(y0 + r, H) if H < th else y0 + r for r in range(th)])
            for x0 in origins(W, tw, ox):
                sx = np.array([mirror(x0 + c, W) if W < tw else x0 + c for c in range(tw)])
                out.append(a[b][:, sy[:, None], sx[None, :]])
    return torch.from_numpy(np.stack(out))


def fold(z, dims, tile, overlap, wy, wx, maps=()):
    """The scatter form in float64.  z: [B * T, C, th, tw] (or None), maps: [B * T, th, tw] each; wy / wx: array-likes.  Returns
    (probs [B,C,H,W] float64 or None, [blended maps])."""
    B, H, W = dims
    (th, tw), (oy, ox) = tile, overlap
    ys, xs = origins(H, th, oy), origins(W, tw, ox)
    w2 = torch.as_tensor(np.asarray(wy, dtype=np.float64))[:, None] * torch.as_tensor(np.asarray(wx, dtype=np.float64))[None, :]
    p = F.softmax(z.double(), dim=1) if z is not None else None
    acc = torch.zeros(B, z.shape[1], H, W, dtype=torch.float64) if z is not None else None
    macc = [torch.zeros(B, H, W, dtype=torch.float64) for _ in maps]
    norm = torch.zeros(B, H, W, dtype=torch.float64)
    g = 0
    for b in range(B):
        for y0 in ys:
            for x0 in xs:
                hh, ww = min(th, H - y0), min(tw, W - x0)
                w = w2[:hh, :ww]
                norm[b, y0:y0 + hh, x0:x0 + ww] += w
                if acc is not None:
                    acc[b, :, y0:y0 + hh, x0:x0 + ww] += w * p[g, :, :hh, :ww]
                for m, a in zip(maps, macc):
                    a[b, y0:y0 + hh, x0:x0 + ww] += w * m[g, :hh, :ww].double()
                g += 1
    assert z is None or g == z.shape[0]
    return (acc / norm[:, None] if acc is not None else None), [a / norm for a in macc]


def n_tiles(case):
    return case.B * len(origins(case.H, case.tile[0], case.overlap[0])) * len(origins(case.W, case.tile[1], case.overlap[1]))


def case_logits(case):
    """Seeded logits ~ N(0, gain^2) of every tile, [B * T, C, th, tw] (CPU, fp32)."""
    gen = torch.Generator().manual_seed(2000 + sum(map(ord, case.name)))
    return torch.randn(n_tiles(case), case.C, *case.tile, generator=gen) * case.gain


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """(case, CPU logits, float64 probs) of a case under a named window: computed once, shared, never written."""
    case = next(c for c in CASES if c.name == name)
    z = case_logits(case)
    ref, _ = fold(z, (case.B, case.H, case.W), case.tile, case.overlap, window(case.tile[0], kind), window(case.tile[1], kind))
    return case, z, ref


def chunked(t, per=TILES_PER_CHUNK):
    """The tiles of t in separately allocated chunks of `per` (the last may be shorter)."""
    return [t[k:k + per].clone() for k in range(0, t.shape[0], per)]


def clear_pixels(ref, margin=MARGIN):
    top2 = ref.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > margin


def check_mask(mask, ref, name=""):
    """mask == the float64 arg-max wherever the float64 top-2 margin exceeds MARGIN; at most MAX_EXCLUDED of the pixels under it."""
    if name in MASK_EXEMPT:
        return
    clear = clear_pixels(ref)
    excluded = 1.0 - float(clear.double().mean())
    assert excluded <= MAX_EXCLUDED, f"{excluded:.4f} of the pixels under the margin"
    assert torch.equal(mask.cpu()[clear], ref.argmax(dim=1)[clear])


def check_result(res, ref, name=""):
    """The bars on a TiledResult with all three outputs; returns (probs error, conf error) against float64."""
    probs, mask, conf = res.probs.cpu(), res.mask.cpu(), res.conf.cpu()
    e_p = float((probs.double() - ref).abs().max())
    e_c = float((conf.double() - ref.max(dim=1).values).abs().max())
    assert e_p <= TAU and e_c <= TAU, (name, e_p, e_c, TAU)
    assert float((probs.double().sum(1) - 1).abs().max()) <= TAU
    check_mask(mask, ref, name)
    assert torch.equal(mask, probs.argmax(dim=1))                                  # lowest index on ties, as torch
    assert float((conf - probs.max(dim=1).values).abs().max()) <= SELF_CONF
    return e_p, e_c


def _ptr(t):
    return t.data_ptr() if isinstance(t, torch.Tensor) else t


def raw_cut(x, out, tile, overlap, g0, g1, over=None, struct=None):
    """uaps_tile_cut through the raw entry point; x / out: tensors or raw addresses (dims then come from `over`)."""
    from uaps_amd import _lib
    call = struct if struct is not None else _lib.TileCutCall()
    base = call.base if struct is not None else call
    base.struct_size = C.sizeof(call)
    if isinstance(x, torch.Tensor):
        base.B, base.Cin, base.H, base.W = x.shape
        base.stream = _lib.current_stream(x.device) if x.is_cuda else None
    (base.th, base.tw), (base.oy, base.ox), base.g0, base.g1 = tile, overlap, g0, g1
    base.x, base.out = _ptr(x), _ptr(out)
    for k, v in (over or {}).items():
        setattr(base, k, v)
    return _lib.lib().uaps_tile_cut(C.byref(call))


def raw_fold(chunks, dims, tile, overlap, wy, wx, probs=None, mask=None, conf=None, maps=(), map_out=(), per=None, n_classes=None,
             over=None, struct=None):
    """uaps_tile_fold through the raw entry point.  chunks: a list of tensors (or raw addresses, with n_classes and per given), maps: a
    list of such lists; dims = (B, H, W); `over` replaces fields after they are filled in ("logits3": None clears a table entry)."""
    from uaps_amd import _lib
    call = struct if struct is not None else _lib.TileFoldCall()
    base = call.base if struct is not None else call
    base.struct_size = C.sizeof(call)
    chunks = list(chunks)
    base.B, base.H, base.W = dims
    first = chunks[0] if chunks else maps[0][0]
    base.C = n_classes if n_classes is not None else (chunks[0].shape[1] if chunks else 0)
    (base.th, base.tw), (base.oy, base.ox) = tile, overlap
    base.n_chunks = len(chunks) if chunks else len(maps[0])
    base.tiles_per_chunk = per if per is not None else first.shape[0]
    base.n_maps = len(maps)
    for k, z in enumerate(chunks):
        base.logits[k] = _ptr(z)
    for m, cs in enumerate(maps):
        for k, t in enumerate(cs):
            base.maps[m][k] = _ptr(t)
    for m, t in enumerate(map_out):
        base.map_out[m] = _ptr(t)
    base.wy, base.wx = _ptr(wy), _ptr(wx)
    base.probs, base.mask, base.conf = (_ptr(t) if t is not None else None for t in (probs, mask, conf))
    if isinstance(first, torch.Tensor) and first.is_cuda:
        base.stream = _lib.current_stream(first.device)
    for k, v in (over or {}).items():
        name = k.rstrip("0123456789")
        if name in ("logits", "map_out") and name != k:
            getattr(base, name)[int(k[len(name):])] = v
        elif name == "maps" and name != k:
            base.maps[0][int(k[len(name):])] = v
        else:
            setattr(base, k, v)
    return _lib.lib().uaps_tile_fold(C.byref(call))

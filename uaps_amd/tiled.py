"""Tiled (sliding-window) full-resolution inference on the two kernels of csrc/tiled.hip: an image of any size is cut into overlapping
tiles of the size the network runs at, the network runs on the tiles, and the tiles' probability maps are blended under a separable
window so that seams do not show (what MONAI's sliding_window_inference and nnU-Net do).

Geometry per axis, image extent n, tile extent t, overlap 0 <= o <= t // 2, stride s = t - o (include/uaps_hip.h, "Tiled"):
    n <= t   one tile at origin 0, positions >= n mirrored without repeating the edge (`mirror_index`)
    n >  t   origins 0, s, 2s, ... while < n - t, then a last origin n - t: the last tile is clamped into the image
Tiles are numbered g = b * T + iy * nx + ix, image-major.

`tile_cut` is the input side of one chunk of tiles, `tile_fold` the output side of all tiles in one launch (softmax per covering tile,
weighted by wy[r] * wx[c], summed in ascending tile order, divided by the weight sum), `predict_tiled` the loop around a model.  CPU
tensors take a torch composition, as in the other modules; on a ROCm device a missing kernel is an error.  One-channel sigmoid heads,
TTA inside tiles, a margin-crop mode, uint8 sources, a captured tile forward, overlaps above half a tile and training on tiles are out
of scope."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

WANT = ("probs", "mask", "conf")
WINDOWS = ("uniform", "triangle", "gauss")


class TilePlan(NamedTuple):
    """ys / xs: the tiles' origins along y / x, ascending; tile = (th, tw); overlap = (oy, ox)."""
    ys: Tuple[int, ...]
    xs: Tuple[int, ...]
    tile: Tuple[int, int]
    overlap: Tuple[int, int]


class TiledResult(NamedTuple):
    """probs: fp32 [B,C,H,W], the weighted mean of the tiles' softmax; mask: int64 [B,H,W], its arg-max (lowest index among equal
    values); conf: fp32 [B,H,W], its largest value; maps: a tuple of blended [B,H,W] maps.  None for what was not asked for."""
    probs: Optional[torch.Tensor]
    mask: Optional[torch.Tensor]
    conf: Optional[torch.Tensor]
    maps: Tuple[torch.Tensor, ...]


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what}: an int or a pair expected")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def axis_origins(n: int, t: int, o: int) -> Tuple[int, ...]:
    """The origins of one axis (the restatement of uaps_tile_origins)."""
    n, t, o = int(n), int(t), int(o)
    if n < 1 or t < 1:
        raise ValueError("tile_plan: image and tile extents are >= 1")
    if o < 0 or o > t // 2:
        raise ValueError(f"tile_plan: overlap {o} outside [0, tile // 2 = {t // 2}]")
    if n <= t:
        return (0,)
    return tuple(range(0, n - t, t - o)) + (n - t,)


def mirror_index(i: int, n: int) -> int:
    """The source of position i of an axis of n pixels, mirrored without repeating the edge; defined for any i >= 0 and n >= 1."""
    if n == 1:
        return 0
    j = i % (2 * (n - 1))
    return j if j < n else 2 * (n - 1) - j


def tile_plan(H: int, W: int, tile=(256, 256), overlap=32) -> TilePlan:
    th, tw = _pair(tile, "tile")
    oy, ox = _pair(overlap, "overlap")
    return TilePlan(axis_origins(H, th, oy), axis_origins(W, tw, ox), (th, tw), (oy, ox))


def tile_window(t: int, kind: str = "triangle") -> torch.Tensor:
    """fp32 [t] on the CPU.  "uniform": ones; "triangle": min(k + 1, t - k) (integers: exact in fp32); "gauss": exp(-((k - (t-1)/2) /
    (t/8))^2 / 2) in float64, rounded to fp32 (MONAI's sigma = t / 8)."""
    t = int(t)
    if t < 1:
        raise ValueError("tile_window: t >= 1")
    k = np.arange(t, dtype=np.float64)
    if kind == "uniform":
        w = np.ones(t)
    elif kind == "triangle":
        w = np.minimum(k + 1, t - k)
    elif kind == "gauss":
        w = np.exp(-0.5 * ((k - (t - 1) / 2.0) / (t / 8.0)) ** 2)
    else:
        raise ValueError(f"tile_window: kind is one of {WINDOWS}")
    return torch.from_numpy(w.astype(np.float32))


def _windows(window, tile):
    """(wy [th], wx [tw]) fp32 on the CPU, checked: finite and > 0."""
    th, tw = tile
    if isinstance(window, str):
        wy, wx = tile_window(th, window), tile_window(tw, window)
    else:
        if not isinstance(window, (tuple, list)) or len(window) != 2 or not all(isinstance(w, torch.Tensor) for w in window):
            raise TypeError(f"window: one of {WINDOWS} or a pair of 1-D tensors (wy [th], wx [tw])")
        wy, wx = (w.detach().to("cpu", torch.float32).contiguous() for w in window)
        if wy.shape != (th,) or wx.shape != (tw,):
            raise ValueError(f"window: shapes ({th},) and ({tw},) expected, got {tuple(wy.shape)} and {tuple(wx.shape)}")
    for w in (wy, wx):
        if not bool(torch.isfinite(w).all()) or not bool((w > 0).all()):
            raise ValueError("window: every weight must be finite and > 0")
    return wy, wx


def _sources(origin, t, n):
    """The source index of every position of the tile at `origin` along an axis of n pixels."""
    return [mirror_index(origin + k, n) if n < t else origin + k for k in range(t)]


def tile_cut(x: torch.Tensor, plan: TilePlan, g0: int = 0, g1: Optional[int] = None) -> torch.Tensor:
    """[g1 - g0, Cin, th, tw]: the tiles g0 <= g < g1 (default: all B * T) of x [B,Cin,H,W], copied bit for bit."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise TypeError("tile_cut: float32 [B,Cin,H,W] expected")
    B, Cin, H, W = x.shape
    (th, tw), (oy, ox) = plan.tile, plan.overlap
    if plan.ys != axis_origins(H, th, oy) or plan.xs != axis_origins(W, tw, ox):
        raise ValueError(f"tile_cut: the plan is not tile_plan({H}, {W}, {plan.tile}, {plan.overlap})")
    ny, nx = len(plan.ys), len(plan.xs)
    total = B * ny * nx
    g1 = total if g1 is None else int(g1)
    g0 = int(g0)
    if not 0 <= g0 < g1 <= total:
        raise ValueError(f"tile_cut: 0 <= g0 < g1 <= {total} expected, got [{g0}, {g1})")
    if not x.is_cuda:
        x = x.detach()
        tiles = []
        for g in range(g0, g1):
            b, q = divmod(g, ny * nx)
            iy, ix = divmod(q, nx)
            sy = torch.tensor(_sources(plan.ys[iy], th, H))
            sx = torch.tensor(_sources(plan.xs[ix], tw, W))
            tiles.append(x[b][:, sy][:, :, sx])
        return torch.stack(tiles)
    x = x.detach().contiguous()
    out = torch.empty((g1 - g0, Cin, th, tw), dtype=torch.float32, device=x.device)
    _lib.call("uaps_tile_cut", _lib.TileCutCall, x.device, B=B, Cin=Cin, H=H, W=W, th=th, tw=tw, oy=oy, ox=ox, g0=g0, g1=g1,
              x=x.data_ptr(), out=out.data_ptr())
    return out


def _as_chunks(t, what, dims):
    """A tensor or a sequence of tensors -> a list of float32 chunks of `dims` dimensions."""
    chunks = [t] if isinstance(t, torch.Tensor) else list(t)
    if not chunks or any(not isinstance(c, torch.Tensor) or c.dim() != dims or c.dtype != torch.float32 for c in chunks):
        raise TypeError(f"tile_fold: {what}: float32 tensors of {dims} dimensions expected")
    return chunks


def _check_chunking(chunks, total, what):
    """Every chunk but the last holds tiles_per_chunk tiles, the last the rest: returns tiles_per_chunk."""
    if len(chunks) > _lib.TILE_MAX_CHUNKS:
        raise ValueError(f"tile_fold: {what}: {len(chunks)} chunks, at most {_lib.TILE_MAX_CHUNKS} (use a larger batch_tiles)")
    tpc = chunks[0].shape[0]
    sizes = [c.shape[0] for c in chunks]
    if tpc < 1 or sum(sizes) != total or any(n != tpc for n in sizes[:-1]) or not 1 <= sizes[-1] <= tpc:
        raise ValueError(f"tile_fold: {what}: chunks of {sizes} tiles do not split {total} tiles evenly with a shorter last chunk")
    return tpc


def _fold_composed(z, maps, plan, B, H, W, wy, wx):
    """The scatter form in the tensors' dtype: acc += w * softmax(tile), norm += w over the tiles in ascending order, then divide."""
    (th, tw), ny, nx = plan.tile, len(plan.ys), len(plan.xs)
    ref = z if z is not None else maps[0]
    w2 = (wy[:, None] * wx[None, :]).to(ref.dtype)
    p = F.softmax(z, dim=1) if z is not None else None
    acc = torch.zeros((B, z.shape[1], H, W), dtype=ref.dtype) if z is not None else None
    macc = [torch.zeros((B, H, W), dtype=ref.dtype) for _ in maps]
    norm = torch.zeros((H, W), dtype=ref.dtype)
    for iy, y0 in enumerate(plan.ys):
        for ix, x0 in enumerate(plan.xs):
            hh, ww = min(th, H - y0), min(tw, W - x0)           # the part of the tile that is image, not mirror padding
            w = w2[:hh, :ww]
            norm[y0:y0 + hh, x0:x0 + ww] += w
            for b in range(B):
                g = (b * ny + iy) * nx + ix
                if acc is not None:
                    acc[b, :, y0:y0 + hh, x0:x0 + ww] += w * p[g, :, :hh, :ww]
                for m, a in zip(maps, macc):
                    a[b, y0:y0 + hh, x0:x0 + ww] += w * m[g, :hh, :ww]
    return (acc / norm if acc is not None else None), [a / norm for a in macc]


def tile_fold(chunks, plan: TilePlan, shape, window="triangle", maps: Sequence = (), want: Sequence[str] = WANT) -> TiledResult:
    """The output side.  chunks: the network's logits on the tiles, one tensor [B * T, C, th, tw] or a sequence of chunk tensors
    [n_k, C, th, tw] in tile order (every chunk of the same n, the last may be shorter; at most 32), read where they lie; None: blend
    the maps alone (`want` is then ignored).  shape: (B, H, W) of the images (a [B, Cin, H, W] shape is accepted).  window: "uniform",
    "triangle", "gauss" or a pair of 1-D tensors (wy [th], wx [tw]), finite and > 0.  maps: up to 2 per-tile scalar maps [., th, tw],
    chunked like the logits, blended by the same weights into [B, H, W]."""
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (3, 4):
        raise ValueError("tile_fold: shape is (B, H, W)")
    B, H, W = shape[0], shape[-2], shape[-1]
    (th, tw), (oy, ox) = plan.tile, plan.overlap
    if B < 1 or plan.ys != axis_origins(H, th, oy) or plan.xs != axis_origins(W, tw, ox):
        raise ValueError(f"tile_fold: the plan is not tile_plan({H}, {W}, {plan.tile}, {plan.overlap})")
    total = B * len(plan.ys) * len(plan.xs)
    maps = list(maps)
    if len(maps) > _lib.TILE_MAX_MAPS:
        raise ValueError(f"tile_fold: at most {_lib.TILE_MAX_MAPS} maps")
    want = tuple(want) if chunks is not None else ()
    if any(k not in WANT for k in want) or (not want and not maps):
        raise ValueError(f"tile_fold: want is a subset of {WANT}, non-empty unless maps are given")
    zs = _as_chunks(chunks, "logits", 4) if chunks is not None and want else None
    ms = [_as_chunks(m, "maps", 3) for m in maps]
    tpc = None
    for what, cs in ([("logits", zs)] if zs is not None else []) + [("maps", m) for m in ms]:
        t = _check_chunking(cs, total, what)
        if tpc is not None and (t != tpc or len(cs) != n_chunks):
            raise ValueError("tile_fold: the maps are chunked like the logits")
        tpc, n_chunks = t, len(cs)
        tail = (zs[0].shape[1],) if what == "logits" else ()
        if any(c.shape[1:] != tail + (th, tw) or c.device != cs[0].device for c in cs):
            raise TypeError(f"tile_fold: {what}: chunks [n, {'C, ' if tail else ''}{th}, {tw}] on one device expected")
    first = zs[0] if zs is not None else ms[0][0]
    dev = first.device
    if any(m[0].device != dev for m in ms):
        raise TypeError("tile_fold: logits and maps on one device expected")
    Cc = zs[0].shape[1] if zs is not None else 0
    if zs is not None and not 2 <= Cc <= _lib.SEG_MAX_CLASSES:
        raise ValueError(f"tile_fold: 2..{_lib.SEG_MAX_CLASSES} classes (one-channel sigmoid heads have no form here)")
    wy, wx = _windows(window, plan.tile)
    if not first.is_cuda:
        z = torch.cat([c.detach() for c in zs]) if zs is not None else None
        probs, mout = _fold_composed(z, [torch.cat([c.detach() for c in m]) for m in ms], plan, B, H, W, wy, wx)
        top = probs.max(dim=1) if probs is not None else None
        return TiledResult(probs if "probs" in want else None, top.indices if "mask" in want else None,
                           top.values if "conf" in want else None, tuple(mout))
    zs = [c.detach().contiguous() for c in zs] if zs is not None else None
    ms = [[c.detach().contiguous() for c in m] for m in ms]
    wy, wx = wy.to(dev), wx.to(dev)
    probs = torch.empty((B, Cc, H, W), dtype=torch.float32, device=dev) if "probs" in want else None
    mask = torch.empty((B, H, W), dtype=torch.int64, device=dev) if "mask" in want else None
    conf = torch.empty((B, H, W), dtype=torch.float32, device=dev) if "conf" in want else None
    mout = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in ms]
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.call("uaps_tile_fold", _lib.TileFoldCall, dev, B=B, C=Cc, H=H, W=W, th=th, tw=tw, oy=oy, ox=ox, n_chunks=n_chunks,
              tiles_per_chunk=tpc, n_maps=len(ms), logits=[ptr(z) for z in zs or ()], maps=[[ptr(c) for c in cs] for cs in ms],
              wy=ptr(wy), wx=ptr(wx), probs=ptr(probs), mask=ptr(mask), conf=ptr(conf), map_out=[ptr(t) for t in mout])
    return TiledResult(probs, mask, conf, tuple(mout))


@torch.no_grad()
def predict_tiled(model: torch.nn.Module, images: torch.Tensor, tile=(256, 256), overlap=32, window="triangle",
                  batch_tiles: Optional[int] = None, uncertainty=False, want: Sequence[str] = WANT) -> TiledResult:
    """Sliding-window inference around the main head of `model` (model.eval(), no_grad): per chunk of `batch_tiles` tiles (default: all
    of them) one tile_cut and one forward (`tta.main_logits`), then one tile_fold over every chunk.  uncertainty=True: the full forward
    instead, and consistency.uncertainty_map(main, aux1) per chunk, blended into maps[0]; "auto": that where the model has an auxiliary
    head, nothing otherwise.  The tile must be a multiple of tta.default_size_multiple(model)."""
    from . import consistency
    from .tta import default_size_multiple, main_logits
    if images.dim() != 4 or images.dtype != torch.float32:
        raise TypeError("predict_tiled: float32 [B,Cin,H,W] expected")
    B, _, H, W = images.shape
    plan = tile_plan(H, W, tile, overlap)
    m = default_size_multiple(model)
    if plan.tile[0] % m or plan.tile[1] % m:
        raise ValueError(f"predict_tiled: the tile {plan.tile} must be a multiple of {m} for this model")
    _windows(window, plan.tile)                                   # a bad window fails before any forward
    total = B * len(plan.ys) * len(plan.xs)
    bt = total if batch_tiles is None else int(batch_tiles)
    if bt < 1:
        raise ValueError("predict_tiled: batch_tiles >= 1")
    bt = min(bt, total)
    if math.ceil(total / bt) > _lib.TILE_MAX_CHUNKS:
        raise ValueError(f"predict_tiled: {total} tiles in chunks of {bt} are more than {_lib.TILE_MAX_CHUNKS} chunks: use a larger batch_tiles")
    model.eval()
    logits, umaps = [], []
    for g0 in range(0, total, bt):
        t = tile_cut(images, plan, g0, min(g0 + bt, total))
        if uncertainty:
            out = model(t)
            heads = out if isinstance(out, (tuple, list)) else (out,)
            if heads[0].dim() == 4 and heads[0].shape[1] == 1:        # (tile_fold's refusal, before the uncertainty kernel sees the pair)
                raise ValueError("predict_tiled: 2..8 classes (one-channel sigmoid heads have no form here)")
            if len(heads) < 2:
                if uncertainty != "auto":
                    raise ValueError("the uncertainty map needs an auxiliary head")
                uncertainty = False
            else:
                umaps.append(consistency.uncertainty_map(heads[0], heads[1]))
            logits.append(heads[0])
        else:
            logits.append(main_logits(model, t))
    return tile_fold(logits, plan, (B, H, W), window, maps=(umaps,) if umaps else (), want=want)

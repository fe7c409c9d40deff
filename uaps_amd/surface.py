"""Boundary metrics on the kernels of csrc/surface.hip: an exact squared Euclidean distance transform and, built on it, the Hausdorff
distance, its percentile (HD95), the average symmetric surface distance (ASSD) and the surface Dice at a tolerance (NSD), under
medpy's conventions (hd95 / asd: 4-connected surfaces, the percentile of the two directed distance sets pooled).

`surface_distances` reduces the prediction and the target to one int64 row per (image, class) -- counts, maxima, fixed-point sums and
the two ranked squared distances of the percentile -- without a host synchronisation; `SurfaceResult` forms the metrics from that table
on the device, and `summary()` is the one device-to-host copy.  Every entry of the table is an integer: exact, and the same bits from
run to run.  Pixels are isotropic, maps 2-D, 1 <= H, W <= 4096, 1 <= num_classes <= 8.

CPU tensors take the numpy restatements below (a separable transform with a chunked brute-force row pass; no scipy), as in the other
modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._checks import LABEL_DTYPE_CODE as _DTYPE_CODE, as_labels

SURFACE_COLUMNS = ("n_pred", "n_gt", "max_pg", "max_gp", "sum16_pg", "sum16_gp", "within_pg", "within_gp", "rank_lo", "rank_hi",
                   "q_lo", "q_hi")
NO_FEATURE = 2 ** 30                     # UAPS_EDT_NO_FEATURE: distance_transform_sq of an image without a zero pixel
MAX_EXTENT = 4096                        # UAPS_SURFACE_MAX_EXTENT
MAX_CLASSES = 8                          # UAPS_MAX_CLASSES
SUM_ONE = 65536.0                        # sum16 = sum of floor(2^16 sqrt(d2))
_ws = _lib.Workspace()


class SurfaceResult(NamedTuple):
    """table: int64 [B,C,12], columns SURFACE_COLUMNS; percentile and tolerance as they were passed.  Every property is a float64
    [B,C] tensor on the table's device, NaN where the pair is not valid (no surface pixel in the prediction or in the target)."""
    table: torch.Tensor
    percentile: float = 95.0
    tolerance: Optional[float] = None

    def _col(self, name: str) -> torch.Tensor:
        return self.table[..., SURFACE_COLUMNS.index(name)]

    def _masked(self, v: torch.Tensor) -> torch.Tensor:
        return torch.where(self.valid, v, torch.full_like(v, float("nan")))

    @property
    def valid(self) -> torch.Tensor:
        """bool [B,C]: both surfaces have a pixel."""
        return (self._col("n_pred") > 0) & (self._col("n_gt") > 0)

    @property
    def hd(self) -> torch.Tensor:
        return self._masked(torch.maximum(self._col("max_pg"), self._col("max_gp")).to(torch.float64).sqrt())

    @property
    def hd95(self) -> torch.Tensor:
        """numpy's linear percentile of the pooled distances (medpy's hd95 at percentile 95)."""
        n = (self._col("n_pred") + self._col("n_gt")).to(torch.float64)
        h = (n - 1.0) * (self.percentile / 100.0)
        lo, hi = self._col("q_lo").to(torch.float64).sqrt(), self._col("q_hi").to(torch.float64).sqrt()
        return self._masked(lo + (hi - lo) * (h - self._col("rank_lo").to(torch.float64)))

    def _asd(self, s: str, n: str) -> torch.Tensor:
        return self._masked(self._col(s).to(torch.float64) / SUM_ONE / self._col(n).clamp(min=1).to(torch.float64))

    @property
    def asd_pg(self) -> torch.Tensor:
        return self._asd("sum16_pg", "n_pred")

    @property
    def asd_gp(self) -> torch.Tensor:
        return self._asd("sum16_gp", "n_gt")

    @property
    def assd(self) -> torch.Tensor:
        return (self.asd_pg + self.asd_gp) / 2.0

    @property
    def nsd(self) -> torch.Tensor:
        if self.tolerance is None:
            raise ValueError("SurfaceResult.nsd: surface_distances was called without a tolerance")
        n = (self._col("n_pred") + self._col("n_gt")).clamp(min=1).to(torch.float64)
        return self._masked((self._col("within_pg") + self._col("within_gp")).to(torch.float64) / n)

    def summary(self, classes: Optional[Sequence[int]] = None) -> Dict[str, float]:
        """One device-to-host copy: the means of hd95, assd, hd (and nsd with a tolerance) over the valid pairs of `classes`
        (default 1 .. C-1) and their number, "pairs".  NaN means where there is no valid pair."""
        Cn = self.table.shape[1]
        classes = list(range(1, Cn)) if classes is None else [int(c) for c in classes]
        if any(c < 0 or c >= Cn for c in classes):
            raise ValueError(f"SurfaceResult.summary: classes lie in [0, {Cn})")
        names = ["hd95", "assd", "hd"] + (["nsd"] if self.tolerance is not None else [])
        stack = torch.stack([getattr(self, n) for n in names] + [self.valid.to(torch.float64)])[:, :, classes]
        host = stack.reshape(len(names) + 1, -1).cpu().numpy()
        ok = host[-1] > 0
        out = {n: (float(host[i][ok].mean()) if ok.any() else float("nan")) for i, n in enumerate(names)}
        out["pairs"] = int(ok.sum())
        return out


# ------------------------------------------------------------------------------------------------ numpy restatements
def _column_distance(feature: np.ndarray) -> np.ndarray:
    """int64 [H,W]: the distance along the column to the nearest feature pixel, MAX_EXTENT * 8 where the column has none."""
    H, W = feature.shape
    none = MAX_EXTENT * 8
    g = np.full((H, W), none, dtype=np.int64)
    run = np.full(W, none, dtype=np.int64)
    for y in range(H):
        run = np.where(feature[y], 0, np.minimum(run + 1, none))
        g[y] = run
    run = np.full(W, none, dtype=np.int64)
    for y in range(H - 1, -1, -1):
        run = np.where(feature[y], 0, np.minimum(run + 1, none))
        g[y] = np.minimum(g[y], run)
    return g


def _edt_sq_np(feature: np.ndarray) -> np.ndarray:
    """int64 [H,W]: the squared distance of every pixel to the nearest True pixel of `feature`; NO_FEATURE everywhere when it has none.
    Separable: D2(y, x) = min over x' of (x - x')^2 + g(y, x')^2, the row pass by brute force over chunks of rows."""
    H, W = feature.shape
    if not feature.any():
        return np.full((H, W), NO_FEATURE, dtype=np.int64)
    g = _column_distance(feature)
    g2 = g * g
    xs = np.arange(W, dtype=np.int64)
    out = np.empty((H, W), dtype=np.int64)
    xstep = max(1, min(W, (1 << 22) // W))
    ystep = max(1, (1 << 22) // (xstep * W))
    for x0 in range(0, W, xstep):
        dx2 = (xs[x0:x0 + xstep, None] - xs[None, :]) ** 2                  # [x, x']
        for y0 in range(0, H, ystep):
            out[y0:y0 + ystep, x0:x0 + xstep] = (g2[y0:y0 + ystep, None, :] + dx2[None]).min(axis=2)
    return out


def _surface_np(m: np.ndarray, c: int) -> np.ndarray:
    """bool [H,W]: m == c with a 4-neighbour that is != c or outside the image."""
    fg = np.pad(m == c, 1, constant_values=False)
    inner = fg[:-2, 1:-1] & fg[2:, 1:-1] & fg[1:-1, :-2] & fg[1:-1, 2:]
    return fg[1:-1, 1:-1] & ~inner


def _isqrt16_np(d2: np.ndarray) -> np.ndarray:
    """floor(2^16 sqrt(d2)) = isqrt(d2 << 32), exact: a float64 start corrected by integer comparison."""
    v = d2.astype(np.int64) << 32
    r = np.floor(np.sqrt(d2.astype(np.float64)) * SUM_ONE).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def _ranks(n: int, percentile: float):
    h = float(n - 1) * (percentile / 100.0)
    lo = min(max(int(math.floor(h)), 0), n - 1)
    return lo, min(lo + 1, n - 1)


def _surface_cpu(pred: np.ndarray, target: np.ndarray, Cn: int, percentile: float, tol_d2: Optional[int]) -> np.ndarray:
    B = pred.shape[0]
    table = np.zeros((B, Cn, len(SURFACE_COLUMNS)), dtype=np.int64)
    for b in range(B):
        for c in range(Cn):
            sp, sg = _surface_np(pred[b], c), _surface_np(target[b], c)
            row = table[b, c]
            row[0], row[1] = int(sp.sum()), int(sg.sum())
            if not row[0] or not row[1]:
                continue
            pg, gp = _edt_sq_np(sg)[sp], _edt_sq_np(sp)[sg]
            row[2], row[3] = pg.max(), gp.max()
            row[4], row[5] = _isqrt16_np(pg).sum(), _isqrt16_np(gp).sum()
            if tol_d2 is not None:
                row[6], row[7] = int((pg <= tol_d2).sum()), int((gp <= tol_d2).sum())
            pooled = np.sort(np.concatenate([pg, gp]))
            row[8], row[9] = _ranks(len(pooled), percentile)
            row[10], row[11] = pooled[row[8]], pooled[row[9]]
    return table


# ------------------------------------------------------------------------------------------------ public functions
def _check_extent(what: str, H: int, W: int, B: int) -> None:
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty map")
    if H > MAX_EXTENT or W > MAX_EXTENT:
        raise ValueError(f"{what}: 1 <= H, W <= {MAX_EXTENT}")


def distance_transform_sq(mask: torch.Tensor) -> torch.Tensor:
    """The exact squared Euclidean distance of every pixel of a bool or integer [H,W] or [B,H,W] mask to the nearest zero pixel, int32,
    0 at zero pixels: scipy.ndimage.distance_transform_edt(mask) squared.  An image without a zero pixel gets NO_FEATURE everywhere."""
    if mask.dim() not in (2, 3):
        raise TypeError("distance_transform_sq: [H,W] or [B,H,W] expected")
    m = as_labels(mask.detach())
    m3 = (m if m.dim() == 3 else m[None]).contiguous()
    B, H, W = m3.shape
    _check_extent("distance_transform_sq", H, W, B)
    if not m3.is_cuda:
        a = m3.numpy()
        out = torch.from_numpy(np.stack([_edt_sq_np(a[b] == 0) for b in range(B)]).astype(np.int32))
        return out.reshape(mask.shape)
    dev = m3.device
    out = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    _lib.call("uaps_edt_sq", _lib.EdtCall, dev, _ws, _lib.workspace_bytes("uaps_edt_workspace_bytes", B, H, W),
              B=B, H=H, W=W, mask_dtype=_DTYPE_CODE[m3.dtype], mask=m3.data_ptr(), out=out.data_ptr())
    return out.reshape(mask.shape)


def tolerance_d2(tolerance: Optional[float]) -> Optional[int]:
    """floor(tolerance^2), the integer the kernels compare squared distances with."""
    if tolerance is None:
        return None
    t = float(tolerance)
    if not (t >= 0.0) or math.isinf(t):
        raise ValueError("surface_distances: tolerance is a finite number >= 0")
    return min(int(math.floor(t * t)), 2 ** 62)


def surface_distances(pred: torch.Tensor, target: torch.Tensor, num_classes: int, *, percentile: float = 95.0,
                      tolerance: Optional[float] = None) -> SurfaceResult:
    """The boundary table of integer label maps pred, target [B,H,W] (uint8, int32 or int64; a label outside [0, num_classes) belongs
    to no class).  pred may be [B,C,H,W] float32 scores: their arg-max is taken first, the lowest index among equal scores.
    percentile: of the pooled directed distances (hd95); tolerance: in pixels, for nsd.  Does not synchronise with the host."""
    Cn = int(num_classes)
    if not 1 <= Cn <= MAX_CLASSES:
        raise ValueError(f"surface_distances: 1 <= num_classes <= {MAX_CLASSES}")
    percentile = float(percentile)
    if not 0.0 <= percentile <= 100.0:
        raise ValueError("surface_distances: 0 <= percentile <= 100")
    tol = tolerance_d2(tolerance)
    if target.dim() != 3 or target.dtype not in _DTYPE_CODE:
        raise TypeError("surface_distances: target is a uint8, int32 or int64 [B,H,W] label map")
    B, H, W = target.shape
    _check_extent("surface_distances", H, W, B)
    scores = pred.dim() == 4
    if scores:
        if pred.dtype != torch.float32 or tuple(pred.shape) != (B, Cn, H, W):
            raise TypeError("surface_distances: scores are float32 [B,num_classes,H,W]")
    elif pred.dim() != 3 or pred.dtype not in _DTYPE_CODE or pred.shape != target.shape:
        raise TypeError("surface_distances: pred is a uint8, int32 or int64 label map of the target's shape, or [B,C,H,W] scores")
    if pred.device != target.device:
        raise TypeError("surface_distances: pred and target live on one device")
    pred, target = pred.detach().contiguous(), target.detach().contiguous()
    if not target.is_cuda:
        p = pred.numpy()
        p = p.argmax(axis=1) if scores else p
        table = _surface_cpu(p.astype(np.int64), target.numpy().astype(np.int64), Cn, percentile, tol)
        return SurfaceResult(torch.from_numpy(table), percentile, tolerance)
    dev = target.device
    table = torch.empty((B, Cn, len(SURFACE_COLUMNS)), dtype=torch.int64, device=dev)
    _lib.call("uaps_surface_distances", _lib.SurfaceCall, dev, _ws, _lib.workspace_bytes("uaps_surface_workspace_bytes", B, Cn, H, W),
              B=B, C=Cn, H=H, W=W, target_dtype=_DTYPE_CODE[target.dtype], target=target.data_ptr(),
              pred=None if scores else pred.data_ptr(), pred_scores=pred.data_ptr() if scores else None,
              pred_dtype=0 if scores else _DTYPE_CODE[pred.dtype], percentile_frac=percentile / 100.0,
              has_tolerance=0 if tol is None else 1, tol_d2=0 if tol is None else tol, table=table.data_ptr())
    return SurfaceResult(table, percentile, tolerance)

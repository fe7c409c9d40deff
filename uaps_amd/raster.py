"""Polygon rasterisation on the kernels of csrc/raster.hip: polygon rings back into a label map -- the inverse of `contours.contours`.
It answers what a simplified polygon still covers (the IoU of every simplified defect against its traced pixels), turns COCO /
labelme polygon ground truth into the label maps and class maps that label_instances, match_instances, detection_match,
surface_distances and score_curves(regions=...) take, and closes the loop: rasterize_contours(contours(inst)) reproduces inst.labels.

`rasterize_contours(res)` takes a `contours.ContourResult`, a `simplify.SimplifiedContours` or a `RingSet` (rings_from_polygons,
rings_from_coco) and returns a `RasterResult`.  Exact integers, no float, the same bits from run to run and from both edge forms; one
host read, of the total of bit-plane words, sizes the plane buffer.

Conventions (they are the definition; pycocotools, OpenCV's fillPoly and scikit-image are not dependencies and parity with them is
UNPINNED):
  ring set        points int32 [N,2] as (y, x); ring_offsets int32 [L+1]; rings int64 [L,stride] with the image in column 0 and the
                  label in column 1 -- the arrays of a ContourResult (stride 7).  Coordinates are integers in units of 2^-F pixel,
                  F = frac_bits in 0..4, 0 <= y, x <= 4096 * 2^F (values outside are clamped into that range); F = 0 is the corner
                  lattice of `contours`
  closing         a ring of n points has n edges, the last one closes it; rings of fewer than 3 points, of an image outside [0, B)
                  or of a label outside [1, max_instances] contribute nothing.  Rings may reach outside the H x W frame: clipped
  sample point    pixel (r, c) is sampled at its centre (r + 1/2, c + 1/2)
  crossing rule   int64 throughout, doubled units, s = 2^F: a row's centre is Yc = (2 r + 1) s; an edge A -> B crosses row r iff
                  min(2 ya, 2 yb) <= Yc < max(2 ya, 2 yb) -- half-open, so a vertex on a centre row counts once and horizontal
                  edges never cross.  With (Y0, X0) the doubled endpoint of smaller Y, dy > 0 and dx the doubled differences from
                  it to the other endpoint, num = X0 dy + (Yc - Y0) dx, and the first column at or right of the crossing is
                  c0 = ceil((num - s dy) / (2 s dy)) clamped to [0, W]: a centre exactly on an edge counts as right of it, and a
                  crossing at c0 = W toggles nothing
  fill rule       even-odd per label: pixel (r, c) belongs to label k iff the number of crossings of k's edges in row r with
                  c0 <= c is odd.  Orientation is irrelevant; a hole ring subtracts from its own label; a ring of another label
                  inside the hole is independent
  label map       a pixel takes the LOWEST label that owns it, `background` where none does; overlap[b] counts the pixels of image
                  b owned by more than one label.  With `classes` (a class per label) mask = classes[label], 0 where no label owns
                  the pixel: what label_instances takes for polygon ground truth
  stats           per label: area, the pixels it owns whatever other labels own them too, and inter, those of them where the
                  reference label map equals the label
Deviation from pycocotools: the parts of one COCO object (several polygons in one "segmentation") that overlap XOR under the
even-odd rule; pycocotools takes their union.

CPU tensors take the numpy restatement below (every crossing as a key, one sort, the odd ones paired into runs), as in the other
modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG
from .contours import ContourResult
from .simplify import SimplifiedContours

RASTER_COLUMNS = ("area", "inter")
MAX_EXTENT, MAX_FRAC_BITS, WAVE_ROWS = _lib.RASTER_MAX_EXTENT, _lib.RASTER_MAX_FRAC_BITS, _lib.RASTER_WAVE_ROWS
assert len(RASTER_COLUMNS) == _lib.RASTER_COLUMNS
_ws = _lib.Workspace()


class RingSet(NamedTuple):
    """Polygon rings that did not come from `contours`: points int32 [N,2] as (y, x) in units of 2^-frac_bits pixel; ring_offsets
    int32 [L+1]; rings int64 [L,2], (image, label); classes int64 [B,max_instances], the class of every label (0 where there is
    none); size: (H, W) of the frame or None; frac_bits.  Built on the host (rings_from_polygons, rings_from_coco); to(device)
    moves the four tensors."""
    points: torch.Tensor
    ring_offsets: torch.Tensor
    rings: torch.Tensor
    classes: torch.Tensor
    size: Optional[Tuple[int, int]] = None
    frac_bits: int = 0

    def to(self, device) -> "RingSet":
        return self._replace(points=self.points.to(device), ring_offsets=self.ring_offsets.to(device), rings=self.rings.to(device),
                             classes=self.classes.to(device))


def _frac(frac_bits) -> int:
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or not 0 <= frac_bits <= MAX_FRAC_BITS:
        raise ValueError(f"frac_bits is an integer in [0, {MAX_FRAC_BITS}]")
    return int(frac_bits)


def _size(size, who: str) -> Tuple[int, int]:
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise TypeError(f"{who}: size is (H, W)") from None
    if not (1 <= H <= MAX_EXTENT and 1 <= W <= MAX_EXTENT):
        raise ValueError(f"{who}: 1 <= H, W <= {MAX_EXTENT}")
    return H, W


def quantise_points(yx, frac_bits: int, size=None) -> np.ndarray:
    """Pixel coordinates [n,2] as (y, x), integers or floats, in units of 2^-frac_bits pixel: floor(v 2^F + 0.5) (exact for
    integers), clamped into the frame [0, H 2^F] x [0, W 2^F] -- into 0 .. 4096 2^F without a size.  int32 [n,2]."""
    F = _frac(frac_bits)
    a = np.asarray(yx)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("a ring is an [n,2] array of (y, x)")
    if a.dtype.kind in "iu":
        q = a.astype(np.int64) << F
    elif a.dtype.kind == "f":
        if not np.isfinite(a).all():
            raise ValueError("a ring's coordinates are finite")
        q = np.floor(a.astype(np.float64) * float(1 << F) + 0.5).astype(np.int64)
    else:
        raise TypeError("a ring's coordinates are integers or floats")
    hi = (MAX_EXTENT << F, MAX_EXTENT << F) if size is None else (size[0] << F, size[1] << F)
    return np.stack([np.clip(q[:, 0], 0, hi[0]), np.clip(q[:, 1], 0, hi[1])], axis=1).astype(np.int32)


def _ring_set(rows, B: int, size, F: int, max_instances) -> RingSet:
    """rows: (image, label, class or None, int32 [n,2]) in output order."""
    top = max([r[1] for r in rows], default=0)
    M = max(1, top) if max_instances is None else int(max_instances)
    if M < 1 or top > M:
        raise ValueError(f"max_instances is at least the largest label ({top})")
    classes = np.zeros((B, M), dtype=np.int64)
    for b, k, cls, _ in rows:
        if cls is not None:
            classes[b, k - 1] = cls
    pts = np.concatenate([r[3] for r in rows]) if rows else np.zeros((0, 2), dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(r[3]) for r in rows])]).astype(np.int32)
    rings = np.array([[r[0], r[1]] for r in rows], dtype=np.int64).reshape(-1, 2)
    return RingSet(torch.from_numpy(np.ascontiguousarray(pts, dtype=np.int32)), torch.from_numpy(offsets), torch.from_numpy(rings),
                   torch.from_numpy(classes), size, F)


def rings_from_polygons(polys, frac_bits: int = 0, *, size=None, max_instances: Optional[int] = None) -> RingSet:
    """The RingSet of polygons in the format of ContourResult.polygons(): per image a list of dicts {"label": k, "outer": [rings],
    "holes": [rings]} (a "cls" key, where present, gives the label's class), every ring an [n,2] array of (y, x) in PIXELS.  Integer
    coordinates are taken exactly (lossless: polygons() at frac_bits 0 gives back the traced rings), floats are quantised as
    quantise_points says.  Outer and hole rings are treated alike: the fill is even-odd.  Runs on the host."""
    F = _frac(frac_bits)
    size = None if size is None else _size(size, "rings_from_polygons")
    rows = []
    for b, image in enumerate(polys):
        for rec in image:
            k = int(rec["label"])
            if k < 1:
                raise ValueError("rings_from_polygons: labels start at 1")
            for ring in list(rec.get("outer", ())) + list(rec.get("holes", ())):
                rows.append((b, k, rec.get("cls"), quantise_points(ring, F, size)))
    return _ring_set(rows, len(polys), size, F, max_instances)


def rings_from_coco(annotations, image_ids, category_to_class, frac_bits: int = 4, *, size=None,
                    max_instances: Optional[int] = None) -> RingSet:
    """The RingSet of COCO annotation dicts: image b is image_ids[b]; the annotations of an image are numbered 1, 2, ... in the order
    they come, each a label of class category_to_class(category_id) (a callable or a mapping); every flat [x0, y0, x1, y1, ...] list
    of "segmentation" is one ring.  Coordinates are quantised to 2^-frac_bits pixel (quantise_points) and clamped into the frame
    `size`.  Annotations of other images are skipped; an RLE "segmentation" (a dict) raises.  Overlapping parts of ONE object XOR
    under the even-odd rule -- pycocotools takes their union.  Runs on the host."""
    F = _frac(frac_bits)
    size = None if size is None else _size(size, "rings_from_coco")
    index = {i: b for b, i in enumerate(image_ids)}
    if len(index) != len(image_ids):
        raise ValueError("rings_from_coco: image_ids are distinct")
    count = [0] * len(image_ids)
    rows = []
    for ann in annotations:
        b = index.get(ann["image_id"])
        if b is None:
            continue
        seg = ann["segmentation"]
        if isinstance(seg, dict):
            raise ValueError("rings_from_coco: an RLE segmentation is no polygon (instances.rle_to_mask decodes those)")
        count[b] += 1
        cat = ann["category_id"]
        cls = int(category_to_class(cat) if callable(category_to_class) else category_to_class[cat])
        for flat in seg:
            xy = np.asarray(flat, dtype=np.float64).reshape(-1, 2)
            rows.append((b, count[b], cls, quantise_points(xy[:, ::-1], F, size)))
    return _ring_set(rows, len(image_ids), size, F, max_instances)


class RasterResult(NamedTuple):
    """labels: int64 [B,H,W], the lowest label that owns a pixel, `background` where none does; mask: int64 [B,H,W],
    classes[label] (0 where no label owns the pixel), or None without classes; stats: int64 [B,max_instances,2], columns
    RASTER_COLUMNS; overlap: int64 [B], the pixels owned by more than one label; contours: the input (a ContourResult, a
    SimplifiedContours or a RingSet); reference_area: int64 [B,max_instances], the pixels of every label in the reference, or None
    without one; frac_bits."""
    labels: torch.Tensor
    mask: Optional[torch.Tensor]
    stats: torch.Tensor
    overlap: torch.Tensor
    contours: object
    reference_area: Optional[torch.Tensor]
    frac_bits: int = 0

    def iou(self) -> torch.Tensor:
        """float64 [B,max_instances] on the labels' device: inter / (reference_area + area - inter), NaN where neither side has a
        pixel.  Needs a reference."""
        if self.reference_area is None:
            raise ValueError("RasterResult.iou: rasterised without a reference")
        area, inter = self.stats[..., 0], self.stats[..., 1]
        union = self.reference_area + area - inter
        return torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.full_like(union, float("nan"), dtype=torch.float64))

    def fidelity(self) -> dict:
        """One device-to-host copy: {"iou": float64 ndarray [B,max_instances], "mean": per image the mean IoU over the labels
        with one (NaN without any), "min": likewise the smallest, "overlap": per image the pixels owned by more than one label}."""
        B, M = self.stats.shape[:2]
        packed = torch.cat([self.iou().reshape(-1), self.overlap.double()]).cpu().numpy()
        iou = packed[:B * M].reshape(B, M)
        have = ~np.isnan(iou)
        mean = [float(iou[b][have[b]].mean()) if have[b].any() else math.nan for b in range(B)]
        low = [float(iou[b][have[b]].min()) if have[b].any() else math.nan for b in range(B)]
        return {"iou": iou, "mean": mean, "min": low, "overlap": [int(v) for v in packed[B * M:]]}

    def records(self) -> List[List[dict]]:
        """contours.records() (of a RingSet: one {"label": k} per label with a ring) with `raster_area` and, with a reference,
        `raster_iou` added to each defect."""
        B, M = self.stats.shape[:2]
        if isinstance(self.contours, RingSet):
            rings = self.contours.rings.cpu().numpy()
            recs = [[{"label": int(k)} for k in np.unique(rings[rings[:, 0] == b, 1]) if 1 <= k <= M] for b in range(B)]
        else:
            recs = self.contours.records()
        area = self.stats[..., 0].double()
        cols = [area] if self.reference_area is None else [area, self.iou()]
        host = torch.stack(cols).cpu().numpy()
        for b, rows in enumerate(recs):
            for r in rows:
                k = r["label"]
                if 1 <= k <= M:
                    r["raster_area"] = int(host[0, b, k - 1])
                    if len(cols) == 2:
                        r["raster_iou"] = float(host[1, b, k - 1])
        return recs


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -((-a) // b)


def _raster_cpu(points, offsets, image, label, B, H, W, M, F, reference, classes, background):
    """(labels, mask or None, stats, overlap) as numpy arrays."""
    s, lim = 1 << F, MAX_EXTENT << F
    N, L = len(points), len(image)
    offsets = offsets.astype(np.int64)
    if len(offsets) != L + 1 or (L and (offsets[0] != 0 or offsets[-1] != N or (np.diff(offsets) < 0).any())):
        raise ValueError("rasterize_contours: ring_offsets ascend from 0 to the number of points")
    n = np.diff(offsets)
    ok = (n >= 3) & (image >= 0) & (image < B) & (label >= 1) & (label <= M)
    ring = np.repeat(np.arange(L, dtype=np.int64), n)
    idx = np.arange(N, dtype=np.int64)
    nxt = np.where(idx + 1 == offsets[1:][ring], offsets[:-1][ring], idx + 1) if N else idx
    p = np.clip(points.astype(np.int64), 0, lim) * 2
    ya, xa, yb, xb = p[:, 0], p[:, 1], p[nxt, 0], p[nxt, 1]
    up = ya < yb
    Y0, X0, dy, dx = np.where(up, ya, yb), np.where(up, xa, xb), np.abs(yb - ya), np.where(up, xb - xa, xa - xb)
    ra, rb = np.maximum(_cdiv(Y0 - s, 2 * s), 0), np.minimum((Y0 + dy - s - 1) // (2 * s), H - 1)
    rows = np.where(ok[ring] & (dy > 0), np.maximum(rb - ra + 1, 0), 0) if N else np.zeros(0, dtype=np.int64)
    edge = np.repeat(idx, rows)                                          # one element per (edge, row it crosses)
    r = ra[edge] + (np.arange(len(edge), dtype=np.int64) - np.repeat(np.cumsum(rows) - rows, rows))
    num = X0[edge] * dy[edge] + ((2 * r + 1) * s - Y0[edge]) * dx[edge]
    c0 = np.clip(_cdiv(num - s * dy[edge], 2 * s * dy[edge]), 0, W)
    entry = image[ring[edge]] * M + (label[ring[edge]] - 1)
    # a key per crossing; those that occur an odd number of times, in order, pair up into the runs of one (label, row)
    keys, times = np.unique((entry * H + r) * (W + 1) + c0, return_counts=True)
    odd = keys[(times & 1) == 1]
    first, last = odd[0::2], odd[1::2]
    assert len(first) == len(last) and (first // (W + 1) == last // (W + 1)).all()       # closed rings: an even count a row
    line, length = first // (W + 1), last - first
    which = np.repeat(np.arange(len(line), dtype=np.int64), length)     # one element per owned pixel
    col = first[which] % (W + 1) + (np.arange(len(which), dtype=np.int64) - np.repeat(np.cumsum(length) - length, length))
    e = line[which] // H
    flat, lab = (e // M) * (H * W) + (line[which] % H) * W + col, e % M + 1
    cover = np.bincount(flat, minlength=B * H * W)
    order = np.lexsort((lab, flat))                                     # a pixel's owners together, the lowest label first
    f2 = flat[order]
    lead = np.ones(len(f2), dtype=bool)
    lead[1:] = f2[1:] != f2[:-1]
    paint = np.zeros(B * H * W, dtype=np.int64)
    paint[f2[lead]] = lab[order][lead]
    stats = np.zeros((B * M, 2), dtype=np.int64)
    stats[:, 0] = np.bincount(e, minlength=B * M)
    if reference is not None:
        stats[:, 1] = np.bincount(e[reference.reshape(-1)[flat] == lab], minlength=B * M)
    labels = np.where(paint > 0, paint, background).reshape(B, H, W)
    mask = None
    if classes is not None:
        rowsel = np.repeat(np.arange(B, dtype=np.int64), H * W)
        mask = np.where(paint > 0, classes.reshape(B, M)[rowsel, np.maximum(paint, 1) - 1], 0).reshape(B, H, W)
    return labels, mask, stats.reshape(B, M, 2), (cover.reshape(B, -1) >= 2).sum(axis=1).astype(np.int64)


def _cut(v) -> int:
    """edge_wave_rows as the C ABI takes it: None = the default (0), 0 = every edge by a wave (UAPS_RASTER_ALL_WAVE)."""
    if v is None:
        return 0
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > MAX_EXTENT:
        raise ValueError(f"rasterize_contours: edge_wave_rows is None or an integer in [0, {MAX_EXTENT}]")
    return _lib.RASTER_ALL_WAVE if v == 0 else int(v)


def reference_areas(reference: torch.Tensor, M: int) -> torch.Tensor:
    """int64 [B,M]: the pixels of every label 1..M of an integer label map [B,H,W]."""
    B = reference.shape[0]
    k = reference.reshape(B, -1).to(torch.int64)
    k = torch.where((k >= 1) & (k <= M), k, torch.zeros_like(k))
    return torch.zeros((B, M + 1), dtype=torch.int64, device=reference.device).scatter_add_(1, k, torch.ones_like(k))[:, 1:].contiguous()


def rasterize_contours(res, *, size=None, reference=None, classes=None, background: int = 0,
                       edge_wave_rows: Optional[int] = None) -> RasterResult:
    """The label map of the rings of `res` -- a contours.ContourResult, a simplify.SimplifiedContours or a RingSet -- by the rules of
    the module's docstring: a RasterResult.
    size: (H, W) of the frame; None = the frame of res.instances (of a RingSet: its size).  1 <= H, W <= 4096.
    reference: an integer label map [B,H,W] on the rings' device, or True for res.instances.labels (of a SimplifiedContours: its
    source's): `inter`, reference_area and iou() are taken against it.
    classes: an integer [B,max_instances] tensor, a class per label, or True for the class column of res.instances.table; None = none
    (of a RingSet: its own classes).  With classes the class map `mask` is written too.
    background: the label of the pixels no ring owns.
    edge_wave_rows: an edge that crosses more rows than this is walked by a whole wave (64 by default); 0 = every edge, 4096 = none.
    It changes the time, never a bit.
    ring_offsets must ascend from 0 to the number of points.  The CPU path checks that and raises; the device path does NOT (it
    would cost a host synchronisation): there, points that no ring holds are left out silently -- memory-safe, but not an error.
    One host read (the total of bit-plane words); an input whose rings own no pixel returns without the second launch."""
    src = res.contours if isinstance(res, SimplifiedContours) else res
    inst = None
    if isinstance(src, ContourResult):
        points, offsets, rings, F = src.points, src.ring_offsets, src.rings, 0
        B, M = src.summary.shape[:2]
        inst = (res.source if isinstance(res, SimplifiedContours) else src).instances
        frame = tuple(inst.labels.shape[1:]) if inst is not None and inst.labels.dim() == 3 else None
    elif isinstance(src, RingSet):
        points, offsets, rings, F = src.points, src.ring_offsets, src.rings, _frac(src.frac_bits)
        if src.classes.dim() != 2:
            raise TypeError("rasterize_contours: a RingSet's classes are int64 [B,max_instances]")
        B, M = src.classes.shape
        frame = src.size
        if classes is None:
            classes = src.classes
    else:
        raise TypeError("rasterize_contours: a contours.ContourResult, a simplify.SimplifiedContours or a RingSet expected")
    if points.dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 2 or offsets.dtype != torch.int32 or offsets.dim() != 1 or \
            rings.dtype != torch.int64 or rings.dim() != 2 or rings.shape[1] < 2 or offsets.shape[0] != rings.shape[0] + 1:
        raise TypeError("rasterize_contours: points int32 [N,2], ring_offsets int32 [L+1] and rings int64 [L,stride] expected")
    if size is None and frame is None:
        raise ValueError("rasterize_contours: size=(H, W) is needed")
    H, W = _size(frame if size is None else size, "rasterize_contours")
    if B < 1 or M < 1:
        raise ValueError("rasterize_contours: an empty batch")
    if B * H * W * 8 >= _TOO_BIG or B * M * 16 >= _TOO_BIG:
        raise ValueError("rasterize_contours: labels (B*H*W*8) and sums (B*max_instances*16) below 2 GiB")
    if isinstance(background, bool) or not isinstance(background, (int, np.integer)):
        raise TypeError("rasterize_contours: background is an integer")
    cut = _cut(edge_wave_rows)
    dev = points.device
    if reference is True:
        if inst is None:
            raise ValueError("rasterize_contours: reference=True needs a result with instances")
        reference = inst.labels
    if classes is True:
        if inst is None:
            raise ValueError("rasterize_contours: classes=True needs a result with instances")
        classes = inst.table[:, :, 0]
    ref_area = None
    if reference is not None:
        if not isinstance(reference, torch.Tensor) or reference.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64) or \
                tuple(reference.shape) != (B, H, W) or reference.device != dev:
            raise TypeError(f"rasterize_contours: the reference is an integer [{B},{H},{W}] label map on the rings' device")
        ref_area = inst.table[:, :, 1].contiguous() if inst is not None and reference is inst.labels and inst.table.shape[1] == M \
            else reference_areas(reference, M)
        reference = reference.detach().to(torch.int32).contiguous()
    if classes is not None:
        if not isinstance(classes, torch.Tensor) or classes.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64) or \
                tuple(classes.shape) != (B, M) or classes.device != dev:
            raise TypeError(f"rasterize_contours: classes is an integer [{B},{M}] tensor on the rings' device")
        classes = classes.detach().to(torch.int64).contiguous()
    L, N = rings.shape[0], points.shape[0]
    done = lambda labels, mask, stats, overlap: RasterResult(labels, mask, stats, overlap, res, ref_area, F)
    empty = lambda: done(torch.full((B, H, W), int(background), dtype=torch.int64, device=dev),
                         None if classes is None else torch.zeros((B, H, W), dtype=torch.int64, device=dev),
                         torch.zeros((B, M, 2), dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))
    if L == 0 or N == 0:
        return empty()
    points, offsets, rings = (t.detach().contiguous() for t in (points, offsets, rings))
    if not points.is_cuda:
        r = rings.numpy()
        out = _raster_cpu(points.numpy(), offsets.numpy(), r[:, 0], r[:, 1], B, H, W, M, F,
                          None if reference is None else reference.numpy(), None if classes is None else classes.numpy(), int(background))
        return done(*(None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)) for a in out))
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    need = _lib.workspace_bytes("uaps_raster_workspace_bytes", N, L, B, H, W, M)
    common = dict(B=B, H=H, W=W, max_instances=M, frac_bits=F, ring_stride=rings.shape[1], edge_wave_rows=cut, n_points=N, n_rings=L,
                  points=points.data_ptr(), ring_offsets=offsets.data_ptr(), rings=rings.data_ptr())
    _lib.call("uaps_raster_plan", _lib.RasterCall, dev, _ws, need, totals=totals.data_ptr(), **common)
    words = int(totals[0])                                               # the one host read
    if words == 0:
        return empty()
    if words * 8 >= _TOO_BIG:
        raise ValueError("rasterize_contours: the bit planes of the labels' boxes reach 2 GiB")
    planes = torch.empty(words, dtype=torch.int64, device=dev)
    labels = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    mask = None if classes is None else torch.empty((B, H, W), dtype=torch.int64, device=dev)
    stats = torch.empty((B, M, 2), dtype=torch.int64, device=dev)
    overlap = torch.empty(B, dtype=torch.int64, device=dev)
    _lib.call("uaps_raster_fill", _lib.RasterCall, dev, _ws, need, n_words=words, planes=planes.data_ptr(),
              reference=None if reference is None else reference.data_ptr(), classes=None if classes is None else classes.data_ptr(),
              background=int(background), labels=labels.data_ptr(), mask=None if mask is None else mask.data_ptr(),
              stats=stats.data_ptr(), overlap=overlap.data_ptr(), **common)
    return done(labels, mask, stats, overlap)

"""Splitting of touching defects on the kernels of csrc/split.hip.

Two pits that touch through a narrow neck are one connected component: `label_instances` counts them once and every descriptor and
score after it treats them as one defect.  `split_instances` undoes that with the classical marker rule -- erode every defect to its
cores, grow the cores back inside the defect, cut where the fronts meet (the geodesic zones of influence of the markers; a
marker-controlled watershed on a constant relief).  The result is a pure function of the input: every comparison with it is exact.

The rule (inst: an InstanceResult, the source defects; `connectivity` the one it was labelled with):
  * marker pixels   pixels with labels > 0 where, with radius=r, D >= ceil(r^2) -- D = surface.distance_transform_sq(inst.labels), as
                    shapes.shape_descriptors(thickness=True) forms it (where defects of different classes touch it is the thickness
                    of their union; an image without a background pixel has NO_FEATURE everywhere), or the caller's int32
                    distance= plane -- or, with markers=, where that bool / uint8 plane is non-zero;
  * markers         maximal sets of marker pixels of ONE source label under `connectivity`, with at least min_marker_area pixels;
                    a marker's id is the image-local raster index of its first pixel, plus 1;
  * owners          round 0: a marker's pixels own its id, every other pixel 0.  One synchronous round: every defect pixel with
                    owner 0 takes the smallest non-zero owner among its neighbours of the same source label, all pixels reading the
                    state of the round's start.  The result is the state after min(max_iters, rounds until nothing changes)
                    rounds; converged[b] says whether image b is at the fixed point.  There, every pixel of a defect that holds a
                    marker is owned by the marker nearest to it in geodesic distance inside the defect (chessboard under
                    8-connectivity, city-block under 4), ties going to the marker with the lowest first pixel;
  * pieces          maximal connected sets of equal (source label, owner), numbered and tabulated exactly as label_instances does
                    it.  A defect without a marker stays one piece; at the fixed point a defect with k markers becomes k pieces;
                    with max_iters cut short the still unowned pixels form pieces of their own.

CPU tensors take the numpy restatement below (whole-plane rounds on shifted copies; instances._label_image's union-find for markers
and pieces), as in the other modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_instances, check_plane
from .instances import FIXED_ONE, InstanceResult, _label_cpu, _label_image

MAX_EXTENT, MAX_ITERS, MAX_SUB_ITERS = _lib.SPLIT_MAX_EXTENT, _lib.SPLIT_MAX_ITERS, _lib.SPLIT_MAX_SUB_ITERS
_ws = _lib.Workspace()
_N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
_N8 = _N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


class SplitInstances(InstanceResult):
    """The pieces' InstanceResult as inference.predict_instances(split=) returns it: `.split` holds the SplitResult it came from."""
    split = None


class SplitResult(NamedTuple):
    """instances: the pieces, an ordinary InstanceResult (the class column is the SOURCE defect's class, -1 where the source label has
    no row in source.table); parent: int32 [B,max_instances], the source label of piece k, 0 in empty rows; pieces: int32
    [B,source.max_instances], how many rows of `parent` name each source defect; converged: bool [B]; source: the InstanceResult
    that was split."""
    instances: InstanceResult
    parent: torch.Tensor
    pieces: torch.Tensor
    converged: torch.Tensor
    source: InstanceResult

    def records(self) -> List[List[dict]]:
        """The instance records with `parent` (the source label) and `pieces_of_parent` (how many pieces that source defect has; None
        where its label has no row in the source table) added.  One device-to-host copy."""
        inst = self.instances
        B, M = inst.table.shape[:2]
        Ms = self.pieces.shape[1]
        packed = torch.cat([inst.table.reshape(B, -1), inst.count.to(torch.int64).reshape(B, 1), self.parent.to(torch.int64),
                            self.pieces.to(torch.int64)], dim=1).cpu().numpy()
        out = []
        for b in range(B):
            rows, n = packed[b, :M * 9].reshape(M, 9), int(packed[b, M * 9])
            parent, pieces = packed[b, M * 9 + 1:M * 9 + 1 + M], packed[b, M * 9 + 1 + M:]
            recs = []
            for k in range(min(n, M)):
                r = rows[k]
                area = int(r[1])
                means = [float(r[7 + j]) / FIXED_ONE / area if j < inst.n_maps else None for j in range(2)]
                p = int(parent[k])
                recs.append({"label": k + 1, "cls": int(r[0]), "area": area, "bbox": (int(r[2]), int(r[3]), int(r[4]), int(r[5])),
                             "mean0": means[0], "mean1": means[1], "parent": p,
                             "pieces_of_parent": int(pieces[p - 1]) if 1 <= p <= Ms else None})
            out.append(recs)
        return out


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def radius_d2(radius) -> int:
    """ceil(radius^2) as an exact integer: what the marker rule compares the squared distances with."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError("split_instances: radius is a positive number")
    r = float(radius)
    if not math.isfinite(r) or r <= 0:
        raise ValueError("split_instances: radius is a positive number")
    d2 = math.ceil(Fraction(r) ** 2)
    if d2 >= _TOO_BIG:
        raise ValueError("split_instances: radius^2 < 2^31")
    return int(d2)


def band_rows(H: int, W: int, sub_iters: int = 0) -> Tuple[int, int]:
    """(rows, columns) a tile of the growth kernel owns on an H x W image at `sub_iters` rounds a launch (0: the default)."""
    rows, cols = C.c_int(), C.c_int()
    _lib.check(_lib.lib().uaps_split_band_rows(int(H), int(W), int(sub_iters), C.byref(rows), C.byref(cols)), "uaps_split_band_rows")
    return rows.value, cols.value


def _round(lab: np.ndarray, own: np.ndarray, offsets) -> Tuple[np.ndarray, bool]:
    """One synchronous round on one image: (the new owners, whether any pixel took one)."""
    H, W = lab.shape
    none = np.int64(2 ** 62)
    pl, po = np.pad(lab, 1), np.pad(own, 1)
    best = np.full((H, W), none)
    for dy, dx in offsets:
        nl, no = pl[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], po[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        best = np.minimum(best, np.where((nl == lab) & (no > 0), no, none))
    take = (lab > 0) & (own == 0) & (best < none)
    return np.where(take, best, own), bool(take.any())


def _owners_cpu(lab: np.ndarray, marker: np.ndarray, conn8: bool, min_marker_area: int, max_iters: int) -> Tuple[np.ndarray, bool]:
    """One image: the owner plane int64 [H,W] after the rounds and whether it is a fixed point."""
    H, W = lab.shape
    roots = _label_image(np.where((lab > 0) & marker, lab, 0).astype(np.int64), conn8, 0)
    fg = roots >= 0
    area = np.bincount(roots[fg], minlength=H * W)
    own = np.where(fg & (area[np.where(fg, roots, 0)] >= min_marker_area), roots + 1, 0).reshape(H, W)
    offsets = _N8 if conn8 else _N4
    for _ in range(max_iters):
        new, changed = _round(lab, own, offsets)
        if not changed:
            return own, True
        own = new
    return own, not _round(lab, own, offsets)[1]


def _split_cpu(inst, marker, maps, connectivity, min_marker_area, max_iters, min_area, M) -> SplitResult:
    lab = inst.labels.numpy().astype(np.int64)
    B = lab.shape[0]
    Ms = inst.max_instances
    own = np.zeros_like(lab)
    converged = np.ones(B, dtype=bool)
    for b in range(B):
        own[b], converged[b] = _owners_cpu(lab[b], marker[b], connectivity == 8, min_marker_area, max_iters)
    code = np.where(lab > 0, (lab << 32) | own, 0)
    res = _label_cpu(torch.from_numpy(code), maps, connectivity, 0, min_area, M)
    table, src_table = res.table.numpy(), inst.table.numpy()
    parent = np.zeros((B, M), dtype=np.int32)
    pieces = np.zeros((B, Ms), dtype=np.int32)
    for b in range(B):
        n = min(int(res.count[b]), M)
        src = table[b, :n, 0] >> 32
        parent[b, :n] = src
        known = src <= Ms
        table[b, :n, 0] = np.where(known, src_table[b, np.where(known, src - 1, 0), 0], -1)
        pieces[b] = np.bincount(src[known] - 1, minlength=Ms)
    return SplitResult(res, torch.from_numpy(parent), torch.from_numpy(pieces), torch.from_numpy(converged), inst)


def split_instances(inst: InstanceResult, *, radius=None, distance: Optional[torch.Tensor] = None,
                    markers: Optional[torch.Tensor] = None, maps: Sequence[torch.Tensor] = (), connectivity: int = 8,
                    min_marker_area: int = 1, max_iters: int = 256, min_area: int = 1, max_instances: Optional[int] = None,
                    _sub_iters: int = 0, _band_rows=0) -> SplitResult:
    """The defects of `inst` (instances.label_instances at `connectivity`) cut into the zones of their markers; the module's text has
    the rule.  Exactly one of radius (a positive number; with it optionally distance=, an int32 [B,H,W] plane in the place of
    distance_transform_sq(inst.labels)) and markers (bool / uint8 [B,H,W]).  maps: zero, one or two float32 [B,H,W] tensors summed
    over each piece as label_instances sums them.  Pieces below min_area pixels get label 0 and no row.  max_instances: rows of the
    pieces' table (default: inst's).  1 <= max_iters <= 65536; H, W <= 4096, B*H*W*8 < 2 GiB and a workspace of 24 bytes a pixel
    below 2 GiB.  _sub_iters (rounds a launch, 0..16) and _band_rows (rows, or (rows, columns) of a tile) force what the kernel
    plans by itself; they change no bit of the result.  Does not synchronise with the host."""
    labels, B, H, W, Ms = check_instances("split_instances", inst, MAX_EXTENT)
    if (radius is None) == (markers is None):
        raise ValueError("split_instances: exactly one of radius and markers")
    if distance is not None and radius is None:
        raise ValueError("split_instances: distance= is the plane radius= is compared with")
    d2 = radius_d2(radius) if radius is not None else 0
    if distance is not None:
        distance = check_plane("split_instances", distance, labels)
    if markers is not None:
        if not isinstance(markers, torch.Tensor) or markers.dtype not in (torch.bool, torch.uint8):
            raise TypeError("split_instances: bool or uint8 [B,H,W] markers expected")
        if markers.shape != labels.shape or markers.device != labels.device:
            raise ValueError(f"split_instances: markers {tuple(markers.shape)} on {markers.device}, labels {tuple(labels.shape)} on {labels.device}")
    if isinstance(maps, torch.Tensor):
        maps = (maps,)
    maps = tuple(maps)
    if len(maps) > 2:
        raise ValueError("split_instances: at most two maps")
    for t in maps:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != labels.shape or t.device != labels.device:
            raise TypeError("split_instances: maps are float32 [B,H,W] tensors on the labels' device")
    if connectivity not in (4, 8):
        raise ValueError("split_instances: connectivity is 4 or 8")
    for name, v in (("min_marker_area", min_marker_area), ("min_area", min_area)):
        if not _is_int(v) or v < 1:
            raise ValueError(f"split_instances: {name} is an integer >= 1")
    if not _is_int(max_iters) or not 1 <= max_iters <= MAX_ITERS:
        raise ValueError(f"split_instances: max_iters in 1..{MAX_ITERS}")
    M = Ms if max_instances is None else max_instances
    if not _is_int(M) or M < 1:
        raise ValueError("split_instances: max_instances is an integer >= 1")
    rows, cols = _band_rows if isinstance(_band_rows, (tuple, list)) else (_band_rows, 0)
    if not _is_int(_sub_iters) or not 0 <= _sub_iters <= MAX_SUB_ITERS or not _is_int(rows) or not _is_int(cols) or rows < 0 or cols < 0:
        raise ValueError(f"split_instances: _sub_iters in 0..{MAX_SUB_ITERS}, _band_rows >= 0")
    if B * H * W * 8 >= _TOO_BIG or B * H * W * 24 + B * (H * W // 64 + 8) + 1536 >= _TOO_BIG or B * max(M, Ms) * 72 >= _TOO_BIG:
        raise ValueError("split_instances: B*H*W*8 < 2 GiB, the workspace (24 bytes a pixel) and the tables below 2 GiB")
    min_marker_area, min_area = min(int(min_marker_area), 2 ** 31 - 1), min(int(min_area), 2 ** 31 - 1)
    labels = labels.detach().contiguous()
    src_table = inst.table.detach().contiguous()
    maps = [t.detach().contiguous() for t in maps]
    if radius is not None and distance is None:
        from .surface import distance_transform_sq
        distance = distance_transform_sq(labels)
    if markers is not None:
        markers = markers.detach().contiguous()
        markers = markers.view(torch.uint8) if markers.dtype == torch.bool else markers
    else:
        distance = distance.detach().contiguous()
    if not labels.is_cuda:
        marker = markers.numpy() != 0 if markers is not None else distance.numpy() >= d2
        return _split_cpu(inst._replace(labels=labels, table=src_table), marker, maps, connectivity, min_marker_area, int(max_iters),
                          min_area, int(M))._replace(source=inst)
    dev = labels.device
    out = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    table = torch.empty((B, M, 9), dtype=torch.int64, device=dev)
    parent = torch.empty((B, M), dtype=torch.int32, device=dev)
    pieces = torch.empty((B, Ms), dtype=torch.int32, device=dev)
    converged = torch.empty((B,), dtype=torch.uint8, device=dev)
    _lib.call("uaps_split_instances", _lib.SplitCall, dev, _ws, _lib.workspace_bytes("uaps_split_workspace_bytes", B, H, W),
              B=B, H=H, W=W, connectivity=connectivity, d2=d2, min_marker_area=min_marker_area, max_iters=int(max_iters),
              sub_iters=int(_sub_iters), band_rows=int(rows), tile_cols=int(cols), min_area=min_area, max_instances=int(M),
              source_rows=Ms, source_labels=labels.data_ptr(), source_table=src_table.data_ptr(),
              distance=None if markers is not None else distance.data_ptr(),
              markers=markers.data_ptr() if markers is not None else None,
              map0=maps[0].data_ptr() if len(maps) > 0 else None, map1=maps[1].data_ptr() if len(maps) > 1 else None,
              labels=out.data_ptr(), count=count.data_ptr(), table=table.data_ptr(), parent=parent.data_ptr(),
              pieces=pieces.data_ptr(), converged=converged.data_ptr())
    return SplitResult(InstanceResult(out, count, table, len(maps)), parent, pieces, converged.view(torch.bool), inst)


SPLIT_KEYS = ("radius", "min_marker_area", "max_iters")


def split_keywords(split, what: str) -> dict:
    """The split_instances keywords of a `split` argument of inference: a radius, or a dict with "radius" and any of min_marker_area
    and max_iters.  Checked here, before any forward runs."""
    if isinstance(split, dict):
        kw = dict(split)
        if "radius" not in kw or not set(kw) <= set(SPLIT_KEYS):
            raise ValueError(f"{what}: a split dict holds \"radius\" and any of {SPLIT_KEYS[1:]}")
    else:
        kw = {"radius": split}
    radius_d2(kw["radius"])
    return kw

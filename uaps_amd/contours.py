"""Defect contours on the kernels of csrc/contours.hip: where the EDGE of every defect of a defect list is -- crack-following loops
between the pixels, as closed polygon rings, for overlays, COCO / labelme annotation files and reports.

`contours(inst, connectivity=8)` takes the `labels` of an `instances.InstanceResult` and returns the boundary of every defect as
rings of corner-lattice points, outer rings and hole rings, exact integers, the same bits from run to run.  One host read, of the
two totals (rings, points), sizes the outputs; nothing else synchronises.  `polygons()`, `records()` and `to_coco()` are one
device-to-host copy each.

Conventions (they are the definition; OpenCV, scikit-image and shapely are not dependencies and parity with them is UNPINNED):
  pixel           (y, x) is the closed unit square [x, x + 1] x [y, y + 1]; ring points lie on the corner lattice 0..H x 0..W, as (y, x)
  directed edges  for a label k in [1, max_instances] every unit side between a pixel of k and anything else (another label, 0, a
                  label outside [1, max_instances], the frame) is an edge with the defect on its RIGHT; directions E, S, W, N = 0..3:
                  top side of (y, x) from (y, x) heading E, right side from (y, x + 1) heading S, bottom side from (y + 1, x + 1)
                  heading W, left side from (y + 1, x) heading N.  Outer rings run clockwise on the screen (as the hull does), hole
                  rings counter-clockwise
  successor       the next edge leaves the end vertex of this one; unique but at a saddle vertex (the label on exactly the two
                  diagonal pixels of the 2 x 2 window), where connectivity 8 turns left (d + 3 mod 4: the diagonal pixels stay on
                  one ring) and connectivity 4 right (d + 1: they separate) -- the duality shape_descriptors and fill_holes use
  ring            one cycle of the successor map; length = its unit edges; area2 = sum of x y' - x' y over its edges (> 0 outer,
                  < 0 hole); points = the start vertices of the edges whose direction differs from their predecessor's (a saddle
                  vertex can occur twice; the first point is not repeated; even, at least 4)
  start           the ring's smallest vertex (y, then x): visited once, always a turn; outer rings leave it heading E, holes S
  order           rings by (image, start y, start x, direction of the start edge): a raster order, NOT grouped by label; within a
                  connected defect the outer ring comes first and its holes follow in raster order.  The host methods group by
                  label with a stable sort

CPU tensors take the numpy restatement below (edge planes, a dense key -> id lookup, pointer doubling, one lexsort), as in the other
modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_instances
from .instances import InstanceResult

RING_COLUMNS = ("image", "label", "y", "x", "points", "length", "area2")
CONTOUR_COLUMNS = ("rings", "points", "perimeter", "area2")
MAX_EXTENT = _lib.CONTOUR_MAX_EXTENT
assert len(RING_COLUMNS) == _lib.CONTOUR_RING_COLUMNS and len(CONTOUR_COLUMNS) == _lib.CONTOUR_COLUMNS
_ws = _lib.Workspace()


class ContourResult(NamedTuple):
    """points: int32 [N,2], (y, x); ring_offsets: int32 [L+1]; rings: int64 [L,7], columns RING_COLUMNS; summary: int64
    [B,max_instances,4], columns CONTOUR_COLUMNS, the sums over each label's rings, zero in rows without a pixel; instances: the
    InstanceResult it describes; connectivity: the saddle rule it was traced with; also: what inference.predict_instances would
    have returned without contours= (a hull.HullResult, a shapes.ShapeResult, a skeleton.SkeletonStats) or None; rounds: the
    pointer-doubling rounds that ran (0 on the CPU path's empty input)."""
    points: torch.Tensor
    ring_offsets: torch.Tensor
    rings: torch.Tensor
    summary: torch.Tensor
    instances: InstanceResult
    connectivity: int = 8
    also: Optional[object] = None
    rounds: int = 0

    def _host(self):
        """(rings [L,7], points [N,2], offsets [L+1], count [B]) as int64 arrays: one copy."""
        L, N, B = self.rings.shape[0], self.points.shape[0], self.instances.count.shape[0]
        packed = torch.cat([self.rings.reshape(-1), self.points.reshape(-1).to(torch.int64), self.ring_offsets.to(torch.int64),
                            self.instances.count.to(torch.int64).to(self.rings.device)]).cpu().numpy()
        a, b, c = 7 * L, 7 * L + 2 * N, 7 * L + 2 * N + L + 1
        return packed[:a].reshape(L, 7), packed[a:b].reshape(N, 2), packed[b:c], packed[c:c + B]

    def _grouped(self):
        """Per image a dict label -> the indices of its rings in output order (a stable sort by (image, label)), and the host arrays."""
        rings, points, offsets, count = self._host()
        B, M = self.summary.shape[:2]
        order = np.argsort(rings[:, 0] * (M + 1) + rings[:, 1], kind="stable")
        groups = [dict() for _ in range(B)]
        for r in order:
            groups[int(rings[r, 0])].setdefault(int(rings[r, 1]), []).append(int(r))
        return groups, rings, points, offsets, count

    def polygons(self) -> List[List[dict]]:
        """One device-to-host copy; per image a list with one dict per defect row (the rows of instances.records()):
        {"label": k, "outer": [int32 ndarray [n,2] of (y, x), ...], "holes": [...]}.  "outer" holds every ring of the label with
        area2 > 0 (one for a connected defect), "holes" those with area2 < 0, each in output order.  Holes are NOT attached to
        the outer ring that encloses them."""
        groups, rings, points, offsets, count = self._grouped()
        M = self.summary.shape[1]
        pts = points.astype(np.int32)
        out = []
        for b, by_label in enumerate(groups):
            rows = []
            for k in range(1, min(int(count[b]), M) + 1):
                rec = {"label": k, "outer": [], "holes": []}
                for r in by_label.get(k, ()):
                    rec["outer" if rings[r, 6] > 0 else "holes"].append(pts[offsets[r]:offsets[r + 1]].copy())
                rows.append(rec)
            out.append(rows)
        return out

    def records(self) -> List[List[dict]]:
        """instances.records() -- also.records() where `also` is attached -- with `rings`, `contour_points`, `perimeter_crack` (the
        rings' unit edges: shape_descriptors' crack perimeter) and `holes_traced` (the rings with area2 < 0) added to each defect."""
        recs = self.also.records() if self.also is not None else self.instances.records()
        groups, rings, _, _, _ = self._grouped()
        for b, rows in enumerate(recs):
            for r in rows:
                mine = groups[b].get(r["label"], [])
                r["rings"] = len(mine)
                r["contour_points"] = int(sum(rings[i, 4] for i in mine))
                r["perimeter_crack"] = int(sum(rings[i, 5] for i in mine))
                r["holes_traced"] = int(sum(1 for i in mine if rings[i, 6] < 0))
        return recs

    def to_coco(self, image_ids=None, category_of=None) -> List[dict]:
        """One device-to-host copy (and instances.records()'s); a list of COCO annotation dicts, one per defect row, ids from 1:
        "image_id" image_ids[b] (b itself without image_ids), "category_id" category_of(cls) -- a callable or a mapping; the
        class itself without one -- "segmentation" one flat [x0, y0, x1, y1, ...] list per OUTER ring, "bbox" [x, y, w, h] of
        those, "area" the pixel count (half the sum of area2 over ALL rings of the label), "iscrowd" 0.
        Limitation: COCO's polygon format cannot subtract holes.  A defect with hole rings gets "iscrowd" 1 and still only its
        outer polygons; the RLE mask COCO expects for crowd regions (instances.mask_to_rle / format_rle) is not emitted here."""
        groups, rings, points, offsets, _ = self._grouped()
        recs = self.instances.records()
        out = []
        for b, rows in enumerate(recs):
            for rec in rows:
                mine = groups[b].get(rec["label"], [])
                outer = [points[offsets[i]:offsets[i + 1]] for i in mine if rings[i, 6] > 0]
                if not outer:
                    continue
                allp = np.concatenate(outer)
                y0, x0, y1, x1 = int(allp[:, 0].min()), int(allp[:, 1].min()), int(allp[:, 0].max()), int(allp[:, 1].max())
                cls = rec["cls"]
                cat = cls if category_of is None else (category_of(cls) if callable(category_of) else category_of[cls])
                out.append({"id": len(out) + 1, "image_id": b if image_ids is None else image_ids[b], "category_id": cat,
                            "segmentation": [[float(v) for yx in p for v in (yx[1], yx[0])] for p in outer],
                            "bbox": [float(x0), float(y0), float(x1 - x0), float(y1 - y0)],
                            "area": float(sum(int(rings[i, 6]) for i in mine)) / 2.0,
                            "iscrowd": 1 if any(rings[i, 6] < 0 for i in mine) else 0})
        return out


_DY = np.array([0, 1, 0, -1], dtype=np.int64)
_DX = np.array([1, 0, -1, 0], dtype=np.int64)


def _trace_image(lab: np.ndarray, M: int, conn8: bool):
    """One image: (rings [L,7] with column 0 left zero, points [N,2], rounds)."""
    H, W = lab.shape
    P = np.zeros((H + 2, W + 2), dtype=np.int64)
    P[1:-1, 1:-1] = np.where((lab >= 1) & (lab <= M), lab, 0)
    a, b, c, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]         # NW, NE, SW, SE of vertex (Y, X): [H+1, W+1] each
    exist = np.stack([(d > 0) & (b != d), (c > 0) & (d != c), (a > 0) & (c != a), (b > 0) & (a != b)], axis=-1).reshape(-1)
    owner = np.stack([d, c, a, b], axis=-1).reshape(-1)
    keys = np.nonzero(exist)[0]                                          # dense keys (vertex * 4 + direction), ascending: the edge ids
    E = len(keys)
    if E == 0:
        return np.zeros((0, 7), dtype=np.int64), np.zeros((0, 2), dtype=np.int64), 0
    ident = np.cumsum(exist) - 1                                        # dense key -> id where an edge exists
    direction, vertex = keys & 3, keys >> 2
    Y, X = vertex // (W + 1), vertex % (W + 1)
    k = owner[keys]
    end = (Y + _DY[direction]) * (W + 1) + X + _DX[direction]
    succ = np.full(E, -1, dtype=np.int64)
    first = 3 if conn8 else 1
    for turn in (4 - first, 0, first):                                  # the last assignment wins: the preferred turn goes last
        key2 = end * 4 + ((direction + turn) & 3)
        ok = exist[key2] & (owner[key2] == k)
        succ = np.where(ok, ident[key2], succ)
    ids = np.arange(E, dtype=np.int64)
    prev = np.empty(E, dtype=np.int64)
    prev[succ] = ids
    # pointer doubling along the predecessors: (the smallest id among the 2^r edges that end here, how far back it lies)
    low, back, jump, hop, rounds = ids.copy(), np.zeros(E, dtype=np.int64), prev.copy(), 1, 0
    while True:
        rounds += 1
        better = low[jump] < low
        if not better.any():
            break
        low, back, jump, hop = np.where(better, low[jump], low), np.where(better, back[jump] + hop, back), jump[jump], hop * 2
    order = np.lexsort((back, low))                                     # ring after ring (leaders ascend), by rank inside
    starts = np.nonzero(back[order] == 0)[0]
    turns = (direction[prev] != direction)[order]
    term = np.where(direction == 0, -Y, np.where(direction == 1, X, np.where(direction == 2, Y, -X)))[order]
    lead = order[starts]
    rings = np.zeros((len(starts), 7), dtype=np.int64)
    rings[:, 1], rings[:, 2], rings[:, 3] = k[lead], Y[lead], X[lead]
    rings[:, 4] = np.add.reduceat(turns.astype(np.int64), starts)
    rings[:, 5] = np.diff(np.append(starts, E))
    rings[:, 6] = np.add.reduceat(term, starts)
    at = order[turns]
    return rings, np.stack([Y[at], X[at]], axis=1), rounds


def _contours_cpu(labels: np.ndarray, M: int, connectivity: int):
    B = labels.shape[0]
    summary = np.zeros((B, M, 4), dtype=np.int64)
    all_rings, all_points, rounds = [], [], 0
    for b in range(B):
        rings, points, r = _trace_image(labels[b], M, connectivity == 8)
        rings[:, 0] = b
        rounds = max(rounds, r)
        np.add.at(summary[b], rings[:, 1] - 1, np.stack([np.ones(len(rings), dtype=np.int64), rings[:, 4], rings[:, 5], rings[:, 6]], axis=1))
        all_rings.append(rings)
        all_points.append(points)
    rings, points = np.concatenate(all_rings), np.concatenate(all_points).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(rings[:, 4])]).astype(np.int32)
    return points, offsets, rings, summary, rounds


def contours(inst: InstanceResult, connectivity: int = 8) -> ContourResult:
    """The boundary rings of the defects of `inst` (instances.label_instances, inference.predict_instances): a ContourResult.
    connectivity: the saddle rule, 8 or 4 -- the one `inst` was labelled with gives every defect exactly one outer ring.  Labels
    outside [1, max_instances] bound other labels' rings and have none of their own.
    1 <= H, W <= 4096, B*H*W*32 < 2 GiB (a workspace of about 192 bytes a pixel, every array of it below 2 GiB) and a summary below
    2 GiB.  One host read (the totals); an input without a labelled pixel returns empty tensors without a second launch."""
    labels, B, H, W, M = check_instances("contours", inst, MAX_EXTENT)
    if connectivity not in (4, 8):
        raise ValueError("contours: connectivity is 4 or 8")
    if B * H * W * 32 >= _TOO_BIG or B * M * 32 >= _TOO_BIG:
        raise ValueError("contours: B*H*W*32 < 2 GiB and a summary below 2 GiB")
    labels = labels.detach().contiguous()
    if not labels.is_cuda:
        points, offsets, rings, summary, rounds = _contours_cpu(labels.numpy(), M, connectivity)
        return ContourResult(torch.from_numpy(points), torch.from_numpy(offsets), torch.from_numpy(rings), torch.from_numpy(summary),
                             inst, connectivity, None, rounds)
    dev = labels.device
    summary = torch.empty((B, M, 4), dtype=torch.int64, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    need = _lib.workspace_bytes("uaps_contours_workspace_bytes", B, H, W, M)
    common = dict(B=B, H=H, W=W, max_instances=M, connectivity=connectivity, labels=labels.data_ptr())
    _lib.call("uaps_contours_trace", _lib.ContourCall, dev, _ws, need, summary=summary.data_ptr(), totals=totals.data_ptr(), **common)
    L, N, rounds, _ = (int(v) for v in totals.tolist())                 # the one host read
    points = torch.empty((N, 2), dtype=torch.int32, device=dev)
    offsets = torch.zeros(1, dtype=torch.int32, device=dev) if L == 0 else torch.empty(L + 1, dtype=torch.int32, device=dev)
    rings = torch.empty((L, 7), dtype=torch.int64, device=dev)
    if L > 0:
        _lib.call("uaps_contours_write", _lib.ContourCall, dev, _ws, need, n_rings=L, n_points=N, ring_capacity=L, point_capacity=N,
                  points=points.data_ptr(), ring_offsets=offsets.data_ptr(), rings=rings.data_ptr(), **common)
    return ContourResult(points, offsets, rings, summary, inst, connectivity, None, rounds)

"""Defect convex hulls on the kernels of csrc/hull.hip: what a row of the defect list says about a defect's EXTENT -- how long it
is between its two farthest points, how wide under a caliper, the tightest rotated box around it, and how much of its hull it fills.

`hull_descriptors(inst)` takes the `labels` of an `instances.InstanceResult` and returns, per defect, seventeen exact integers
(HULL_COLUMNS): the number of strict hull vertices, twice the hull area, the farthest pair of vertices, and the edges that minimise
the caliper width and the area of the flush rectangle.  Nothing in it synchronises with the host.  `HullResult.props()` is the one
device-to-host copy.

Conventions (they are the definition; scikit-image and OpenCV are not dependencies and parity with them is UNPINNED):
  pixel           (y, x) is the closed unit square [x, x + 1] x [y, y + 1]; a one-pixel defect has 4 vertices, hull area 1, maximum
                  Feret diameter sqrt(2) and width 1 -- no defect is degenerate
  hull            of the squares of ALL pixels that carry the label, connected or not; vertices on the corner lattice 0..W x 0..H;
                  only strict vertices count
  order           from the smallest vertex (y, then x) along the horizontal top edge towards +x: clockwise on the screen
  edge i          from v_i to v_{i+1} with e = (ex, ey);  c(p) = ex (py - vy) - ey (px - vx) >= 0 on the hull: the distance from the
                  edge's line times |e|;  d(p) = ex (px - vx) + ey (py - vy): the position along the edge times |e|
  Feret pair      (y0, x0) < (y1, x1) lexicographically; among tied pairs the smallest (y0, x0, y1, x1)
  width           the edge that minimises C^2 / |e|^2, C the largest c over the vertices; feret_min = w_c / |e|
  rectangle       the edge that minimises (dmax - dmin) C / |e|^2; flush with that edge
  ties            both minimisations compare the fractions exactly; the edge with the lowest index wins
  angles          of an undirected line, in (-pi/2, pi/2], from +x towards +y (rows grow downwards), as shapes' `orientation`

CPU tensors take the numpy restatement below (row extents, monotone chain, Python-integer comparisons), as in the other modules;
on a ROCm device a missing kernel is an error."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_instances
from .instances import InstanceResult, add_props, host_tables

HULL_COLUMNS = ("nv", "area2", "fmax_sq", "f_y0", "f_x0", "f_y1", "f_x1", "w_ey", "w_ex", "w_c",
                "r_y", "r_x", "r_ey", "r_ex", "r_dmin", "r_dmax", "r_c")
MAX_EXTENT = _lib.HULL_MAX_EXTENT
assert len(HULL_COLUMNS) == _lib.HULL_COLUMNS
_ws = _lib.Workspace()

PROPS = ("hull_vertices", "hull_area", "solidity", "feret_max", "feret_max_angle", "feret_min", "feret_min_angle", "feret_aspect",
         "rect_length", "rect_width", "rect_area", "rect_angle", "rect_cy", "rect_cx", "rectangularity")


def _axis_angle(dx: int, dy: int) -> float:
    """The angle in (-pi/2, pi/2] of the undirected line along (dx, dy), from +x towards +y."""
    if dx < 0 or (dx == 0 and dy < 0):
        dx, dy = -dx, -dy
    return math.atan2(float(dy), float(dx))


class HullResult(NamedTuple):
    """table: int64 [B,max_instances,17], columns HULL_COLUMNS, zero in rows without a pixel; instances: the InstanceResult it
    describes; also: what inference.predict_instances would have returned without hull= (a shapes.ShapeResult, a
    skeleton.SkeletonStats) or None."""
    table: torch.Tensor
    instances: InstanceResult
    also: Optional[object] = None

    def props(self) -> Dict[str, np.ndarray]:
        """One device-to-host copy; a dict of float64 arrays [B,max_instances], NaN in rows without a component.  Every value is a
        few correctly rounded float64 operations on the exact integers; with A = area, E = w_ex^2 + w_ey^2 of the width edge,
        F = r_ex^2 + r_ey^2 and D = r_dmax - r_dmin of the rectangle edge:
          hull_vertices = nv;  hull_area = area2 / 2;  solidity = 2 A / area2
          feret_max = sqrt(fmax_sq);  feret_max_angle: the line through the pair
          feret_min = w_c / sqrt(E);  feret_min_angle: the direction the width is measured in, the normal (-w_ey, w_ex) of the edge
          feret_aspect = feret_min / feret_max
          rect_length, rect_width = the larger and the smaller of D / sqrt(F) and r_c / sqrt(F);  rect_area = D r_c / F
          rect_angle: the longer side's -- the edge's where D >= r_c, else its normal's
          rect_cy = (2 F r_y + (r_dmin + r_dmax) r_ey + r_c r_ex) / (2 F),  rect_cx = (2 F r_x + (r_dmin + r_dmax) r_ex - r_c r_ey) / (2 F)
          rectangularity = A F / (D r_c)"""
        hl, tb = host_tables(self.table, self.instances)
        B, M = hl.shape[:2]
        out = {n: np.full((B, M), np.nan, dtype=np.float64) for n in PROPS}
        for b in range(B):
            for k in range(M):
                A = int(tb[b, k, 1])
                if A <= 0 or int(hl[b, k, 0]) <= 0:
                    continue
                nv, area2, fsq, fy0, fx0, fy1, fx1, wey, wex, wc, ry, rx, rey, rex, dmin, dmax, rc = (int(v) for v in hl[b, k])
                E, F, D = wex * wex + wey * wey, rex * rex + rey * rey, dmax - dmin
                put = lambda name, v: out[name].__setitem__((b, k), v)
                put("hull_vertices", float(nv)); put("hull_area", area2 / 2); put("solidity", (2 * A) / area2)
                fmax, fmin = math.sqrt(fsq), wc / math.sqrt(E)
                put("feret_max", fmax); put("feret_max_angle", _axis_angle(fx1 - fx0, fy1 - fy0))
                put("feret_min", fmin); put("feret_min_angle", _axis_angle(-wey, wex))
                put("feret_aspect", fmin / fmax)
                root = math.sqrt(F)
                along, across = D / root, rc / root
                put("rect_length", max(along, across)); put("rect_width", min(along, across))
                put("rect_area", (D * rc) / F)
                put("rect_angle", _axis_angle(rex, rey) if D >= rc else _axis_angle(-rey, rex))
                put("rect_cy", (2 * F * ry + (dmin + dmax) * rey + rc * rex) / (2 * F))
                put("rect_cx", (2 * F * rx + (dmin + dmax) * rex - rc * rey) / (2 * F))
                put("rectangularity", (A * F) / (D * rc))
        return out

    def rect_corners(self) -> np.ndarray:
        """One device-to-host copy; float64 [B,max_instances,4,2]: the minimum-area rectangle's corners as (y, x), in hull order
        (from the corner behind the edge's start along the edge, then across the defect), for drawing; NaN in rows without a
        component.  The corner at (d, c) is (r_y, r_x) + (d (r_ey, r_ex) + c (r_ex, -r_ey)) / F, each coordinate one division."""
        hl, tb = host_tables(self.table, self.instances)
        B, M = hl.shape[:2]
        out = np.full((B, M, 4, 2), np.nan, dtype=np.float64)
        for b in range(B):
            for k in range(M):
                if int(tb[b, k, 1]) <= 0 or int(hl[b, k, 0]) <= 0:
                    continue
                ry, rx, rey, rex, dmin, dmax, rc = (int(v) for v in hl[b, k, 10:17])
                F = rex * rex + rey * rey
                for j, (d, c) in enumerate(((dmin, 0), (dmax, 0), (dmax, rc), (dmin, rc))):
                    out[b, k, j, 0] = (F * ry + d * rey + c * rex) / F
                    out[b, k, j, 1] = (F * rx + d * rex - c * rey) / F
        return out

    def records(self) -> List[List[dict]]:
        """instances.records() -- also.records() where `also` is attached -- with every key of props() added to each defect."""
        return add_props(self.also.records() if self.also is not None else self.instances.records(), self.props())


def _strict_chain(points):
    """The monotone-chain rule over points (x, y) given in hull order: b stays between a and c only where c_ab(c) > 0."""
    st = []
    for c in points:
        while len(st) >= 2:
            a, b = st[-2], st[-1]
            if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) > 0:
                break
            st.pop()
        st.append(c)
    return st


def _measure(V) -> List[int]:
    """The 17 columns of the strict vertices V, (x, y) in hull order."""
    nv = len(V)
    x = np.array([p[0] for p in V], dtype=np.int64)
    y = np.array([p[1] for p in V], dtype=np.int64)
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    area2 = int((x * yn - xn * y).sum())
    d2 = (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2
    fsq = int(d2.max())
    pair = min(tuple(sorted(((int(y[i]), int(x[i])), (int(y[j]), int(x[j]))))) for i, j in np.argwhere(np.triu(d2 == fsq, 1)))
    ex, ey = xn - x, yn - y
    px, py = x[None, :] - x[:, None], y[None, :] - y[:, None]           # [edge, vertex]: p - v
    c = ex[:, None] * py - ey[:, None] * px
    d = ex[:, None] * px + ey[:, None] * py
    cm, dmin, dmax = c.max(axis=1), d.min(axis=1), d.max(axis=1)
    e2 = ex * ex + ey * ey
    best_w = best_r = None
    for i in range(nv):
        C, E, D = int(cm[i]), int(e2[i]), int(dmax[i] - dmin[i])
        if best_w is None or C * C * best_w[1] < best_w[0] * E:         # strict: ties stay with the lower index
            best_w = (C * C, E, i)
        if best_r is None or D * C * best_r[1] < best_r[0] * E:
            best_r = (D * C, E, i)
    w, r = best_w[2], best_r[2]
    return [nv, area2, fsq, pair[0][0], pair[0][1], pair[1][0], pair[1][1], int(ey[w]), int(ex[w]), int(cm[w]),
            int(y[r]), int(x[r]), int(ey[r]), int(ex[r]), int(dmin[r]), int(dmax[r]), int(cm[r])]


def _hull_cpu(labels: np.ndarray, M: int) -> np.ndarray:
    """The table on the host: per image the column extents of every (label, row) by np.minimum.at / np.maximum.at, then per label the
    two chains of lattice-line extremes, reduced by the monotone-chain rule, and the columns from exact integers."""
    B, H, W = labels.shape
    table = np.zeros((B, M, 17), dtype=np.int64)
    for b in range(B):
        lab = labels[b]
        y, x = np.nonzero((lab >= 1) & (lab <= M))
        if len(y) == 0:
            continue
        k = lab[y, x].astype(np.int64) - 1
        present = np.unique(k)
        slot = np.full(M, -1, dtype=np.int64)
        slot[present] = np.arange(len(present))
        xmin = np.full((len(present), H), W, dtype=np.int64)
        xmax = np.full((len(present), H), -1, dtype=np.int64)
        np.minimum.at(xmin, (slot[k], y), x)
        np.maximum.at(xmax, (slot[k], y), x)
        for s, kk in enumerate(present):
            has = xmax[s] >= 0
            rows = np.nonzero(has)[0]
            y0, y1 = int(rows[0]), int(rows[-1])
            left, right = [], []
            for Y in range(y0, y1 + 2):
                cand = [r for r in (Y - 1, Y) if y0 <= r <= y1 and has[r]]
                if cand:
                    left.append((min(int(xmin[s, r]) for r in cand), Y))
                    right.append((max(int(xmax[s, r]) for r in cand) + 1, Y))
            rc, lc = _strict_chain(right), _strict_chain(left[::-1])
            table[b, kk] = _measure([lc[-1]] + rc + lc[:-1])
    return table


def hull_descriptors(inst: InstanceResult) -> HullResult:
    """The hull table of the defects of `inst` (instances.label_instances, inference.predict_instances): int64
    [B,max_instances,17], columns HULL_COLUMNS, row k - 1 of image b for the pixels labelled k; rows without a pixel are zero.
    The hull is that of the label's pixels wherever they are: the instance table's box is not consulted.
    1 <= H, W <= 4096, B*H*W*8 < 2 GiB, and a table and a workspace (B * max_instances * (H + 1) * 8 bytes) below 2 GiB.
    Does not synchronise with the host."""
    labels, B, H, W, M = check_instances("hull_descriptors", inst, MAX_EXTENT)
    if B * H * W * 8 >= _TOO_BIG or B * M * 136 >= _TOO_BIG or B * M * (H + 1) * 8 + 256 >= _TOO_BIG:
        raise ValueError("hull_descriptors: B*H*W*8 < 2 GiB, and a table and a workspace below 2 GiB")
    labels = labels.detach().contiguous()
    if not labels.is_cuda:
        return HullResult(torch.from_numpy(_hull_cpu(labels.numpy(), M)), inst)
    dev = labels.device
    table = torch.empty((B, M, 17), dtype=torch.int64, device=dev)
    _lib.call("uaps_hull_descriptors", _lib.HullCall, dev, _ws, _lib.workspace_bytes("uaps_hull_workspace_bytes", B, H, W, M),
              B=B, H=H, W=W, max_instances=M, labels=labels.data_ptr(), table=table.data_ptr())
    return HullResult(table, inst)

"""Contour simplification on the kernels of csrc/simplify.hip: exact Ramer-Douglas-Peucker on the rings of `contours.contours`, so
that a slanted edge of n pixels is two points and not a staircase of 2 n -- for annotation files and overlays.

`simplify_contours(res, epsilon=1.0)` takes a `contours.ContourResult` and returns a `SimplifiedContours` whose `.contours` is a
ContourResult of the kept points.  Exact integers, no float, the same bits from run to run and from every kernel form; one host
read, of the total of kept points, sizes the output.

Conventions (they are the definition; OpenCV's approxPolyDP and shapely are not dependencies and parity with them is UNPINNED):
  ring            n >= 4 points p_0 .. p_{n-1}, p_0 its start vertex; index n means p_0 again; coordinates in 0 .. contours.MAX_EXTENT
  tolerance       epsilon, a float in pixels, 0 <= epsilon <= 64, quantised on the host to sixteenths: e16 = floor(16 epsilon + 0.5);
                  everything else uses e16, and the result reports epsilon16 and epsilon = e16 / 16
  deviation       of a point P from the SEGMENT (not the line) A -> B, a fraction num / den of squared pixels; with d = B - A,
                  L2 = |d|^2, t = (P - A) . d:   L2 == 0 (two visits of a saddle vertex): num = |P - A|^2, den = 1;
                  t <= 0: num = |P - A|^2 L2, den = L2;   t >= L2: num = |P - B|^2 L2, den = L2;   otherwise num = cross(d, P - A)^2,
                  den = L2.  |P - A|^2, L2 and |cross| are at most 2^25, so num <= 2^50 and every comparison stays inside int64
  exceeds         P exceeds the tolerance where 256 num > e16^2 den; the comparison is strict
  split rule      for an interval (i, j) with j > i + 1: the interior index k with the largest num (den is common to them), the
                  lowest k among the equal; if it exceeds the tolerance k is kept and the rule goes on in (i, k) and (k, j),
                  otherwise nothing inside is kept.  The result does not depend on the order the intervals are taken in
  closed rings    anchor a = 0, anchor b = the index with the largest |p_i - p_0|^2 (the lowest among the equal); the split rule
                  runs on (0, b) and (b, n)
  triangle        if neither top-level interval splits, the index with the largest num over both (they share A, B and den; the
                  lowest among the equal) is kept all the same, and the rule goes on in its two halves like after any other
                  split -- so that every dropped point stays within the tolerance of the segment between the kept points that
                  bracket it.  Its num is > 0 because a traced ring has a non-zero area: a simplified ring has at least three
                  points that are not collinear
  output          the kept points of a ring in source order, p_0 first; rings keep their order
NOT promised: a simplified ring may touch or cross itself or another ring, and the sign of its own area is not guaranteed.  Outer /
hole classification therefore keeps using the SOURCE ring's area2.

CPU tensors take the numpy restatement below (an explicit stack per ring), as in the other modules; on a ROCm device a missing
kernel is an error."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .contours import ContourResult, MAX_EXTENT

WAVE_MAX, LDS_MAX, MAX_E16 = _lib.SIMPLIFY_WAVE_MAX, _lib.SIMPLIFY_LDS_MAX, _lib.SIMPLIFY_MAX_E16
_ws = _lib.Workspace()


class SimplifiedContours(NamedTuple):
    """contours: a ContourResult of the kept points -- new points and ring_offsets; rings equal to the source's but column `points`
    (the kept count): length and area2 stay the exact values of the traced ring, they describe the defect, and polygons() /
    to_coco() classify outer and hole rings by them; summary with its `points` column recomputed; instances, connectivity, also
    and rounds carried over.  source: the input.  epsilon16: the tolerance in sixteenths of a pixel; epsilon = epsilon16 / 16.
    ring_stats: int64 [L,2] on the device, (points of the source ring, area2 of the simplified ring).
    A simplified ring may touch or cross itself or another ring, and the sign of its own area is not guaranteed."""
    contours: ContourResult
    source: ContourResult
    epsilon: float
    epsilon16: int
    ring_stats: torch.Tensor

    def polygons(self) -> List[List[dict]]:
        """contours.polygons(): the simplified rings, outer / hole by the source ring's area2."""
        return self.contours.polygons()

    def records(self) -> List[List[dict]]:
        """contours.records(): `contour_points` counts the kept points; `perimeter_crack` stays the traced rings'."""
        return self.contours.records()

    def to_coco(self, image_ids=None, category_of=None) -> List[dict]:
        """contours.to_coco(): "segmentation" the simplified outer rings, "bbox" the box of the polygons emitted, "area" still the
        pixel count."""
        return self.contours.to_coco(image_ids, category_of)

    def reduction(self) -> dict:
        """One device-to-host copy: {"source_points", "points", "ratio" (kept / source, 1.0 without a point), "per_image": a list
        of (source points, kept points) per image}."""
        B = self.contours.summary.shape[0]
        packed = torch.cat([self.ring_stats[:, 0], self.contours.rings[:, 4], self.contours.rings[:, 0]]).cpu().numpy()
        L = self.ring_stats.shape[0]
        src, kept, image = packed[:L], packed[L:2 * L], packed[2 * L:]
        per = [(int(src[image == b].sum()), int(kept[image == b].sum())) for b in range(B)]
        total, left = int(src.sum()), int(kept.sum())
        return {"source_points": total, "points": left, "ratio": left / total if total else 1.0, "per_image": per}


def quantise(epsilon) -> int:
    """e16 = floor(16 epsilon + 0.5) of a tolerance in pixels; anything but a number in [0, 64] raises."""
    if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float, np.integer, np.floating)):
        raise TypeError("simplify_contours: epsilon is a number of pixels")
    e = float(epsilon)
    if math.isnan(e) or e < 0.0 or e > 64.0:
        raise ValueError("simplify_contours: 0 <= epsilon <= 64")
    return int(math.floor(16.0 * e + 0.5))


def _nums(p: np.ndarray, i: int, j: int, n: int):
    """(num of the interior indices i + 1 .. j - 1 against the segment p_i -> p_j, den)."""
    a, b = p[i], p[j % n]
    q = p[i + 1:j] - a
    d = b - a
    L2 = int(d[0] * d[0] + d[1] * d[1])
    q2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
    if L2 == 0:
        return q2, 1
    t = q[:, 0] * d[0] + q[:, 1] * d[1]
    r = p[i + 1:j] - b
    cross = d[1] * q[:, 0] - d[0] * q[:, 1]
    return np.where(t <= 0, q2 * L2, np.where(t >= L2, (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) * L2, cross * cross)), L2


def _simplify_ring(p: np.ndarray, tol: int) -> np.ndarray:
    """The kept indices of one ring (int64 [n,2] points), ascending; tol = e16^2."""
    n = len(p)
    if n < 3:
        return np.arange(n)
    far = p[1:] - p[0]
    b = 1 + int(np.argmax(far[:, 0] * far[:, 0] + far[:, 1] * far[:, 1]))            # (argmax: the first of the equal)
    keep = np.zeros(n, dtype=bool)
    keep[0] = keep[b] = True
    stack, top = [], []
    for (i, j) in ((0, b), (b, n)):
        if j > i + 1:
            num, den = _nums(p, i, j, n)
            assert int(num.max()) <= 1 << 50 and den <= 1 << 25
            k = int(np.argmax(num))
            top.append((int(num[k]), i + 1 + k, den, i, j))
    if not any(256 * m > tol * den for m, _, den, _, _ in top):                       # never below a triangle
        m, k, _, i, j = max(top, key=lambda c: (c[0], -c[1]))
        if m > 0:
            keep[k] = True
            stack += [(i, k), (k, j)]
    else:
        for m, k, den, i, j in top:
            if 256 * m > tol * den:
                keep[k] = True
                stack += [(i, k), (k, j)]
    while stack:
        i, j = stack.pop()
        if j <= i + 1:
            continue
        num, den = _nums(p, i, j, n)
        k = int(np.argmax(num))
        if 256 * int(num[k]) > tol * den:
            keep[i + 1 + k] = True
            stack += [(i, i + 1 + k), (i + 1 + k, j)]
    return np.nonzero(keep)[0]


def _simplify_cpu(points: np.ndarray, offsets: np.ndarray, rings: np.ndarray, summary: np.ndarray, e16: int):
    assert 0 <= e16 <= MAX_E16 and (points.size == 0 or (points.min() >= 0 and points.max() <= MAX_EXTENT))    # num <= 2^50
    pts = points.astype(np.int64)
    L = len(rings)
    out, counts, stats = [], np.zeros(L, dtype=np.int64), np.zeros((L, 2), dtype=np.int64)
    for r in range(L):
        p = pts[offsets[r]:offsets[r + 1]]
        q = p[_simplify_ring(p, e16 * e16)]
        nxt = np.roll(q, -1, axis=0)
        counts[r] = len(q)
        stats[r] = (len(p), int((q[:, 1] * nxt[:, 0] - nxt[:, 1] * q[:, 0]).sum()))
        out.append(q)
    new_rings = rings.copy()
    new_rings[:, 4] = counts
    new_summary = summary.copy()
    M = summary.shape[1]
    ok = (rings[:, 1] >= 1) & (rings[:, 1] <= M)
    np.add.at(new_summary[..., 1], (rings[ok, 0], rings[ok, 1] - 1), counts[ok] - stats[ok, 0])
    new_points = (np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)).astype(np.int32)
    new_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return new_points, new_offsets, new_rings, new_summary, stats


def _threshold(v, cap: int, what: str) -> int:
    """A form's threshold as the C ABI takes it: None = the default (0), 0 = no ring takes the form (UAPS_SIMPLIFY_OFF)."""
    if v is None:
        return 0
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > cap:
        raise ValueError(f"simplify_contours: {what} is None or an integer in [0, {cap}]")
    return _lib.SIMPLIFY_OFF if v == 0 else int(v)


def simplify_contours(res: ContourResult, epsilon: float = 1.0, *, wave_max: Optional[int] = None,
                      lds_max: Optional[int] = None) -> SimplifiedContours:
    """The rings of `res` (contours.contours, inference.predict_instances(contours=True)) simplified by the split rule of the
    module's docstring at the tolerance `epsilon` (pixels, quantised to sixteenths): a SimplifiedContours.
    wave_max, lds_max: the largest point count of a ring that takes the one-ring-a-wave form (64 at most) and the LDS form (2048 at
    most); None = those, 0 = no ring takes the form.  They change the time, never a bit.
    One host read (the total of kept points); an input without a ring returns empty tensors without a launch.
    A simplified ring may touch or cross itself or another ring, and the sign of its own area is not guaranteed."""
    if not isinstance(res, ContourResult):
        raise TypeError("simplify_contours: a contours.ContourResult expected")
    e16 = quantise(epsilon)
    wave, lds = _threshold(wave_max, WAVE_MAX, "wave_max"), _threshold(lds_max, LDS_MAX, "lds_max")
    points, offsets, rings, summary = res.points, res.ring_offsets, res.rings, res.summary
    if points.dtype != torch.int32 or points.dim() != 2 or offsets.dtype != torch.int32 or rings.dtype != torch.int64 or \
            rings.dim() != 2 or rings.shape[1] != 7 or offsets.shape[0] != rings.shape[0] + 1 or summary.dtype != torch.int64 or \
            summary.dim() != 3 or summary.shape[2] != 4:
        raise TypeError("simplify_contours: the tensors of a contours.ContourResult expected")
    L, N = rings.shape[0], points.shape[0]
    B, M = summary.shape[:2]
    done = lambda p, o, r, s, stats: SimplifiedContours(res._replace(points=p, ring_offsets=o, rings=r, summary=s), res, e16 / 16.0, e16, stats)
    if L == 0 or N == 0:
        return done(points.clone(), offsets.clone(), rings.clone(), summary.clone(), torch.zeros((L, 2), dtype=torch.int64, device=rings.device))
    if not points.is_cuda:
        out = _simplify_cpu(points.numpy(), offsets.numpy(), rings.numpy(), summary.numpy(), e16)
        return done(*(torch.from_numpy(a) for a in out))
    dev = points.device
    points, offsets, rings, summary = (t.detach().contiguous() for t in (points, offsets, rings, summary))
    summary_out = torch.empty_like(summary)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    need = _lib.workspace_bytes("uaps_contours_simplify_workspace_bytes", N, L)
    common = dict(B=B, max_instances=M, e16=e16, wave_max=wave, lds_max=lds, n_points=N, n_rings=L, points=points.data_ptr(),
                  ring_offsets=offsets.data_ptr(), rings=rings.data_ptr())
    _lib.call("uaps_contours_simplify_mark", _lib.SimplifyCall, dev, _ws, need, summary_in=summary.data_ptr(),
              summary_out=summary_out.data_ptr(), totals=totals.data_ptr(), **common)
    kept = int(totals[1])                                                # the one host read
    new_points = torch.empty((kept, 2), dtype=torch.int32, device=dev)
    new_offsets = torch.empty(L + 1, dtype=torch.int32, device=dev)
    new_rings = torch.empty((L, 7), dtype=torch.int64, device=dev)
    stats = torch.empty((L, 2), dtype=torch.int64, device=dev)
    _lib.call("uaps_contours_simplify_write", _lib.SimplifyCall, dev, _ws, need, n_points_out=kept, ring_capacity=L, point_capacity=kept,
              points_out=new_points.data_ptr(), ring_offsets_out=new_offsets.data_ptr(), rings_out=new_rings.data_ptr(),
              ring_stats=stats.data_ptr(), **common)
    return done(new_points, new_offsets, new_rings, summary_out, stats)

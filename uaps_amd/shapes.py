"""Defect shape descriptors on the kernels of csrc/shapes.hip: what a row of the defect list says about a defect's SHAPE.

`shape_descriptors(inst)` takes the `labels` of an `instances.InstanceResult` and returns, per defect, eleven exact integers --
the raw moments up to order two, Gray's bit-quad counts and the maximum and sum of an optional integer plane (SHAPE_COLUMNS).
Nothing in it synchronises with the host.  `ShapeResult.props()` is the one device-to-host copy: it forms centroid, covariance,
principal axes, orientation, eccentricity, the two perimeters, compactness, Euler number, hole count, extent, equivalent diameter and
(with a plane) the plane's maximum and mean -- with `thickness=True` the inradius -- from exact Python-integer numerators.

Conventions (they are the definition; scikit-image is not a dependency and parity with its `regionprops` is UNPINNED: nothing here
was compared with it):
  coordinates     absolute integer pixel coordinates, row y and column x; the centroid of one pixel at (y, x) is (y, x)
  moments         population (not sample) central moments of the pixel centres: var_x = sum (x - cx)^2 / area
  l1 >= l2        the eigenvalues of [[var_x, cov_xy], [cov_xy, var_y]]; major_axis = 4 sqrt(l1), minor_axis = 4 sqrt(l2): the axes of
                  the ellipse with the same second moments
  orientation     1/2 atan2(2 cov_xy, var_x - var_y) in (-pi/2, pi/2]: the angle of the major axis from +x towards +y (rows grow
                  downwards); 0 where both arguments are 0
  bit quads       over the (H+1) x (W+1) windows of 2 x 2 pixels, the frame padded with "no component": q1, q2 (edge-adjacent pair),
                  q3, qd (diagonal pair) count the windows with 1, 2, 2, 3 pixels of the component
  perimeter_crack q1 + q2 + q3 + 2 qd: the number of pixel edges between the component and anything else, the frame included
  perimeter       q2 + (q1 + q3 + 2 qd) / sqrt(2): Duda's bit-quad estimate (Pratt, Digital Image Processing)
  euler, holes    euler = (q1 - q3 - 2 qd) / 4 under connectivity 8 and (q1 - q3 + 2 qd) / 4 under 4; holes = 1 - euler: the components
                  of the complement of the defect that do not reach the frame, under the complementary connectivity (components'
                  fill_holes rule)

CPU tensors take the numpy restatement below, as in the other modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_instances, check_plane
from .instances import InstanceResult, add_props, host_tables

SHAPE_COLUMNS = ("sy", "sx", "syy", "sxy", "sxx", "q1", "q2", "q3", "qd", "pmax", "psum")
MAX_EXTENT = _lib.SHAPE_MAX_EXTENT
assert len(SHAPE_COLUMNS) == _lib.SHAPE_COLUMNS


def _isqrt_float(n: int) -> float:
    """sqrt of a non-negative Python integer of any size: the integer root of n scaled to about 160 bits, rounded once to float64."""
    if n < 2 ** 52:
        return math.sqrt(n)
    e = (160 - n.bit_length()) // 2
    if e >= 0:
        return float(math.isqrt(n << (2 * e))) / 2.0 ** e
    return float(math.isqrt(n >> (-2 * e))) * 2.0 ** (-e)


def _ratio(num: int, den: int) -> float:
    """num / den of Python integers, correctly rounded (int / int is, in CPython)."""
    return num / den


class ShapeResult(NamedTuple):
    """table: int64 [B,max_instances,11], columns SHAPE_COLUMNS, zero in rows without a component; instances: the InstanceResult it
    describes; connectivity: the one the instances were labelled with (it decides the sign of qd in the Euler number); has_plane:
    "none", "plane" or "thickness"."""
    table: torch.Tensor
    instances: InstanceResult
    connectivity: int = 8
    has_plane: str = "none"

    def props(self) -> Dict[str, np.ndarray]:
        """One device-to-host copy; a dict of float64 arrays [B,max_instances], NaN in rows without a component.  Every value is a
        few correctly rounded float64 operations on exact integer numerators: with A = area, N20 = A sxx - sx^2, N02 = A syy - sy^2,
        N11 = A sxy - sx sy, disc = (N20 - N02)^2 + 4 N11^2 and det = N20 N02 - N11^2,
          var_x = N20 / A^2, var_y = N02 / A^2, cov_xy = N11 / A^2, l1 = (N20 + N02 + sqrt(disc)) / (2 A^2), l2 = det / (A^4 l1)
        (the product form: no subtraction of nearly equal numbers), 0 where l1 = 0."""
        sh, tb = host_tables(self.table, self.instances)
        B, M = sh.shape[:2]
        names = ["centroid_y", "centroid_x", "var_x", "var_y", "cov_xy", "l1", "l2", "major_axis", "minor_axis", "eccentricity",
                 "orientation", "perimeter_crack", "perimeter", "compactness", "euler", "holes", "extent", "equivalent_diameter"]
        if self.has_plane != "none":
            names += ["plane_max", "plane_mean"]
        if self.has_plane == "thickness":
            names.append("inradius")
        out = {n: np.full((B, M), np.nan, dtype=np.float64) for n in names}
        sign = -1 if self.connectivity == 8 else 1
        for b in range(B):
            for k in range(M):
                A = int(tb[b, k, 1])
                if A <= 0:
                    continue
                sy, sx, syy, sxy, sxx, q1, q2, q3, qd, pmax, psum = (int(v) for v in sh[b, k])
                N20, N02, N11 = A * sxx - sx * sx, A * syy - sy * sy, A * sxy - sx * sy
                disc, det = (N20 - N02) ** 2 + 4 * N11 * N11, N20 * N02 - N11 * N11
                A2 = A * A
                put = lambda name, v: out[name].__setitem__((b, k), v)
                put("centroid_y", _ratio(sy, A)); put("centroid_x", _ratio(sx, A))
                put("var_x", _ratio(N20, A2)); put("var_y", _ratio(N02, A2)); put("cov_xy", _ratio(N11, A2))
                root = _isqrt_float(disc)
                l1 = (float(N20 + N02) + root) / float(2 * A2)
                l2 = 0.0 if l1 == 0.0 else max(_ratio(det, A2 * A2) / l1, 0.0)
                put("l1", l1); put("l2", l2)
                put("major_axis", 4.0 * math.sqrt(l1)); put("minor_axis", 4.0 * math.sqrt(l2))
                put("eccentricity", 0.0 if l1 == 0.0 else math.sqrt(max(1.0 - l2 / l1, 0.0)))
                put("orientation", 0.0 if (N11 == 0 and N20 == N02) else 0.5 * math.atan2(float(2 * N11), float(N20 - N02)))
                put("perimeter_crack", float(q1 + q2 + q3 + 2 * qd))
                per = q2 + (q1 + q3 + 2 * qd) / math.sqrt(2.0)
                put("perimeter", per)
                put("compactness", 4.0 * math.pi * A / (per * per))
                e4 = q1 - q3 + sign * 2 * qd
                put("euler", e4 / 4.0); put("holes", 1.0 - e4 / 4.0)
                box = (int(tb[b, k, 4]) - int(tb[b, k, 2])) * (int(tb[b, k, 5]) - int(tb[b, k, 3]))
                put("extent", _ratio(A, box) if box > 0 else float("nan"))
                put("equivalent_diameter", math.sqrt(4.0 * A / math.pi))
                if self.has_plane != "none":
                    put("plane_max", float(pmax)); put("plane_mean", _ratio(psum, A))
                if self.has_plane == "thickness":
                    put("inradius", math.sqrt(pmax))
        return out

    def records(self) -> List[List[dict]]:
        """instances.records() with every key of props() added to each defect's dict (two device-to-host copies)."""
        return add_props(self.instances.records(), self.props())


def _shapes_cpu(labels: np.ndarray, plane: Optional[np.ndarray], M: int) -> np.ndarray:
    """The table on the host: np.add.at over the pixels for the sums, and for the quads the four corner planes of every window, from
    which each label that occurs in a window gets its count by comparisons among the four."""
    B, H, W = labels.shape
    table = np.zeros((B, M, 11), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    for b in range(B):
        lab = labels[b].astype(np.int64)
        lab = np.where((lab >= 1) & (lab <= M), lab, 0)
        t = table[b]
        sel = lab > 0
        k = lab[sel] - 1
        y, x = yy[sel], xx[sel]
        for col, v in enumerate((y, x, y * y, x * y, x * x)):
            np.add.at(t[:, col], k, v)
        if plane is not None:
            p = np.maximum(plane[b].astype(np.int64), 0)[sel]
            np.maximum.at(t[:, 9], k, p)
            np.add.at(t[:, 10], k, p)
        pad = np.zeros((H + 2, W + 2), dtype=np.int64)
        pad[1:-1, 1:-1] = lab
        c = [pad[:-1, :-1], pad[:-1, 1:], pad[1:, :-1], pad[1:, 1:]]           # a b / c d of every window
        diag = {0: 3, 1: 2, 2: 1, 3: 0}
        for i in range(4):
            first = c[i] > 0
            for j in range(i):
                first &= c[j] != c[i]                   # the first corner, in raster order, that carries this label speaks for it
            same = [c[j] == c[i] for j in range(4)]
            n = same[0].astype(np.int64) + same[1] + same[2] + same[3]
            kk = c[i] - 1
            np.add.at(t[:, 5], kk[first & (n == 1)], 1)
            np.add.at(t[:, 7], kk[first & (n == 3)], 1)
            two = first & (n == 2)
            d = two & same[diag[i]]
            np.add.at(t[:, 8], kk[d], 1)
            np.add.at(t[:, 6], kk[two & ~d], 1)
    return table


def shape_descriptors(inst: InstanceResult, plane: Optional[torch.Tensor] = None, *, thickness: bool = False,
                      connectivity: int = 8) -> ShapeResult:
    """The shape table of the defects of `inst` (instances.label_instances, inference.predict_instances): int64
    [B,max_instances,11], columns SHAPE_COLUMNS, row k - 1 of image b for the pixels labelled k; rows without a component are zero.
    connectivity: the one `inst` was labelled with -- an InstanceResult does not carry it, and the hole count of props() depends on
    it (the table itself does not).
    plane: an optional int32 [B,H,W] tensor on the labels' device; the table's last two columns are the maximum and the sum of
    max(plane, 0) over each defect.
    thickness=True (no plane then): plane = surface.distance_transform_sq(inst.labels), the squared distance of every pixel to
    the nearest pixel of NO component, so that props()["inradius"] = sqrt(pmax) is the radius of the largest disc centred in the
    defect.  Where defects of different classes touch it is the thickness of their union; an image every pixel of which belongs
    to a component has no such pixel and gets surface.NO_FEATURE.  distance_transform_sq limits H and W to 4096.
    1 <= H, W <= 16384 and label_instances' limits.  Does not synchronise with the host."""
    labels, B, H, W, M = check_instances("shape_descriptors", inst, MAX_EXTENT)
    if connectivity not in (4, 8):
        raise ValueError("shape_descriptors: connectivity is 4 or 8")
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG or B * M * 88 >= _TOO_BIG:
        raise ValueError("shape_descriptors: H*W < 2^31, B*H*W*8 < 2 GiB and a table below 2 GiB")
    kind = "none"
    if thickness:
        if plane is not None:
            raise ValueError("shape_descriptors: thickness=True forms its own plane")
        from .surface import distance_transform_sq
        plane, kind = distance_transform_sq(labels), "thickness"
    elif plane is not None:
        plane, kind = check_plane("shape_descriptors", plane, labels), "plane"
    labels = labels.detach().contiguous()
    plane = None if plane is None else plane.detach().contiguous()
    if not labels.is_cuda:
        table = torch.from_numpy(_shapes_cpu(labels.numpy(), None if plane is None else plane.numpy(), M))
        return ShapeResult(table, inst, int(connectivity), kind)
    dev = labels.device
    table = torch.empty((B, M, 11), dtype=torch.int64, device=dev)
    _lib.call("uaps_shape_descriptors", _lib.ShapeCall, dev, B=B, H=H, W=W, max_instances=M, labels=labels.data_ptr(),
              plane=None if plane is None else plane.data_ptr(), table=table.data_ptr())
    return ShapeResult(table, inst, int(connectivity), kind)

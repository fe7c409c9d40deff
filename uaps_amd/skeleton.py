"""Defect skeletons on the kernels of csrc/skeleton.hip: what a row of the defect list says about a crack's COURSE.

`skeletonize(mask, num_classes)` thins every selected class of an int64 label map [B,H,W] to a one-pixel-wide, 8-connected skeleton
with Guo and Hall's two-subiteration parallel thinning (CACM 32(3), 1989, algorithm A1; the rule behind bwmorph('thin') and
scikit-image's `thin` -- neither is a dependency and parity with them is UNPINNED: nothing here was compared with them).
`skeleton_descriptors(inst, skel)` counts, per defect of an `instances.InstanceResult`, the skeleton's pixels, links, ends and branch
points and the largest and summed squared distance to the defect's rim along it, as exact integers; `SkeletonStats.props()` is the
one device-to-host copy and forms length, widths, end and branch counts from them.  Nothing else synchronises with the host.

The rule (it is the definition).  With the neighbours P2..P9 = N, NE, E, SE, S, SW, W, NW of a pixel, outside the image = 0,
  C  = [!P2 & (P3 | P4)] + [!P4 & (P5 | P6)] + [!P6 & (P7 | P8)] + [!P8 & (P9 | P2)]
  N1 = (P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8),  N2 = (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9),  N = min(N1, N2)
a foreground pixel is deleted in a sub-iteration iff C == 1, 2 <= N <= 3 and (P2 | P3 | !P5) & P4 == 0 in the first sub-iteration
of an iteration, (P6 | P7 | !P9) & P8 == 0 in the second.  A sub-iteration is a pure function of the previous plane; an iteration
is the two in that order; the result is the plane after exactly min(max_iters, iterations to the fixed point) iterations.

On a label map every selected class is thinned on its own plane `mask == c`; a selected pixel that thinning removes becomes the
background, and every other value (ignore labels, unselected classes, values >= num_classes) passes through and is never claimed.

CPU tensors take the numpy restatement below (shifted boolean arrays, the counts formed as integers; no scipy), as in the other
modules; on a ROCm device a missing kernel is an error."""
from __future__ import annotations

import ctypes as C
import math
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_classes, check_instances, check_plane
from .instances import InstanceResult, add_props, host_tables

SKELETON_COLUMNS = ("n_skel", "n_orth", "n_diag", "n_end", "n_branch", "d2max", "d2sum")
MAX_CLASSES, MAX_ITERS, MAX_SUB_ITERS, MAX_EXTENT = _lib.SKEL_MAX_CLASSES, _lib.SKEL_MAX_ITERS, _lib.SKEL_MAX_SUB_ITERS, _lib.SKEL_MAX_EXTENT
assert len(SKELETON_COLUMNS) == _lib.SKEL_COLUMNS
_ws = _lib.Workspace()


class SkeletonResult(NamedTuple):
    """mask: int64 [B,H,W], the label map with every selected class thinned; converged: bool [B] on the mask's device, True exactly
    where the returned image is a fixed point for every selected class; classes, background, max_iters: what the call was made with."""
    mask: torch.Tensor
    converged: torch.Tensor
    classes: Tuple[int, ...]
    background: int = 0
    max_iters: int = 64


def _neighbours(p: np.ndarray):
    """P2..P9 of every pixel of the bool plane [H,W]: N, NE, E, SE, S, SW, W, NW, False outside the image."""
    H, W = p.shape
    q = np.pad(p, 1)
    at = lambda dy, dx: q[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)


def _sub_iteration(p: np.ndarray, second: bool) -> np.ndarray:
    P2, P3, P4, P5, P6, P7, P8, P9 = _neighbours(p)
    i8 = lambda a: a.astype(np.int8)
    Cn = i8(~P2 & (P3 | P4)) + i8(~P4 & (P5 | P6)) + i8(~P6 & (P7 | P8)) + i8(~P8 & (P9 | P2))
    N1 = i8(P9 | P2) + i8(P3 | P4) + i8(P5 | P6) + i8(P7 | P8)
    N2 = i8(P2 | P3) + i8(P4 | P5) + i8(P6 | P7) + i8(P8 | P9)
    N = np.minimum(N1, N2)
    third = ((P6 | P7 | ~P9) & P8) if second else ((P2 | P3 | ~P5) & P4)
    return p & ~((Cn == 1) & (N >= 2) & (N <= 3) & ~third)


def _iteration(p: np.ndarray) -> np.ndarray:
    return _sub_iteration(_sub_iteration(p, False), True)


def _thin_plane(p: np.ndarray, max_iters: int) -> Tuple[np.ndarray, bool]:
    """The plane after min(max_iters, iterations to the fixed point) iterations, and whether it is a fixed point."""
    for _ in range(max_iters):
        q = _iteration(p)
        if np.array_equal(q, p):
            return p, True
        p = q
    return p, bool(np.array_equal(_iteration(p), p))


def _skeleton_cpu(mask: torch.Tensor, classes, background: int, max_iters: int) -> Tuple[torch.Tensor, torch.Tensor]:
    m = mask.numpy()
    out = m.copy()
    B = m.shape[0]
    jobs = [(b, c) for b in range(B) for c in classes]
    run = lambda bc: _thin_plane(m[bc[0]] == bc[1], max_iters)
    threads = max(1, min(len(jobs), torch.get_num_threads()))
    if threads > 1:
        with ThreadPoolExecutor(threads) as pool:
            results = list(pool.map(run, jobs))
    else:
        results = [run(j) for j in jobs]
    conv = np.ones(B, dtype=bool)
    for (b, c), (plane, fixed) in zip(jobs, results):
        out[b][(m[b] == c) & ~plane] = background
        conv[b] &= fixed
    return torch.from_numpy(out), torch.from_numpy(conv)


def skeletonize(mask: torch.Tensor, num_classes: int, *, classes: Optional[Sequence[int]] = None, background: int = 0,
                max_iters: int = 64, _band_rows: int = 0, _sub_iters: int = 0) -> SkeletonResult:
    """Guo-Hall thinning of the int64 label map [B,H,W]; a new tensor.  classes: at most 8 distinct values in [0, num_classes) other
    than `background` (default: all of them), each thinned on its own plane; every other value passes through untouched.
    max_iters: 1..2048 iterations (two sub-iterations each) at most; `converged` tells per image whether the result is a fixed point.
    1 <= H, W <= 4096 and B*H*W*8 < 2 GiB.  Does not synchronise with the host; the number of launches is fixed by the arguments."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or mask.dtype != torch.int64:
        raise TypeError("skeletonize: int64 [B,H,W] label map expected")
    num_classes, background = int(num_classes), int(background)
    if not 1 <= num_classes <= _lib.SEG_MAX_CLASSES:
        raise ValueError(f"skeletonize: num_classes in 1..{_lib.SEG_MAX_CLASSES}")
    if not -2 ** 31 <= background < 2 ** 31:
        raise ValueError("skeletonize: the background is a 32-bit value")
    classes = check_classes("skeletonize", classes, num_classes, background, MAX_CLASSES)
    if isinstance(max_iters, bool) or int(max_iters) != max_iters or not 1 <= int(max_iters) <= MAX_ITERS:
        raise ValueError(f"skeletonize: max_iters is an integer in 1..{MAX_ITERS}")
    max_iters, band, S = int(max_iters), int(_band_rows), int(_sub_iters)
    B, H, W = mask.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("skeletonize: empty mask")
    if H > MAX_EXTENT or W > MAX_EXTENT or B * H * W * 8 >= _TOO_BIG:
        raise ValueError(f"skeletonize: H, W <= {MAX_EXTENT} and B*H*W*8 < 2 GiB")
    if band < 0 or (S != 0 and (S < 2 or S > MAX_SUB_ITERS or S % 2)):
        raise ValueError(f"skeletonize: _band_rows >= 0 and _sub_iters even in 2..{MAX_SUB_ITERS}")
    mask = mask.detach().contiguous()
    if not mask.is_cuda:
        out, conv = _skeleton_cpu(mask, classes, background, max_iters)
        return SkeletonResult(out, conv, classes, background, max_iters)
    dev = mask.device
    out = torch.empty_like(mask)
    conv = torch.empty((B,), dtype=torch.uint8, device=dev)
    _lib.call("uaps_skeletonize", _lib.SkeletonCall, dev, _ws, _lib.workspace_bytes("uaps_skeleton_workspace_bytes", B, H, W, len(classes)),
              B=B, H=H, W=W, n_classes=len(classes), classes=classes, background=background, max_iters=max_iters, sub_iters=S,
              band_rows=band, mask=mask.data_ptr(), out=out.data_ptr(), converged=conv.data_ptr())
    return SkeletonResult(out, conv.view(torch.bool), classes, background, max_iters)


def band_rows(H: int, W: int, n_classes: int, sub_iters: int = 0) -> int:
    """The band height the library chooses (what `_band_rows=0` resolves to) for launches of `sub_iters` sub-iterations (0: chosen)."""
    rows = C.c_int()
    _lib.check(_lib.lib().uaps_skeleton_band_rows(int(H), int(W), int(n_classes) + 1, int(sub_iters), C.byref(rows)), "uaps_skeleton_band_rows")
    return rows.value


class SkeletonStats(NamedTuple):
    """table: int64 [B,max_instances,7], columns SKELETON_COLUMNS, zero in rows without a component; instances: the InstanceResult
    it describes; skeleton: the SkeletonResult; has_plane: whether d2max / d2sum were formed (thickness=True); shapes: the
    shapes.ShapeResult of the same defects where inference.predict_instances was asked for both."""
    table: torch.Tensor
    instances: InstanceResult
    skeleton: SkeletonResult
    has_plane: bool = True
    shapes: Optional[object] = None

    def props(self) -> Dict[str, np.ndarray]:
        """One device-to-host copy; a dict of float64 arrays [B,max_instances], NaN in rows without a component:
          length = n_orth + sqrt(2) n_diag;  endpoints = n_end;  branch_points = n_branch;  skeleton_pixels = n_skel
          width_mean = area / (length + 1): a straight one-pixel line has width 1
          width_max = 2 sqrt(d2max) - 1 and width_rms = 2 sqrt(d2sum / n_skel) - 1 (with a plane; NaN where n_skel == 0, which
          happens when the skeleton was cut by classes)."""
        sk, tb = host_tables(self.table, self.instances)
        B, M = sk.shape[:2]
        names = ["length", "endpoints", "branch_points", "width_mean", "skeleton_pixels"]
        if self.has_plane:
            names += ["width_max", "width_rms"]
        out = {n: np.full((B, M), np.nan, dtype=np.float64) for n in names}
        for b in range(B):
            for k in range(M):
                area = int(tb[b, k, 1])
                if area <= 0:
                    continue
                n_skel, n_orth, n_diag, n_end, n_branch, d2max, d2sum = (int(v) for v in sk[b, k])
                length = n_orth + math.sqrt(2.0) * n_diag
                out["length"][b, k] = length
                out["endpoints"][b, k] = float(n_end)
                out["branch_points"][b, k] = float(n_branch)
                out["width_mean"][b, k] = area / (length + 1.0)
                out["skeleton_pixels"][b, k] = float(n_skel)
                if self.has_plane:
                    out["width_max"][b, k] = 2.0 * math.sqrt(d2max) - 1.0 if n_skel > 0 else float("nan")
                    out["width_rms"][b, k] = 2.0 * math.sqrt(d2sum / n_skel) - 1.0 if n_skel > 0 else float("nan")
        return out

    def records(self) -> List[List[dict]]:
        """instances.records() -- shapes.records() where `shapes` is attached -- with every key of props() added to each defect."""
        return add_props(self.shapes.records() if self.shapes is not None else self.instances.records(), self.props())


def _stats_cpu(labels: np.ndarray, skel: np.ndarray, classes, plane: Optional[np.ndarray], M: int) -> np.ndarray:
    """The table on the host: the defect of every skeleton pixel as one padded plane, its eight shifts, np.add.at per column."""
    B, H, W = labels.shape
    table = np.zeros((B, M, 7), dtype=np.int64)
    for b in range(B):
        lab = labels[b].astype(np.int64)
        e = np.where((lab >= 1) & (lab <= M) & np.isin(skel[b], classes), lab, 0)
        q = np.pad(e, 1)
        on = e > 0
        at = lambda dy, dx: (q[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == e) & on
        N, NE, E, SE, S, SW, Wl, NW = at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)
        ring = [N, NE, E, SE, S, SW, Wl, NW]
        links = sum(r.astype(np.int64) for r in ring)
        rises = sum((~ring[i] & ring[(i + 1) % 8]).astype(np.int64) for i in range(8))
        k = e[on] - 1
        t = table[b]
        cols = (np.ones_like(e), E.astype(np.int64) + S, (SE & ~E & ~S).astype(np.int64) + (SW & ~Wl & ~S),
                (links == 1).astype(np.int64), (rises >= 3).astype(np.int64))
        for col, v in enumerate(cols):
            np.add.at(t[:, col], k, v[on])
        if plane is not None:
            p = np.maximum(plane[b].astype(np.int64), 0)[on]
            np.maximum.at(t[:, 5], k, p)
            np.add.at(t[:, 6], k, p)
    return table


def skeleton_descriptors(inst: InstanceResult, skel: SkeletonResult, *, thickness: bool = True, _plane: Optional[torch.Tensor] = None) -> SkeletonStats:
    """The skeleton table of the defects of `inst` (instances.label_instances): int64 [B,max_instances,7], columns SKELETON_COLUMNS,
    row k - 1 of image b.  A pixel is a skeleton pixel of defect k iff inst.labels is k (1 <= k <= max_instances) there and
    skel.mask is one of skel.classes; two skeleton pixels are linked iff they are 8-adjacent and belong to the same defect.
      n_skel    skeleton pixels;  n_orth  links between edge-adjacent skeleton pixels, each once
      n_diag    links between diagonally adjacent skeleton pixels where neither pixel edge-adjacent to both is a skeleton pixel of the
                defect (a staircase corner is not counted twice), each once
      n_end     skeleton pixels with exactly one linked neighbour
      n_branch  skeleton pixels whose cyclic sequence of eight neighbours (linked or not) has at least three 0 -> 1 transitions
      d2max, d2sum   with thickness=True the maximum and sum over the skeleton pixels of surface.distance_transform_sq(inst.labels),
                as shape_descriptors forms it (H, W <= 4096 then); 0 without
    Limits: those of shape_descriptors.  Does not synchronise with the host.  (_plane: an int32 [B,H,W] plane in place of the
    distance transform, for tests.)"""
    if not isinstance(inst, InstanceResult) or not isinstance(skel, SkeletonResult):
        raise TypeError("skeleton_descriptors: an instances.InstanceResult and a SkeletonResult expected")
    labels, B, H, W, M = check_instances("skeleton_descriptors", inst, _lib.SHAPE_MAX_EXTENT)
    sk = skel.mask
    if not isinstance(sk, torch.Tensor) or sk.dtype != torch.int64 or sk.shape != labels.shape or sk.device != labels.device:
        raise TypeError("skeleton_descriptors: the skeleton is an int64 map of the labels' shape on their device")
    classes = tuple(int(c) for c in skel.classes)
    if not 1 <= len(classes) <= MAX_CLASSES:
        raise ValueError(f"skeleton_descriptors: 1..{MAX_CLASSES} skeleton classes")
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG or B * M * 56 >= _TOO_BIG:
        raise ValueError("skeleton_descriptors: H*W < 2^31, B*H*W*8 < 2 GiB and a table below 2 GiB")
    plane = None
    if _plane is not None:
        plane = check_plane("skeleton_descriptors", _plane, labels)
    elif thickness:
        from .surface import distance_transform_sq
        plane = distance_transform_sq(labels)
    labels, sk = labels.detach().contiguous(), sk.detach().contiguous()
    plane = None if plane is None else plane.detach().contiguous()
    if not labels.is_cuda:
        table = torch.from_numpy(_stats_cpu(labels.numpy(), sk.numpy(), classes, None if plane is None else plane.numpy(), M))
        return SkeletonStats(table, inst, skel, plane is not None)
    dev = labels.device
    table = torch.empty((B, M, 7), dtype=torch.int64, device=dev)
    _lib.call("uaps_skeleton_stats", _lib.SkeletonStatsCall, dev, B=B, H=H, W=W, max_instances=M, n_classes=len(classes), classes=classes,
              labels=labels.data_ptr(), skel=sk.data_ptr(), plane=None if plane is None else plane.data_ptr(), table=table.data_ptr())
    return SkeletonStats(table, inst, skel, plane is not None)

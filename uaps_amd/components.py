"""Component clean-up of a label map on the kernels of csrc/components.hip: area opening, clear border, hole filling.

`morphology` works on shape -- a footprint removes salt and bridges gaps.  `components` works on content, what no footprint can
express: drop every defect below n pixels whatever its shape, drop the defects that touch the frame, make a ring-shaped or porous
defect solid.  `inference.predict_instances(..., components=steps)` and `inference.evaluate(..., components=steps)` put it between
the arg-max mask (after the `cleanup=` morphology chain, where one is given) and the defect list.

A step is ("area_open", n), ("clear_border",) or ("fill_holes", n) with n >= 1, or None for "every hole".  A component is a maximal
set of equal-valued pixels connected under `connectivity`, as `label_instances` defines it.
  area_open n     every component of a selected class with fewer than n pixels becomes the background (label_instances' min_area rule).
  clear_border    every component of a selected class with a pixel in row 0, row H-1, column 0 or column W-1 becomes the background.
  fill_holes n    for every selected class c, a hole of c is a connected component of the complement of (mask == c) -- background,
                  other classes and ignore labels alike -- without a pixel on the image border, connected under the COMPLEMENTARY
                  connectivity (4 for defects of connectivity 8, 8 for 4: scipy's binary_fill_holes with the cross by default).  A
                  hole of at most n pixels, counting all of them, is filled.  Only background pixels are rewritten; every other value
                  inside a hole stays and is never claimed; a background pixel in filled holes of several classes goes to the smallest.

CPU tensors take the numpy restatement below (on instances._label_image's union-find; no scipy), as in the other modules; on a ROCm
device a missing kernel is an error."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_classes
from .instances import _label_image

KINDS = tuple(_lib.COMP_KINDS)
MAX_STEPS, MAX_CLASSES = _lib.COMP_MAX_STEPS, _lib.COMP_MAX_CLASSES
_ws = _lib.Workspace()


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_steps(steps) -> Tuple[tuple, ...]:
    """The chain as a tuple of ("area_open", n) / ("clear_border",) / ("fill_holes", n or None), or the ValueError that names what
    is wrong with it."""
    if isinstance(steps, (str, bytes)) or not hasattr(steps, "__iter__"):
        raise ValueError("components: steps is a sequence of (\"area_open\", n), (\"clear_border\",) and (\"fill_holes\", n) tuples")
    steps = tuple(steps)
    if not 1 <= len(steps) <= MAX_STEPS:
        raise ValueError(f"components: 1..{MAX_STEPS} steps")
    out = []
    for s in steps:
        if isinstance(s, (str, bytes)) or not hasattr(s, "__iter__"):
            raise ValueError("components: a step is a tuple whose first entry is one of " + ", ".join(KINDS))
        s = tuple(s)
        if not s or s[0] not in _lib.COMP_KINDS:
            raise ValueError(f"components: a step's kind is one of {KINDS}")
        kind = s[0]
        if kind == "clear_border":
            if len(s) != 1:
                raise ValueError("components: clear_border takes no argument: (\"clear_border\",)")
            out.append((kind,))
            continue
        if len(s) != 2:
            raise ValueError(f"components: a {kind} step is (\"{kind}\", n)")
        n = s[1]
        if n is None and kind == "fill_holes":
            out.append((kind, None))
            continue
        if not _is_int(n) or n < 1:
            raise ValueError(f"components: n of {kind} is an integer >= 1" + (" or None" if kind == "fill_holes" else ""))
        out.append((kind, int(n)))
    return tuple(out)


def _plane_words(plane: np.ndarray, conn8: bool):
    """roots [H*W] (-1 outside `plane`), and per root index the area and whether the component has a pixel on the image border."""
    H, W = plane.shape
    roots = _label_image(plane.astype(np.int64), conn8, 0)
    idx = np.nonzero(roots >= 0)[0]
    area = np.bincount(roots[idx], minlength=H * W)
    edge = np.zeros((H, W), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    border = np.zeros(H * W, dtype=bool)
    border[roots[idx[edge.reshape(-1)[idx]]]] = True
    return roots, area, border


def _step_cpu(img: np.ndarray, step, classes, background: int, connectivity: int) -> np.ndarray:
    H, W = img.shape
    flat = img.reshape(-1)
    out = flat.copy()
    if step[0] == "fill_holes":
        free = flat == background
        for c in classes:                                   # ascending: the smallest class claims first
            roots, area, border = _plane_words(img != c, connectivity == 4)
            r = np.where(roots >= 0, roots, 0)
            hole = (roots >= 0) & ~border[r]
            if step[1] is not None:
                hole &= area[r] <= step[1]
            claim = free & hole
            out[claim] = c
            free &= ~claim
        return out.reshape(H, W)
    # one labelling for all classes: equal values belong together, the background forms nothing
    roots = _label_image(img, connectivity == 8, background)
    idx = np.nonzero(roots >= 0)[0]
    r = np.where(roots >= 0, roots, 0)
    if step[0] == "area_open":
        drop = np.bincount(roots[idx], minlength=H * W)[r] < step[1]
    else:
        edge = np.zeros((H, W), dtype=bool)
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
        border = np.zeros(H * W, dtype=bool)
        border[roots[idx[edge.reshape(-1)[idx]]]] = True
        drop = border[r]
    out[(roots >= 0) & drop & np.isin(flat, classes)] = background
    return out.reshape(H, W)


def _components_cpu(mask: torch.Tensor, steps, classes, background: int, connectivity: int) -> torch.Tensor:
    m = mask.numpy().copy()
    classes = sorted(classes)
    for step in steps:
        for b in range(m.shape[0]):
            m[b] = _step_cpu(m[b], step, classes, background, connectivity)
    return torch.from_numpy(m)


def components(mask: torch.Tensor, steps, num_classes: int, *, classes: Optional[Sequence[int]] = None, background: int = 0,
               connectivity: int = 8) -> torch.Tensor:
    """The chain `steps` applied to the int64 label map [B,H,W]; a new tensor.  classes: at most 8 distinct values in
    [0, num_classes) other than `background` (default: all of them); every other value passes through untouched.  connectivity
    (4 or 8) is that of the defects; holes are connected under the other one.  H*W < 2^31, B*H*W*8 < 2 GiB, and a workspace
    (8 bytes a pixel and class with a fill_holes step, 8 a pixel without, and the map once more) below 2 GiB."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or mask.dtype != torch.int64:
        raise TypeError("components: int64 [B,H,W] label map expected")
    steps = check_steps(steps)
    num_classes, background = int(num_classes), int(background)
    if not 1 <= num_classes <= _lib.SEG_MAX_CLASSES:
        raise ValueError(f"components: num_classes in 1..{_lib.SEG_MAX_CLASSES}")
    if not -2 ** 31 <= background < 2 ** 31:
        raise ValueError("components: the background is a 32-bit value")
    classes = check_classes("components", classes, num_classes, background, MAX_CLASSES)
    if connectivity not in (4, 8):
        raise ValueError("components: connectivity is 4 or 8")
    B, H, W = mask.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("components: empty mask")
    planes = len(classes) if any(s[0] == "fill_holes" for s in steps) else 1
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG or B * H * W * (8 * planes + 8) + 768 >= _TOO_BIG:
        raise ValueError("components: H*W < 2^31, B*H*W*8 < 2 GiB and a workspace below 2 GiB")
    if not mask.is_cuda:
        return _components_cpu(mask.detach().contiguous(), steps, classes, background, int(connectivity))
    dev = mask.device
    mask = mask.detach().contiguous()
    out = torch.empty_like(mask)
    _lib.call("uaps_components", _lib.ComponentsCall, dev, _ws, _lib.workspace_bytes("uaps_components_workspace_bytes", B, H, W, planes),
              B=B, H=H, W=W, n_steps=len(steps), kind=[_lib.COMP_KINDS[s[0]] for s in steps],
              n=[0 if len(s) == 1 else (_lib.COMP_ALL if s[1] is None else min(s[1], _lib.COMP_ALL)) for s in steps],
              n_classes=len(classes), classes=classes, background=background, connectivity=int(connectivity),
              mask=mask.data_ptr(), out=out.data_ptr())
    return out

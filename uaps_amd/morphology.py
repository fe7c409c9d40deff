"""Mask clean-up morphology on the kernel of csrc/morph.hip.

`morphology` applies a chain of erode / dilate / open / close / boundary steps to an int64 label map [B,H,W] -- what argmax, predict
and TTAResult.mask produce -- in one launch that reads the map once and writes it once.  Opening removes salt, closing bridges pepper
and hairline gaps; `inference.predict_instances(..., cleanup=steps)` and `inference.evaluate(..., cleanup=steps)` put it between the
arg-max mask and the defect list.

A step is a triple (op, footprint, radius): op in OPS, footprint in FOOTPRINTS, radius 1..15.  A footprint of radius r is the set of
offsets (dy, dx) with |dy| <= r and |dx| <= w(dy): square w = r, cross (the L1 ball) w = r - |dy|, disk w = floor(sqrt(r^2 - dy^2)).
Erosion takes what lies outside the image as foreground, dilation as background (scipy's border_value 1 and 0): an opening does not
eat a defect that touches the edge.

On a label map every selected class is processed on its own plane; then a pixel keeps its class where its plane's result holds it,
a value that is neither selected nor the background (an ignore label) always stays and is never claimed, and a background or
just-removed pixel goes to the smallest selected class whose result covers it, else to the background.

CPU tensors take the numpy restatement below (row runs counted on a prefix sum; no scipy), as in the other modules; on a ROCm device a
missing kernel is an error."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_classes

OPS = tuple(_lib.MORPH_OPS)
FOOTPRINTS = tuple(_lib.MORPH_FOOTPRINTS)
MAX_STEPS, MAX_CLASSES, MAX_RADIUS, MAX_REACH, MAX_EXTENT = _lib.MORPH_MAX_STEPS, _lib.MORPH_MAX_CLASSES, 15, 64, 4096


def half_widths(footprint: str, radius: int) -> List[int]:
    """w(|dy|) for |dy| = 0 .. radius: the footprint is the union of the centred row runs [-w(dy), w(dy)]."""
    r = int(radius)
    if footprint == "square":
        return [r] * (r + 1)
    if footprint == "cross":
        return [r - d for d in range(r + 1)]
    if footprint == "disk":
        out = []
        for d in range(r + 1):
            w = 0
            while (w + 1) * (w + 1) + d * d <= r * r:
                w += 1
            out.append(w)
        return out
    raise ValueError(f"morphology: footprint is one of {FOOTPRINTS}")


def check_steps(steps) -> Tuple[Tuple[str, str, int], ...]:
    """The chain as a tuple of (op, footprint, radius), or the ValueError that names what is wrong with it."""
    if isinstance(steps, (str, bytes)) or not hasattr(steps, "__iter__"):
        raise ValueError("morphology: steps is a sequence of (op, footprint, radius) triples")
    steps = tuple(tuple(s) for s in steps)
    if not 1 <= len(steps) <= MAX_STEPS:
        raise ValueError(f"morphology: 1..{MAX_STEPS} steps")
    out = []
    for s in steps:
        if len(s) != 3:
            raise ValueError("morphology: a step is (op, footprint, radius)")
        op, fp, r = s[0], s[1], int(s[2])
        if op not in _lib.MORPH_OPS:
            raise ValueError(f"morphology: op is one of {OPS}")
        if fp not in _lib.MORPH_FOOTPRINTS:
            raise ValueError(f"morphology: footprint is one of {FOOTPRINTS}")
        if not 1 <= r <= MAX_RADIUS or r != s[2]:
            raise ValueError(f"morphology: radius is an integer in 1..{MAX_RADIUS}")
        out.append((op, fp, r))
    if chain_reach(out) > MAX_REACH:
        raise ValueError(f"morphology: the chain reaches further than {MAX_REACH} pixels (r per erode / dilate / boundary, 2r per open / close)")
    return tuple(out)


def chain_reach(steps) -> int:
    """How far a pixel's result looks: r per erode / dilate / boundary step, 2r per open / close step."""
    return sum(2 * r if op in ("open", "close") else r for op, _, r in steps)


def _primitive(plane: np.ndarray, hw: Sequence[int], erode: bool) -> np.ndarray:
    """Erosion (outside = 1) or dilation (outside = 0) of one binary plane [H,W]: per row offset dy, the run [x - w, x + w] of the
    padded source row is full (erode) or non-empty (dilate), counted on a prefix sum along the row."""
    H, W = plane.shape
    r = len(hw) - 1
    pad = np.pad(plane, r, constant_values=bool(erode))
    cs = np.zeros((H + 2 * r, W + 2 * r + 1), dtype=np.int32)
    np.cumsum(pad, axis=1, out=cs[:, 1:])
    out = np.full((H, W), bool(erode))
    for dy in range(-r, r + 1):
        w = hw[abs(dy)]
        rows = slice(r + dy, r + dy + H)
        cnt = cs[rows, r + w + 1:r + w + 1 + W] - cs[rows, r - w:r - w + W]
        out = out & (cnt == 2 * w + 1) if erode else out | (cnt > 0)
    return out


def _step_plane(plane: np.ndarray, op: str, hw) -> np.ndarray:
    if op == "erode":
        return _primitive(plane, hw, True)
    if op == "dilate":
        return _primitive(plane, hw, False)
    if op == "open":
        return _primitive(_primitive(plane, hw, True), hw, False)
    if op == "close":
        return _primitive(_primitive(plane, hw, False), hw, True)
    return plane & ~_primitive(plane, hw, True)             # boundary


def _morph_cpu(mask: torch.Tensor, steps, classes, background: int) -> torch.Tensor:
    m = mask.numpy().copy()
    classes = sorted(classes)
    for op, fp, r in steps:
        hw = half_widths(fp, r)
        for b in range(m.shape[0]):
            img = m[b]
            results = [_step_plane(img == c, op, hw) for c in classes]
            kept = np.zeros(img.shape, dtype=bool)
            for c, res in zip(classes, results):
                kept |= (img == c) & res
            selected = np.isin(img, classes)
            free = ~kept & (selected | (img == background))     # background or just removed; everything else passes through
            new = np.where(free, background, img)
            for c, res in zip(classes, results):
                claim = free & res
                new[claim] = c
                free &= ~claim
            m[b] = new
    return torch.from_numpy(m)


def morphology(mask: torch.Tensor, steps, num_classes: int, *, classes: Optional[Sequence[int]] = None, background: int = 0,
               _band_rows: int = 0) -> torch.Tensor:
    """The chain `steps` applied to the int64 label map [B,H,W]; a new tensor.  classes: at most 8 distinct values in
    [0, num_classes) other than `background` (default: all of them); every other value passes through untouched.
    1 <= H, W <= 4096, B*H*W*8 < 2 GiB, and the chain's reach (chain_reach) is at most 64 pixels."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or mask.dtype != torch.int64:
        raise TypeError("morphology: int64 [B,H,W] label map expected")
    steps = check_steps(steps)
    num_classes, background = int(num_classes), int(background)
    if not 1 <= num_classes <= _lib.SEG_MAX_CLASSES:
        raise ValueError(f"morphology: num_classes in 1..{_lib.SEG_MAX_CLASSES}")
    if not -2 ** 31 <= background < 2 ** 31:
        raise ValueError("morphology: the background is a 32-bit value")
    classes = check_classes("morphology", classes, num_classes, background, MAX_CLASSES)
    B, H, W = mask.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("morphology: empty mask")
    if H > MAX_EXTENT or W > MAX_EXTENT or B * H * W * 8 >= _TOO_BIG:
        raise ValueError(f"morphology: H, W <= {MAX_EXTENT} and B*H*W*8 < 2 GiB")
    if int(_band_rows) < 0:
        raise ValueError("morphology: _band_rows >= 0")
    if not mask.is_cuda:
        return _morph_cpu(mask.detach().contiguous(), steps, classes, background)
    dev = mask.device
    mask = mask.detach().contiguous()
    out = torch.empty_like(mask)
    _lib.call("uaps_morphology", _lib.MorphCall, dev, B=B, H=H, W=W, n_steps=len(steps), op=[_lib.MORPH_OPS[s[0]] for s in steps],
              footprint=[_lib.MORPH_FOOTPRINTS[s[1]] for s in steps], radius=[s[2] for s in steps], n_classes=len(classes),
              classes=classes, background=background, band_rows=int(_band_rows), mask=mask.data_ptr(), out=out.data_ptr())
    return out


def band_rows(H: int, W: int, n_classes: int, reach: int) -> int:
    """The band height the library chooses (what `_band_rows=0` resolves to)."""
    rows = C.c_int()
    _lib.check(_lib.lib().uaps_morph_band_rows(int(H), int(W), int(n_classes) + 1, int(reach), C.byref(rows)), "uaps_morph_band_rows")
    return rows.value

"""Hysteresis thresholding of score maps and binary reconstruction of label maps on the kernels of csrc/hysteresis.hip.

`argmax` decides every pixel on its own: a weak defect pixel whose background probability is 0.55 is lost, a speckle of 0.51 is kept.
`hysteresis` decides regions (Canny's rule): a connected region of pixels at or above a LOW threshold is kept only if it holds a pixel
at or above a HIGH one.  `reconstruct` is its general form, binary morphological reconstruction: keep the components of a label map
that hold a marker -- opening by reconstruction (erode with `morphology`, then grow the survivors back to their true shape), or
"keep the predicted defects that touch ground truth".  Both are content-based like area opening, but the content is a second map.

Rule of `hysteresis` (scores fp32 [B,C,H,W]; with from_logits the softmax over all C channels, the sigmoid for C = 1, is formed first):
  * the selected classes never hold the background; for C = 1 the one channel is the score of class 1;
  * a pixel's class c* is the arg-max of its scores over the SELECTED classes only, the lowest class on ties -- the background's score
    takes no part, so a pixel whose overall arg-max is the background can still be a candidate;
  * the pixel is a candidate of c* iff s[c*] >= low[c*] and a seed iff s[c*] >= high[c*], compared in fp32; a pixel with a NaN among
    its selected scores is neither;
  * components are maximal sets of candidates of ONE class under `connectivity`; a component survives iff it holds a seed and has at
    least min_area pixels; the result holds the class on surviving pixels and `background` elsewhere.
Rule of `reconstruct` (mask int64 [B,H,W], markers bool / uint8 [B,H,W]): a component of a selected class of `mask` survives iff one of
its own pixels has a non-zero marker and it has at least min_area pixels; dropped pixels become `background`; every other value
(ignore labels, unselected classes) passes through untouched, and a marker on such a pixel marks nothing.

`inference.predict_instances(..., hysteresis=(low, high))` and `inference.evaluate(..., hysteresis=...)` put the hysteresis mask in the
arg-max's place, which is also what lets a one-channel sigmoid model produce a defect list.

CPU tensors take the numpy restatement below (on instances._label_image's union-find; no scipy), as in the other modules; on a ROCm
device a missing kernel is an error."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG, check_classes
from .instances import _label_image

MAX_CLASSES = _lib.HYST_MAX_CLASSES
_ws = _lib.Workspace()


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_thresholds(low, high, n: int) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """low and high as n fp32-rounded floats each (a scalar serves every class), or the ValueError that names what is wrong."""
    out = []
    for name, v in (("low", low), ("high", high)):
        if isinstance(v, (str, bytes)) or isinstance(v, bool):
            raise ValueError(f"hysteresis: {name} is a float or a sequence of floats, one per selected class")
        if hasattr(v, "__iter__") and getattr(v, "ndim", 1) != 0:
            vals = [float(t) for t in v]
            if len(vals) != n:
                raise ValueError(f"hysteresis: {name} has {len(vals)} entries for {n} selected classes")
        else:
            try:
                vals = [float(v)] * n
            except (TypeError, ValueError):
                raise ValueError(f"hysteresis: {name} is a float or a sequence of floats, one per selected class") from None
        if any(math.isnan(t) for t in vals):
            raise ValueError(f"hysteresis: {name} holds a NaN")
        out.append(tuple(float(np.float32(t)) for t in vals))           # rounded to fp32: what the kernel compares against
    if any(l > h for l, h in zip(*out)):
        raise ValueError("hysteresis: low <= high for every selected class")
    return out[0], out[1]


def _check_common(who: str, background, connectivity, min_area) -> Tuple[int, int, int]:
    if not _is_int(background) or not -2 ** 31 <= background < 2 ** 31:
        raise ValueError(f"{who}: the background is a 32-bit value")
    if connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity is 4 or 8")
    if not _is_int(min_area) or min_area < 1:
        raise ValueError(f"{who}: min_area is an integer >= 1")
    return int(background), int(connectivity), min(int(min_area), 2 ** 31 - 1)


def _check_size(who: str, B: int, H: int, W: int, C: int) -> None:
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{who}: empty input")
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG or B * C * H * W * 4 >= _TOO_BIG or B * H * W * 16 + 768 >= _TOO_BIG:
        raise ValueError(f"{who}: H*W < 2^31, every tensor and the workspace (16 bytes a pixel) below 2 GiB")


def _keep_cpu(code: np.ndarray, seed: np.ndarray, conn8: bool, min_area: int) -> np.ndarray:
    """code int64 [H,W] (0: forms nothing), seed bool [H,W] -> bool [H,W]: the pixels of the components of equal codes that hold a
    seed and at least min_area pixels."""
    H, W = code.shape
    roots = _label_image(code, conn8, 0)
    fg = roots >= 0
    idx = np.nonzero(fg)[0]
    area = np.bincount(roots[idx], minlength=H * W)
    seeded = np.zeros(H * W, dtype=bool)
    seeded[roots[idx[seed.reshape(-1)[idx]]]] = True
    r = np.where(fg, roots, 0)
    return (fg & seeded[r] & (area[r] >= min_area)).reshape(H, W)


def _codes_cpu(scores: torch.Tensor, from_logits: bool, classes, low, high):
    """code int64 [B,H,W] (class + 1 on candidates, 0 elsewhere) and seed bool [B,H,W] of the score form, compared in fp32."""
    s = scores.detach().float()
    if from_logits:
        s = torch.sigmoid(s) if s.shape[1] == 1 else torch.softmax(s, dim=1)
    s = s.numpy()
    sel = s[:, [0] * len(classes)] if s.shape[1] == 1 else s[:, list(classes)]      # [B,K,H,W]
    bad = np.isnan(sel).any(axis=1)
    k = np.argmax(np.where(np.isnan(sel), -np.inf, sel), axis=1)                    # the first of equal scores: the lowest class
    best = np.take_along_axis(sel, k[:, None], axis=1)[:, 0]
    lo, hi = np.asarray(low, dtype=np.float32)[k], np.asarray(high, dtype=np.float32)[k]
    with np.errstate(invalid="ignore"):
        cand, seed = ~bad & (best >= lo), ~bad & (best >= hi)
    code = np.where(cand, np.asarray(classes, dtype=np.int64)[k] + 1, 0)
    return code, seed


def _sorted_selection(classes, low, high):
    order = sorted(range(len(classes)), key=lambda i: classes[i])
    return tuple(classes[i] for i in order), tuple(low[i] for i in order), tuple(high[i] for i in order)


def hysteresis(scores: torch.Tensor, low, high, *, from_logits: bool = False, classes: Optional[Sequence[int]] = None,
               background: int = 0, connectivity: int = 8, min_area: int = 1) -> torch.Tensor:
    """The hysteresis mask int64 [B,H,W] of the fp32 score maps [B,C,H,W], 1 <= C <= 8 (the module's text has the rule).  low, high:
    floats or sequences with one entry per selected class, in the order of `classes`; rounded to fp32; +-inf allowed.  classes: at
    most 8 distinct classes in [0, C) other than `background` (default: all of them; C = 1: [1], the one channel's class).
    H*W < 2^31, every tensor and a workspace of 16 bytes a pixel below 2 GiB."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 4 or scores.dtype != torch.float32:
        raise TypeError("hysteresis: float32 [B,C,H,W] scores expected")
    B, Cc, H, W = scores.shape
    if not 1 <= Cc <= _lib.SEG_MAX_CLASSES:
        raise ValueError(f"hysteresis: 1..{_lib.SEG_MAX_CLASSES} channels")
    background, connectivity, min_area = _check_common("hysteresis", background, connectivity, min_area)
    if Cc == 1 and classes is None and background != 1:
        classes = (1,)
    classes = check_classes("hysteresis", classes, max(Cc, 2), background, MAX_CLASSES)
    if Cc == 1 and classes != (1,):
        raise ValueError("hysteresis: the one channel of a sigmoid head is the score of class 1: classes is [1] and the background is not 1")
    low, high = check_thresholds(low, high, len(classes))
    classes, low, high = _sorted_selection(classes, low, high)
    _check_size("hysteresis", B, H, W, Cc)
    if not scores.is_cuda:
        code, seed = _codes_cpu(scores, bool(from_logits), classes, low, high)
        out = np.full((B, H, W), background, dtype=np.int64)
        for b in range(B):
            keep = _keep_cpu(code[b], seed[b], connectivity == 8, min_area)
            out[b][keep] = code[b][keep] - 1
        return torch.from_numpy(out)
    dev = scores.device
    scores = scores.detach().contiguous()
    out = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    _lib.call("uaps_hysteresis", _lib.HysteresisCall, dev, _ws, _lib.workspace_bytes("uaps_hysteresis_workspace_bytes", B, H, W),
              B=B, C=Cc, H=H, W=W, from_logits=1 if from_logits else 0, n_classes=len(classes), classes=classes, low=low, high=high,
              background=background, connectivity=connectivity, min_area=min_area, scores=scores.data_ptr(), out=out.data_ptr())
    return out


def reconstruct(mask: torch.Tensor, markers: torch.Tensor, num_classes: int, *, classes: Optional[Sequence[int]] = None,
                background: int = 0, connectivity: int = 8, min_area: int = 1) -> torch.Tensor:
    """Binary reconstruction of the int64 label map [B,H,W] from the bool / uint8 markers [B,H,W]; a new tensor (the module's text has
    the rule).  classes: at most 8 distinct values in [0, num_classes) other than `background` (default: all of them)."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or mask.dtype != torch.int64:
        raise TypeError("reconstruct: int64 [B,H,W] label map expected")
    if not isinstance(markers, torch.Tensor) or markers.dtype not in (torch.bool, torch.uint8):
        raise TypeError("reconstruct: bool or uint8 [B,H,W] markers expected")
    if markers.shape != mask.shape or markers.device != mask.device:
        raise ValueError(f"reconstruct: markers {tuple(markers.shape)} on {markers.device}, mask {tuple(mask.shape)} on {mask.device}")
    num_classes = int(num_classes)
    if not 1 <= num_classes <= _lib.SEG_MAX_CLASSES:
        raise ValueError(f"reconstruct: num_classes in 1..{_lib.SEG_MAX_CLASSES}")
    background, connectivity, min_area = _check_common("reconstruct", background, connectivity, min_area)
    classes = tuple(sorted(check_classes("reconstruct", classes, num_classes, background, MAX_CLASSES)))
    B, H, W = mask.shape
    _check_size("reconstruct", B, H, W, 1)
    mask = mask.detach().contiguous()
    markers = markers.detach().contiguous()
    markers = markers.view(torch.uint8) if markers.dtype == torch.bool else markers
    if not mask.is_cuda:
        m, seed = mask.numpy(), markers.numpy() != 0
        code = np.where(np.isin(m, classes), m + 1, 0)
        out = m.copy()
        for b in range(B):
            keep = _keep_cpu(code[b], seed[b], connectivity == 8, min_area)
            out[b][(code[b] != 0) & ~keep] = background
        return torch.from_numpy(out)
    dev = mask.device
    out = torch.empty_like(mask)
    _lib.call("uaps_hysteresis", _lib.HysteresisCall, dev, _ws, _lib.workspace_bytes("uaps_hysteresis_workspace_bytes", B, H, W),
              B=B, C=0, H=H, W=W, n_classes=len(classes), classes=classes, background=background, connectivity=connectivity,
              min_area=min_area, mask=mask.data_ptr(), markers=markers.data_ptr(), out=out.data_ptr())
    return out

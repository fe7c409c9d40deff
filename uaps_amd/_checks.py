"""Argument checks the post-processing wrappers share (instances, surface, matching, detection, curves, morphology, components,
shapes, skeleton, hull, contours)."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

TOO_BIG = 2 ** 31                        # the kernels index pixels and bytes with 32-bit integers
LABEL_DTYPE_CODE = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}       # UAPS_LABEL_*


def as_labels(t: torch.Tensor) -> torch.Tensor:
    """uint8, int32 and int64 travel as they are; bool and the other integer types are widened first."""
    if t.dtype in LABEL_DTYPE_CODE:
        return t
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if t.dtype in (torch.int8, torch.int16):
        return t.to(torch.int32)
    raise TypeError(f"an integer or bool tensor expected, got {t.dtype}")


def check_classes(what: str, classes, num_classes: int, background: int, limit: int) -> Tuple[int, ...]:
    """The classes a clean-up chain works on: 1..limit distinct values in [0, num_classes) other than the background (None: all)."""
    if classes is None:
        classes = [c for c in range(num_classes) if c != background]
    classes = tuple(int(c) for c in classes)
    if not 1 <= len(classes) <= limit or len(set(classes)) != len(classes):
        raise ValueError(f"{what}: 1..{limit} distinct classes")
    if any(c < 0 or c >= num_classes or c == background for c in classes):
        raise ValueError(f"{what}: classes lie in [0, num_classes) and differ from the background")
    return classes


def check_instances(who: str, inst, max_extent: int) -> Tuple[torch.Tensor, int, int, int, int]:
    """What every descriptor of an instances.InstanceResult asks of it: int32 [B,H,W] labels, an int64 [B,max_instances,9] table,
    nothing empty and H, W <= max_extent.  Returns (labels, B, H, W, max_instances).  The caller's byte limits stay with the caller.
    A caller's own checks (connectivity, classes) come after all of these: of two faults at once, the one listed here is reported."""
    from .instances import InstanceResult
    if not isinstance(inst, InstanceResult):
        raise TypeError(f"{who}: an instances.InstanceResult expected")
    labels = inst.labels
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.dtype != torch.int32:
        raise TypeError(f"{who}: int32 [B,H,W] labels expected")
    B, H, W = labels.shape
    if inst.table.dim() != 3 or inst.table.shape[0] != B or inst.table.shape[2] != 9:
        raise TypeError(f"{who}: the instance table is int64 [B,max_instances,9]")
    M = int(inst.max_instances)
    if B < 1 or H < 1 or W < 1 or M < 1:
        raise ValueError(f"{who}: empty labels")
    if H > max_extent or W > max_extent:
        raise ValueError(f"{who}: H and W up to {max_extent}")
    return labels, B, H, W, M


def check_plane(who: str, plane, labels: torch.Tensor) -> torch.Tensor:
    """The optional plane of shape_descriptors and skeleton_descriptors: int32, of the labels' shape, on their device."""
    if not isinstance(plane, torch.Tensor) or plane.dtype != torch.int32 or plane.shape != labels.shape or plane.device != labels.device:
        raise TypeError(f"{who}: the plane is an int32 [B,H,W] tensor on the labels' device")
    return plane


def check_instance_pair(who: str, pred, target, num_classes: int, max_classes: int):
    """The two InstanceResults of match_instances and detection_match: one device, one shape, 1 <= num_classes <= max_classes,
    H*W < 2^31 and a dense pair matrix below 2 GiB.  Returns (B, H, W, Mp, Mg, num_classes, valid); valid: bool [B], false where
    either side has more components than table rows."""
    from .instances import InstanceResult
    for r, what in ((pred, "pred"), (target, "target")):
        if not isinstance(r, InstanceResult):
            raise TypeError(f"{who}: {what} is a result of label_instances")
    if pred.labels.device != target.labels.device:
        raise ValueError(f"{who}: pred is on {pred.labels.device}, target on {target.labels.device}")
    if pred.labels.shape != target.labels.shape:
        raise ValueError(f"{who}: pred labels {tuple(pred.labels.shape)}, target labels {tuple(target.labels.shape)}")
    Cn = int(num_classes)
    if not 1 <= Cn <= max_classes:
        raise ValueError(f"{who}: 1 <= num_classes <= {max_classes}")
    B, H, W = pred.labels.shape
    Mp, Mg = pred.max_instances, target.max_instances
    if H * W >= TOO_BIG:
        raise ValueError(f"{who}: H*W < 2^31")
    if B * Mp * Mg * 4 >= TOO_BIG:
        raise ValueError(f"{who}: the dense pair matrix of B * {Mp} * {Mg} * 4 bytes reaches 2 GiB: lower max_instances")
    return B, H, W, Mp, Mg, Cn, ~(pred.overflow | target.overflow)


def pair_operands(pred, target) -> Dict[str, torch.Tensor]:
    """The six contiguous operands of a pair call, under the call's field names; the caller holds them until the call is made."""
    return {side + "_" + name: getattr(r, name).contiguous() for side, r in (("pred", pred), ("target", target))
            for name in ("labels", "count", "table")}


def pair_matrix_np(pred, target, b: int, agnostic: bool):
    """The numpy restatement of image b's pair matrix (csrc/pair_count.hpp): inter[p - 1, g - 1] counts the pixels that carry
    prediction number p and ground-truth number g, both up to their side's min(count, max_instances) and of one class (agnostic:
    of any).  Returns (inter, n_pred, n_gt)."""
    tp_, tg_ = pred.table.numpy(), target.table.numpy()
    np_, ng = max(0, min(int(pred.count[b]), tp_.shape[1])), max(0, min(int(target.count[b]), tg_.shape[1]))
    p, g = pred.labels[b].numpy().reshape(-1).astype(np.int64), target.labels[b].numpy().reshape(-1).astype(np.int64)
    sel = (p >= 1) & (p <= np_) & (g >= 1) & (g <= ng)
    p, g = p[sel] - 1, g[sel] - 1
    if not agnostic:
        same = tp_[b, p, 0] == tg_[b, g, 0]
        p, g = p[same], g[same]
    inter = np.bincount(p * ng + g, minlength=np_ * ng).reshape(np_, ng) if np_ and ng else np.zeros((np_, ng), dtype=np.int64)
    return inter, np_, ng

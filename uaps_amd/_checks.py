"""Argument checks the post-processing wrappers share (instances, surface, matching, curves, morphology, components, shapes)."""
from __future__ import annotations

from typing import Tuple

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

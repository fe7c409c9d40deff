"""What the loss wrappers of mean_teacher.py, cct_dct.py and cps.py share."""
from __future__ import annotations

import torch

from . import _lib, fused


def _logits(t: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_device(t, what)
    if t.dtype != torch.float32 or t.dim() != 4:
        raise ValueError(f"{what}: float32 [N,C,H,W] logits expected, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: contiguous logits expected")
    return t


def _grad_scalar(g, ref):
    return torch.zeros((), dtype=torch.float32, device=ref.device) if g is None else g.contiguous().to(torch.float32)


class _Halves(torch.autograd.Function):
    """rows [:B] and [B:] of forward_pair's logits; their two gradients are joined by one kernel (fused.cat_batches)."""

    @staticmethod
    def forward(ctx, both, B):
        ctx.B = B
        return both[:B], both[B:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        ref = ga if ga is not None else gb
        ga = ga.contiguous() if ga is not None else torch.zeros_like(ref)
        gb = gb.contiguous() if gb is not None else torch.zeros_like(ref)
        return fused.cat_batches(ga, gb), None

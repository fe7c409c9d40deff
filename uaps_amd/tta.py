"""Multi-scale + horizontal-flip test-time augmentation: the reference's `BaseNet.forward(x, tta=True)` (utilities/base.py:24-46) on the
two kernels of csrc/tta.hip.

    scales = [0.5, 0.75, 1.0, 1.5, 2.0];  h, w = x.shape[-2:]
    for s in scales:
        cur  = interpolate(x, (int(h*s), int(w*s)), bilinear, align_corners=True)
        acc  = (acc +) interpolate(softmax(net(cur), 1),                 (h, w), bilinear, align_corners=True)
        acc +=        interpolate(softmax(net(cur.flip(3)), 1).flip(3), (h, w), bilinear, align_corners=True)
    return acc                      # the SUM of 10 probability maps, not normalised

`tta_views` is the input side of one scale (resize, and the same values mirrored behind it: one forward of 2B images serves both
views -- eval-mode BatchNorm uses running statistics, the images do not interact), `tta_fold` the output side of all scales in one
launch (softmax at the four source corners, bilinear mix, running sums in registers, in the reference's order), `predict_tta` the
loop around a model.  CPU tensors take the torch composition above, as in the other modules; on a ROCm device a missing kernel is an
error.  One-channel sigmoid heads, vertical flips / rot90 views, per-view weights, a captured (hipGraph) TTA and TTA while training are
out of scope."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib

DEFAULT_SCALES = (0.5, 0.75, 1.0, 1.5, 2.0)
WANT = ("probs", "mask", "conf")


class TTAResult(NamedTuple):
    """probs: fp32 [B,C,H,W], the SUM of the views' probability maps (not normalised); mask: int64 [B,H,W], its arg-max (lowest
    index among equal sums); conf: fp32 [B,H,W], the largest sum / number of views.  None for what was not asked for."""
    probs: Optional[torch.Tensor]
    mask: Optional[torch.Tensor]
    conf: Optional[torch.Tensor]


def scaled_sizes(H: int, W: int, scales: Sequence[float] = DEFAULT_SCALES, size_multiple: int = 1):
    """[(h, w)] per scale.  size_multiple == 1: the reference's int(H * s).  size_multiple == m > 1 (an extension: the U-Net needs
    multiples of 16, ResUAPS of 8): the nearest positive multiple, max(m, m * floor(H * s / m + 0.5))."""
    m = int(size_multiple)
    if m < 1:
        raise ValueError("size_multiple must be >= 1")

    def one(n, s):
        return int(n * s) if m == 1 else max(m, m * int(math.floor(n * s / m + 0.5)))
    sizes = [(one(H, s), one(W, s)) for s in scales]
    if any(h < 1 or w < 1 for h, w in sizes):
        raise ValueError(f"scales {tuple(scales)} give an empty view of a {H} x {W} image")
    return sizes


def _resize(t, size):
    return F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=True)


def tta_views(x: torch.Tensor, size: Tuple[int, int], flip: bool = True) -> torch.Tensor:
    """[2B,Cin,h,w]: x resized to `size` (bilinear, align_corners=True) in images 0..B-1 and its horizontal flip in B..2B-1;
    flip=False: the first B only."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise TypeError("tta_views: float32 [B,Cin,H,W] expected")
    h, w = int(size[0]), int(size[1])
    if not x.is_cuda:
        r = _resize(x, (h, w))
        return torch.cat([r, r.flip(3)]) if flip else r
    x = x.detach().contiguous()
    B, Cin, H, W = x.shape
    out = torch.empty(((2 if flip else 1) * B, Cin, h, w), dtype=torch.float32, device=x.device)
    _lib.call("uaps_tta_views", _lib.TTAViewsCall, x.device, B=B, Cin=Cin, H=H, W=W, h=h, w=w, flip=1 if flip else 0, x=x.data_ptr(),
              out=out.data_ptr())
    return out


def _check_fold(logits_list, flip):
    S = len(logits_list)
    if not 1 <= S <= _lib.TTA_MAX_SCALES:
        raise ValueError(f"tta_fold: 1..{_lib.TTA_MAX_SCALES} scales")
    z0 = logits_list[0]
    n = 2 if flip else 1
    for z in logits_list:
        if z.dim() != 4 or z.dtype != torch.float32 or z.device != z0.device or z.shape[:2] != z0.shape[:2]:
            raise TypeError("tta_fold: float32 [(2 if flip else 1) * B, C, h, w] logits on one device, one batch and class count")
    if z0.shape[0] % n:
        raise ValueError("tta_fold: with flip the logits hold 2B images, plain first")
    return S, z0.shape[0] // n, z0.shape[1]


def _fold_composed(logits_list, out_size, flip, B):
    """The reference's loop on the views' logits, in its order."""
    acc = None
    for z in logits_list:
        p = _resize(F.softmax(z[:B], dim=1), out_size)
        acc = p if acc is None else acc + p
        if flip:
            acc = acc + _resize(F.softmax(z[B:], dim=1).flip(3), out_size)
    return acc


def tta_fold(logits_list, out_size: Tuple[int, int], flip: bool = True, want: Sequence[str] = WANT) -> TTAResult:
    """The output side: logits_list[s] = the network's logits [(2 if flip else 1) * B, C, h_s, w_s] on tta_views of scale s.  Returns
    TTAResult(probs, mask, conf) at `out_size`, None for what `want` leaves out."""
    logits_list = list(logits_list)
    want = tuple(want)
    if not want or any(k not in WANT for k in want):
        raise ValueError(f"tta_fold: want is a non-empty subset of {WANT}")
    S, B, Cc = _check_fold(logits_list, flip)
    H, W = int(out_size[0]), int(out_size[1])
    views = S * (2 if flip else 1)
    z0 = logits_list[0]
    if not z0.is_cuda:
        acc = _fold_composed(logits_list, (H, W), flip, B)
        top = acc.max(dim=1)
        return TTAResult(acc if "probs" in want else None, top.indices if "mask" in want else None,
                         top.values / views if "conf" in want else None)
    zs = [z.detach().contiguous() for z in logits_list]
    dev = z0.device
    probs = torch.empty((B, Cc, H, W), dtype=torch.float32, device=dev) if "probs" in want else None
    mask = torch.empty((B, H, W), dtype=torch.int64, device=dev) if "mask" in want else None
    conf = torch.empty((B, H, W), dtype=torch.float32, device=dev) if "conf" in want else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.call("uaps_tta_fold", _lib.TTAFoldCall, dev, S=S, B=B, C=Cc, H=H, W=W, flip=1 if flip else 0, logits=[ptr(z) for z in zs],
              h=[z.shape[2] for z in zs], w=[z.shape[3] for z in zs], probs_sum=ptr(probs), mask=ptr(mask), conf=ptr(conf))
    return TTAResult(probs, mask, conf)


def main_logits(model: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    """The main head: `forward_main` where the model has one, else the first of its heads, or the tensor of a one-head model."""
    fm = getattr(model, "forward_main", None)
    if fm is not None:
        return fm(x)
    out = model(x)
    return out[0] if isinstance(out, (tuple, list)) else out


def default_size_multiple(model) -> int:
    """16 for the U-Net family (four 2x2 poolings), 8 for ResUAPS (its forward refuses other sizes), else the reference's 1."""
    from .res_uaps import ResUAPS
    from .unet import UNet, UNet_UAPS
    if isinstance(model, ResUAPS):
        return 8
    return 16 if isinstance(model, (UNet, UNet_UAPS)) else 1


@torch.no_grad()
def predict_tta(model: torch.nn.Module, images: torch.Tensor, scales: Sequence[float] = DEFAULT_SCALES, flip: bool = True,
                size_multiple: Optional[int] = None, joined: bool = True, want: Sequence[str] = WANT) -> TTAResult:
    """BaseNet.forward(x, tta=True) around the main head of `model` (model.eval(), no_grad): per scale one tta_views and ONE forward of
    2B images (joined=False: two forwards of B, the reference's ten), then one tta_fold over all scales.  size_multiple=None: 16 for
    the U-Net family, 8 for ResUAPS; 1 gives the reference's int(H * s) sizes."""
    model.eval()
    B, _, H, W = images.shape
    m = default_size_multiple(model) if size_multiple is None else size_multiple
    logits = []
    for size in scaled_sizes(H, W, scales, m):
        v = tta_views(images, size, flip)
        if joined or not flip:
            logits.append(main_logits(model, v))
        else:
            logits.append(torch.cat([main_logits(model, v[:B]), main_logits(model, v[B:])]))
    return tta_fold(logits, (H, W), flip, want)

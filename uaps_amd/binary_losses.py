"""One-channel sigmoid (binary) heads on the hand-written kernels of csrc/loss_binary.hip: the reference's binary loss family.

  bce_loss, dice_loss, jaccard_loss, tversky_loss     utilities/pytorch_losses.py:9-28 and the num_classes == 1 branches (:70-79,
                                                      :108-117, :153-162)
  FocalLoss, JaccardLoss, DiceLoss, BCEJaccardLoss, BCEDiceLoss, BCEFocalLoss, iou, jaccard, f_score     utilities/losses_2.py
  sigmoid_mse_loss, sigmoid_kl_loss                   the sigmoid=True branches of utilities/losses_1.py:9-48
  BinarySegLoss                                       any weighted subset of {bce, focal, jaccard, fscore, dice2, jaccard2, tversky2}
                                                      as ONE criterion
  bin_confusion, bin_metrics_from_confusion           the 2 x 2 confusion matrix of sigmoid(z) > threshold and its scores

Every term is a function of one sigmoid per pixel and four global sums (n, P = sum p, G = sum g, I = sum g p), so whatever is
selected costs one forward launch that reads each logit once (+ its finalize launch) and one backward launch.  The target is either
integer labels in {0, 1} ([B,H,W] or [B,1,H,W]) or a float soft target in [0, 1] of the logits' shape; a label outside {0, 1} enters
no term and is counted (`bin_scalars(...)["bad"]`, must be 0); a float target is not range-checked.

`seg_losses` (two and more channels, softmax) is untouched and still refuses one channel; these entry points refuse anything else.
CPU tensors do not crash: every entry point then computes the same quantities with torch ops (`compose`), as seg_losses.py does.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lossutil import _grad_scalar
from .seg_losses import _host_list

TERMS = ("bce", "focal", "jaccard", "fscore", "dice2", "jaccard2", "tversky2")     # bit t of UAPS_BIN_* = 1 << TERMS.index(name)
S_OFF = {"term": 0, "loss": 7, "bad": 8, "n": 9, "P": 10, "G": 11, "I": 12, "gP": 13, "gI": 14, "k_bce": 15, "k_focal": 16,
         "nscalars": _lib.BIN_NSCALARS}                                             # UAPS_BIN_S_* (include/uaps_hip.h)

_ws = _lib.Workspace()


def bin_scalars(scalars: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Views into the scalar block of uaps_binloss_fwd (no copies, no sync): the seven terms by name (0 where not selected), loss,
    bad, and the sums n, P = sum p, G = sum g, I = sum g p."""
    out = {name: scalars[S_OFF["term"] + t] for t, name in enumerate(TERMS)}
    out.update({k: scalars[S_OFF[k]] for k in ("loss", "bad", "n", "P", "G", "I")})
    return out


def _scalar(v, what: str) -> Optional[float]:
    """None, a host number or a one-element tensor (read back once and cached by identity and version) as a host float."""
    if v is None:
        return None
    if torch.is_tensor(v):
        if v.numel() != 1:
            raise ValueError(f"{what}: a scalar expected, got {tuple(v.shape)}")
        return _host_list(v)[0]
    return float(v)


class _Spec:
    """What a criterion computes: the term mask and coefficients and every parameter as host values."""

    def __init__(self, coefs: Dict[str, float], pos_weight=None, focal_alpha: float = 0.8, focal_gamma: float = 2.0,
                 focal_mean: bool = True, beta: float = 1.0, tversky=(0.5, 0.5), eps: float = 1e-7):
        if not coefs:
            raise ValueError("BinarySegLoss: no terms selected")
        for k in coefs:
            if k not in TERMS:
                raise ValueError(f"BinarySegLoss: unknown term {k!r}; known: {', '.join(TERMS)}")
        self.coefs = {k: float(v) for k, v in coefs.items()}
        self.names = tuple(k for k in TERMS if k in self.coefs)
        self.mask = sum(1 << TERMS.index(k) for k in self.names)
        self.pos_weight = pos_weight
        self.focal_alpha, self.focal_gamma, self.focal_mean = float(focal_alpha), float(focal_gamma), bool(focal_mean)
        self.beta, self.tversky, self.eps = float(beta), (float(tversky[0]), float(tversky[1])), float(eps)
        self._static = not torch.is_tensor(pos_weight)
        self._cparams: Dict[bool, _lib.BinLossParams] = {}

    def cparams(self, target_float: bool) -> _lib.BinLossParams:
        p = self._cparams.get(target_float)
        if p is not None:
            return p
        w = _scalar(self.pos_weight, "pos_weight")
        p = _lib.BinLossParams()
        p.struct_size, p.terms, p.target_float = C.sizeof(_lib.BinLossParams), self.mask, int(target_float)
        for k, v in self.coefs.items():
            p.coef[TERMS.index(k)] = v
        p.has_pos_weight, p.pos_weight = int(w is not None), 1.0 if w is None else w
        p.focal_alpha, p.focal_gamma, p.focal_mean = self.focal_alpha, self.focal_gamma, int(self.focal_mean)
        p.beta, p.eps = self.beta, self.eps
        p.tversky_alpha, p.tversky_beta = self.tversky
        if self._static:
            self._cparams[target_float] = p
        return p


@functools.lru_cache(maxsize=64)
def _spec_of(term: str, pos_weight: Optional[float] = None, beta: float = 1.0, tversky=(0.5, 0.5), eps: float = 1e-7) -> _Spec:
    """The one-term criterion of a functional entry point, built once per parameter set: a `_Spec` caches its ctypes record, and
    rebuilding both on every call is the host cost DESIGN.md 3.14 records for SegLoss."""
    return _Spec({term: 1.0}, pos_weight=pos_weight, beta=beta, tversky=tversky, eps=eps)


def _check(logits: torch.Tensor, target: torch.Tensor, what: str):
    """The logits [B,1,H,W] fp32 and the target as the kernels take it: int64 [B,H,W] labels or a float32 map of the logits' shape."""
    if logits.dim() != 4:
        raise ValueError(f"{what}: logits must be [B,1,H,W], got {tuple(logits.shape)}")
    B, Cc, H, W = logits.shape
    if Cc != 1:
        raise ValueError(f"{what}: the one-channel sigmoid form, the logits have {Cc} channels; the softmax family is uaps_amd.seg_losses")
    if logits.dtype != torch.float32:
        raise TypeError(f"{what}: logits must be float32 (the reference computes the loss in fp32), got {logits.dtype}")
    if tuple(target.shape) not in ((B, H, W), (B, 1, H, W)):
        raise ValueError(f"{what}: target must be [B,H,W] or [B,1,H,W] = {B, H, W}, got {tuple(target.shape)}")
    if target.device != logits.device:
        raise ValueError(f"{what}: target on {target.device}, logits on {logits.device}")
    if target.is_floating_point():
        return target.reshape(B, 1, H, W).to(torch.float32).contiguous()
    return target.reshape(B, H, W).to(torch.int64).contiguous()


def compose(spec: _Spec, logits: torch.Tensor, target: torch.Tensor):
    """The same quantities as the kernels from torch ops on whatever device the tensors live on (the CPU path of every entry point;
    tools/bench_binloss.py runs it on the GPU as the composed baseline).  `target` as `_check` returns it.  Returns (loss, scalars):
    `loss` differentiable through autograd, `scalars` in the layout of `S_OFF` with the backward's factor slots left at 0."""
    F = torch.nn.functional
    z = logits.reshape(-1)
    if target.is_floating_point():
        g, ok = target.reshape(-1).to(z.dtype), None
        bad = z.new_zeros(())
    else:
        t = target.reshape(-1)
        okb = (t == 0) | (t == 1)
        ok, g = okb.to(z.dtype), (t == 1).to(z.dtype)
        bad = (~okb).sum().to(z.dtype)
    m = (lambda v: v) if ok is None else (lambda v: v * ok)
    p = torch.sigmoid(z)
    n = z.new_tensor(float(z.numel())) if ok is None else ok.sum()
    nd = n.clamp(min=1.0)                            # no label in range: the means are 0, as the kernels define it
    P, G, I = m(p).sum(), m(g).sum(), m(g * p).sum()
    zero = z.new_zeros(())
    term = {k: zero for k in TERMS}
    if "bce" in spec.coefs:
        w = _scalar(spec.pos_weight, "pos_weight")
        pw = None if w is None else z.new_tensor(w)
        term["bce"] = m(F.binary_cross_entropy_with_logits(z, g, pos_weight=pw, reduction="none")).sum() / nd
    if "focal" in spec.coefs:
        l0 = F.binary_cross_entropy_with_logits(z, g, reduction="none")
        f = m(spec.focal_alpha * (1 - torch.exp(-l0)) ** spec.focal_gamma * l0).sum()           # e^{-l0} not detached (losses_2.py:20)
        term["focal"] = f / nd if spec.focal_mean else f
    eps = spec.eps
    if "jaccard" in spec.coefs:
        term["jaccard"] = 1 - (I + eps) / (G + P - I + eps)
    if "fscore" in spec.coefs:
        b2 = spec.beta ** 2
        term["fscore"] = 1 - ((1 + b2) * I + eps) / ((1 + b2) * I + b2 * (G - I) + (P - I) + eps)
    In, An, Nn = n - P - G + I, n - P, n - G
    if "dice2" in spec.coefs:
        term["dice2"] = 1 - 0.5 * (2 * I / (P + G + eps) + 2 * In / (An + Nn + eps))
    if "jaccard2" in spec.coefs:
        term["jaccard2"] = 1 - 0.5 * (I / (P + G - I + eps) + In / (An + Nn - In + eps))
    if "tversky2" in spec.coefs:
        al, be = spec.tversky
        term["tversky2"] = 1 - 0.5 * (I / (I + al * (P - I) + be * (G - I) + eps) + In / (In + al * (An - In) + be * (Nn - In) + eps))
    loss = sum(spec.coefs[k] * term[k] for k in spec.names)
    with torch.no_grad():
        head = torch.stack([term[k].detach() for k in TERMS] + [loss.detach(), bad, n, P.detach(), G, I.detach()])
        scalars = torch.cat([head, z.new_zeros(S_OFF["nscalars"] - head.numel())]).to(torch.float32)
    return loss, scalars


def _fwd(prm: _lib.BinLossParams, z: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    B, _, H, W = z.shape
    dev = z.device
    L = _lib.lib()
    need = C.c_size_t()
    _lib.check(L.uaps_binloss_workspace_bytes(B, H, W, C.byref(need)), "uaps_binloss_workspace_bytes")
    ws = _ws.get(dev, need.value)
    scalars = torch.empty(S_OFF["nscalars"], dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        rc = L.uaps_binloss_fwd(z.data_ptr(), t.data_ptr(), C.byref(prm), B, H, W, scalars.data_ptr(), ws.data_ptr(), ws.numel(),
                                _lib.current_stream(dev))
    _lib.check(rc, "uaps_binloss_fwd")
    return scalars


def _bwd(prm: _lib.BinLossParams, z: torch.Tensor, t: torch.Tensor, scalars: torch.Tensor, g: torch.Tensor, dz: torch.Tensor) -> None:
    B, _, H, W = z.shape
    with _lib.device_guard(z.device):
        rc = _lib.lib().uaps_binloss_bwd(z.data_ptr(), t.data_ptr(), C.byref(prm), scalars.data_ptr(), g.data_ptr(), B, H, W,
                                         dz.data_ptr(), _lib.current_stream(z.device))
    _lib.check(rc, "uaps_binloss_bwd")


class _BinLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, t, z):
        ctx.set_materialize_grads(False)
        prm = spec.cparams(t.is_floating_point())
        scalars = _fwd(prm, z, t)
        ctx.save_for_backward(t, scalars, z)
        ctx.prm = prm
        ctx.mark_non_differentiable(scalars)
        return scalars[S_OFF["loss"]].clone(), scalars

    @staticmethod
    def backward(ctx, g_loss, _g_scalars):
        t, scalars, z = ctx.saved_tensors
        if g_loss is None:
            return None, None, None
        dz = torch.empty_like(z)
        _bwd(ctx.prm, z, t, scalars, _grad_scalar(g_loss, z), dz)
        return None, None, dz


class BinLossOut(NamedTuple):
    loss: torch.Tensor          # sum_t coef_t * term_t (differentiable, 0-dim)
    scalars: torch.Tensor       # see bin_scalars()


def _run(spec: _Spec, logits: torch.Tensor, target: torch.Tensor, what: str) -> BinLossOut:
    t = _check(logits, target, what)
    if not logits.is_cuda:
        return BinLossOut(*compose(spec, logits, t))
    return BinLossOut(*_BinLossFn.apply(spec, t, logits.contiguous()))


class BinarySegLoss:
    """A weighted sum of binary terms as one fused criterion.

    terms           {name: coefficient}, names from `TERMS`: "bce" (optional scalar pos_weight), "focal" (losses_2.FocalLoss on
                    logits), "jaccard" (losses_2.JaccardLoss), "fscore" (losses_2.DiceLoss; beta), and the two-channel [pos, neg]
                    forms of pytorch_losses.py at one channel: "dice2", "jaccard2", "tversky2"
    pos_weight      None, a host number or a one-element tensor (a device tensor is read back once and cached by identity and version)
    focal_alpha, focal_gamma, focal_size_average     as losses_2.FocalLoss (0.8, 2, reduce=True)
    beta            of "fscore";  tversky: (alpha, beta) of "tversky2";  eps: every region term's epsilon

    `criterion(logits [B,1,H,W] float32, target)` returns (loss, scalars); `bin_scalars(scalars)` names the terms, the sums and the
    bad-label count.  target: integer labels in {0, 1}, [B,H,W] or [B,1,H,W], or a float soft target in [0, 1] of the logits' shape."""

    def __init__(self, terms: Dict[str, float], pos_weight=None, focal_alpha: float = 0.8, focal_gamma: float = 2.0, beta: float = 1.0,
                 tversky=(0.5, 0.5), eps: float = 1e-7, focal_size_average: bool = True):
        self.spec = _Spec(dict(terms), pos_weight=pos_weight, focal_alpha=focal_alpha, focal_gamma=focal_gamma,
                          focal_mean=focal_size_average, beta=beta, tversky=tversky, eps=eps)

    @property
    def term_names(self):
        return self.spec.names

    def __call__(self, logits: torch.Tensor, target: torch.Tensor) -> BinLossOut:
        return _run(self.spec, logits, target, "BinarySegLoss")


# ---- the reference's own call signatures ---------------------------------------------------------------------------------------------

def bce_loss(true: torch.Tensor, logits: torch.Tensor, pos_weight=None) -> torch.Tensor:
    """utilities/pytorch_losses.py:9-28: F.binary_cross_entropy_with_logits(logits, true.float(), pos_weight=pos_weight), the mean."""
    return _run(_spec_of("bce", pos_weight=_scalar(pos_weight, "pos_weight")), logits, true, "bce_loss").loss


def dice_loss(true: torch.Tensor, logits: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """utilities/pytorch_losses.py:54-89, the num_classes == 1 branch (:70-79): the mean over [sigmoid, 1 - sigmoid] of the dice ratio.
    One channel only (the softmax form at two and more channels is `uaps_amd.dice_loss` / `seg_losses`)."""
    return _run(_spec_of("dice2", eps=float(eps)), logits, true, "dice_loss").loss


def jaccard_loss(true: torch.Tensor, logits: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """utilities/pytorch_losses.py:92-128, the num_classes == 1 branch (:108-117)."""
    return _run(_spec_of("jaccard2", eps=float(eps)), logits, true, "jaccard_loss").loss


def tversky_loss(true: torch.Tensor, logits: torch.Tensor, alpha: float, beta: float, eps: float = 1e-7) -> torch.Tensor:
    """utilities/pytorch_losses.py:131-175, the num_classes == 1 branch (:153-162)."""
    return _run(_spec_of("tversky2", tversky=(float(alpha), float(beta)), eps=float(eps)), logits, true, "tversky_loss").loss


class FocalLoss(torch.nn.Module):
    """utilities/losses_2.py:7-26: alpha (1 - e^{-BCE})^gamma BCE per element, its mean (reduce=True) or the map (reduce=False).  The
    gradient flows through e^{-BCE}: the reference does not detach it.  logits=True with reduce=True runs the fused kernels;
    logits=False (probabilities in: no sigmoid to share) and reduce=False (a map, no reduction) are the torch composition."""

    def __init__(self, alpha: float = 0.8, gamma: float = 2, logits: bool = False, reduce: bool = True):
        super().__init__()
        self.alpha, self.gamma, self.logits, self.reduce = alpha, gamma, logits, reduce
        self.spec = _Spec({"focal": 1.0}, focal_alpha=alpha, focal_gamma=gamma)

    def forward(self, inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        if self.logits and self.reduce and inputs.dim() == 4 and inputs.shape[1] == 1:
            return _run(self.spec, inputs, targets, "FocalLoss").loss
        F = torch.nn.functional
        t = targets.to(inputs.dtype)
        bce = (F.binary_cross_entropy_with_logits if self.logits else F.binary_cross_entropy)(inputs, t, reduction="none")
        f = self.alpha * (1 - torch.exp(-bce)) ** self.gamma * bce
        return f.mean() if self.reduce else f


def _activate(pr: torch.Tensor, activation):
    if activation is None or activation == "none":
        return pr
    if activation == "sigmoid":
        return torch.sigmoid(pr)
    if activation == "softmax2d":
        return torch.softmax(pr, dim=-3)
    raise NotImplementedError("Activation implemented for sigmoid and softmax2d")


def _fused_ok(pr: torch.Tensor, gt: torch.Tensor, activation) -> bool:
    return activation == "sigmoid" and pr.is_cuda and pr.dim() == 4 and pr.shape[1] == 1 and pr.dtype == torch.float32


def _score_from_sums(spec: _Spec, pr, gt, what: str, ratio) -> torch.Tensor:
    """`ratio(P, G, I)` of the fused forward's sums, with the gradient of 1 - loss of `spec`'s one term.  Not the value 1 - loss:
    fp32 rounds a loss next to 1 to 1 and the score it stands for to 0 (an all-background target: iou = eps / (P + eps) ~ 1e-10)."""
    out = _run(spec, pr, gt, what)
    s = bin_scalars(out.scalars)
    val = ratio(s["P"], s["G"], s["I"])
    if out.loss.requires_grad:
        val = val + (out.loss.detach() - out.loss)               # adds an exact 0 that carries d(1 - loss)/dz
    return val


def _counts(pr, gt, threshold):
    """(tp, sum pr, sum gt) of the thresholded prediction from the confusion kernel (integer labels, 0 < threshold < 1)."""
    cm = bin_confusion(pr, gt.reshape(pr.shape[0], pr.shape[2], pr.shape[3]), threshold).to(torch.float64)   # exact up to 2^53
    return cm[1, 1], cm[0, 1] + cm[1, 1], cm[1, 0] + cm[1, 1]


def iou(pr: torch.Tensor, gt: torch.Tensor, eps: float = 1e-7, threshold: Optional[float] = None, activation="sigmoid") -> torch.Tensor:
    """utilities/losses_2.py:108-139: (I + eps) / (sum gt + sum pr - I + eps) of activation(pr), thresholded when `threshold` is given.
    On the GPU with activation "sigmoid" and [B,1,H,W] fp32 logits: threshold None comes from the fused forward's sums
    (differentiable); a threshold in (0, 1) with integer labels comes from `bin_confusion`.  Every other form (activation None /
    "softmax2d", a float `gt` with a threshold, CPU tensors) is the torch composition."""
    if _fused_ok(pr, gt, activation):
        if threshold is None:
            return _score_from_sums(_spec_of("jaccard", eps=float(eps)), pr, gt, "iou", lambda P, G, I: (I + eps) / (G + P - I + eps))
        if not gt.is_floating_point() and 0 < threshold < 1:
            tp, sp, sg = _counts(pr, gt, threshold)
            return ((tp + eps) / (sg + sp - tp + eps)).to(torch.float32)
    p = _activate(pr, activation)
    if threshold is not None:
        p = (p > threshold).float()
    g = gt.reshape(p.shape).to(p.dtype) if gt.numel() == p.numel() else gt.to(p.dtype)
    inter = torch.sum(g * p)
    return (inter + eps) / (torch.sum(g) + torch.sum(p) - inter + eps)


jaccard = iou


def f_score(pr: torch.Tensor, gt: torch.Tensor, beta: float = 1, eps: float = 1e-7, threshold: Optional[float] = None,
            activation="sigmoid") -> torch.Tensor:
    """utilities/losses_2.py:145-180: ((1 + b2) tp + eps) / ((1 + b2) tp + b2 fn + fp + eps).  The same paths as `iou`."""
    b2 = beta ** 2
    if _fused_ok(pr, gt, activation):
        if threshold is None:
            return _score_from_sums(_spec_of("fscore", beta=float(beta), eps=float(eps)), pr, gt, "f_score",
                                    lambda P, G, I: ((1 + b2) * I + eps) / ((1 + b2) * I + b2 * (G - I) + (P - I) + eps))
        if not gt.is_floating_point() and 0 < threshold < 1:
            tp, sp, sg = _counts(pr, gt, threshold)
            return (((1 + b2) * tp + eps) / ((1 + b2) * tp + b2 * (sg - tp) + (sp - tp) + eps)).to(torch.float32)
    p = _activate(pr, activation)
    if threshold is not None:
        p = (p > threshold).float()
    g = gt.reshape(p.shape).to(p.dtype) if gt.numel() == p.numel() else gt.to(p.dtype)
    tp = torch.sum(g * p)
    fp, fn = torch.sum(p) - tp, torch.sum(g) - tp
    return ((1 + b2) * tp + eps) / ((1 + b2) * tp + b2 * fn + fp + eps)


class JaccardLoss(torch.nn.Module):
    """utilities/losses_2.py:29-38: 1 - iou(y_pr, y_gt, eps, threshold=None, activation)."""
    __name__ = "jaccard_loss"

    def __init__(self, eps: float = 1e-7, activation="sigmoid"):
        super().__init__()
        self.activation, self.eps = activation, eps

    def forward(self, y_pr: torch.Tensor, y_gt: torch.Tensor) -> torch.Tensor:
        if _fused_ok(y_pr, y_gt, self.activation):
            return _run(_spec_of("jaccard", eps=float(self.eps)), y_pr, y_gt, "JaccardLoss").loss
        return 1 - iou(y_pr, y_gt, eps=self.eps, threshold=None, activation=self.activation)


class DiceLoss(torch.nn.Module):
    """utilities/losses_2.py:41-50: 1 - f_score(y_pr, y_gt, beta=1, eps, threshold=None, activation='sigmoid') -- the reference
    hard-wires the sigmoid there whatever `activation` says (:50), and so does this."""
    __name__ = "dice_loss"

    def __init__(self, eps: float = 1e-7, activation="sigmoid"):
        super().__init__()
        self.activation, self.eps = activation, eps

    def forward(self, y_pr: torch.Tensor, y_gt: torch.Tensor) -> torch.Tensor:
        if _fused_ok(y_pr, y_gt, "sigmoid"):
            return _run(_spec_of("fscore", eps=float(self.eps)), y_pr, y_gt, "DiceLoss").loss
        return 1 - f_score(y_pr, y_gt, beta=1.0, eps=self.eps, threshold=None, activation="sigmoid")


class _TwoTerm(torch.nn.Module):
    """a region term + BCE as ONE fused criterion on [B,1,H,W] logits (two launches forward, one backward)."""
    terms: Dict[str, float] = {}

    def __init__(self, eps: float = 1e-7, activation="sigmoid"):
        super().__init__()
        self.activation, self.eps = activation, eps
        self.spec = _Spec(dict(self.terms), eps=eps)

    def forward(self, y_pr: torch.Tensor, y_gt: torch.Tensor) -> torch.Tensor:
        return _run(self.spec, y_pr, y_gt, type(self).__name__).loss


class BCEJaccardLoss(_TwoTerm):
    """utilities/losses_2.py:53-63: JaccardLoss + BCEWithLogitsLoss(mean).  The sigmoid form (the reference's default activation)."""
    __name__ = "bce_jaccard_loss"
    terms = {"jaccard": 1.0, "bce": 1.0}


class BCEDiceLoss(_TwoTerm):
    """utilities/losses_2.py:81-91: 0.4 * DiceLoss + 0.6 * BCEWithLogitsLoss(mean); the reference's `loss_calc`."""
    __name__ = "bce_dice_loss"
    terms = {"fscore": 0.4, "bce": 0.6}


class BCEFocalLoss(_TwoTerm):
    """utilities/losses_2.py:94-105.  In the reference `class BCEFocalLoss(DiceLoss, FocalLoss)` calls `super().forward` twice and
    both calls resolve to DiceLoss.forward (the first base in the method resolution order): it returns dice + dice = TWICE the dice
    term, no focal and no BCE part.  This reproduces what the reference computes, not what its name says."""
    __name__ = "bce_focal_loss"
    terms = {"fscore": 2.0}


# ---- the sigmoid consistency pair ------------------------------------------------------------------------------------------------------

def _pair(a: torch.Tensor, b: torch.Tensor, what: str):
    if a.shape != b.shape:
        raise AssertionError(f"{what}: two tensors of the same size expected")               # losses_1.py:17,37 assert
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError(f"{what}: float32 expected")
    return a.contiguous(), b.contiguous()


class _SigmoidMse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        out = torch.empty_like(a)
        with _lib.device_guard(a.device):
            rc = _lib.lib().uaps_sigmoid_mse_fwd(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), _lib.current_stream(a.device))
        _lib.check(rc, "uaps_sigmoid_mse_fwd")
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        da = torch.empty_like(a)
        with _lib.device_guard(a.device):
            rc = _lib.lib().uaps_sigmoid_mse_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), a.numel(), da.data_ptr(),
                                                 _lib.current_stream(a.device))
        _lib.check(rc, "uaps_sigmoid_mse_bwd")
        return da, None


class _SigmoidKl(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        dev = a.device
        L = _lib.lib()
        need = C.c_size_t()
        _lib.check(L.uaps_binloss_workspace_bytes(1, 1, 1, C.byref(need)), "uaps_binloss_workspace_bytes")
        ws = _ws.get(dev, need.value)
        out = torch.empty((), dtype=torch.float32, device=dev)
        with _lib.device_guard(dev):
            rc = L.uaps_sigmoid_kl_fwd(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.current_stream(dev))
        _lib.check(rc, "uaps_sigmoid_kl_fwd")
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a)
        g = _grad_scalar(g, a)
        with _lib.device_guard(a.device):
            rc = _lib.lib().uaps_sigmoid_kl_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), a.numel(), da.data_ptr(),
                                                _lib.current_stream(a.device))
        _lib.check(rc, "uaps_sigmoid_kl_bwd")
        return da, None


def sigmoid_mse_loss(input_logits: torch.Tensor, target_logits: torch.Tensor) -> torch.Tensor:
    """utilities/losses_1.py:9-26 with sigmoid=True: (sigmoid(input) - sigmoid(target))^2, the elementwise map.  The gradient goes to
    the first argument only, as `consistency.softmax_mse_loss` treats its target."""
    a, b = _pair(input_logits, target_logits.detach(), "sigmoid_mse_loss")
    if not a.is_cuda:
        return (torch.sigmoid(a) - torch.sigmoid(b)) ** 2
    return _SigmoidMse.apply(a, b)


def sigmoid_kl_loss(input_logits: torch.Tensor, target_logits: torch.Tensor) -> torch.Tensor:
    """utilities/losses_1.py:29-48 with sigmoid=True: F.kl_div(log(sigmoid(input)), sigmoid(target), reduction='mean') (0-dim), with
    log sigmoid computed as -softplus(-x) (finite where the reference's log(sigmoid(x)) underflows to -inf).  Gradient to the first
    argument only."""
    a, b = _pair(input_logits, target_logits.detach(), "sigmoid_kl_loss")
    if not a.is_cuda:
        t = torch.sigmoid(b)
        return (torch.xlogy(t, t) - t * torch.nn.functional.logsigmoid(a)).mean()
    return _SigmoidKl.apply(a, b)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------------

def logit_cut(threshold: float) -> np.float32:
    """logit(threshold) as the kernel compares against it: sigmoid(z) > threshold is evaluated as z > float32(logit(threshold))."""
    return np.float32(math.log(threshold) - math.log1p(-threshold))


def bin_confusion(logits: torch.Tensor, labels: torch.Tensor, threshold: float = 0.5, out: torch.Tensor = None) -> torch.Tensor:
    """counts[t, p] = #pixels with label t in {0, 1} whose prediction sigmoid(z) > threshold is p (int64 [2,2], exact).  Evaluated
    as z > logit(threshold) (`logit_cut`); a label outside {0, 1} is not counted.  logits [B,1,H,W] float32, labels [B,H,W] or
    [B,1,H,W] of an integer type."""
    if logits.dim() != 4 or logits.shape[1] != 1 or logits.dtype != torch.float32:
        raise TypeError(f"bin_confusion: logits must be float32 [B,1,H,W], got {logits.dtype} {tuple(logits.shape)}")
    B, _, H, W = logits.shape
    if tuple(labels.shape) not in ((B, H, W), (B, 1, H, W)):
        raise ValueError(f"bin_confusion: labels must be [B,H,W] or [B,1,H,W], got {tuple(labels.shape)}")
    if labels.is_floating_point():
        raise TypeError(f"bin_confusion: integer labels expected, got {labels.dtype}")
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"bin_confusion: threshold must lie in (0, 1), got {threshold}")
    z = logits.detach().contiguous()
    y = labels.reshape(B, H, W).to(torch.int64).contiguous()
    if not z.is_cuda:
        pred = (z.reshape(B, H, W) > float(logit_cut(threshold))).to(torch.int64)
        ok = (y == 0) | (y == 1)
        cm = torch.bincount((2 * y + pred)[ok], minlength=4).reshape(2, 2)
        if out is not None:
            out.copy_(cm)
            return out
        return cm
    counts = out if out is not None else torch.empty((2, 2), dtype=torch.int64, device=z.device)
    with _lib.device_guard(z.device):
        rc = _lib.lib().uaps_bin_confusion(z.data_ptr(), y.data_ptr(), B, H, W, float(threshold), counts.data_ptr(),
                                           _lib.current_stream(z.device))
    _lib.check(rc, "uaps_bin_confusion")
    return counts


def bin_metrics_from_confusion(cm, smooth: float = 1e-10) -> Dict[str, float]:
    """Scores of the positive class from a 2 x 2 confusion matrix counts[t, p]: iou, dice (F1), precision, recall, accuracy (NaN where
    a denominator is 0), plus miou / mdice exactly as `metrics.metrics_from_confusion` gives them for the same matrix -- its
    conventions: the background class 0 is left out, a class without ground-truth pixels is NaN, `smooth` in both -- so that
    `trainer.score_validation` takes the 2 x 2 matrices unchanged and reports the same numbers."""
    from .metrics import metrics_from_confusion
    if isinstance(cm, torch.Tensor):
        cm = cm.cpu().numpy()
    cm = np.asarray(cm, dtype=np.float64)
    if cm.shape != (2, 2):
        raise ValueError(f"bin_metrics_from_confusion: a 2 x 2 matrix expected, got {cm.shape}")
    tn, fp, fn, tp = cm[0, 0], cm[0, 1], cm[1, 0], cm[1, 1]

    def ratio(a, b):
        return float(a / b) if b else float("nan")
    m = metrics_from_confusion(cm, smooth)
    return {"iou": ratio(tp, tp + fp + fn), "dice": ratio(2 * tp, 2 * tp + fp + fn), "precision": ratio(tp, tp + fp),
            "recall": ratio(tp, tp + fn), "acc": ratio(tp + tn, cm.sum()), "miou": m["miou"], "mdice": m["mdice"]}

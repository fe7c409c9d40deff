"""The reference's supervised loss library on the hand-written kernels of csrc/loss_seg.hip:

  ce_loss, jaccard_loss, tversky_loss     utilities/pytorch_losses.py:31-51, :92-128, :131-175
  FocalLoss, DiceLoss                     utilities/losses_1.py:63-97, :100-136
  SegLoss                                 any weighted subset of {ce, focal, dice, jaccard, tversky, dice_sq} as ONE criterion: the
                                          reference's empty ce_dice / ce_jaccard / focal_loss stubs (pytorch_losses.py:178-187) made real

Every term is a function of one softmax per pixel and a few per-class sums, so whatever is selected costs the same two passes: one
forward launch that reads each logit once (+ its finalize launch) and one backward launch.  `losses.ce_loss` / `losses.dice_loss`
(the forms UAPS_train.py uses) are untouched; `uaps_amd.ce_loss` stays that one, the class-weighted form here is
`uaps_amd.seg_losses.ce_loss`.

Ignored pixels (a defined extension): a pixel whose label equals the ignore index enters NO term -- the per-class sums exclude it
and focal divides by the number of valid pixels.  The reference's region losses raise on such a label (torch.eye(C)[true] indexes out
of range); with no ignored pixel every term equals the reference's.  A label outside [0, C) that is not the ignore index enters no
term either and is counted (`seg_scalars(...)["bad"]`, must be 0).

CPU tensors do not crash: every entry point then computes the same quantities with torch ops (`compose`), as unet.py does for modules.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Sequence, Union

import torch

from . import _lib
from ._lossutil import _grad_scalar

MAX_CLASSES = 8                # UAPS_MAX_CLASSES (include/uaps_hip.h)
TERMS = ("ce", "focal", "dice", "jaccard", "tversky", "dice_sq")         # bit t of UAPS_SEG_* = 1 << TERMS.index(name)
NO_IGNORE = -2 ** 63           # uaps_segloss_params::ignore_index for "nothing ignored": a value no label takes

_ws = _lib.Workspace()


def s_off(Cc: int) -> Dict[str, int]:
    """The scalar block of uaps_segloss_fwd (include/uaps_hip.h, UAPS_SEG_S_*)."""
    return {"term": 0, "loss": 6, "bad": 7, "n_valid": 8, "w_sum": 9, "k_ce": 10, "k_focal": 11, "A": 16, "I": 16 + Cc, "N": 16 + 2 * Cc,
            "Z": 16 + 3 * Cc, "gA": 16 + 4 * Cc, "gI": 16 + 5 * Cc, "gZ": 16 + 6 * Cc, "n": _lib.seg_nscalars(Cc)}


def seg_scalars(scalars: torch.Tensor, Cc: int) -> Dict[str, torch.Tensor]:
    """Views into the scalar block (no copies, no sync): the six terms by name (0 where not selected), loss, bad, n_valid, w_sum and
    the per-class sums A = sum p, I = sum p [y = c], N = #[y = c], Z = sum p^2 (Z only when dice_sq is selected)."""
    o = s_off(Cc)
    out = {name: scalars[o["term"] + t] for t, name in enumerate(TERMS)}
    out.update({k: scalars[o[k]] for k in ("loss", "bad", "n_valid", "w_sum")})
    out.update({k: scalars[o[k]:o[k] + Cc] for k in ("A", "I", "N", "Z")})
    return out


def _per_class(v, Cc: int, what: str):
    """A host list of C floats from None (ones), a host sequence or a tensor."""
    if v is None:
        return [1.0] * Cc
    v = _host_list(v) if torch.is_tensor(v) else [float(x) for x in v]
    if len(v) != Cc:
        raise ValueError(f"{what}: {len(v)} values for {Cc} classes")
    return v


_readback: Dict[int, tuple] = {}


def _host_list(t: torch.Tensor):
    """The values of a (device) tensor as a host list, read back once and cached by identity and version: an unchanged tensor costs
    no synchronisation on later calls, changing it in place costs one."""
    hit = _readback.get(id(t))
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        return hit[2]
    import weakref
    vals = [float(x) for x in t.detach().reshape(-1).cpu().tolist()]
    if len(_readback) > 64:
        _readback.clear()
    _readback[id(t)] = (weakref.ref(t), t._version, vals)
    return vals


class _Spec:
    """What a criterion computes: the term mask and coefficients and every per-class parameter as host values (None = all ones)."""

    def __init__(self, coefs: Dict[str, float], class_weight=None, ignore_index=None, focal_gamma=2.0, focal_alpha=None, focal_mean=True,
                 tversky=(0.5, 0.5), dice_sq_weight=None, eps=1e-7, smooth=1e-5):
        if not coefs:
            raise ValueError("SegLoss: no terms selected")
        for k in coefs:
            if k not in TERMS:
                raise ValueError(f"SegLoss: unknown term {k!r}; known: {', '.join(TERMS)}")
        self.coefs = {k: float(v) for k, v in coefs.items()}
        self.names = tuple(k for k in TERMS if k in self.coefs)
        self.mask = sum(1 << TERMS.index(k) for k in self.names)
        self.class_weight, self.focal_alpha, self.dice_sq_weight = class_weight, focal_alpha, dice_sq_weight
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.focal_gamma, self.focal_mean = float(focal_gamma), bool(focal_mean)
        self.tversky = (float(tversky[0]), float(tversky[1]))
        self.eps, self.smooth = float(eps), float(smooth)
        # host-valued parameters never change: one uaps_segloss_params per class count (a tensor's values are looked up every call)
        self._static = not any(torch.is_tensor(v) for v in (class_weight, focal_alpha, dice_sq_weight))
        self._cparams: Dict[int, _lib.SegLossParams] = {}

    def per_class(self, Cc: int):
        if isinstance(self.focal_alpha, (float, int)) and not isinstance(self.focal_alpha, bool):
            if Cc != 2:
                raise ValueError(f"FocalLoss: a float alpha means [alpha, 1 - alpha] and needs 2 classes, the logits have {Cc}")
            alpha = [float(self.focal_alpha), 1.0 - float(self.focal_alpha)]
        else:
            alpha = _per_class(self.focal_alpha, Cc, "focal alpha")
        return _per_class(self.class_weight, Cc, "class weights"), alpha, _per_class(self.dice_sq_weight, Cc, "DiceLoss weights")

    def cparams(self, Cc: int) -> _lib.SegLossParams:
        p = self._cparams.get(Cc)
        if p is not None:
            return p
        w, alpha, dsq = self.per_class(Cc)
        p = _lib.SegLossParams()
        p.struct_size, p.terms = C.sizeof(_lib.SegLossParams), self.mask
        for k, v in self.coefs.items():
            p.coef[TERMS.index(k)] = v
        for c in range(Cc):
            p.class_weight[c], p.focal_alpha[c], p.dice_sq_weight[c] = w[c], alpha[c], dsq[c]
        p.focal_gamma, p.focal_mean = self.focal_gamma, int(self.focal_mean)
        p.tversky_alpha, p.tversky_beta = self.tversky
        p.eps, p.smooth = self.eps, self.smooth
        p.ignore_index = NO_IGNORE if self.ignore_index is None else self.ignore_index
        if self._static:
            self._cparams[Cc] = p
        return p


def _check(logits: torch.Tensor, labels: torch.Tensor, what: str):
    if logits.dim() != 4:
        raise ValueError(f"{what}: logits must be [B,C,H,W], got {tuple(logits.shape)}")
    B, Cc, H, W = logits.shape
    if Cc == 1:
        raise NotImplementedError(f"{what}: the one-channel sigmoid branch belongs to the binary heads this project never uses")
    if not 2 <= Cc <= MAX_CLASSES:
        raise ValueError(f"{what}: {Cc} classes, supported 2..{MAX_CLASSES}")
    if logits.dtype != torch.float32:
        raise TypeError(f"{what}: logits must be float32 (the reference computes the loss in fp32), got {logits.dtype}")
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if tuple(labels.shape) != (B, H, W):
        raise ValueError(f"{what}: labels must be [B,H,W] or [B,1,H,W] = {B, H, W}, got {tuple(labels.shape)}")
    if labels.device != logits.device:
        raise ValueError(f"{what}: labels on {labels.device}, logits on {logits.device}")
    if labels.is_floating_point():
        raise TypeError(f"{what}: integer labels expected, got {labels.dtype}")
    return labels.to(torch.int64).contiguous()


def compose(spec: _Spec, logits: torch.Tensor, y: torch.Tensor):
    """The same quantities as the kernels from torch ops on whatever device the tensors live on (the CPU path of every entry point;
    tools/bench_segloss.py runs it on the GPU as the composed baseline).  Returns (loss, scalars): `loss` differentiable through
    autograd, `scalars` in the layout of `s_off` with the backward's factor slots (k_ce, k_focal, gA, gI, gZ) left at 0."""
    B, Cc, H, W = logits.shape
    w, alpha, dsq = (torch.tensor(v, dtype=logits.dtype, device=logits.device) for v in spec.per_class(Cc))
    ign = NO_IGNORE if spec.ignore_index is None else spec.ignore_index
    inside = (y >= 0) & (y < Cc)
    valid = inside & (y != ign)
    bad = (~inside & (y != ign)).sum()
    yc = torch.where(valid, y, torch.zeros_like(y))
    v = valid.to(logits.dtype)
    logp = torch.log_softmax(logits, dim=1)
    p = logp.exp()
    onehot = torch.nn.functional.one_hot(yc, Cc).permute(0, 3, 1, 2).to(logits.dtype) * v.unsqueeze(1)
    pv = p * v.unsqueeze(1)
    A, I, N, Z = pv.sum((0, 2, 3)), (pv * onehot).sum((0, 2, 3)), onehot.sum((0, 2, 3)), (pv * pv).sum((0, 2, 3))
    nll = -(logp * onehot).sum(1)
    n_valid = v.sum()
    zero = logits.new_zeros(())
    term = {k: zero for k in TERMS}
    w_sum = zero
    if "ce" in spec.coefs:
        wy = w[yc] * v
        w_sum = wy.sum()
        term["ce"] = (wy * nll).sum() / w_sum
    if "focal" in spec.coefs:
        q = (p.detach() * (1.0 - onehot)).sum(1) * v                      # 1 - p_y, detached (losses_1.py:85)
        f = (alpha[yc] * v * q ** spec.focal_gamma * nll).sum()
        term["focal"] = f / n_valid if spec.focal_mean else f
    if "dice" in spec.coefs:
        term["dice"] = 1.0 - (2.0 * I / (A + N + spec.eps)).mean()
    if "jaccard" in spec.coefs:
        term["jaccard"] = 1.0 - (I / (A + N - I + spec.eps)).mean()
    if "tversky" in spec.coefs:
        al, be = spec.tversky
        term["tversky"] = 1.0 - (I / (I + al * (A - I) + be * (N - I) + spec.eps)).mean()
    if "dice_sq" in spec.coefs:
        term["dice_sq"] = (dsq * (1.0 - (2.0 * I + spec.smooth) / (Z + N + spec.smooth))).sum() / Cc
    else:
        Z = torch.zeros_like(Z)
    loss = sum(spec.coefs[k] * term[k] for k in spec.names)
    with torch.no_grad():
        head = torch.stack([term[k].detach() for k in TERMS] + [loss.detach(), bad.to(logits.dtype), n_valid, w_sum.detach()])
        scalars = torch.cat([head, logits.new_zeros(6), A, I, N, Z, logits.new_zeros(3 * Cc)]).to(torch.float32)
    return loss, scalars


def _fwd(prm: _lib.SegLossParams, z: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    B, Cc, H, W = z.shape
    dev = z.device
    L = _lib.lib()
    need = C.c_size_t()
    _lib.check(L.uaps_segloss_workspace_bytes(B, Cc, H, W, C.byref(need)), "uaps_segloss_workspace_bytes")
    ws = _ws.get(dev, need.value)
    scalars = torch.empty(_lib.seg_nscalars(Cc), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        rc = L.uaps_segloss_fwd(z.data_ptr(), y.data_ptr(), C.byref(prm), B, Cc, H, W, scalars.data_ptr(), ws.data_ptr(), ws.numel(),
                                _lib.current_stream(dev))
    _lib.check(rc, "uaps_segloss_fwd")
    return scalars


def _bwd(prm: _lib.SegLossParams, z: torch.Tensor, y: torch.Tensor, scalars: torch.Tensor, g: torch.Tensor, dz: torch.Tensor) -> None:
    B, Cc, H, W = z.shape
    with _lib.device_guard(z.device):
        rc = _lib.lib().uaps_segloss_bwd(z.data_ptr(), y.data_ptr(), C.byref(prm), scalars.data_ptr(), g.data_ptr(), B, Cc, H, W,
                                         dz.data_ptr(), _lib.current_stream(z.device))
    _lib.check(rc, "uaps_segloss_bwd")


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, y, z):
        ctx.set_materialize_grads(False)
        prm = spec.cparams(z.shape[1])
        scalars = _fwd(prm, z, y)
        ctx.save_for_backward(y, scalars, z)
        ctx.prm = prm
        ctx.mark_non_differentiable(scalars)
        return scalars[s_off(z.shape[1])["loss"]].clone(), scalars

    @staticmethod
    def backward(ctx, g_loss, _g_scalars):
        y, scalars, z = ctx.saved_tensors
        if g_loss is None:
            return None, None, None
        dz = torch.empty_like(z)
        _bwd(ctx.prm, z, y, scalars, _grad_scalar(g_loss, z), dz)
        return None, None, dz


class SegLossOut(NamedTuple):
    loss: torch.Tensor          # sum_t coef_t * term_t (differentiable, 0-dim)
    scalars: torch.Tensor       # see seg_scalars()


def _run(spec: _Spec, logits: torch.Tensor, labels: torch.Tensor, what: str) -> SegLossOut:
    y = _check(logits, labels, what)
    if not logits.is_cuda:
        return SegLossOut(*compose(spec, logits, y))
    return SegLossOut(*_SegLossFn.apply(spec, y, logits.contiguous()))


class SegLoss:
    """A weighted sum of supervised terms as one fused criterion.

    terms           {name: coefficient}, names from `TERMS`: "ce" (class-weighted cross entropy), "focal", "dice", "jaccard", "tversky",
                    "dice_sq" (losses_1.DiceLoss: squared probabilities in the denominator, per-class weights, smooth 1e-5)
    class_weight    per-class weights of "ce" (host sequence or tensor; a device tensor is read back once and cached by identity
                    and version: changing it in place costs one synchronisation)
    ignore_index    label value that enters no term (None: nothing is ignored)
    focal_gamma, focal_alpha    as FocalLoss; a float alpha means [alpha, 1 - alpha] and needs 2 classes
    tversky         (alpha, beta)
    dice_sq_weight  per-class weights of "dice_sq"
    eps             the denominators' epsilon of dice / jaccard / tversky

    `criterion(logits [B,C,H,W] float32, labels [B,H,W] or [B,1,H,W])` returns (loss, scalars); `seg_scalars(scalars, C)` names the
    terms, the per-class sums and the bad-label count.  All selected terms cost the same two passes over the logits."""

    def __init__(self, terms: Dict[str, float], class_weight=None, ignore_index: Optional[int] = None, focal_gamma: float = 2.0,
                 focal_alpha=None, tversky=(0.5, 0.5), dice_sq_weight=None, eps: float = 1e-7, focal_size_average: bool = True):
        self.spec = _Spec(dict(terms), class_weight=class_weight, ignore_index=ignore_index, focal_gamma=focal_gamma,
                          focal_alpha=focal_alpha, focal_mean=focal_size_average, tversky=tversky, dice_sq_weight=dice_sq_weight, eps=eps)

    @property
    def term_names(self):
        return self.spec.names

    def __call__(self, logits: torch.Tensor, labels: torch.Tensor) -> SegLossOut:
        return _run(self.spec, logits, labels, "SegLoss")


# ---- the reference's own call signatures ---------------------------------------------------------------------------------------------

def ce_loss(true: torch.Tensor, logits: torch.Tensor, weights, ignore: int = 255) -> torch.Tensor:
    """utilities/pytorch_losses.py:31-51: F.cross_entropy(logits, true, ignore_index=ignore, weight=weights), the weighted mean over
    the pixels that are not ignored (NaN when all are, as torch).  `weights`: None, a host sequence or a tensor [C]; a device tensor is
    read back once and cached by identity and version (changing it in place costs one synchronisation)."""
    return _run(_Spec({"ce": 1.0}, class_weight=weights, ignore_index=ignore), logits, true, "ce_loss").loss


def jaccard_loss(true: torch.Tensor, logits: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """utilities/pytorch_losses.py:92-128 (multi-class branch)."""
    return _run(_Spec({"jaccard": 1.0}, eps=eps), logits, true, "jaccard_loss").loss


def tversky_loss(true: torch.Tensor, logits: torch.Tensor, alpha: float, beta: float, eps: float = 1e-7) -> torch.Tensor:
    """utilities/pytorch_losses.py:131-175 (multi-class branch)."""
    return _run(_Spec({"tversky": 1.0}, tversky=(alpha, beta), eps=eps), logits, true, "tversky_loss").loss


class FocalLoss(torch.nn.Module):
    """utilities/losses_1.py:63-97: mean (or sum) over the pixels of -alpha_y (1 - p_y)^gamma log p_y with p_y detached inside the
    modulating factor, as the reference has it (:85).  A float `alpha` becomes [alpha, 1 - alpha] and needs 2 classes; a list is per
    class; None is all ones.  input: logits [N,C,H,W] (or [N,C,L]), target: the classes, N H W values."""

    def __init__(self, gamma: float = 2, alpha: Union[None, float, Sequence[float]] = None, size_average: bool = True):
        super().__init__()
        self.gamma, self.alpha, self.size_average = gamma, alpha, size_average
        self.spec = _Spec({"focal": 1.0}, focal_gamma=gamma, focal_alpha=alpha, focal_mean=size_average)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if input.dim() < 3:
            raise NotImplementedError("FocalLoss: [N,C] inputs are not built; pass the segmentation logits [N,C,H,W]")
        if input.dim() != 4:
            input = input.reshape(input.shape[0], input.shape[1], -1, 1)
        N, _, H, W = input.shape
        if target.numel() != N * H * W:
            raise ValueError(f"FocalLoss: {target.numel()} targets for {N * H * W} pixels")
        return _run(self.spec, input, target.reshape(N, H, W), "FocalLoss").loss


class DiceLoss(torch.nn.Module):
    """utilities/losses_1.py:100-136: (1 / C) sum_c weight_c (1 - (2 I_c + 1e-5) / (sum p_c^2 + N_c + 1e-5)).
    softmax=True: `inputs` are logits and the fused kernels run.  softmax=False: `inputs` are probabilities the caller formed, not
    logits; that form runs as plain torch ops (nothing to fuse: no softmax to share)."""

    def __init__(self, n_classes: int):
        super().__init__()
        self.n_classes = int(n_classes)

    def forward(self, inputs: torch.Tensor, target: torch.Tensor, weight=None, softmax: bool = False) -> torch.Tensor:
        if inputs.dim() != 4 or inputs.shape[1] != self.n_classes:
            raise ValueError(f"DiceLoss: inputs must be [B,{self.n_classes},H,W], got {tuple(inputs.shape)}")
        if softmax:
            return _run(_Spec({"dice_sq": 1.0}, dice_sq_weight=weight), inputs, target, "DiceLoss").loss
        y = _check(inputs, target, "DiceLoss")
        w = torch.tensor(_per_class(weight, self.n_classes, "DiceLoss weights"), dtype=inputs.dtype, device=inputs.device)
        onehot = torch.nn.functional.one_hot(y, self.n_classes).permute(0, 3, 1, 2).to(inputs.dtype)
        inter, z_sum, y_sum = (inputs * onehot).sum((0, 2, 3)), (inputs * inputs).sum((0, 2, 3)), onehot.sum((0, 2, 3))
        return (w * (1.0 - (2.0 * inter + 1e-5) / (z_sum + y_sum + 1e-5))).sum() / self.n_classes

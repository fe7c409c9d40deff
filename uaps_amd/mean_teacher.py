"""Mean Teacher (MT/MT_train.py) and uncertainty-aware Mean Teacher (UAMT/UA_MT_train.py) on the single-decoder `UNet`, the
network of `BaselineTrainer`, with the hand-written kernels of csrc/loss_mean_teacher.hip:

  ema_update       update_ema_variables (MT_train.py:79-83)            one multi-tensor launch over the teacher's parameters
  teacher_inputs   x_u + clamp(0.1 randn, -0.2, 0.2) (UA_MT_train.py:180-194)   all (1 + T) B teacher inputs of a step, one launch
  mc_consistency   UA_MT_train.py:194-214 / MT_train.py:199            fused forward + closed-form student gradient

The T Monte-Carlo teacher passes of a UAMT step (the reference's T/2 forwards of 2B images each, UA_MT_train.py:188-196) run as
ONE forward of T B images under `fused.stat_groups(T // 2)`: every group of 2B images keeps the BatchNorm statistics, the
running-statistics update and the dropout draws of one reference forward.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _lib, conv, fused, losses, perturb, sibling
from ._lossutil import _Halves
from .trainer import SegTrainer, _module_prefixed, load_state_dict_any_prefix

MAX_T = 16                     # UAPS_MC_MAX_T (include/uaps_hip.h)
# The teacher noise draws from the Philox key perturb.manual_seed(seed, rank) sets, at counters of its own: the perturbation and
# dropout draws of the same key start at offset 0 and would need 2^62 counters to reach these.
NOISE_STREAM = 1 << 62


# ---- EMA teacher update ---------------------------------------------------------------------------------------------------------

def ema_alpha(decay: float, global_step: int) -> Tuple[float, float]:
    """(alpha, 1 - alpha) of update_ema_variables, in double: alpha = min(1 - 1/(global_step + 1), decay)."""
    alpha = min(1.0 - 1.0 / (float(global_step) + 1.0), float(decay))
    return alpha, 1.0 - alpha


class _EmaCounter:
    """What conv.optimizer_stepped needs of an optimizer: the teacher's parameters get a staleness counter cell of their own, bumped
    by every update, so their packed weights and BatchNorm parameter bounds are rebuilt -- and no other model's are thrown away."""

    def __init__(self, params):
        self.param_groups = [{"params": list(params)}]


class _EmaPlan:
    def __init__(self, ema_params, params):
        self.counter = _EmaCounter(ema_params)
        self.pairs = list(zip(ema_params, params))
        self.key = None

    def arrays(self):
        key = tuple((e.data_ptr(), p.data_ptr()) for e, p in self.pairs)
        if key != self.key:
            n = len(self.pairs)
            self.e = (C.c_void_p * n)(*[k[0] for k in key])
            self.p = (C.c_void_p * n)(*[k[1] for k in key])
            self.n = (C.c_long * n)(*[e.numel() for e, _ in self.pairs])
            self.key = key
        return self.e, self.p, self.n


def _plan(ema_model: torch.nn.Module, model: torch.nn.Module) -> _EmaPlan:
    plan = getattr(ema_model, "_uaps_ema_plan", None)
    if plan is None or plan.model_id != id(model):
        ema_params, params = list(ema_model.parameters()), list(model.parameters())
        if len(ema_params) != len(params):
            raise ValueError(f"ema_update: the teacher has {len(ema_params)} parameter tensors, the student {len(params)}")
        for e, p in zip(ema_params, params):
            if e.shape != p.shape or e.dtype != torch.float32 or p.dtype != torch.float32 or e.device != p.device:
                raise ValueError(f"ema_update: teacher / student parameters differ: {tuple(e.shape)} {e.dtype} {e.device} vs "
                                 f"{tuple(p.shape)} {p.dtype} {p.device}")
            if not (e.is_contiguous() and p.is_contiguous()):
                raise ValueError("ema_update: non-contiguous parameter")
            _lib.require_device(e, "ema_update")
        plan = _EmaPlan(ema_params, params)
        plan.model_id = id(model)
        object.__setattr__(ema_model, "_uaps_ema_plan", plan)     # (not a submodule / parameter: plain attribute)
    return plan


@torch.no_grad()
def ema_update(ema_model: torch.nn.Module, model: torch.nn.Module, decay: float, global_step: int) -> None:
    """update_ema_variables(model, ema_model, decay, global_step) of MT_train.py:79-83 / UA_MT_train.py:79-83 as one kernel launch:
    ema = ema * alpha + (1 - alpha) * param for every parameter (BatchNorm buffers untouched, as in the reference), then the
    teacher's parameters are marked as changed for the packed-weight and bound caches."""
    plan = _plan(ema_model, model)
    alpha, oma = ema_alpha(decay, global_step)
    e, p, n = plan.arrays()
    dev = plan.pairs[0][0].device
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_ema_update(e, p, n, len(plan.pairs), float(alpha), float(oma), _lib.current_stream(dev))
    _lib.check(rc, "uaps_ema_update")
    conv.optimizer_stepped(plan.counter)


# ---- teacher inputs ---------------------------------------------------------------------------------------------------------------

_noise_rng = perturb.RngState(0, NOISE_STREAM)


def _default_noise_rng() -> perturb.RngState:
    """The process's perturbation key at counters from NOISE_STREAM on (restarted when perturb.manual_seed changes the key)."""
    key = perturb.rng().seed
    if _noise_rng.seed != key:
        _noise_rng.seed, _noise_rng.offset = key, NOISE_STREAM
    return _noise_rng


def teacher_inputs(x_u: torch.Tensor, T: int, rng: Optional[perturb.RngState] = None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[(1 + T) B, Cin, H, W]: row r = x_u[r % B] + clamp(0.1 n, -0.2, 0.2) (UA_MT_train.py:180-181 for rows [0, B), :190-194 for
    the T Monte-Carlo rows).  `noise`: the n of every row, recorded (tests); else drawn on the device from `rng` (default: the
    process's perturbation key at counter offset NOISE_STREAM)."""
    _lib.require_device(x_u, "teacher_inputs")
    if x_u.dtype != torch.float32 or x_u.dim() != 4:
        raise ValueError(f"teacher_inputs: float32 [B,C,H,W] expected, got {x_u.dtype} {tuple(x_u.shape)}")
    if not 0 <= int(T) <= MAX_T:
        raise ValueError(f"teacher_inputs: T = {T} outside [0, {MAX_T}]")
    x_u = x_u.contiguous()
    B, Ci, H, W = x_u.shape
    out = torch.empty(((1 + T) * B, Ci, H, W), dtype=torch.float32, device=x_u.device)
    L = _lib.lib()
    with _lib.device_guard(x_u.device):
        st = _lib.current_stream(x_u.device)
        if noise is not None:
            if noise.shape != out.shape or noise.dtype != torch.float32 or noise.device != x_u.device:
                raise ValueError(f"teacher_inputs: noise of shape {tuple(out.shape)} (float32, on {x_u.device}) expected")
            noise = noise.contiguous()
            rc = L.uaps_teacher_noise_apply(x_u.data_ptr(), noise.data_ptr(), B, Ci, H, W, int(T), out.data_ptr(), st)
        else:
            seed, off = (rng or _default_noise_rng()).reserve(out.numel())
            rc = L.uaps_teacher_noise(x_u.data_ptr(), B, Ci, H, W, int(T), seed, off, out.data_ptr(), st)
    _lib.check(rc, "uaps_teacher_noise")
    return out


# ---- fused consistency --------------------------------------------------------------------------------------------------------------

_ws = _lib.Workspace()


def _workspace(dev: torch.device) -> torch.Tensor:
    n = C.c_size_t()
    _lib.check(_lib.lib().uaps_mc_consistency_workspace_bytes(C.byref(n)), "uaps_mc_consistency_workspace_bytes")
    return _ws.get(dev, n.value)


class _McConsistency(torch.autograd.Function):
    """loss of UA_MT_train.py:194-214 (mask mode: mc given) or MT_train.py:199 (mc None); gradient to the student logits only."""

    @staticmethod
    def forward(ctx, student, teacher, mc, T, threshold, want_uncertainty):
        dev = student.device
        B, Cc, H, W = student.shape
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if mc is not None else None
        unc = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_uncertainty else None
        ws = _workspace(dev)
        with _lib.device_guard(dev):
            rc = _lib.lib().uaps_mc_consistency_fwd(student.data_ptr(), teacher.data_ptr(), mc.data_ptr() if mc is not None else None,
                                                    int(T), B, Cc, H, W, float(threshold), mask.data_ptr() if mask is not None else None,
                                                    unc.data_ptr() if unc is not None else None, out3.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), _lib.current_stream(dev))
        _lib.check(rc, "uaps_mc_consistency_fwd")
        ctx.masked = mask is not None
        ctx.save_for_backward(student, teacher, mask, out3)
        ctx.mark_non_differentiable(*([out3] + ([mask] if mask is not None else []) + ([unc] if unc is not None else [])))
        return out3[0].clone(), out3, mask, unc

    @staticmethod
    def backward(ctx, g, *_unused):
        student, teacher, mask, out3 = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        g = g.contiguous()
        ds = torch.empty_like(student)
        B, Cc, H, W = student.shape
        with _lib.device_guard(student.device):
            rc = _lib.lib().uaps_mc_consistency_bwd(student.data_ptr(), teacher.data_ptr(), mask.data_ptr() if ctx.masked else None,
                                                    g.data_ptr(), out3.data_ptr() if ctx.masked else None, B, Cc, H, W, ds.data_ptr(),
                                                    _lib.current_stream(student.device))
        _lib.check(rc, "uaps_mc_consistency_bwd")
        return ds, None, None, None, None, None


class McOut:
    """loss (0-dim device tensor, differentiable w.r.t. the student), sums = (loss, sum m d, sum m) on the device, mask uint8
    [B,H,W] (mask mode), uncertainty [B,1,H,W] (on request)."""
    __slots__ = ("loss", "sums", "mask", "uncertainty")

    def __init__(self, loss, sums, mask, uncertainty):
        self.loss, self.sums, self.mask, self.uncertainty = loss, sums, mask, uncertainty


def mc_consistency_full(student: torch.Tensor, teacher: torch.Tensor, mc_logits_or_probs: Optional[torch.Tensor] = None,
                        threshold: Optional[float] = None, T: int = 8, want_uncertainty: bool = False) -> McOut:
    """`mc_consistency` with the mask, the device sums and (want_uncertainty) the uncertainty map beside the loss."""
    for t, what in ((student, "student"), (teacher, "teacher")):
        _lib.require_device(t, "mc_consistency")
        if t.dtype != torch.float32 or t.dim() != 4:
            raise ValueError(f"mc_consistency: {what} logits: float32 [B,C,H,W] expected, got {t.dtype} {tuple(t.shape)}")
    if teacher.shape != student.shape:
        raise ValueError(f"mc_consistency: teacher {tuple(teacher.shape)} vs student {tuple(student.shape)}")
    student, teacher = student.contiguous(), teacher.detach().contiguous()
    mc = None
    if threshold is None:                     # MT mode
        if mc_logits_or_probs is not None or want_uncertainty:
            raise ValueError("mc_consistency: MT mode (threshold None) takes no Monte-Carlo input and has no uncertainty map")
        T = 0
    else:
        if mc_logits_or_probs is None:
            raise ValueError("mc_consistency: mask mode needs the Monte-Carlo teacher logits (or their mean probabilities)")
        mc = mc_logits_or_probs.detach().contiguous()
        _lib.require_device(mc, "mc_consistency")
        n = mc.numel() // student.numel() if student.numel() else 0
        if mc.dtype != torch.float32 or mc.numel() != n * student.numel() or n < 1:
            raise ValueError(f"mc_consistency: Monte-Carlo input {tuple(mc.shape)} {mc.dtype} does not match the logits "
                             f"{tuple(student.shape)}")
        if n == 1 and mc.shape == student.shape:
            T = 0                             # already-averaged probabilities [B,C,H,W]
        elif n != int(T):
            raise ValueError(f"mc_consistency: Monte-Carlo logits hold {n} passes, T = {T}")
        if not 0 <= int(T) <= MAX_T:
            raise ValueError(f"mc_consistency: T = {T} outside [0, {MAX_T}]")
    loss, sums, mask, unc = _McConsistency.apply(student, teacher, mc, int(T), 0.0 if threshold is None else float(threshold),
                                                 bool(want_uncertainty))
    return McOut(loss, sums, mask, unc)


def mc_consistency(student: torch.Tensor, teacher: torch.Tensor, mc_logits_or_probs: Optional[torch.Tensor] = None,
                   threshold: Optional[float] = None, T: int = 8) -> torch.Tensor:
    """The consistency term of UAMT (threshold given) or MT (threshold None) as one fused kernel, gradient to `student` only.

    UAMT, UA_MT_train.py:194-214: `mc_logits_or_probs` is either the raw logits of the T Monte-Carlo teacher passes, [T*B,C,H,W]
    in the reference's `preds` order (pass-major), or the already-averaged probabilities [B,C,H,W] (the call form of
    sibling.uamt_consistency_loss).  loss = sum(m * (softmax(s) - softmax(e))^2) / (2 sum(m) + 1e-16), m = entropy(p_bar) < threshold.
    MT, MT_train.py:199: torch.mean((softmax(s) - softmax(e))^2).  The [T*B,C,H,W] probabilities are never materialised."""
    return mc_consistency_full(student, teacher, mc_logits_or_probs, threshold, T).loss


uamt_threshold = sibling.uamt_threshold


# ---- trainers ------------------------------------------------------------------------------------------------------------------------

class MeanTeacherTrainer(SegTrainer):
    """Mean Teacher (MT/MT_train.py:117-226) on the single-decoder U-Net of BaselineTrainer.  One `train_step` (:175-219):

      1. the student's labelled and unlabelled forwards as one pass (UNet.forward_pair);
      2. the teacher (kept in train mode, as in the reference) on x_u + clamp(0.1 n, -0.2, 0.2) under no_grad;
      3. loss = 0.5 (dice + CE) + cw * mean((softmax(student_u) - softmax(teacher))^2), cw = consistency * sigmoid_rampup(iter // 150,
         rampup), the consistency term 0 while iter_num < 1000 (:194-202);
      4. backward, Adam, then the teacher's EMA update with global_step = iter_num (:212-219).

    Adam(lr), ReduceLROnPlateau(max, min_lr 1e-7, patience 40) (:122-124); training metrics and validation score the student.
    `train_step` returns device scalars (loss, ce, dice, consistency) and the host floats cw (and threshold for UAMT); nothing in
    it synchronises with the host."""

    ramp_divisor_default = 150
    gate_iters = 1000                 # MT_train.py:196: no consistency term before this iteration
    T = 0                             # Monte-Carlo teacher passes (UAMT)

    def __init__(self, model: torch.nn.Module, ema_model: torch.nn.Module, base_lr: float = 1e-3, ema_decay: float = 0.99,
                 consistency: float = 0.1, consistency_rampup: float = 200, seed: int = 1337, ramp_divisor: Optional[int] = None,
                 overlap_comm: bool = True, track_metrics: bool = True):
        super().__init__(model, base_lr=base_lr, consistency=consistency, consistency_rampup=consistency_rampup,
                         ramp_divisor=ramp_divisor, seed=seed, overlap_comm=overlap_comm, track_metrics=track_metrics)
        self.ema_model = ema_model
        self.ema_decay = float(ema_decay)
        for p in ema_model.parameters():      # the teacher is never trained (MT_model.py: ema_model parameters detached)
            p.requires_grad_(False)
        # the teacher noise: perturb.manual_seed(seed, rank)'s key, counters of its own (ranks draw different noise)
        self.noise_rng = perturb.RngState(perturb._mix(seed, self.rank), NOISE_STREAM)

    def _teacher(self, x_u, teacher_noise):
        """(teacher logits on the noisy batch, Monte-Carlo logits [T*B,C,H,W] or None), no autograd."""
        inputs = teacher_inputs(x_u, self.T, self.noise_rng, teacher_noise)
        B = x_u.shape[0]
        with torch.no_grad():
            e = self.ema_model(inputs[:B])                                    # MT_train.py:185-186 / UA_MT_train.py:185-186
            mc = None
            if self.T:
                with fused.stat_groups(self.T // 2):                          # UA_MT_train.py:188-196: T/2 forwards of 2B images
                    mc = self.ema_model(inputs[B:])
        return e, mc

    def _consistency(self, un, e, mc, cw):
        """(consistency term as it enters the loss, its weight, the threshold or None)."""
        return mc_consistency(un, e), self.gated_weight(cw), None           # MT_train.py:199

    def gated_weight(self, cw: float) -> float:
        """The weight the consistency term enters the loss with: 0 before iteration `gate_iters` (MT_train.py:196-197)."""
        return cw if self.iter_num >= self.gate_iters else 0.0

    def train_step(self, x_l: torch.Tensor, y_l: torch.Tensor, x_u: torch.Tensor, w=None,
                   teacher_noise: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """`teacher_noise`: the recorded n of every teacher input row, [(1 + T) B, Cin, H, W] (tests); default: drawn on the device."""
        self._check_batches(x_l, x_u)
        if not self.ema_model.training:
            self.ema_model.train()                   # the reference never switches its teacher to eval mode
        cw = self.consistency_weight()
        gated = self.iter_num < self.gate_iters
        B = x_l.shape[0]
        with self._step() as backward:
            lab, un = _Halves.apply(self.model.forward_pair(x_l, x_u), B)    # MT_train.py:175 + :178 in one pass
            e, mc = self._teacher(x_u, teacher_noise)
            s = losses.uaps_sup_loss((lab,), y_l)                              # :189-192, 0.5 * (dice + CE)
            cons, wc, thr = self._consistency(un, e, mc, cw)
            loss = s.loss + cons * wc                                         # :202
            backward(loss)                                                    # :205-207; Adam (:212) on leaving
        ema_update(self.ema_model, self.model, self.ema_decay, self.iter_num)  # :219
        self._count(lab, y_l)
        sc = losses.sup_scalars(s.scalars, 1, lab.shape[1])
        self.last = {"loss": loss.detach(), "ce": sc["ce"][0], "dice": sc["dice"][0],
                     "consistency": (cons * 0.0 if gated else cons).detach(),     # MT_train.py:197: 0.0 under the gate
                     "sup": s.loss.detach(), "unsup": (cons * wc).detach(), "cw": cw}
        if thr is not None:
            self.last["threshold"] = thr
        return self.last

    def state_for_checkpoint(self, epoch: int, best_dice: float, dataparallel_prefix: bool = True) -> Dict:
        """The reference's keys (epoch, best_dice_1, state_dict, optimizer; UA_MT_train.py:349-354, MT_train.py likewise) plus
        `ema_state_dict` (the teacher, parameters and BatchNorm buffers) and this package's resume keys."""
        ck = super().state_for_checkpoint(epoch, best_dice, dataparallel_prefix)
        ck["ema_state_dict"] = _module_prefixed(self.ema_model.state_dict(), dataparallel_prefix)
        ck["teacher_noise_rng"] = (int(self.noise_rng.seed), int(self.noise_rng.offset))
        return ck

    def load_checkpoint(self, path: str, load_optimizer: bool = True) -> Dict:
        """Loads the student (and optimizer / schedule state); the teacher from `ema_state_dict` when the checkpoint has it.  A
        checkpoint written by the reference's scripts has no teacher (they save the student only): the teacher is then left
        unchanged -- initialise it yourself (e.g. from the student) if that is what you want."""
        ck = super().load_checkpoint(path, load_optimizer)
        if "ema_state_dict" in ck:
            load_state_dict_any_prefix(self.ema_model, ck["ema_state_dict"])
            conv.invalidate_packed_weights()
        if "teacher_noise_rng" in ck:
            self.noise_rng.seed, self.noise_rng.offset = (int(v) for v in ck["teacher_noise_rng"])
        return ck


class UAMTTrainer(MeanTeacherTrainer):
    """Uncertainty-aware Mean Teacher (UAMT/UA_MT_train.py:174-233): as MeanTeacherTrainer, plus T = 8 noisy Monte-Carlo teacher
    passes (ONE forward of T B images under fused.stat_groups(T // 2)), whose mean-softmax entropy masks the consistency:
    threshold = (0.75 + 2.5 cw) ln 2, cw = consistency * sigmoid_rampup(iter // 80, rampup), no iteration gate.  All (1 + T) B
    teacher inputs come from one noise launch."""

    ramp_divisor_default = 80
    gate_iters = 0

    def __init__(self, model: torch.nn.Module, ema_model: torch.nn.Module, T: int = 8, **kw):
        if int(T) < 2 or int(T) % 2 or int(T) // 2 > 8:
            raise ValueError(f"UAMTTrainer: T = {T}: an even number of passes, at most 16 (T/2 BatchNorm groups of 2B images)")
        super().__init__(model, ema_model, **kw)
        self.T = int(T)

    def _consistency(self, un, e, mc, cw):
        thr = uamt_threshold(cw)                                              # UA_MT_train.py:212
        return mc_consistency(un, e, mc, thr, T=self.T), cw, thr              # :199-214

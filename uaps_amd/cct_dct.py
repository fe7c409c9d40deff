"""CCT (CCT/CCT_train.py) on the multi-decoder net with the aux Dropout at p = 0.3 (net_factory("unet_cct")) and DCT
(DCT/DCT_train.py) on the single-decoder `UNet`, with the hand-written kernels of csrc/loss_cct_dct.hip:

  cct_consistency   CCT_train.py:195-200     mean over the aux heads of mean((softmax(main) - softmax(aux_k))^2); one forward
                                             and one backward launch for all heads, both sides trained
  rot90_batch       DCT_train.py:165-175     [x_l; x_u; torch.rot90(x_u, k, [2, 3])] + its max|.| in one launch
  rot_consistency   DCT_train.py:188         mean((softmax(r) - rot90(softmax(u), k))^2), the rotation an index map in the kernel

The trainers restate the reference's step on one grouped forward (per-group BatchNorm statistics and dropout draws of the reference's
separate forwards) and assemble the gradient of each head's halves with package kernels only: one autograd Function per step whose
backward writes the supervised rows with uaps_sup_bwd and the unlabelled / rotated rows with the consistency backward.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, bounds, losses, perturb
from ._lossutil import _grad_scalar, _logits
from .trainer import SegTrainer, _rng_state_numpy, _rng_state_plain

MAX_HEADS = 8                  # UAPS_CCT_MAX_HEADS (include/uaps_hip.h)

_ws = _lib.Workspace()


def _workspace(dev: torch.device) -> torch.Tensor:
    n = C.c_size_t()
    _lib.check(_lib.lib().uaps_cct_dct_workspace_bytes(C.byref(n)), "uaps_cct_dct_workspace_bytes")
    return _ws.get(dev, n.value)


# ---- kernel calls ---------------------------------------------------------------------------------------------------------------

def _cct_fwd(heads, b0, B):
    z0 = heads[0]
    _, Cc, H, W = z0.shape
    out = torch.empty(len(heads), dtype=torch.float32, device=z0.device)
    ws = _workspace(z0.device)
    with _lib.device_guard(z0.device):
        rc = _lib.lib().uaps_cct_consistency_fwd(_lib.ptr_array(heads), len(heads), int(b0), int(B), Cc, H, W, out.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), _lib.current_stream(z0.device))
    _lib.check(rc, "uaps_cct_consistency_fwd")
    return out


def _cct_bwd(heads, b0, B, g, dheads):
    _, Cc, H, W = heads[0].shape
    with _lib.device_guard(g.device):
        rc = _lib.lib().uaps_cct_consistency_bwd(_lib.ptr_array(heads), len(heads), int(b0), int(B), Cc, H, W, g.data_ptr(),
                                                 _lib.ptr_array(dheads), _lib.current_stream(g.device))
    _lib.check(rc, "uaps_cct_consistency_bwd")


def _rot_fwd(r, rb0, u, ub0, B, k):
    _, Cc, H, W = u.shape
    out = torch.empty(2, dtype=torch.float32, device=u.device)
    ws = _workspace(u.device)
    with _lib.device_guard(u.device):
        rc = _lib.lib().uaps_rot_consistency_fwd(r.data_ptr(), int(rb0), u.data_ptr(), int(ub0), int(B), Cc, H, W, int(k), out.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream(u.device))
    _lib.check(rc, "uaps_rot_consistency_fwd")
    return out


def _rot_bwd(r, rb0, u, ub0, B, k, g, dr, du):
    _, Cc, H, W = u.shape
    with _lib.device_guard(u.device):
        rc = _lib.lib().uaps_rot_consistency_bwd(r.data_ptr(), int(rb0), u.data_ptr(), int(ub0), int(B), Cc, H, W, int(k), g.data_ptr(),
                                                 dr.data_ptr(), du.data_ptr(), _lib.current_stream(u.device))
    _lib.check(rc, "uaps_rot_consistency_bwd")


def _sup_fwd(lab, y):
    """uaps_sup_loss's forward over the labelled rows `lab` (D views [B,C,H,W]): the scalar block (0.5/D CE + 0.5/D Dice per head)."""
    D = len(lab)
    B, Cc, H, W = lab[0].shape
    dev = lab[0].device
    L = _lib.lib()
    need = C.c_size_t()
    _lib.check(L.uaps_loss_workspace_bytes(D, B, Cc, H, W, C.byref(need)), "uaps_loss_workspace_bytes")
    ws = losses._workspace(dev, need.value)
    scalars = torch.empty(losses._s_off(D, Cc)["n"], dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        rc = L.uaps_sup_fwd(_lib.ptr_array(lab), y.data_ptr(), D, B, Cc, H, W, 0.5 / D, 0.5 / D, 1e-7, scalars.data_ptr(), ws.data_ptr(),
                            ws.numel(), _lib.current_stream(dev))
    _lib.check(rc, "uaps_sup_fwd")
    return scalars


def _sup_bwd(lab, y, scalars, g, dlab):
    D = len(lab)
    B, Cc, H, W = lab[0].shape
    with _lib.device_guard(g.device):
        rc = _lib.lib().uaps_sup_bwd(_lib.ptr_array(lab), y.data_ptr(), scalars.data_ptr(), 0.5 / D, 0.5 / D, g.data_ptr(), D, B, Cc, H, W,
                                     _lib.ptr_array(dlab), _lib.current_stream(g.device))
    _lib.check(rc, "uaps_sup_bwd")


# ---- public wrappers ---------------------------------------------------------------------------------------------------------------

class _CctConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b0, B, *heads):
        out = _cct_fwd(heads, b0, B)
        ctx.save_for_backward(*heads)
        ctx.window = (b0, B)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g, _unused):
        heads = ctx.saved_tensors
        b0, B = ctx.window
        whole = b0 == 0 and B == heads[0].shape[0]
        dheads = [torch.empty_like(h) if whole else torch.zeros_like(h) for h in heads]
        _cct_bwd(heads, b0, B, _grad_scalar(g, heads[0]), dheads)
        return (None, None) + tuple(dheads)


def cct_consistency_full(heads: Sequence[torch.Tensor], b0: int = 0, B: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`cct_consistency` with the device vector out [D] beside the loss: out[0] = the loss, out[k] = sum of the k-th term's squares."""
    heads = [_logits(h, "cct_consistency") for h in heads]
    if not 2 <= len(heads) <= MAX_HEADS:
        raise ValueError(f"cct_consistency: {len(heads)} heads, supported 2..{MAX_HEADS} (the main head and at least one auxiliary)")
    if any(h.shape != heads[0].shape or h.device != heads[0].device for h in heads):
        raise ValueError("cct_consistency: all heads must share shape and device")
    N = heads[0].shape[0]
    B = N - int(b0) if B is None else int(B)
    if not (0 <= int(b0) and B >= 1 and int(b0) + B <= N):
        raise ValueError(f"cct_consistency: window [{b0}, {int(b0) + B}) outside the {N} rows")
    return _CctConsistency.apply(int(b0), B, *heads)


def cct_consistency(heads: Sequence[torch.Tensor], b0: int = 0, B: Optional[int] = None) -> torch.Tensor:
    """CCT_train.py:195-200 on rows [b0, b0 + B) of the D head logits [N,C,H,W] (heads[0] the main decoder): (1/(D-1)) sum_k
    mean((softmax(main) - softmax(aux_k))^2), the gradient to every head (the reference detaches nothing), rows outside the window 0."""
    return cct_consistency_full(heads, b0, B)[0]


class _RotConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, k, r, u):
        out = _rot_fwd(r, 0, u, 0, u.shape[0], k)
        ctx.save_for_backward(r, u)
        ctx.k = k
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g, _unused):
        r, u = ctx.saved_tensors
        dr, du = torch.empty_like(r), torch.empty_like(u)
        _rot_bwd(r, 0, u, 0, u.shape[0], ctx.k, _grad_scalar(g, u), dr, du)
        return None, dr, du


def _rot_shapes(r, u, k):
    B, Cc, H, W = u.shape
    want = (B, Cc, W, H) if k % 2 else (B, Cc, H, W)
    if tuple(r.shape) != want:
        raise ValueError(f"rot_consistency: rotated logits {tuple(r.shape)}, expected {want} for k = {k}")


def rot_consistency(r: torch.Tensor, u: torch.Tensor, k: int) -> torch.Tensor:
    """DCT_train.py:188: mean((softmax(r) - torch.rot90(softmax(u), k, [2, 3]))^2) with r the logits of the rotated forward
    [B,C,H',W'] and u those of the plain one [B,C,H,W]; the gradient goes to both.  No rotated or softmaxed tensor is formed."""
    if int(k) not in (0, 1, 2, 3):
        raise ValueError(f"rot_consistency: k = {k} outside 0..3")
    r, u = _logits(r, "rot_consistency"), _logits(u, "rot_consistency")
    _rot_shapes(r, u, int(k))
    return _RotConsistency.apply(int(k), r, u)[0]


def rot90_batch(x_l: torch.Tensor, x_u: torch.Tensor, k: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The DCT step's input (DCT_train.py:165-175) by one kernel: (cat([x_l, x_u, rot90(x_u, k, [2, 3])]), None), or -- k odd on a
    non-square batch, where the rotated images are [B, Cin, W, H] -- (cat([x_l, x_u]), rot90(x_u, k, [2, 3])).  max|.| of what is
    written is taken on the way (the first convolution's weight gradient then runs in the fp16 form)."""
    if int(k) not in (0, 1, 2, 3):
        raise ValueError(f"rot90_batch: k = {k} outside 0..3")
    for t in (x_l, x_u):
        _lib.require_device(t, "rot90_batch")
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape != x_u.shape or t.device != x_u.device:
            raise ValueError(f"rot90_batch: two float32 [B,Cin,H,W] batches of one shape expected, got {tuple(x_l.shape)}, {tuple(x_u.shape)}")
    k = int(k)
    x_l, x_u = x_l.contiguous(), x_u.contiguous()
    B, Ci, H, W = x_u.shape
    split = k % 2 == 1 and H != W
    out = torch.empty(((2 if split else 3) * B, Ci, H, W), dtype=torch.float32, device=x_u.device)
    rot = torch.empty((B, Ci, W, H), dtype=torch.float32, device=x_u.device) if split else None
    am = bounds.new_amax(x_u.device) if bounds.enabled() else None
    with _lib.device_guard(x_u.device):
        rc = _lib.lib().uaps_rot90_batch_h(_lib.mk_hints((), am) if am is not None else None, x_l.data_ptr(), x_u.data_ptr(), B, Ci, H, W, k,
                                           out.data_ptr(), rot.data_ptr() if split else None, _lib.current_stream(x_u.device))
    _lib.check(rc, "uaps_rot90_batch")
    if am is not None:
        bounds.put(out, am)
        if rot is not None:
            bounds.put(rot, am)            # (the bound of both tensors: an upper bound of each)
    return out, rot


# ---- one step's loss: supervised rows + consistency rows, both halves of the gradient by package kernels ------------------------------

class _CctStep(torch.autograd.Function):
    """heads: D logit tensors [2B,C,H,W] of forward_pair.  Outputs (sup, sup scalars, consistency, consistency out[D]): the supervised
    loss of rows [:B] (uaps_sup_loss: (sum CE + sum Dice) / 2D) and the CCT consistency of rows [B:]."""

    @staticmethod
    def forward(ctx, y, B, *heads):
        ctx.set_materialize_grads(False)
        lab = [h[:B] for h in heads]
        scalars = _sup_fwd(lab, y)
        cons = _cct_fwd(heads, B, B)
        ctx.save_for_backward(y, scalars, *heads)
        ctx.B = B
        ctx.mark_non_differentiable(scalars, cons)
        return scalars[losses._s_off(len(heads), heads[0].shape[1])["sup"]].clone(), scalars, cons[0].clone(), cons

    @staticmethod
    def backward(ctx, g_sup, _g_scalars, g_cons, _g_out):
        y, scalars, *heads = ctx.saved_tensors
        B = ctx.B
        dheads = [torch.empty_like(h) for h in heads]
        _sup_bwd([h[:B] for h in heads], y, scalars, _grad_scalar(g_sup, heads[0]), dheads)           # rows [:B]
        _cct_bwd(heads, B, B, _grad_scalar(g_cons, heads[0]), dheads)                                  # rows [B:]
        return (None, None) + tuple(dheads)


class _DctStep(torch.autograd.Function):
    """main: [3B,C,H,W] logits of the grouped forward (labelled, unlabelled, rotated), or [2B,C,H,W] with the rotated forward's
    logits `rot` [B,C,W,H] beside it (odd k on a non-square batch).  Outputs (sup, sup scalars, consistency, (loss, sum))."""

    @staticmethod
    def forward(ctx, y, B, k, main, rot):
        ctx.set_materialize_grads(False)
        scalars = _sup_fwd([main[:B]], y)
        r, rb0 = (main, 2 * B) if rot is None else (rot, 0)
        cons = _rot_fwd(r, rb0, main, B, B, k)
        ctx.save_for_backward(y, scalars, main, rot)
        ctx.meta = (B, k)
        ctx.mark_non_differentiable(scalars, cons)
        return scalars[losses._s_off(1, main.shape[1])["sup"]].clone(), scalars, cons[0].clone(), cons

    @staticmethod
    def backward(ctx, g_sup, _g_scalars, g_cons, _g_out):
        y, scalars, main, rot = ctx.saved_tensors
        B, k = ctx.meta
        dmain = torch.empty_like(main)
        drot = torch.empty_like(rot) if rot is not None else None
        _sup_bwd([main[:B]], y, scalars, _grad_scalar(g_sup, main), [dmain])                          # rows [:B]
        r, rb0, dr = (main, 2 * B, dmain) if rot is None else (rot, 0, drot)
        _rot_bwd(r, rb0, main, B, B, k, _grad_scalar(g_cons, main), dr, dmain)                        # rows [B:2B] (+ [2B:3B])
        return None, None, None, dmain, drot


# ---- trainers ------------------------------------------------------------------------------------------------------------------------

class _ComparisonTrainer(SegTrainer):
    """What CCTTrainer, DCTTrainer and CPSTrainer share beyond SegTrainer (cw = consistency * sigmoid_rampup(iter // 150, rampup)
    with no gate, CCT_train.py:194, DCT_train.py:186): checkpoints that also hold the perturbation streams -- the Philox (key,
    counter) of the dropout / noise draws and numpy's global generator (FeatureDropout thresholds)."""

    def _stream_state(self) -> Dict:
        r = perturb.rng()
        return {"perturb_rng": (int(r.seed), int(r.offset)), "np_global_rng": _rng_state_plain(np.random.mtrand._rand)}

    def _load_stream_state(self, ck: Dict) -> None:
        if "perturb_rng" in ck:
            r = perturb.rng()
            r.seed, r.offset = (int(v) for v in ck["perturb_rng"])
        if "np_global_rng" in ck:
            np.random.set_state(_rng_state_numpy(ck["np_global_rng"]))

    def state_for_checkpoint(self, epoch: int, best_dice: float, dataparallel_prefix: bool = True) -> Dict:
        """The reference's keys (epoch, best_dice_1, state_dict, optimizer), this package's resume keys, the perturbation streams."""
        ck = super().state_for_checkpoint(epoch, best_dice, dataparallel_prefix)
        ck.update(self._stream_state())
        return ck

    def load_checkpoint(self, path: str, load_optimizer: bool = True) -> Dict:
        ck = super().load_checkpoint(path, load_optimizer)
        self._load_stream_state(ck)
        return ck


def _step_scalars(scalars, D, Cc, s, cons, cw, loss) -> Dict:
    """The device scalars a CCT / DCT step returns: ce and dice summed over the D heads, as the reference logs them."""
    sc = losses.sup_scalars(scalars, D, Cc)
    ce, dice = (sc["ce"][0], sc["dice"][0]) if D == 1 else (sc["ce"].sum(), sc["dice"].sum())
    return {"ce": ce, "dice": dice, "consistency": cons.detach(), "sup": s.detach(), "unsup": (cons * cw).detach(), "cw": cw,
            "loss": loss.detach()}


class CCTTrainer(_ComparisonTrainer):
    """Cross-consistency training (CCT/CCT_train.py:161-214) on net_factory("unet_cct") (UNet_UAPS with the aux Dropout at p = 0.3).
    One `train_step`:

      1. the labelled and unlabelled forwards (:163, :170) as one pass (UNet_UAPS.forward_pair: per-half BatchNorm statistics and
         perturbation draws);
      2. supervised = (sum of the four heads' CE + Dice) / 8 on the labelled rows (:177-192);
      3. loss = supervised + cw * (1/3) sum_k mean((softmax(main) - softmax(aux_k))^2) on the unlabelled rows (:194-202), every head
         trained; cw = 0.1 sigmoid_rampup(iter // 150, 200);
      4. backward and Adam (:205-212).

    Returns device scalars loss, ce and dice (summed over the heads, as the reference logs them, :188-189), consistency, sup, unsup and
    the host float cw; nothing in it synchronises with the host."""

    def train_step(self, x_l: torch.Tensor, y_l: torch.Tensor, x_u: torch.Tensor, w=None) -> Dict[str, torch.Tensor]:
        self._check_batches(x_l, x_u, y_l)
        cw = self.consistency_weight()
        B = x_l.shape[0]
        y = y_l.to(torch.int64).contiguous()
        with self._step() as backward:
            heads = self.model.forward_pair(x_l, x_u)                                   # CCT_train.py:163 + :170 in one pass
            s, scalars, cons, _ = _CctStep.apply(y, B, *heads)                         # :177-200
            loss = s + cons * cw                                                       # :202
            backward(loss)                                                             # :205-207; Adam (:212) on leaving
        self._count(heads[0][:B], y_l)
        self.last = _step_scalars(scalars, len(heads), heads[0].shape[1], s, cons, cw, loss)
        return self.last


class DCTTrainer(_ComparisonTrainer):
    """Dual-consistency training with rotations (DCT/DCT_train.py:162-197) on the single-decoder `UNet`.  One `train_step`:

      1. rot_times k in 0..3 (:173) from the trainer's own generator, keyed by (seed, rank) and saved in checkpoints (the reference
         draws from Python's unseeded `random`); `train_step(..., rot_times=k)` forces it;
      2. the labelled, unlabelled and rotated forwards (:165, :170, :175) as ONE forward of 3B images under stat_groups(3) on the
         output of one uaps_rot90_batch launch -- for odd k on a non-square batch the rotated images have another shape: forward_pair
         plus a forward of the rotated batch;
      3. loss = 0.5 (CE + Dice) + cw * mean((softmax(rot) - rot90(softmax(un), k))^2) (:179-191), cw = 0.1 sigmoid_rampup(iter // 150);
      4. backward and Adam (:194-197).

    Returns device scalars (loss, ce, dice, consistency, sup, unsup) and the host values cw and rot_times."""

    def __init__(self, model: torch.nn.Module, **kw):
        super().__init__(model, **kw)
        self.rot_rng = np.random.RandomState(perturb._mix(kw.get("seed", 1337), self.rank) & 0xFFFFFFFF)

    def draw_rot_times(self) -> int:
        return int(self.rot_rng.randint(0, 4))                                         # random.randrange(0, 4)

    def train_step(self, x_l: torch.Tensor, y_l: torch.Tensor, x_u: torch.Tensor, w=None,
                   rot_times: Optional[int] = None) -> Dict[str, torch.Tensor]:
        self._check_batches(x_l, x_u, y_l)
        k = self.draw_rot_times() if rot_times is None else int(rot_times)
        if k not in (0, 1, 2, 3):
            raise ValueError(f"DCTTrainer: rot_times = {k} outside 0..3")
        cw = self.consistency_weight()
        B = x_l.shape[0]
        y = y_l.to(torch.int64).contiguous()
        with self._step() as backward:
            batch, rot_x = rot90_batch(x_l, x_u, k)                                     # :174
            if rot_x is None:
                main = self.model.forward_groups(batch, groups=3)                       # :165, :170, :175 in one pass
                rot = None
            else:
                main = self.model.forward_groups(batch, groups=2)                       # forward_pair
                rot = self.model(rot_x)
            s, scalars, cons, _ = _DctStep.apply(y, B, k, main, rot)                   # :179-188
            loss = s + cons * cw                                                       # :191
            backward(loss)                                                             # :194-196; Adam (:197) on leaving
        self._count(main[:B], y_l)
        self.last = _step_scalars(scalars, 1, main.shape[1], s, cons, cw, loss)
        self.last["rot_times"] = k
        return self.last

    def state_for_checkpoint(self, epoch: int, best_dice: float, dataparallel_prefix: bool = True) -> Dict:
        ck = super().state_for_checkpoint(epoch, best_dice, dataparallel_prefix)
        ck["rot_rng"] = _rng_state_plain(self.rot_rng)
        return ck

    def load_checkpoint(self, path: str, load_optimizer: bool = True) -> Dict:
        ck = super().load_checkpoint(path, load_optimizer)
        if "rot_rng" in ck:
            self.rot_rng.set_state(_rng_state_numpy(ck["rot_rng"]))
        return ck

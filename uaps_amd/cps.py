"""CPS, cross pseudo supervision (CPS/CPS_train.py) on two `net_factory("unet_f")` networks, with the hand-written kernels of
csrc/loss_cps.hip:

  cps_loss      CPS_train.py:215-245     the 6 CE + 6 Dice terms of both networks -- each against the ground truth, and against the
                                         OTHER network's arg-max on the labelled and on the unlabelled rows -- in one forward launch
                                         (+ its finalize) and one backward launch over both logit tensors
  CPSTrainer    CPS_train.py:112-498     the step, two Adam optimizers, two ReduceLROnPlateau schedulers and two best-checkpoint rules

Pseudo-labels are the arg-max of the LOGITS with the lowest class index among equal logits: torch.argmax(softmax(z)) of the reference
except at pixels where the fp32 softmax rounds two different logits to the same probability.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, conv, losses, metrics
from . import dist as udist
from ._lossutil import _grad_scalar, _logits
from .cct_dct import _ComparisonTrainer
from .trainer import score_validation

MAX_CLASSES = 8                # UAPS_MAX_CLASSES (include/uaps_hip.h)
TERMS = ("m1_gt", "m2_gt", "m1_lab_pseudo2", "m2_lab_pseudo1", "m1_un_pseudo2", "m2_un_pseudo1")

_ws = _lib.Workspace()


def s_off(Cc: int) -> Dict[str, int]:
    """The scalar block of uaps_cps_fwd (include/uaps_hip.h, UAPS_CPS_S_*): offsets of ce[6], dice[6], sup, labeled_cps, cps, bad,
    and the per-term per-class rows a1, a2, inter, card [6][C]; "n" = the block's length."""
    return {"ce": 0, "dice": 6, "sup": 12, "labeled_cps": 13, "cps": 14, "bad": 15, "a1": 16, "a2": 16 + 6 * Cc, "inter": 16 + 12 * Cc,
            "card": 16 + 18 * Cc, "n": 16 + 24 * Cc}


def cps_scalars(scalars: torch.Tensor, Cc: int) -> Dict[str, torch.Tensor]:
    """Views into the scalar block: ce [6] and dice [6] in the order of `TERMS`, sup, labeled_cps, cps, bad, inter / card [6, C]."""
    o = s_off(Cc)
    out = {k: scalars[o[k]] for k in ("sup", "labeled_cps", "cps", "bad")}
    out["ce"], out["dice"] = scalars[o["ce"]:o["ce"] + 6], scalars[o["dice"]:o["dice"] + 6]
    for k in ("a1", "a2", "inter", "card"):
        out[k] = scalars[o[k]:o[k] + 6 * Cc].view(6, Cc)
    return out


def _workspace(dev: torch.device, N: int, b_lab: int, Cc: int, H: int, W: int) -> torch.Tensor:
    n = C.c_size_t()
    _lib.check(_lib.lib().uaps_cps_workspace_bytes(N, b_lab, Cc, H, W, C.byref(n)), "uaps_cps_workspace_bytes")
    return _ws.get(dev, n.value)


def _fwd(z1, z2, y, b_lab, want_pseudo=True):
    N, Cc, H, W = z1.shape
    dev = z1.device
    ws = _workspace(dev, N, b_lab, Cc, H, W)
    scalars = torch.empty(s_off(Cc)["n"], dtype=torch.float32, device=dev)
    p1 = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if want_pseudo else None
    p2 = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if want_pseudo else None
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_cps_fwd(z1.data_ptr(), z2.data_ptr(), y.data_ptr(), N, int(b_lab), Cc, H, W, 1e-7,
                                     p1.data_ptr() if want_pseudo else None, p2.data_ptr() if want_pseudo else None,
                                     scalars.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream(dev))
    _lib.check(rc, "uaps_cps_fwd")
    return scalars, p1, p2


def _bwd(z1, z2, y, b_lab, scalars, g_sup, g_lcps, g_cps, dz1, dz2):
    N, Cc, H, W = z1.shape
    with _lib.device_guard(z1.device):
        rc = _lib.lib().uaps_cps_bwd(z1.data_ptr(), z2.data_ptr(), y.data_ptr(), scalars.data_ptr(), g_sup.data_ptr(), g_lcps.data_ptr(),
                                     g_cps.data_ptr(), N, int(b_lab), Cc, H, W, dz1.data_ptr(), dz2.data_ptr(),
                                     _lib.current_stream(z1.device))
    _lib.check(rc, "uaps_cps_bwd")


class _CpsLoss(torch.autograd.Function):
    """Outputs (sup, labeled_cps, cps, scalars, pseudo1, pseudo2); the gradient goes to both logit tensors, the pseudo-labels carry
    none (the reference detaches them, CPS_train.py:228-239)."""

    @staticmethod
    def forward(ctx, y, b_lab, z1, z2):
        ctx.set_materialize_grads(False)
        scalars, p1, p2 = _fwd(z1, z2, y, b_lab)
        ctx.save_for_backward(y, scalars, z1, z2)
        ctx.b_lab = b_lab
        ctx.mark_non_differentiable(scalars, p1, p2)
        o = s_off(z1.shape[1])
        return scalars[o["sup"]].clone(), scalars[o["labeled_cps"]].clone(), scalars[o["cps"]].clone(), scalars, p1, p2

    @staticmethod
    def backward(ctx, g_sup, g_lcps, g_cps, _gs, _g1, _g2):
        y, scalars, z1, z2 = ctx.saved_tensors
        dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
        _bwd(z1, z2, y, ctx.b_lab, scalars, _grad_scalar(g_sup, z1), _grad_scalar(g_lcps, z1), _grad_scalar(g_cps, z1), dz1, dz2)
        return None, None, dz1, dz2


def cps_loss(z1: torch.Tensor, z2: torch.Tensor, y: torch.Tensor, b_lab: int):
    """CPS_train.py:215-245 on the logits z1, z2 [N,C,H,W] of the two networks, rows [:b_lab] labelled (y int64 [b_lab,H,W]) and rows
    [b_lab:] unlabelled.  Returns (sup, labeled_cps, cps, scalars, pseudo1, pseudo2): the three differentiable sums
    (loss = sup + cw * cps + cw * labeled_cps, :250), the scalar block (`cps_scalars`: the twelve terms) and the two networks'
    pseudo-labels as uint8 [N,H,W]."""
    z1, z2 = _logits(z1, "cps_loss"), _logits(z2, "cps_loss")
    if z1.shape != z2.shape or z1.device != z2.device:
        raise ValueError(f"cps_loss: the two logit tensors must share shape and device, got {tuple(z1.shape)} and {tuple(z2.shape)}")
    N, Cc, H, W = z1.shape
    b_lab = int(b_lab)
    if not 2 <= Cc <= MAX_CLASSES:
        raise ValueError(f"cps_loss: {Cc} classes, supported 2..{MAX_CLASSES}")
    if not 1 <= b_lab < N:
        raise ValueError(f"cps_loss: b_lab = {b_lab} must leave labelled and unlabelled rows in a batch of {N}")
    _lib.require_device(y, "cps_loss")
    if y.dtype != torch.int64 or tuple(y.shape) != (b_lab, H, W) or y.device != z1.device:
        raise ValueError(f"cps_loss: int64 labels [{b_lab},{H},{W}] on {z1.device} expected, got {y.dtype} {tuple(y.shape)} on {y.device}")
    return _CpsLoss.apply(y.contiguous(), b_lab, z1, z2)


class CPSTrainer(_ComparisonTrainer):
    """Cross pseudo supervision (CPS/CPS_train.py:112-498) on two independently initialised `net_factory("unet_f")` networks.  One
    `train_step`:

      1. both networks in train mode, each on the labelled and the unlabelled batch (:195-207) as one pass (UNet.forward_pair: per-half
         BatchNorm statistics and dropout draws); only the `dp0` logits are formed, the deep-supervision heads enter no loss term;
      2. sup = 0.5 (CE + Dice) of each network against the ground truth (:215-224);
      3. labeled_cps / cps = 0.5 CE + 0.5 Dice of each network against the other's arg-max on the labelled / unlabelled rows (:228-245);
      4. loss = sup + cw * cps + cw * labeled_cps, cw = 0.1 sigmoid_rampup(iter // 150, 200) (:247-250);
      5. one backward, Adam on each network (:252-261).

    `model`, `optimizer`, `scheduler` are network 1's, `model2`, `optimizer2`, `scheduler2` network 2's.  Returns device scalars loss,
    ce_1, dice_1, ce_2, dice_2, cps, labeled_cps, sup, unsup, the host float cw and the two networks' pseudo-labels of the step
    (pseudo1, pseudo2: uint8 [2B,H,W], for logging); nothing in it synchronises with the host.
    Single process only: the gradient buckets of `dist` hold one model."""

    plateau_min_lr, plateau_patience = 1e-7, 50          # CPS_train.py:118-119
    log_keys = ("loss", "ce_1", "dice_1", "ce_2", "dice_2", "cps", "labeled_cps", "sup", "unsup")
    weight_keys = ("cw",)
    net_suffixes = ("_1", "_2")

    def __init__(self, model1: torch.nn.Module, model2: torch.nn.Module, base_lr: float = 1e-3, consistency: float = 0.1,
                 consistency_rampup: float = 200, seed: int = 1337, ramp_divisor: int = 150, track_metrics: bool = True):
        if udist.world_size() > 1:
            raise NotImplementedError("CPSTrainer: data-parallel training of the two networks is not built (dist.GradBuckets holds one "
                                      "model); run it in a single process")
        if model1 is model2:
            raise ValueError("CPSTrainer: two networks expected, the same module was passed twice")
        super().__init__(model1, base_lr=base_lr, consistency=consistency, consistency_rampup=consistency_rampup, seed=seed,
                         ramp_divisor=ramp_divisor, track_metrics=track_metrics)
        self.model2 = model2
        params2 = list(model2.parameters())
        if params2[0].device != self.device:
            raise ValueError(f"CPSTrainer: both networks on one device expected ({self.device} vs {params2[0].device})")
        self.optimizer2, self.scheduler2 = self._new_optimizer(params2, base_lr)                           # CPS_train.py:115-119
        self._cms2: List[torch.Tensor] = []
        self.best_dice = [0.0, 0.0]                       # :457-472 (the reference starts from False == 0)
        self.patience = [0, 0]

    @property
    def models(self) -> Tuple[torch.nn.Module, torch.nn.Module]:
        return self.model, self.model2

    def _networks(self):
        return (self.model, self.optimizer, self.scheduler), (self.model2, self.optimizer2, self.scheduler2)

    def train_step(self, x_l: torch.Tensor, y_l: torch.Tensor, x_u: torch.Tensor, w=None) -> Dict[str, torch.Tensor]:
        self._check_batches(x_l, x_u, y_l)
        cw = self.consistency_weight()                                                 # :247
        B = x_l.shape[0]
        y = y_l.to(torch.int64).contiguous()
        with self._step(conv._allowed_cached(self.model2), models=self.models, optimizers=(self.optimizer, self.optimizer2)) as backward:
            z1 = self.model.forward_pair(x_l, x_u)                                      # :195 + :206 in one pass
            z2 = self.model2.forward_pair(x_l, x_u)                                     # :196 + :207
            sup, lcps, cps, scalars, p1, p2 = cps_loss(z1, z2, y, B)                    # :215-245
            loss = sup + cw * cps + cw * lcps                                           # :250
            backward(loss)                                                              # :252-255; both Adams (:260-261) on leaving
        self._count(z1[:B], y_l)                                                        # :274-278
        if self.track_metrics:
            self._cms2.append(metrics.seg_confusion(z2[:B], y_l))
        sc = cps_scalars(scalars, z1.shape[1])
        self.last = {"loss": loss.detach(), "ce_1": sc["ce"][0], "dice_1": sc["dice"][0], "ce_2": sc["ce"][1], "dice_2": sc["dice"][1],
                     "cps": cps.detach(), "labeled_cps": lcps.detach(), "sup": sup.detach(), "unsup": (cw * cps + cw * lcps).detach(),
                     "cw": cw, "pseudo1": p1, "pseudo2": p2}
        return self.last

    def epoch_metrics2(self, reset: bool = True) -> Dict[str, float]:
        """`epoch_metrics` of network 2 (CPS_train.py:277-278, 299-300)."""
        return self._score_steps(self._cms2, reset)

    def _train_metrics(self):
        return self.epoch_metrics(), self.epoch_metrics2()

    @torch.no_grad()
    def validate(self, batches, pooled: bool = False) -> Dict[str, float]:
        """CPS_train.py:350-413: both networks in eval mode on every batch; per network and batch CE, 1 - mDice, mIoU, mDice and
        accuracy, averaged over the batches.  Keys end in _1 / _2; "loss" is the reference's 0.5 (dice_loss_1 + ce_1) +
        0.5 (dice_loss_2 + ce_2) (:377).  mdice_1 / mdice_2 feed the two schedulers (:414-415) and the two best-checkpoint rules
        (:457-472).  One device->host copy at the end."""
        cms, ces = [], []
        for m in self.models:
            m.eval()
        for x, yv in batches:
            for m in self.models:
                z = m.forward_main(x)
                ces.append(losses.ce_loss(z, yv))
                cms.append(metrics.seg_confusion(z, yv))
        if not cms:
            return {k + s: float("nan") for k in ("miou", "mdice", "acc", "ce", "dice_loss") for s in ("_1", "_2")} | {"loss": float("nan")}
        cm = torch.stack(cms).cpu().numpy()
        ce = torch.stack(ces).double().cpu().numpy()
        self.check_errors()
        out: Dict[str, float] = {"loss": 0.0}
        for i, s in enumerate(self.net_suffixes):
            m = score_validation(cm[i::2], ce[i::2], pooled)
            out["loss"] += float(m.pop("loss"))
            out.update({k + s: float(v) for k, v in m.items()})
        return out

    # -- fit(): SegTrainer's loop, per network one scheduler, one strict-'>' rule (note_validation) and one file --
    def _fit_begin(self, best_dice, checkpoint_path):
        """`checkpoint_path`: a (path 1, path 2) pair, or one path "x.pth" that becomes "x_1.pth" / "x_2.pth" (the reference writes
        CPS_10p_1.pth / CPS_10p_2.pth, CPS_train.py:487, :498).  `best_dice`: the pair to resume from (the checkpoints' best_dice_1 /
        best_dice_2); None keeps the trainer's bookkeeping."""
        if best_dice is not None:
            self.best_dice = [float(best_dice[0]), float(best_dice[1])]
        return checkpoint_paths(checkpoint_path)

    def _save_network(self, i: int, path: str, epoch: int) -> None:
        self.save_checkpoint(path, epoch, which=i + 1)                                                      # :479-498

    # -- checkpoints (CPS_train.py:479-498): one file per network --
    def state_for_checkpoint(self, epoch: int, best_dice: Optional[float] = None, dataparallel_prefix: bool = False, which: int = 1) -> Dict:
        """Network `which`'s checkpoint: the reference's keys (epoch, best_dice_1 or best_dice_2, state_dict, optimizer; CPS saves the
        bare model's state_dict, no `module.` prefix) plus this package's resume keys -- iter_num, the scheduler, that network's
        best-checkpoint bookkeeping and the perturbation streams (Philox key / counter, numpy's global generator)."""
        if which not in (1, 2):
            raise ValueError(f"CPSTrainer: network {which}, expected 1 or 2")
        i = which - 1
        ck = self._net_state(self._networks()[i], epoch, "best_dice" + self.net_suffixes[i],
                             self.best_dice[i] if best_dice is None else best_dice, dataparallel_prefix)
        ck.update(self._stream_state())
        ck["patience"] = int(self.patience[i])
        return ck

    def save_checkpoint(self, path, epoch: int, best_dice=None, which: Optional[int] = None):
        """`which` = 1 or 2: that network's file at `path`.  `which` = None: both, `path` as in `fit` (a pair, or one path that gets the
        _1 / _2 suffixes); `best_dice`: None (the trainer's bookkeeping), one value or a pair."""
        if which is None:
            paths = checkpoint_paths(path)
            bd = best_dice if isinstance(best_dice, (tuple, list)) else (best_dice, best_dice)
            for i in (0, 1):
                self.save_checkpoint(paths[i], epoch, bd[i], which=i + 1)
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.state_for_checkpoint(epoch, best_dice, which=which), path)

    def load_checkpoint(self, path, load_optimizer: bool = True) -> Tuple[Dict, Dict]:
        """Resume both networks from the two files (`path` as in `fit`).  The iteration counter and the perturbation streams are
        taken from network 1's file (both files of one save hold the same)."""
        paths = checkpoint_paths(path)
        net1, net2 = self._networks()
        ck2 = self._load_net_state(net2, paths[1], load_optimizer)
        ck1 = self._load_net_state(net1, paths[0], load_optimizer)
        self._load_stream_state(ck1)
        for i, (ck, key) in enumerate(((ck1, "best_dice_1"), (ck2, "best_dice_2"))):
            if key in ck:
                self.best_dice[i] = float(ck[key])
            if "patience" in ck:
                self.patience[i] = int(ck["patience"])
        return ck1, ck2


def checkpoint_paths(path) -> Optional[Tuple[str, str]]:
    """(file of network 1, file of network 2): a pair as given, one path "x.pth" -> ("x_1.pth", "x_2.pth"), None -> None."""
    if path is None:
        return None
    if isinstance(path, (tuple, list)):
        if len(path) != 2:
            raise ValueError("CPSTrainer: a pair of checkpoint paths expected")
        return str(path[0]), str(path[1])
    root, ext = os.path.splitext(str(path))
    return root + "_1" + ext, root + "_2" + ext

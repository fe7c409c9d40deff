"""UCC, uncertainty-guided cross-head co-training with cross-cut-mix (UCC/UCC_train.py) on the two-head `net_factory("unet_ucc")`,
with the hand-written kernels of csrc/loss_ucc.hip:

  cutmix_rects   cross_cutmix.py:60-75, :89, :114   the rectangles and apply flags of one generate_mix_data / generate_crossmix_data call
  cutmix_batch   cross_cutmix.py:78-123             [mix(x_l) ; crossmix(x_wk) ; crossmix(x_st)], the mixed labels and max|.|: one launch
  ucc_loss       UCC_train.py:186-240               the 4 CE + 4 Dice terms, the two KL variance maps, sup, ps_1, ps_2 and ps in one
                                                    forward launch (+ its finalize) and one backward launch over both logit tensors
  UCCTrainer     UCC_train.py:98-418                the step, Adam, ReduceLROnPlateau and the best-checkpoint rule

Pseudo-labels are the arg-max of the LOGITS with the lowest class index among equal logits (the CPS rule, uaps_amd.cps).
`sibling.ucc_pseudo_supervision` stays the reference-shaped, composed form of the unsupervised part.
"""
from __future__ import annotations

import ctypes as C
import random
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, bounds, metrics, perturb
from ._lossutil import _grad_scalar, _logits
from .cct_dct import _ComparisonTrainer
from .trainer import _rng_state_numpy, _rng_state_plain

MAX_CLASSES = 8                # UAPS_MAX_CLASSES (include/uaps_hip.h)
MAX_BATCH = 64                 # UAPS_UCC_MAX_BATCH: the rectangles of a batch travel as kernel arguments
TERMS = ("h1_gt", "h2_gt", "h1_st_pseudo1", "h2_st_pseudo2")
P_MIX, P_CROSSMIX = 0.2, 0.3   # cross_cutmix.py:78, :101

_ws = _lib.Workspace()


# ---- the rectangles -------------------------------------------------------------------------------------------------------------------

def cutmix_rects(B: int, H: int, W: int, np_rng: np.random.RandomState, py_rng: random.Random, p: float) -> np.ndarray:
    """The draws of one generate_mix_data (p = 0.2) or generate_crossmix_data (p = 0.3) call, in the reference's order: per image
    generate_cutout_mask (cross_cutmix.py:60-75: w, x_start, y_start from `randint`, h = np.round(area / w), int() of the ends) from
    `np_rng`, then `random.random() < p` from `py_rng`.  Returns int32 [B, 5]: (flag, y0, y1, x0, x1), the mask's zero block being rows
    [y0, y1) and columns [x0, x1).  With the generators seeded like the reference's globals the masks and flags are the reference's."""
    rects = np.zeros((int(B), 5), dtype=np.int32)
    for i in range(int(B)):
        cutout_area = H * W / 2                                   # ratio = 2
        w = np_rng.randint(W / 2 + 1, W)
        h = np.round(cutout_area / w)
        x_start = np_rng.randint(0, W - w + 1)
        y_start = np_rng.randint(0, H - h + 1)
        x_end, y_end = int(x_start + w), int(y_start + h)
        flag = py_rng.random() < p
        rects[i] = (int(flag), y_start, min(y_end, H), x_start, min(x_end, W))     # (a slice past the edge ends at the edge)
    return rects


def _check_rects(r, B: int, H: int, W: int, what: str) -> np.ndarray:
    r = np.ascontiguousarray(np.asarray(r), dtype=np.int32)
    if r.shape != (B, 5):
        raise ValueError(f"cutmix_batch: {what}: int [{B}, 5] rows (flag, y0, y1, x0, x1) expected, got {r.shape}")
    if ((r[:, 1] < 0) | (r[:, 2] < r[:, 1]) | (r[:, 2] > H) | (r[:, 3] < 0) | (r[:, 4] < r[:, 3]) | (r[:, 4] > W)).any():
        raise ValueError(f"cutmix_batch: {what}: a rectangle lies outside the {H} x {W} image")
    return r


def cutmix_batch(x_l: torch.Tensor, y_l: torch.Tensor, x_wk: torch.Tensor, x_st: torch.Tensor, rects_l,
                 rects_u) -> Tuple[torch.Tensor, torch.Tensor]:
    """The UCC step's input (UCC_train.py:152-153) by one kernel: (cat([mixed x_l, mixed x_wk, mixed x_st]), mixed labels).  `rects_l`
    / `rects_u`: `cutmix_rects` of the labelled mix and of the cross mix.  Image i of the labelled batch takes its rectangle from
    image (i + 1) % B of the ORIGINAL labelled batch; the weak and strong images take theirs from the already mixed labelled image i.
    max|.| of what is written is taken on the way (the first convolution keeps its fp16 form).  Nothing synchronises with the host."""
    for t in (x_l, x_wk, x_st):
        _lib.require_device(t, "cutmix_batch")
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape != x_l.shape or t.device != x_l.device:
            raise ValueError(f"cutmix_batch: three float32 [B,Cin,H,W] batches of one shape expected, got {tuple(x_l.shape)}, "
                             f"{tuple(x_wk.shape)}, {tuple(x_st.shape)}")
    B, Ci, H, W = x_l.shape
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"cutmix_batch: a batch of {B}, supported 1..{MAX_BATCH}")
    _lib.require_device(y_l, "cutmix_batch")
    if y_l.dtype != torch.int64 or tuple(y_l.shape) != (B, H, W) or y_l.device != x_l.device:
        raise ValueError(f"cutmix_batch: int64 labels [{B},{H},{W}] on {x_l.device} expected, got {y_l.dtype} {tuple(y_l.shape)} on {y_l.device}")
    rl, ru = _check_rects(rects_l, B, H, W, "rects_l"), _check_rects(rects_u, B, H, W, "rects_u")
    x_l, x_wk, x_st, y_l = x_l.contiguous(), x_wk.contiguous(), x_st.contiguous(), y_l.contiguous()
    out = torch.empty((3 * B, Ci, H, W), dtype=torch.float32, device=x_l.device)
    y_out = torch.empty_like(y_l)
    am = bounds.new_amax(x_l.device) if bounds.enabled() else None
    with _lib.device_guard(x_l.device):
        rc = _lib.lib().uaps_ucc_cutmix_batch_h(_lib.mk_hints((), am) if am is not None else None, x_l.data_ptr(), x_wk.data_ptr(),
                                                x_st.data_ptr(), y_l.data_ptr(), rl.ctypes.data, ru.ctypes.data, B, Ci, H, W,
                                                out.data_ptr(), y_out.data_ptr(), _lib.current_stream(x_l.device))
    _lib.check(rc, "uaps_ucc_cutmix_batch")
    if am is not None:
        bounds.put(out, am)
    return out, y_out


# ---- the loss block ---------------------------------------------------------------------------------------------------------------------

def s_off(Cc: int) -> Dict[str, int]:
    """The scalar block of uaps_ucc_fwd (include/uaps_hip.h, UAPS_UCC_S_*): offsets of ce[4], dice[4], sup, ps, ps_1, ps_2, the means
    v1, e1, v2, e2, bad, and the per-term per-class rows a1, a2, inter, card [4][C]; "n" = the block's length."""
    return {"ce": 0, "dice": 4, "sup": 8, "ps": 9, "ps_1": 10, "ps_2": 11, "v1": 12, "e1": 13, "v2": 14, "e2": 15, "bad": 16,
            "a1": 20, "a2": 20 + 4 * Cc, "inter": 20 + 8 * Cc, "card": 20 + 12 * Cc, "n": 20 + 16 * Cc}


def ucc_scalars(scalars: torch.Tensor, Cc: int) -> Dict[str, torch.Tensor]:
    """Views into the scalar block: ce [4] and dice [4] in the order of `TERMS`, sup, ps, ps_1, ps_2, v1, e1, v2, e2, bad,
    inter / card [4, C]."""
    o = s_off(Cc)
    out = {k: scalars[o[k]] for k in ("sup", "ps", "ps_1", "ps_2", "v1", "e1", "v2", "e2", "bad")}
    out["ce"], out["dice"] = scalars[o["ce"]:o["ce"] + 4], scalars[o["dice"]:o["dice"] + 4]
    for k in ("a1", "a2", "inter", "card"):
        out[k] = scalars[o[k]:o[k] + 4 * Cc].view(4, Cc)
    return out


def _workspace(dev: torch.device, B: int, Cc: int, H: int, W: int) -> torch.Tensor:
    n = C.c_size_t()
    _lib.check(_lib.lib().uaps_ucc_workspace_bytes(B, Cc, H, W, C.byref(n)), "uaps_ucc_workspace_bytes")
    return _ws.get(dev, n.value)


def _fwd(z1, z2, y, B, want_pseudo=True, want_var=False):
    _, Cc, H, W = z1.shape
    dev = z1.device
    ws = _workspace(dev, B, Cc, H, W)
    scalars = torch.empty(s_off(Cc)["n"], dtype=torch.float32, device=dev)
    p1 = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_pseudo else None
    p2 = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_pseudo else None
    v1 = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_var else None
    v2 = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_var else None
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_ucc_fwd(z1.data_ptr(), z2.data_ptr(), y.data_ptr(), int(B), Cc, H, W, 1e-7,
                                     p1.data_ptr() if want_pseudo else None, p2.data_ptr() if want_pseudo else None,
                                     v1.data_ptr() if want_var else None, v2.data_ptr() if want_var else None,
                                     scalars.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream(dev))
    _lib.check(rc, "uaps_ucc_fwd")
    return scalars, p1, p2, v1, v2


def _bwd(z1, z2, y, B, scalars, g_sup, g_ps, dz1, dz2):
    _, Cc, H, W = z1.shape
    with _lib.device_guard(z1.device):
        rc = _lib.lib().uaps_ucc_bwd(z1.data_ptr(), z2.data_ptr(), y.data_ptr(), scalars.data_ptr(), g_sup.data_ptr(), g_ps.data_ptr(),
                                     int(B), Cc, H, W, dz1.data_ptr(), dz2.data_ptr(), _lib.current_stream(z1.device))
    _lib.check(rc, "uaps_ucc_bwd")


class _UccLoss(torch.autograd.Function):
    """Outputs (sup, ps, scalars, pseudo1, pseudo2, var1, var2); the gradient goes to both logit tensors -- through both softmaxes of
    each KL pair, which the reference does not detach; the pseudo-labels carry none (UCC_train.py:224-225)."""

    @staticmethod
    def forward(ctx, y, B, want_var, z1, z2):
        ctx.set_materialize_grads(False)
        scalars, p1, p2, v1, v2 = _fwd(z1, z2, y, B, True, want_var)
        ctx.save_for_backward(y, scalars, z1, z2)
        ctx.B = B
        nd = [scalars, p1, p2] + ([v1, v2] if want_var else [])
        ctx.mark_non_differentiable(*nd)
        o = s_off(z1.shape[1])
        return scalars[o["sup"]].clone(), scalars[o["ps"]].clone(), scalars, p1, p2, v1, v2

    @staticmethod
    def backward(ctx, g_sup, g_ps, *_unused):
        y, scalars, z1, z2 = ctx.saved_tensors
        dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
        _bwd(z1, z2, y, ctx.B, scalars, _grad_scalar(g_sup, z1), _grad_scalar(g_ps, z1), dz1, dz2)
        return None, None, None, dz1, dz2


def ucc_loss(z1: torch.Tensor, z2: torch.Tensor, y: torch.Tensor, B: int, return_var: bool = False):
    """UCC_train.py:186-240 on the logits z1, z2 [3B,C,H,W] of the two heads: rows [:B] the (mixed) labelled batch with labels y int64
    [B,H,W], rows [B:2B] the weak and rows [2B:] the strong unlabelled batch.  Returns (sup, ps, scalars, pseudo1, pseudo2) -- the two
    differentiable sums (loss = sup + cw * ps, :246), the scalar block (`ucc_scalars`) and the pseudo-labels pseudo_1 = arg-max of
    head 2's weak logits, pseudo_2 = arg-max of head 1's, uint8 [B,H,W] -- and with `return_var` also the two variance maps fp32
    [B,H,W] (:213, :216)."""
    z1, z2 = _logits(z1, "ucc_loss"), _logits(z2, "ucc_loss")
    if z1.shape != z2.shape or z1.device != z2.device:
        raise ValueError(f"ucc_loss: the two logit tensors must share shape and device, got {tuple(z1.shape)} and {tuple(z2.shape)}")
    N, Cc, H, W = z1.shape
    B = int(B)
    if not 2 <= Cc <= MAX_CLASSES:
        raise ValueError(f"ucc_loss: {Cc} classes, supported 2..{MAX_CLASSES}")
    if B < 1 or N != 3 * B:
        raise ValueError(f"ucc_loss: {N} rows are not the labelled, weak and strong blocks of B = {B} images each")
    _lib.require_device(y, "ucc_loss")
    if y.dtype != torch.int64 or tuple(y.shape) != (B, H, W) or y.device != z1.device:
        raise ValueError(f"ucc_loss: int64 labels [{B},{H},{W}] on {z1.device} expected, got {y.dtype} {tuple(y.shape)} on {y.device}")
    out = _UccLoss.apply(y.contiguous(), B, bool(return_var), z1, z2)
    return out if return_var else out[:5]


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------

def _py_rng_plain(rng: random.Random):
    """random.Random.getstate() with the key tuple as a torch tensor: nothing a weights-only unpickler refuses."""
    version, keys, gauss = rng.getstate()
    return (int(version), torch.tensor(keys, dtype=torch.int64), None if gauss is None else float(gauss))


def _py_rng_restore(rng: random.Random, state) -> None:
    version, keys, gauss = state
    keys = keys.tolist() if torch.is_tensor(keys) else list(keys)
    rng.setstate((int(version), tuple(int(k) for k in keys), gauss))


class UCCTrainer(_ComparisonTrainer):
    """UCC (UCC/UCC_train.py:98-418) on `net_factory("unet_ucc")`: a shared encoder, the main decoder on clean and one auxiliary
    decoder on FeatureNoise features.  One `train_step(x_l, y_l, x_wk, x_st)`:

      1. the rectangles and flags of generate_mix_data (p = 0.2) and generate_crossmix_data (p = 0.3) from the trainer's own
         generators, keyed by (seed, rank) and saved in checkpoints (the reference draws from the unseeded globals);
         `train_step(..., rects=(rects_l, rects_u))` forces them;
      2. the mixed labelled, weak and strong batches and the mixed labels by one uaps_ucc_cutmix_batch launch (:152-153);
      3. the three forwards (:168, :176, :181) as ONE forward of 3B images under stat_groups(3) (UNet_UAPS.forward_groups);
      4. sup = 0.5 (CE + Dice) of each head against the mixed labels (:186-202); ps = ps_1 + ps_2, the pseudo-supervised terms of the
         strong rows weighted by mean exp(-variance) plus the mean variance (:213-240); loss = sup + cw * ps,
         cw = 0.1 sigmoid_rampup(iter // 150, 200) (:244-246);
      5. backward and Adam (:249-256).

    Returns device scalars loss, ce (= (ce_1 + ce_2) / 2, :200), dice, ps, ps_1, ps_2, sup, unsup, the host float cw and the
    pseudo-labels of the step (pseudo1, pseudo2: uint8 [B,H,W]); nothing in it synchronises with the host.  Training metrics are
    the main head's against the mixed labels (:264-267; `epoch_metrics2`: the second head's), validation is the main head's."""

    plateau_min_lr, plateau_patience = 1e-8, 50          # UCC_train.py:101
    log_keys = ("loss", "ce", "dice", "ps", "ps_1", "ps_2", "sup", "unsup")
    weight_keys = ("cw",)

    def __init__(self, model: torch.nn.Module, **kw):
        super().__init__(model, **kw)
        key = perturb._mix(kw.get("seed", 1337), self.rank)
        self.cut_np_rng = np.random.RandomState(key & 0xFFFFFFFF)
        self.cut_py_rng = random.Random(key)
        self._cms2 = []

    def draw_rects(self, B: int, H: int, W: int) -> Tuple[np.ndarray, np.ndarray]:
        """(rects of generate_mix_data, rects of generate_crossmix_data), in the order the reference calls them (:152-153)."""
        return (cutmix_rects(B, H, W, self.cut_np_rng, self.cut_py_rng, P_MIX),
                cutmix_rects(B, H, W, self.cut_np_rng, self.cut_py_rng, P_CROSSMIX))

    def _unlabeled_inputs(self, u) -> Sequence[torch.Tensor]:
        """The weak and strong images of the reference's unlabelled items (inputs_U1, inputs_U2, labels_U1, labels_U2), :147."""
        if not isinstance(u, (tuple, list)) or len(u) < 2:
            raise ValueError("UCCTrainer.fit: unlabelled items (x_weak, x_strong, ...) expected")
        return u[0], u[1]

    def train_step(self, x_l: torch.Tensor, y_l: torch.Tensor, x_wk: torch.Tensor, x_st: torch.Tensor, w=None,
                   rects=None) -> Dict[str, torch.Tensor]:
        self._check_batches(x_l, x_wk, y_l)
        self._check_batches(x_l, x_st)
        B, _, H, W = x_l.shape
        rl, ru = self.draw_rects(B, H, W) if rects is None else rects
        cw = self.consistency_weight()                                                 # :244
        y = y_l.to(torch.int64)
        with self._step() as backward:
            batch, y_mix = cutmix_batch(x_l, y, x_wk, x_st, rl, ru)                     # :152-153
            z1, z2 = self.model.forward_groups(batch, 3)                                # :168, :176, :181 in one pass
            sup, ps, scalars, p1, p2 = ucc_loss(z1, z2, y_mix, B)                       # :186-240
            loss = sup + cw * ps                                                        # :246
            backward(loss)                                                              # :249-251; Adam (:256) on leaving
        self._count(z1[:B], y_mix)                                                      # :264, :266
        if self.track_metrics:
            self._cms2.append(metrics.seg_confusion(z2[:B], y_mix))                     # :265, :267
        sc = ucc_scalars(scalars, z1.shape[1])
        self.last = {"loss": loss.detach(), "ce": (sc["ce"][0] + sc["ce"][1]) / 2, "dice": (sc["dice"][0] + sc["dice"][1]) / 2,
                     "ps": ps.detach(), "ps_1": sc["ps_1"], "ps_2": sc["ps_2"], "sup": sup.detach(), "unsup": (cw * ps).detach(),
                     "cw": cw, "pseudo1": p1, "pseudo2": p2}
        return self.last

    def epoch_metrics2(self, reset: bool = True) -> Dict[str, float]:
        """`epoch_metrics` of the second head (UCC_train.py:265, :267)."""
        return self._score_steps(self._cms2, reset)

    # -- checkpoint (UCC_train.py:411-418): the bare model's state_dict, no `module.` prefix --
    def state_for_checkpoint(self, epoch: int, best_dice: float, dataparallel_prefix: bool = False) -> Dict:
        ck = super().state_for_checkpoint(epoch, best_dice, dataparallel_prefix)
        ck["cut_np_rng"] = _rng_state_plain(self.cut_np_rng)
        ck["cut_py_rng"] = _py_rng_plain(self.cut_py_rng)
        return ck

    def load_checkpoint(self, path: str, load_optimizer: bool = True) -> Dict:
        ck = super().load_checkpoint(path, load_optimizer)
        if "cut_np_rng" in ck:
            self.cut_np_rng.set_state(_rng_state_numpy(ck["cut_np_rng"]))
        if "cut_py_rng" in ck:
            _py_rng_restore(self.cut_py_rng, ck["cut_py_rng"])
        return ck

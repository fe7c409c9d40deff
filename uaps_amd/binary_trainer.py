"""BinaryTrainer: the supervised trainer of a one-channel sigmoid head (defect / no-defect), on the kernels of csrc/loss_binary.hip."""
from __future__ import annotations

from typing import Dict

import torch

from . import binary_losses
from .trainer import SegTrainer, score_validation


class BinaryTrainer(SegTrainer):
    """A supervised trainer for `net_factory("unet", class_num=1)` or any model whose first output is [B,1,H,W] logits.

    `loss`: a `binary_losses.BinarySegLoss`; None is {"bce": 0.6, "fscore": 0.4}, the reference's `loss_calc = BCEDiceLoss()`
    (utilities/losses_2.py:81-91, :182).  `threshold`: sigmoid(z) > threshold is the predicted defect mask of the training and
    validation metrics (`binary_losses.bin_confusion`).  The step follows BaselineTrainer's SegLoss step: forward, the fused criterion,
    backward, Adam; it returns "loss", one entry per selected term (the instance's `log_keys`) and "bad_labels" (labels outside {0, 1},
    a device scalar, must be 0).  Labels are [B,H,W] integers in {0, 1}; the loss is a per-rank mean under data parallelism, as
    BaselineTrainer's.  `validate` scores the 2 x 2 confusion matrices with `trainer.score_validation` (its "ce" is the BCE); `fit`,
    the scheduler and the checkpoints are SegTrainer's.  Checkpoints do not hold the criterion or the threshold."""

    weight_keys = ()             # (no consistency term)

    def __init__(self, model: torch.nn.Module, base_lr: float = 1e-3, seed: int = 1337, overlap_comm: bool = True,
                 track_metrics: bool = True, loss=None, threshold: float = 0.5):
        super().__init__(model, base_lr=base_lr, seed=seed, overlap_comm=overlap_comm, track_metrics=track_metrics)
        if loss is None:
            loss = binary_losses.BinarySegLoss({"bce": 0.6, "fscore": 0.4})
        if not isinstance(loss, binary_losses.BinarySegLoss):
            raise TypeError(f"BinaryTrainer: loss must be a binary_losses.BinarySegLoss or None, got {type(loss).__name__}")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"BinaryTrainer: threshold must lie in (0, 1), got {threshold}")
        self.loss, self.threshold = loss, float(threshold)
        self.log_keys = ("loss",) + tuple(loss.term_names)
        self._bce = binary_losses.BinarySegLoss({"bce": 1.0})          # validation's cross entropy

    @staticmethod
    def _main(out) -> torch.Tensor:
        main = out[0] if isinstance(out, (tuple, list)) else out
        if main.dim() != 4 or main.shape[1] != 1:
            raise ValueError(f"BinaryTrainer: the model's first output must be [B,1,H,W] logits, got {tuple(main.shape)}")
        return main

    def train_step(self, x_l: torch.Tensor, y_l: torch.Tensor, x_u=None, w=None) -> Dict[str, torch.Tensor]:
        with self._step() as backward:
            main = self._main(self.model(x_l))
            s = self.loss(main, y_l)
            backward(s.loss)
        self._count(main, y_l)
        sc = binary_losses.bin_scalars(s.scalars)
        self.last = {"loss": s.loss.detach(), **{k: sc[k] for k in self.loss.term_names}, "bad_labels": sc["bad"]}
        return self.last

    def _count(self, logits: torch.Tensor, y_l: torch.Tensor) -> None:
        if self.track_metrics:
            self._cms.append(binary_losses.bin_confusion(logits, y_l, self.threshold))
        self.iter_num += 1

    @torch.no_grad()
    def validate(self, batches, pooled: bool = False) -> Dict[str, float]:
        """SegTrainer.validate for the sigmoid head: eval mode, per batch the BCE and the 2 x 2 confusion matrix at `threshold`; the
        record of `score_validation` (miou / mdice are the defect class's IoU / Dice, NaN for a batch without defect pixels) plus
        "iou" and "dice" of the summed matrix.  One device->host copy at the end."""
        self.model.eval()
        cms, ces = [], []
        for x, y in batches:
            main = self._main(self.model(x))
            ces.append(self._bce(main, y).loss)
            cms.append(binary_losses.bin_confusion(main, y, self.threshold))
        if not cms:
            return {k: float("nan") for k in ("miou", "mdice", "acc", "ce", "loss", "iou", "dice")}
        cm = torch.stack(cms).cpu().numpy()
        ce = torch.stack(ces).double().cpu().numpy()
        self.check_errors()
        m = score_validation(cm, ce, pooled)
        whole = binary_losses.bin_metrics_from_confusion(cm.sum(0))
        m["iou"], m["dice"] = whole["iou"], whole["dice"]
        return m

"""Evaluation path of the reference (UAPS-Testing.ipynb, the only consumer of the checkpoints UAPS_train.py writes):
main-head prediction, the all-heads ensemble of the paper's decoder study, the test-time uncertainty map, and the
per-image score table.  Everything runs on the HIP kernels of this package; nothing here trains."""
from __future__ import annotations

import operator
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import consistency, losses, metrics


@torch.no_grad()
def predict(model: torch.nn.Module, images: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
    """model.eval(); main-head arg-max mask [B,H,W] and the raw head logits (notebook cells 11-13: `output, ax1, _, _ =
    model(image); masked = torch.argmax(output, dim=1)`).  As in the reference, the auxiliary decoders stay perturbed
    in eval mode (Dropout is called with training=True unconditionally, UAPS_unet.py:156-158)."""
    model.eval()
    out = model(images)
    heads = out if isinstance(out, (tuple, list)) else (out,)
    return torch.argmax(heads[0], dim=1), tuple(heads)


@torch.no_grad()
def predict_main(model: torch.nn.Module, images: torch.Tensor) -> torch.Tensor:
    """Main-head arg-max mask with ONLY the encoder and the main decoder run (the paper's "main decoder only" inference row,
    fig_data/decoder-effect.jpg: its time does not depend on the number of auxiliary decoders); the same mask as predict()[0].
    Models without a `forward_main` run every head."""
    model.eval()
    fm = getattr(model, "forward_main", None)
    logits = fm(images) if fm is not None else predict(model, images)[1][0]
    return torch.argmax(logits, dim=1)


_VERSION = operator.attrgetter("_version")


class CapturedMainHead:
    """predict_main for ONE input shape as a replayed hipGraph: at batch 1 the eager call is ~90 launches of a few microseconds of
    work each and is bound by their issue; the replay hands the device the whole chain at once.  Same kernels and arithmetic as
    predict_main (the main decoder has no perturbation: nothing random is baked in).  The packed weights are read through the
    graph's pointers: build a new object after the model's parameters changed (a checkpoint load, a training step).

        run = CapturedMainHead(model, example_images)
        mask = run(images)            # int64 [B,H,W], valid until the next call (clone() it to keep it)
    """

    def __init__(self, model: torch.nn.Module, example: torch.Tensor, warmup: int = 2):
        from . import bounds
        if not example.is_cuda:
            raise ValueError("CapturedMainHead: a GPU tensor expected")
        self.model, self.x = model, example.detach().clone()
        self._tensors = self._params = None
        model.eval()
        cur = torch.cuda.current_stream(example.device)
        side = torch.cuda.Stream(device=example.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side), torch.no_grad():       # warm-up on a side stream (torch's capture recipe): packs the weights, sizes the workspaces
            for _ in range(max(1, warmup)):
                predict_main(model, self.x)
        cur.wait_stream(side)
        torch.cuda.synchronize(example.device)
        bounds.reset_pool()                                  # the zero fill of every max|.| scalar the kernels raise belongs to the graph
        self.graph = torch.cuda.CUDAGraph()
        from . import _lib
        # thread-local error mode: another thread's runtime calls (a DataLoader's pin thread, a watchdog) do not invalidate the capture;
        # quiet_gc: no finaliser of THIS thread runs inside it
        with _lib.quiet_gc(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"), torch.no_grad():
            self.out = predict_main(model, self.x)
        bounds.reset_pool()                                  # eager code must not be handed scalars the replays re-zero
        # the graph reads the packed weights and the BatchNorm buffers through raw addresses: hold the packed buffers (the cache may
        # drop them), and remember what the parameters looked like -- a replay after they changed would silently use stale weights
        from . import conv
        self._held = [(e[3], e[4]) for e in conv._packed.values()]
        self._stamp = self._weights_stamp()

    def _weights_stamp(self):
        """(manual-invalidation generation, number of tensors, sum of the version counters of every parameter and buffer, sum of the
        parameters' optimizer counters).  Every term only ever grows, so a sum changes exactly when one of its terms does.  This runs in
        front of EVERY replay (the tuple-of-tuples form of the first version cost 0.5 ms per call, more than the graph): the versions
        are summed by a C-level loop over a cached list, the optimizer counters are only walked when some optimizer of the process has
        stepped since the last look (conv._shared_cell)."""
        from . import conv
        if self._tensors is None:
            # a model with forward_main runs its encoder and main decoder only (unet.UNet_UAPS): watch those tensors, a third of the net
            mods = [getattr(self.model, n, None) for n in ("encoder", "main_decoder")] if hasattr(self.model, "forward_main") else []
            mods = mods if mods and all(isinstance(m, torch.nn.Module) for m in mods) else [self.model]
            self._params = [p for m in mods for p in m.parameters()]
            self._tensors = self._params + [b for m in mods for b in m.buffers()]
            self._seen_steps, self._cell_sum = -1, 0
        if conv._shared_cell[0] != self._seen_steps:
            self._seen_steps = conv._shared_cell[0]
            self._cell_sum = sum(c[0] for c in (getattr(p, "_uaps_cell", None) for p in self._params) if c is not None)
        return (conv._generation, len(self._tensors), sum(map(_VERSION, self._tensors)), self._cell_sum)

    def stale(self) -> bool:
        """Have the model's parameters or buffers changed since the capture (an optimizer step, a checkpoint load, an in-place edit)?"""
        return self._weights_stamp() != self._stamp

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        if images.shape != self.x.shape or images.device != self.x.device or images.dtype != self.x.dtype:
            raise ValueError(f"CapturedMainHead: captured for {tuple(self.x.shape)} {self.x.dtype} on {self.x.device}")
        if self.stale():
            raise RuntimeError("CapturedMainHead: the model's parameters or buffers changed since the capture (optimizer step, checkpoint "
                               "load, in-place edit): the graph holds the OLD packed weights -- build a new CapturedMainHead")
        self.x.copy_(images, non_blocking=True)
        self.graph.replay()
        return self.out


@torch.no_grad()
def ensemble_from_heads(heads) -> torch.Tensor:
    """Arg-max of the mean softmax of the given head logits: `uaps_unsup_fwd` (csrc/loss_kernels.hpp) with uniform mixing weights --
    its pseudo-label IS argmax_c sum_k w_k softmax(z_k)_c (UAPS_train.py:251-255) -- one pass over the D logit tensors instead of D
    softmax launches and D - 1 adds.  int64 [B,H,W]."""
    D = len(heads)
    if D == 1:
        return torch.argmax(heads[0], dim=1)
    return losses.uaps_unsup_loss(tuple(heads), [1.0 / D] * D, 0.0, 0.0).pseudo


@torch.no_grad()
def predict_ensemble(model: torch.nn.Module, images: torch.Tensor) -> torch.Tensor:
    """Arg-max of the mean softmax over all heads (the "ensemble" rows of the paper's decoder study, README.md:107-111; notebook
    cells 11-19 with every head's softmax averaged), on the loss block's mixing kernel."""
    _, heads = predict(model, images)
    return ensemble_from_heads(heads)


@torch.no_grad()
def predict_with_uncertainty(model: torch.nn.Module, images: torch.Tensor):
    """(mask, uncertainty, confidence): notebook cell 24 -- uncertainty = sum_c KLDivLoss('none')(log_softmax(main),
    softmax(aux1)) per pixel, confidence = 1 - uncertainty."""
    mask, heads = predict(model, images)
    if len(heads) < 2:
        raise ValueError("the uncertainty map needs an auxiliary head")
    var1 = consistency.uncertainty_map(heads[0], heads[1])
    return mask, var1, 1.0 - var1


def _tiled_kwargs(tiled, tta, what):
    """The predict_tiled keywords of a `tiled` argument (True: the defaults); tiled together with tta has no form."""
    if tta:
        raise ValueError(f"{what}: tiled together with tta is not built (TTA inside tiles is out of scope)")
    if tiled is True:
        return {}
    if not isinstance(tiled, dict):
        raise TypeError(f"{what}: tiled is True or a dict of predict_tiled keywords")
    return dict(tiled)


def _surface_kwargs(surface):
    """The keywords of a `surface` argument (True: the defaults)."""
    if surface is True:
        return {}
    if not isinstance(surface, dict) or set(surface) - {"percentile", "tolerance", "classes"}:
        raise TypeError("evaluate: surface is True or a dict with the keywords percentile, tolerance and classes")
    return dict(surface)


def _surface_sums(scored: torch.Tensor, y: torch.Tensor, kw) -> torch.Tensor:
    """float64 [4] on the device: the sums of hd95, assd and nsd (0 without a tolerance) over the valid pairs of the chosen classes
    (default 1 .. C-1) of one batch, and their number."""
    from .surface import surface_distances
    Cn = scored.shape[1]
    r = surface_distances(scored.float(), y, Cn, percentile=kw.get("percentile", 95.0), tolerance=kw.get("tolerance"))
    classes = list(range(1, Cn)) if kw.get("classes") is None else [int(c) for c in kw["classes"]]
    ok = r.valid[:, classes]
    total = lambda v: torch.where(ok, v[:, classes], torch.zeros_like(v[:, classes])).sum()
    nsd = total(r.nsd) if r.tolerance is not None else torch.zeros((), dtype=torch.float64, device=ok.device)
    return torch.stack([total(r.hd95), total(r.assd), nsd, ok.sum().to(torch.float64)])


_INSTANCE_KEYS = {"iou_threshold", "min_area", "connectivity", "max_instances", "classes"}


def _instances_kwargs(instances):
    """The keywords of an `instances` argument (True: the defaults)."""
    if instances is True:
        return {}
    if not isinstance(instances, dict) or set(instances) - _INSTANCE_KEYS:
        raise TypeError("evaluate: instances is True or a dict with the keywords " + ", ".join(sorted(_INSTANCE_KEYS)))
    return dict(instances)


def _instance_sums(scored: torch.Tensor, y: torch.Tensor, kw) -> torch.Tensor:
    """float64 [K,7] on the device: matching.MatchResult.sums of one batch -- the defects of the arg-max of `scored` against the
    defects of `y`, over the chosen classes (default 1 .. C-1)."""
    from .instances import label_instances
    from .matching import match_instances
    lab = {k: kw[k] for k in ("min_area", "connectivity", "max_instances") if k in kw}
    pred = label_instances(torch.argmax(scored, dim=1), **lab)
    target = label_instances(y.to(torch.int64), **lab)
    return match_instances(pred, target, scored.shape[1], iou_threshold=kw.get("iou_threshold", 0.5)).sums(kw.get("classes"))


def _cleaned(mask: torch.Tensor, cleanup, num_classes: int, components=None) -> torch.Tensor:
    """The arg-max mask after the clean-up chain `cleanup` (morphology.morphology's `steps`), then after the component chain
    `components` (components.components' `steps`); either may be None."""
    if cleanup is not None:
        from .morphology import morphology
        mask = morphology(mask, cleanup, num_classes)
    if components is not None:
        from .components import components as component_steps
        mask = component_steps(mask, components, num_classes)
    return mask


def _one_hot_maps(mask: torch.Tensor, num_classes: int) -> torch.Tensor:
    """float32 [B,C,H,W] maps whose arg-max is `mask`: what the scoring kernels take in place of logits."""
    return torch.nn.functional.one_hot(mask, num_classes).permute(0, 3, 1, 2).contiguous().float()


_CURVE_KEYS = {"bins", "fpr_limit", "ece_bins", "classes", "max_instances", "connectivity", "min_area", "uncertainty", "lo", "hi"}


def _curves_kwargs(curves, tta, tiled):
    """The keywords of a `curves` argument (True: the defaults)."""
    if curves is True:
        return {}
    if not isinstance(curves, dict) or set(curves) - _CURVE_KEYS:
        raise TypeError("evaluate: curves is True or a dict with the keywords " + ", ".join(sorted(_CURVE_KEYS)))
    if curves.get("uncertainty") and (tta or tiled):
        raise ValueError("evaluate: curves with uncertainty=True scores the plain forward's uncertainty map: not built under tta or tiled")
    return dict(curves)


def _curve_sums(scored: torch.Tensor, y: torch.Tensor, kw, from_logits: bool):
    """curves.CurveResult.sums of one batch: the class rows (default 1 .. C-1), the top row with its fixed-point sums, and the regions
    of the labels' defects."""
    from .curves import score_curves
    from .instances import label_instances
    lab = {k: kw[k] for k in ("min_area", "connectivity", "max_instances") if k in kw}
    regions = label_instances(y.to(torch.int64), **lab)
    return score_curves(scored.float(), y, classes=kw.get("classes"), bins=kw.get("bins", 1024), top=True, from_logits=from_logits,
                        regions=regions, want_sums=True).sums()


def _uncertainty_sums(heads, y: torch.Tensor, kw):
    """The sums of curves.plane_curves on consistency.uncertainty_map(main, aux1) against "the main head's arg-max is right"."""
    from .curves import plane_curves
    if len(heads) < 2:
        raise ValueError("evaluate: curves with uncertainty=True needs a model with an auxiliary head")
    unc = consistency.uncertainty_map(heads[0], heads[1])
    return plane_curves(unc.float(), torch.argmax(heads[0], dim=1), y, bins=kw.get("bins", 1024), lo=kw.get("lo", 0.0),
                        hi=kw.get("hi", 1.0)).sums()


@torch.no_grad()
def evaluate(model: torch.nn.Module, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], tta=None, tiled=None,
             surface=None, instances=None, curves=None, cleanup=None, components=None) -> Dict[str, float]:
    """The score table of notebook cell 25: mIoU, mDice and pixel accuracy of the main head computed image by image
    (utilities/metrics.py conventions) and averaged over the images, in percent.  tta=True, or a tuple of scales: the arg-max of the
    multi-scale + flip sum of probability maps (tta.predict_tta) is scored instead of the main head's.  tiled=True, or a dict of
    tiled.predict_tiled keywords: images of any size are scored on the blended probability maps of sliding-window inference.
    surface=True, or a dict with the keywords percentile, tolerance and classes: the boundary metrics of surface.surface_distances
    on the same scored maps are added -- "HD95(px)" and "ASSD(px)" (and "NSD(%)" with a tolerance), the means over the valid
    (image, class) pairs of the whole run, and "surface_pairs", their number.  The pairs are summed on the device; one copy at the end.
    instances=True, or a dict with the keywords iou_threshold, min_area, connectivity, max_instances and classes: the defects of the
    scored arg-max mask are matched against the defects of the labels (instances.label_instances on both, matching.match_instances)
    and the per-defect scores are added -- "PQ(%)", "SQ(%)", "RQ(%)", "DefectPrecision(%)", "DefectRecall(%)", "PRO(%)" (the
    overall values of matching.summarize), "defects_gt", "defects_pred" and "instance_images_skipped" (images with more defects than
    max_instances on either side are left out).  Summed on the device; one copy at the end.
    curves=True, or a dict (an empty one: the defaults) with the keywords bins, fpr_limit, ece_bins, classes, max_instances, connectivity, min_area, uncertainty, lo
    and hi: the threshold-sweep scores of curves.score_curves on the scored maps (the logits of the plain path go through the kernel's
    softmax; under tta and tiled the maps are probabilities already) are added -- "AUROC(%)", "AP(%)", "AUPRO(%)" (up to fpr_limit,
    default 0.3, over the defects of the labels), "ECE(%)" (ece_bins groups, default 16) and "curve_images_skipped" (images with more
    real defects than max_instances are left out).  uncertainty=True (plain path only, a model with an auxiliary head) adds
    "UncAUROC(%)" and "AURC": how well consistency.uncertainty_map(main, aux1), binned over [lo, hi] (default 0, 1), marks the wrong
    pixels of the main head.  Summed on the device; one copy at the end.
    cleanup: a morphology.morphology `steps` sequence.  The surface= and instances= branches then score the cleaned arg-max of the
    scored maps, and "mIoU_clean(%)" and "mDice_clean(%)" are added: the same per-image rule on the cleaned mask.  Every other key
    (the curves among them: they score maps, not masks) is what it is without cleanup.
    components: a components.components `steps` sequence (area_open / clear_border / fill_holes), applied to the arg-max mask after
    the cleanup chain where one is given; the same branches and the same two keys then see the mask after both."""
    miou, mdice, acc = [], [], []
    miou_clean, mdice_clean = [], []
    if cleanup is not None:
        from .morphology import check_steps
        cleanup = check_steps(cleanup)
    if components is not None:
        from .components import check_steps as check_component_steps
        components = check_component_steps(components)
    clean = cleanup is not None or components is not None
    curve_kw = _curves_kwargs(curves, tta, tiled) if curves is not None and curves is not False else None      # ({}: the defaults)
    curve_sums = unc_sums = None
    tiled_kw = _tiled_kwargs(tiled, tta, "evaluate") if tiled else None
    surf_kw = _surface_kwargs(surface) if surface else None
    surf_sums = []
    inst_kw = _instances_kwargs(instances) if instances else None
    inst_sums = []
    for x, y in batches:
        if tiled_kw is not None:
            from .tiled import predict_tiled
            scored = predict_tiled(model, x, **{**tiled_kw, "want": ("probs",)}).probs
        elif tta:
            from .tta import DEFAULT_SCALES, predict_tta
            scored = predict_tta(model, x, scales=DEFAULT_SCALES if tta is True else tuple(tta), want=("probs",)).probs
        else:
            heads = predict(model, x)[1]
            scored = heads[0]
            if curve_kw is not None and curve_kw.get("uncertainty"):
                part = _uncertainty_sums(heads, y, curve_kw)
                unc_sums = part if unc_sums is None else unc_sums + part
        if curve_kw is not None:
            part = _curve_sums(scored, y, curve_kw, from_logits=tiled_kw is None and not tta)
            curve_sums = part if curve_sums is None else curve_sums + part
        masked = scored                                      # what the mask-level scores (surface, instances) look at
        if clean:
            masked = _one_hot_maps(_cleaned(torch.argmax(scored, dim=1), cleanup, scored.shape[1], components), scored.shape[1])
            for cm in metrics.seg_confusion_per_image(masked, y).cpu().numpy():
                m = metrics.metrics_from_confusion(cm)
                miou_clean.append(m["miou"]); mdice_clean.append(m["mdice"])
        if surf_kw is not None:
            surf_sums.append(_surface_sums(masked, y, surf_kw))
        if inst_kw is not None:
            inst_sums.append(_instance_sums(masked, y, inst_kw))
        cms = metrics.seg_confusion_per_image(scored, y).cpu().numpy()
        for cm in cms:
            m = metrics.metrics_from_confusion(cm)
            miou.append(m["miou"]); mdice.append(m["mdice"]); acc.append(m["acc"])
    out = {"mIoU(%)": float(np.mean(miou) * 100), "mDice(%)": float(np.mean(mdice) * 100), "Accuracy(%)": float(np.mean(acc) * 100),
           "images": len(acc)}
    if clean:
        out["mIoU_clean(%)"], out["mDice_clean(%)"] = float(np.mean(miou_clean) * 100), float(np.mean(mdice_clean) * 100)
    if surf_kw is not None:
        tot = torch.stack(surf_sums).sum(dim=0).cpu().tolist() if surf_sums else [0.0] * 4
        pairs = int(tot[3])
        mean = lambda v: v / pairs if pairs else float("nan")
        out["HD95(px)"], out["ASSD(px)"] = mean(tot[0]), mean(tot[1])
        if surf_kw.get("tolerance") is not None:
            out["NSD(%)"] = mean(tot[2]) * 100
        out["surface_pairs"] = pairs
    if inst_kw is not None:
        from .matching import SUM_COLUMNS, summarize
        Cn = None if not inst_sums else inst_sums[0].shape[0]
        classes = inst_kw.get("classes")
        classes = list(range(1, (Cn or 0) + 1)) if classes is None else [int(c) for c in classes]
        tot = torch.stack(inst_sums).sum(dim=0).cpu().numpy() if inst_sums else np.zeros((len(classes), len(SUM_COLUMNS)))
        s = summarize(tot, classes, len(acc))
        for key, name in (("PQ(%)", "PQ"), ("SQ(%)", "SQ"), ("RQ(%)", "RQ"), ("DefectPrecision(%)", "precision"),
                          ("DefectRecall(%)", "recall"), ("PRO(%)", "PRO")):
            out[key] = s[name] * 100
        out["defects_gt"], out["defects_pred"], out["instance_images_skipped"] = s["n_gt"], s["n_pred"], s["images_skipped"]
    if curve_kw is not None:
        from .curves import summarize as curve_summarize
        nan = float("nan")
        s = {"AUROC": nan, "AP": nan, "AUPRO": nan, "ECE": nan, "images_skipped": 0}
        if curve_sums is not None:
            Cn = curve_sums.hist.shape[0]                     # the class rows and the top row
            classes = curve_kw.get("classes")
            classes = list(range(1, Cn)) if classes is None else [int(c) for c in classes]
            s = curve_summarize(curve_sums, classes, fpr_limit=curve_kw.get("fpr_limit", 0.3), ece_bins=curve_kw.get("ece_bins", 16))
        for key in ("AUROC", "AP", "AUPRO", "ECE"):
            out[key + "(%)"] = s[key] * 100
        out["curve_images_skipped"] = s["images_skipped"]
        if curve_kw.get("uncertainty"):
            u = {"AUROC": nan, "AURC": nan}
            if unc_sums is not None:
                u = curve_summarize(unc_sums, (), lo=curve_kw.get("lo", 0.0), hi=curve_kw.get("hi", 1.0), plane=True)
            out["UncAUROC(%)"], out["AURC"] = u["AUROC"] * 100, u["AURC"]
    return out


def _with_shapes(inst, shapes, connectivity: int):
    """predict_instances' result: the InstanceResult itself, or with `shapes` the ShapeResult that describes it."""
    if not shapes:
        return inst
    from .shapes import shape_descriptors
    return shape_descriptors(inst, thickness=shapes == "thickness", connectivity=connectivity)


@torch.no_grad()
def predict_instances(model: torch.nn.Module, images: torch.Tensor, *, tta=None, tiled=None, min_area: int = 1, connectivity: int = 8,
                      max_instances: int = 256, cleanup=None, components=None, shapes=False):
    """Defects instead of pixels: instances.label_instances on the main head's arg-max mask, with maps = (confidence, uncertainty).
    The confidence is the main head's largest softmax; with tta (True, or a tuple of scales) mask and confidence are those of
    tta.predict_tta.  The uncertainty is consistency.uncertainty_map(main, aux1) of the plain forward where the model has an auxiliary
    head; a one-head model gets the confidence alone.  tiled (True, or a dict of tiled.predict_tiled keywords): mask, confidence and
    the blended per-tile uncertainty of sliding-window inference, for images of any size.  cleanup (a morphology.morphology `steps`
    sequence): the arg-max mask goes through that chain before it is labelled, under all three paths; the maps are untouched.
    components (a components.components `steps` sequence): likewise, after the cleanup chain where one is given.  Returns an
    instances.InstanceResult (records() lists the defects).
    shapes=True, or "thickness": a shapes.ShapeResult instead -- shapes.shape_descriptors of that InstanceResult (with thickness=True
    for "thickness"), which `.instances` holds; its props() and records() add centroid, axes, orientation, perimeter, holes and the
    like to every defect.  Under all three paths, after the clean-up chains."""
    from . import instances
    if shapes not in (False, True, "thickness"):
        raise ValueError("predict_instances: shapes is False, True or \"thickness\"")
    clean = cleanup is not None or components is not None
    if components is not None:
        from .components import check_steps as check_component_steps
        components = check_component_steps(components)
    if tiled:
        from .tiled import predict_tiled
        # (the class count of the clean-up is the blended maps' channel count: they are asked for beside the mask then)
        kw = {**_tiled_kwargs(tiled, tta, "predict_instances"), "want": ("mask", "conf") + (("probs",) if clean else ())}
        kw.setdefault("uncertainty", "auto")
        r = predict_tiled(model, images, **kw)
        mask = r.mask
        if clean:
            mask = _cleaned(mask, cleanup, r.probs.shape[1], components)
        return _with_shapes(instances.label_instances(mask, (r.conf,) + tuple(r.maps), connectivity=connectivity, min_area=min_area,
                                                      max_instances=max_instances), shapes, connectivity)
    mask, heads = predict(model, images)
    if tta:
        from .tta import DEFAULT_SCALES, predict_tta
        r = predict_tta(model, images, scales=DEFAULT_SCALES if tta is True else tuple(tta), want=("mask", "conf"))
        mask, conf = r.mask, r.conf
    else:
        conf = torch.softmax(heads[0], dim=1).amax(dim=1)
    maps = (conf,) if len(heads) < 2 else (conf, consistency.uncertainty_map(heads[0], heads[1]))
    if clean:
        mask = _cleaned(mask, cleanup, heads[0].shape[1], components)
    return _with_shapes(instances.label_instances(mask, maps, connectivity=connectivity, min_area=min_area, max_instances=max_instances),
                        shapes, connectivity)


def load_for_inference(model: torch.nn.Module, checkpoint_path: str, device: Optional[torch.device] = None) -> Dict:
    """Notebook cell 4: `checkpoint = torch.load(path); model.load_state_dict(checkpoint['state_dict'])` -- accepts the
    `module.`-prefixed keys of the reference's nn.DataParallel checkpoints (UAPS_train.py:443-450) and plain ones."""
    from .trainer import load_state_dict_any_prefix
    ck = torch.load(checkpoint_path, map_location=device or "cpu", weights_only=False)
    load_state_dict_any_prefix(model, ck["state_dict"] if "state_dict" in ck else ck)
    return ck

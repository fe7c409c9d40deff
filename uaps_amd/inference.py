"""Evaluation path of the reference (UAPS-Testing.ipynb, the only consumer of the checkpoints UAPS_train.py writes):
main-head prediction, the all-heads ensemble of the paper's decoder study, the test-time uncertainty map, and the
per-image score table.  Everything runs on the HIP kernels of this package; nothing here trains."""
from __future__ import annotations

import operator
from typing import Dict, Iterable, NamedTuple, Optional, Tuple

import torch

from . import consistency, losses, scoring


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


class _Forward(NamedTuple):
    """scored: fp32 [B,C,H,W] -- the main head's logits (is_logits) or the probability maps of tta / tiled; mask: the arg-max;
    conf: the largest probability; maps: the blended per-tile maps of the tiled path; heads: the raw heads where the plain forward
    ran.  None for what was not asked for."""
    scored: Optional[torch.Tensor]
    is_logits: bool
    mask: Optional[torch.Tensor]
    conf: Optional[torch.Tensor]
    maps: Tuple[torch.Tensor, ...]
    heads: Optional[Tuple[torch.Tensor, ...]]


def _forward(model, images, tta, tiled_kw, want) -> _Forward:
    """One forward down the tiled path (tiled_kw: the checked keywords, or None), the tta path (True, or a tuple of scales) or the
    plain one.  want: among "probs" (-> scored), "mask" and "conf", and "heads": the plain predict() as well under tta."""
    maps = tuple(k for k in want if k != "heads")
    if tiled_kw is not None:
        from .tiled import predict_tiled
        r = predict_tiled(model, images, **{**tiled_kw, "want": maps})
        return _Forward(r.probs, False, r.mask, r.conf, tuple(r.maps), None)
    mask, heads = predict(model, images) if not tta or "heads" in want else (None, None)
    if tta:
        if heads is not None and heads[0].shape[1] == 1:
            raise ValueError("tta: a one-channel sigmoid model has no form under tta (the fold kernel takes 2..8 classes)")
        from .tta import DEFAULT_SCALES, predict_tta
        r = predict_tta(model, images, scales=DEFAULT_SCALES if tta is True else tuple(tta), want=maps)
        return _Forward(r.probs, False, r.mask, r.conf, (), heads)
    conf = torch.softmax(heads[0], dim=1).amax(dim=1) if "conf" in want else None
    return _Forward(heads[0], True, mask, conf, (), heads)


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


_HYSTERESIS_KEYS = ("low", "high", "classes", "background", "min_area")


def _hysteresis_kwargs(hysteresis, what: str, own_connectivity: bool) -> dict:
    """The hysteresis.hysteresis keywords of a `hysteresis` argument: a (low, high) pair, or a dict with "low" and "high" and any of
    classes, background and min_area -- and connectivity where the caller has none of its own (own_connectivity)."""
    if isinstance(hysteresis, dict):
        kw = dict(hysteresis)
        allowed = _HYSTERESIS_KEYS + (("connectivity",) if own_connectivity else ())
        if "low" not in kw or "high" not in kw or not set(kw) <= set(allowed):
            raise ValueError(f"{what}: a hysteresis dict holds \"low\" and \"high\" and any of {allowed[2:]}")
    elif isinstance(hysteresis, (tuple, list)) and len(hysteresis) == 2:
        kw = {"low": hysteresis[0], "high": hysteresis[1]}
    else:
        raise ValueError(f"{what}: hysteresis is a (low, high) pair or a dict of hysteresis keywords")
    return kw


def _hysteresis_mask(f: "_Forward", kw: dict, **more) -> torch.Tensor:
    """The hysteresis mask of a forward's scored maps: from the logits on the plain path, from the probability maps under tta / tiled."""
    from .hysteresis import hysteresis as hysteresis_mask
    return hysteresis_mask(f.scored, from_logits=f.is_logits, **{**kw, **more})


def _one_hot_maps(mask: torch.Tensor, num_classes: int) -> torch.Tensor:
    """float32 [B,C,H,W] maps whose arg-max is `mask`: what the scoring kernels take in place of logits."""
    return torch.nn.functional.one_hot(mask, num_classes).permute(0, 3, 1, 2).contiguous().float()


@torch.no_grad()
def evaluate(model: torch.nn.Module, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], tta=None, tiled=None,
             surface=None, instances=None, curves=None, cleanup=None, components=None, detection=None,
             hysteresis=None, split=None) -> Dict[str, float]:
    """The score table of the main head over `batches` of (images, labels): scoring.ConfusionScorer's mIoU, mDice, pixel accuracy
    and "images", then the keys of every family that is switched on, in this order (each scorer of scoring.py documents its own).
    tta=True, or a tuple of scales: the multi-scale + flip sum of probability maps (tta.predict_tta) is scored instead of the main
    head's logits.  tiled=True, or a dict of tiled.predict_tiled keywords: images of any size are scored on the blended probability
    maps of sliding-window inference; not together with tta.  Both are off for every falsy value.
    cleanup: a morphology.morphology `steps` sequence; components: a components.components `steps` sequence (area_open /
    clear_border / fill_holes), applied to the arg-max mask after the cleanup chain where one is given.  With either, surface= and
    instances= score the cleaned mask and scoring.CleanScorer's two keys are added; every other key is what it is without them.
    surface (scoring.SurfaceScorer), instances (scoring.InstanceScorer): True or a dict of keywords, off for every falsy value.
    curves (scoring.CurveScorer): True or a dict of keywords -- an empty one asks for the defaults; off for None and False.
    detection (scoring.DetectionScorer): True or a dict of keywords, off for every falsy value; it scores the defects of the masked
    maps' arg-max like instances=, its keys come last.
    hysteresis: a (low, high) pair or a dict of hysteresis.hysteresis keywords (low, high, classes, background, min_area,
    connectivity): the hysteresis mask of the scored maps (from the logits on the plain path, from the probability maps under tta /
    tiled) replaces the arg-max as the start of the clean-up chain, and counts as a clean-up: scoring.CleanScorer's two keys are
    added and surface=, instances= and detection= score that mask.  Models of two classes and more; None: off.
    split: a radius or a dict of split.split_instances keywords (radius, min_marker_area, max_iters): the instances= and detection=
    scorers cut the PREDICTION's defects with split.split_instances before they match them (the ground truth is left alone); needs
    one of the two.  None: off, and every key keeps its value."""
    if cleanup is not None:
        from .morphology import check_steps
        cleanup = check_steps(cleanup)
    if components is not None:
        from .components import check_steps as check_component_steps
        components = check_component_steps(components)
    hyst_kw = _hysteresis_kwargs(hysteresis, "evaluate", True) if hysteresis is not None else None
    split_kw = None
    if split is not None:
        from .split import split_keywords
        split_kw = split_keywords(split, "evaluate")
        if not instances and not detection:
            raise ValueError("evaluate: split= cuts the defects the instances= and detection= scorers match: switch one of them on")
    clean = cleanup is not None or components is not None or hyst_kw is not None
    curve = scoring.CurveScorer(curves, plain_path=not (tta or tiled)) if curves is not None and curves is not False else None
    tiled_kw = _tiled_kwargs(tiled, tta, "evaluate") if tiled else None
    base = scoring.ConfusionScorer()
    scorers = [base, scoring.CleanScorer() if clean else None, scoring.SurfaceScorer(surface) if surface else None,
               scoring.InstanceScorer(instances, split_kw) if instances else None, curve,
               scoring.DetectionScorer(detection, split_kw) if detection else None]
    scorers = [s for s in scorers if s is not None]
    for x, y in batches:
        f = _forward(model, x, tta, tiled_kw, ("probs",))
        masked = f.scored
        if clean:
            Cn = f.scored.shape[1]
            if hyst_kw is not None and Cn == 1:
                raise ValueError("evaluate: hysteresis= scores models of two classes and more (one-channel sigmoid heads: bin_confusion)")
            start = torch.argmax(f.scored, dim=1) if hyst_kw is None else _hysteresis_mask(f, hyst_kw)
            masked = _one_hot_maps(_cleaned(start, cleanup, Cn, components), Cn)
        batch = scoring.Batch(f.scored, f.is_logits, masked, y, f.heads)
        for s in scorers:
            s.update(batch)
    out = {}
    for s in scorers:
        out.update(s.result(base.images))
    return out


def _with_shapes(inst, shapes, connectivity: int):
    """predict_instances' result: the InstanceResult itself, or with `shapes` the ShapeResult that describes it."""
    if not shapes:
        return inst
    from .shapes import shape_descriptors
    return shape_descriptors(inst, thickness=shapes == "thickness", connectivity=connectivity)


@torch.no_grad()
def predict_instances(model: torch.nn.Module, images: torch.Tensor, *, tta=None, tiled=None, min_area: int = 1, connectivity: int = 8,
                      max_instances: int = 256, cleanup=None, components=None, shapes=False, skeleton=False, hull=False,
                      contours=False, simplify=None, raster=False, hysteresis=None, split=None):
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
    like to every defect.  Under all three paths, after the clean-up chains.
    skeleton=True, or a dict {"max_iters": n}: a skeleton.SkeletonStats instead -- skeleton.skeletonize of the mask that is labelled
    (after the clean-up chains, every class but 0), then skeleton.skeleton_descriptors of the InstanceResult; its props() and
    records() add length, widths, end and branch counts to every defect.  With shapes also set the ShapeResult is its `.shapes`
    and records() merges both.  Under all three paths.
    hull=True: a hull.HullResult instead -- hull.hull_descriptors of that InstanceResult; its `.also` holds what the same call returns
    without hull= (the ShapeResult, the SkeletonStats, or None for the bare InstanceResult), and its props() and records() add
    solidity, the Feret diameters and the minimum-area rectangle to every defect.  Under all three paths.
    contours=True: a contours.ContourResult instead -- contours.contours of that InstanceResult at the call's connectivity: the
    boundary of every defect as polygon rings (polygons(), to_coco()); its `.also` holds what the same call returns without
    contours= (the HullResult, the ShapeResult, the SkeletonStats, or None for the bare InstanceResult) and its records() adds
    the ring counts and the crack perimeter to theirs.  Under all three paths, after both clean-up chains.
    simplify=epsilon (a float, pixels; needs contours=True): a simplify.SimplifiedContours instead -- simplify.simplify_contours of
    that ContourResult at the tolerance epsilon, the staircases of slanted edges reduced to their corners; its `.source` is the
    ContourResult.  Under all three paths.
    raster=True (needs contours=True): a raster.RasterResult instead -- raster.rasterize_contours of what the same call returns
    without raster= (the ContourResult, or with simplify= the SimplifiedContours), filled against the instance labels: its
    `.contours` holds that result, iou() and fidelity() say what every polygon still covers of its defect.  Under all three paths.
    hysteresis=(low, high), or a dict of hysteresis.hysteresis keywords (low, high, classes, background, min_area): the mask that is
    cleaned and labelled is the hysteresis mask instead of the arg-max -- of the main head's logits on the plain path, of the
    probability maps under tta and tiled -- at the call's connectivity, before the cleanup= and components= chains; every other
    keyword works as before.  A one-channel sigmoid model needs it (ValueError without) and has the plain path alone: the mask is
    class 1 where the rule says so, the confidence is max(p, 1 - p) of the sigmoid, later steps see two classes and no uncertainty
    map is formed.
    split=radius, or a dict of split.split_instances keywords (radius, min_marker_area, max_iters): touching defects are cut apart --
    split.split_instances of the InstanceResult, at the call's connectivity and min_area and with the same confidence / uncertainty
    maps, after label_instances and both clean-up chains and before shapes= / skeleton= / hull= / contours=, which then describe the
    PIECES.  What takes the InstanceResult's place is the pieces' (a split.SplitInstances: an InstanceResult whose `.split` holds
    the SplitResult with parent, pieces, converged and the unsplit source).  Under all three paths."""
    from . import instances
    if raster is not False and raster is not True:
        raise ValueError("predict_instances: raster is False or True")
    if raster and not contours:
        raise ValueError("predict_instances: raster needs contours=True")
    if contours is not False and contours is not True:
        raise ValueError("predict_instances: contours is False or True")
    if simplify is not None:
        from .simplify import quantise
        if not contours:
            raise ValueError("predict_instances: simplify needs contours=True")
        quantise(simplify)
    if hull is not False and hull is not True:
        raise ValueError("predict_instances: hull is False or True")
    if shapes not in (False, True, "thickness"):
        raise ValueError("predict_instances: shapes is False, True or \"thickness\"")
    if not (skeleton is False or skeleton is True or (isinstance(skeleton, dict) and set(skeleton) <= {"max_iters"})):
        raise ValueError("predict_instances: skeleton is False, True or a dict {\"max_iters\": n}")
    clean = cleanup is not None or components is not None
    if components is not None:
        from .components import check_steps as check_component_steps
        components = check_component_steps(components)
    hyst_kw = _hysteresis_kwargs(hysteresis, "predict_instances", False) if hysteresis is not None else None
    split_kw = None
    if split is not None:
        from . import split as split_mod
        split_kw = split_mod.split_keywords(split, "predict_instances")
    tiled_kw, want = None, ("mask", "conf", "heads") + (("probs",) if tta and hyst_kw is not None else ())
    if tiled:
        # (the class count of the clean-up is the blended maps' channel count: they are asked for beside the mask then)
        tiled_kw = _tiled_kwargs(tiled, tta, "predict_instances")
        want = ("mask", "conf") + (("probs",) if clean or skeleton is not False or hyst_kw is not None else ())
        tiled_kw.setdefault("uncertainty", "auto")
    f = _forward(model, images, tta, tiled_kw, want)
    num_classes = (f.scored if f.heads is None else f.heads[0]).shape[1] if f.scored is not None or f.heads is not None else None
    binary = num_classes == 1                   # a one-channel sigmoid head (the plain path: tta and tiled have refused it)
    if binary and hyst_kw is None:
        raise ValueError("predict_instances: a one-channel sigmoid model has no arg-max mask: pass hysteresis=(low, high)")
    conf = f.conf
    if binary:
        p = torch.sigmoid(f.scored)[:, 0]
        conf, num_classes = torch.maximum(p, 1.0 - p), 2
    maps = (conf,) + f.maps
    if f.heads is not None and len(f.heads) >= 2 and not binary:
        maps += (consistency.uncertainty_map(f.heads[0], f.heads[1]),)
    mask = f.mask if hyst_kw is None else _hysteresis_mask(f, hyst_kw, connectivity=connectivity)
    if clean:
        mask = _cleaned(mask, cleanup, num_classes, components)
    inst = instances.label_instances(mask, maps, connectivity=connectivity, min_area=min_area, max_instances=max_instances)
    if split_kw is not None:
        cut = split_mod.split_instances(inst, maps=maps, connectivity=connectivity, min_area=min_area, **split_kw)
        inst = split_mod.SplitInstances(*cut.instances)
        inst.split = cut
    if skeleton is False:
        res = _with_shapes(inst, shapes, connectivity)
    else:
        from .skeleton import skeletonize, skeleton_descriptors
        skel = skeletonize(mask, num_classes, **(skeleton if isinstance(skeleton, dict) else {}))
        stats = skeleton_descriptors(inst, skel)
        res = stats._replace(shapes=_with_shapes(inst, shapes, connectivity)) if shapes else stats
    if hull:
        from .hull import hull_descriptors
        res = hull_descriptors(inst)._replace(also=None if res is inst else res)
    if not contours:
        return res
    from .contours import contours as trace_contours
    traced = trace_contours(inst, connectivity)._replace(also=None if res is inst else res)
    if simplify is not None:
        from .simplify import simplify_contours
        traced = simplify_contours(traced, simplify)
    if not raster:
        return traced
    from .raster import rasterize_contours
    return rasterize_contours(traced, reference=True)


def load_for_inference(model: torch.nn.Module, checkpoint_path: str, device: Optional[torch.device] = None) -> Dict:
    """Notebook cell 4: `checkpoint = torch.load(path); model.load_state_dict(checkpoint['state_dict'])` -- accepts the
    `module.`-prefixed keys of the reference's nn.DataParallel checkpoints (UAPS_train.py:443-450) and plain ones."""
    from .trainer import load_state_dict_any_prefix
    ck = torch.load(checkpoint_path, map_location=device or "cpu", weights_only=False)
    load_state_dict_any_prefix(model, ck["state_dict"] if "state_dict" in ck else ck)
    return ck

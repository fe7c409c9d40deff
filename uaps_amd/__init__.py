"""uaps_amd: MI355X-native training step of UAPS (uncertainty-aware, dynamically mixed pseudo-labels).

Public surface (mirrors the names the reference's UAPS_train.py imports):
  net_factory, UNet_UAPS, UNet                      (utilities/UAPS_net_factory.py, UAPS_unet.py)
  dice_loss, ce_loss, uaps_sup_loss, uaps_unsup_loss, uaps_step_loss   (UAPS_train.py:186-282)
  sigmoid_rampup, get_current_consistency_weight    (utilities/ramps.py, UAPS_train.py:81-87)
  FeatureNoise, Dropout, FeatureDropout             (utilities/UAPS_unet.py:156-185)
  mIoU, mDice, pixel_accuracy, seg_confusion        (utilities/metrics.py)
  softmax_mse_loss, softmax_kl_loss, kl_loss, entropy_map, entropy_minmization   (utilities/losses_1.py, losses_2.py)
  uncertainty_map                                   (UAPS-Testing.ipynb cell 24)
  sibling.cct_consistency_loss / ucc_pseudo_supervision / uamt_consistency_loss   the composed reference-shaped forms (CCT_train.py:195-199,
                                                    UCC_train.py:213-238, UA_MT_train.py:188-214)
  SegTrainer                                        the base of every trainer: optimizer + schedule, step frame, fit, checkpoints
  UAPSTrainer                                       (UAPS_train.py:109-450 step/optimizer/checkpoint)
  MeanTeacherTrainer, UAMTTrainer, ema_update, mc_consistency   (MT/MT_train.py, UAMT/UA_MT_train.py)
  CCTTrainer, DCTTrainer, cct_consistency, rot_consistency, rot90_batch   (CCT/CCT_train.py, DCT/DCT_train.py)
  CPSTrainer, cps_loss, cps_scalars, UNet_f         (CPS/CPS_train.py, utilities/m_unet.py)
  UCCTrainer, ucc_loss, ucc_scalars, cutmix_batch, cutmix_rects   (UCC/UCC_train.py, UCC/cross_cutmix.py; net_factory("unet_ucc"))
  SegLoss, seg_scalars, jaccard_loss, tversky_loss, FocalLoss, DiceLoss, seg_losses.ce_loss   the supervised loss family
                                                    (utilities/pytorch_losses.py, losses_1.py); BaselineTrainer(loss=SegLoss(...))
  BinarySegLoss, bin_scalars, bin_confusion, bin_metrics_from_confusion, sigmoid_mse_loss, sigmoid_kl_loss, BinaryTrainer
                                                    one-channel sigmoid heads; the reference-named binary losses (bce_loss, FocalLoss,
                                                    JaccardLoss, BCEDiceLoss, iou, f_score, ...: utilities/losses_2.py) live in
                                                    `uaps_amd.binary_losses`, beside the softmax names above
  predict_tta, tta_views, tta_fold, scaled_sizes, TTAResult, DEFAULT_SCALES   multi-scale + flip test-time augmentation
                                                    (utilities/base.py:24-46, BaseNet.forward(x, tta=True)); ResUAPS.forward(x, tta=True),
                                                    inference.evaluate(..., tta=True)
  label_instances, InstanceResult, mask_to_rle, rle_to_mask, format_rle, parse_rle, rle_from_strings, RLE
                                                    defect instances (connected components + per-defect table) and the reference's
                                                    run-length masks (utilities/utilities.py:36-63); inference.predict_instances
  predict_tiled, tile_plan, tile_window, tile_cut, tile_fold, TilePlan, TiledResult   sliding-window inference at full resolution:
                                                    overlapping tiles blended under a window; inference.evaluate(..., tiled=True),
                                                    inference.predict_instances(..., tiled=True)
  surface_distances, distance_transform_sq, SurfaceResult, SURFACE_COLUMNS   boundary metrics on an exact device distance transform:
                                                    HD, HD95, ASSD, NSD under medpy's conventions; inference.evaluate(..., surface=True)
  match_instances, MatchResult, MATCH_COLUMNS       defect matching against ground truth (two label_instances results): per-defect
                                                    partner / IoU / covered, PQ, SQ, RQ, defect precision / recall, PRO;
                                                    inference.evaluate(..., instances=True)
  detection_match, DetectionResult, DetectionSums, COCO_THRESHOLDS
                                                    defect detection scores: COCO's greedy assignment of scored defects at up to 32
                                                    IoU thresholds (0.1 .. 1.0) at once, exact integers; AP50, AP75, AP@[.50:.95], AR;
                                                    inference.evaluate(..., detection=True)
  score_curves, plane_curves, CurveResult, CurveSums  threshold-sweep metrics from histograms of quantised scores: pixel AUROC, AP,
                                                    AUPRO, ECE, and AUROC / AURC of the uncertainty map;
                                                    inference.evaluate(..., curves=True)
  morphology                                        mask clean-up on a label map: a fused chain of erode / dilate / open / close /
                                                    boundary steps (square, cross, disk; radius 1..15);
                                                    inference.predict_instances(..., cleanup=steps), inference.evaluate(..., cleanup=steps)
  components                                        component clean-up on a label map: a chain of area_open / clear_border /
                                                    fill_holes steps on the union-find kernels of label_instances;
                                                    inference.predict_instances(..., components=steps), inference.evaluate(..., components=steps)
  shape_descriptors, ShapeResult, SHAPE_COLUMNS     defect shape descriptors from the labels of label_instances: exact moments, bit-quad
                                                    counts and the statistics of a plane per defect in one pass; ShapeResult.props():
                                                    centroid, axes, orientation, perimeter, compactness, holes, inradius;
                                                    inference.predict_instances(..., shapes=True or "thickness")
  skeletonize, skeleton_descriptors, SkeletonResult, SkeletonStats, SKELETON_COLUMNS
                                                    defect skeletons: Guo-Hall thinning of the selected classes of a label map on
                                                    packed bit planes, and per defect the skeleton's links, ends and branch points;
                                                    SkeletonStats.props(): length, mean / max / rms width, end and branch counts;
                                                    inference.predict_instances(..., skeleton=True or {"max_iters": n})
  hull_descriptors, HullResult, HULL_COLUMNS        defect convex hulls from the labels of label_instances: strict vertices, area,
                                                    farthest pair, minimum caliper width and minimum-area rectangle as exact
                                                    integers; HullResult.props(): solidity, Feret diameters, the rotated box;
                                                    inference.predict_instances(..., hull=True)
  contours, ContourResult, RING_COLUMNS, CONTOUR_COLUMNS
                                                    defect contours from the labels of label_instances: crack-following outer and
                                                    hole rings as closed polygons of corner-lattice points, exact integers;
                                                    ContourResult.polygons(), records(), to_coco();
                                                    inference.predict_instances(..., contours=True)
  simplify_contours, SimplifiedContours             contour simplification: exact Ramer-Douglas-Peucker on those rings at a tolerance
                                                    in sixteenths of a pixel, integers only; polygons(), records(), to_coco(),
                                                    reduction(); inference.predict_instances(..., contours=True, simplify=epsilon)
  rasterize_contours, RasterResult, RingSet, rings_from_polygons, rings_from_coco, RASTER_COLUMNS
                                                    polygon rasterisation: the exact even-odd fill of polygon rings (traced,
                                                    simplified, or COCO / labelme ground truth in sixteenths of a pixel) into a
                                                    label map and a class map, integers only; RasterResult.iou(), fidelity(),
                                                    records(); inference.predict_instances(..., contours=True, raster=True)
  hysteresis, reconstruct                           hysteresis thresholding of score maps (a region above `low` is kept iff it holds
                                                    a pixel above `high`) and binary reconstruction of a label map from markers, on
                                                    the union-find kernels of label_instances; one-channel sigmoid heads included;
                                                    inference.predict_instances(..., hysteresis=(low, high)), inference.evaluate(..., hysteresis=...)
  split_instances, SplitResult                      touching defects cut apart: cores by the distance transform (or the caller's
                                                    markers), grown back inside the defect in synchronous rounds on LDS tiles, the
                                                    pieces numbered and tabulated like label_instances' components;
                                                    inference.predict_instances(..., split=radius), inference.evaluate(..., split=...)
"""
from .ramps import sigmoid_rampup, get_current_consistency_weight
from .losses import (dice_loss, ce_loss, uaps_sup_loss, uaps_unsup_loss, uaps_step_loss, uaps_pair_loss, unsup_scalars,
                     sup_scalars)
from .perturb import FeatureNoise, Dropout, FeatureDropout, manual_seed as perturb_manual_seed
from .metrics import mIoU, mDice, pixel_accuracy, seg_confusion, seg_confusion_per_image, metrics_from_confusion, mean_batch_metrics
from .unet import UNet, UNet_UAPS, UNet_f
from .res_uaps import ResUAPS, ResNet, resnet50
from .net_factory import net_factory
from .consistency import (softmax_mse_loss, softmax_kl_loss, kl_loss, entropy_map, entropy_minmization, uncertainty_map)
from .trainer import SegTrainer, UAPSTrainer, BaselineTrainer
from .mean_teacher import MeanTeacherTrainer, UAMTTrainer, ema_update, mc_consistency
from .cct_dct import CCTTrainer, DCTTrainer, cct_consistency, rot_consistency, rot90_batch
from .cps import CPSTrainer, cps_loss, cps_scalars
from .ucc import UCCTrainer, ucc_loss, ucc_scalars, cutmix_batch, cutmix_rects
from .seg_losses import SegLoss, seg_scalars, jaccard_loss, tversky_loss, FocalLoss, DiceLoss
from .binary_losses import BinarySegLoss, bin_scalars, bin_confusion, bin_metrics_from_confusion, sigmoid_mse_loss, sigmoid_kl_loss
from .binary_trainer import BinaryTrainer
from . import binary_losses, binary_trainer
from .pipelines import Recipe, Stage, RECIPES, ViewDraws, draw, augment_views, ArrayBatches, UCCArrayBatches
from . import pipelines
from .tta import predict_tta, tta_views, tta_fold, scaled_sizes, TTAResult, DEFAULT_SCALES
from . import tta
from .instances import label_instances, InstanceResult, mask_to_rle, rle_to_mask, format_rle, parse_rle, rle_from_strings, RLE
from . import instances
from .tiled import predict_tiled, tile_plan, tile_window, tile_cut, tile_fold, TilePlan, TiledResult
from . import tiled
from .surface import surface_distances, distance_transform_sq, SurfaceResult, SURFACE_COLUMNS
from . import surface
from .matching import match_instances, MatchResult, MATCH_COLUMNS
from . import matching
from .detection import detection_match, DetectionResult, DetectionSums, COCO_THRESHOLDS
from . import detection
from .curves import score_curves, plane_curves, CurveResult, CurveSums
from . import curves
from .morphology import morphology          # (the function takes the submodule's name: uaps_amd.morphology(mask, steps, C))
from .components import components          # (likewise: uaps_amd.components(mask, steps, C))
from .shapes import shape_descriptors, ShapeResult, SHAPE_COLUMNS
from . import shapes
from .skeleton import skeletonize, skeleton_descriptors, SkeletonResult, SkeletonStats, SKELETON_COLUMNS
from . import skeleton
from .hull import hull_descriptors, HullResult, HULL_COLUMNS
from . import hull
from .contours import contours, ContourResult, RING_COLUMNS, CONTOUR_COLUMNS      # (the function takes the submodule's name)
from .simplify import simplify_contours, SimplifiedContours
from . import simplify
from .raster import rasterize_contours, RasterResult, RingSet, rings_from_polygons, rings_from_coco, RASTER_COLUMNS
from . import raster
from .hysteresis import hysteresis, reconstruct      # (hysteresis takes the submodule's name: uaps_amd.hysteresis(scores, low, high))
from .split import split_instances, SplitResult
from . import split
from . import augment, cct_dct, conv, cps, data, dist, graph, inference, mean_teacher, optim, seg_losses, sibling, ucc

__all__ = [n for n in dir() if not n.startswith("_")]

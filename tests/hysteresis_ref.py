"""The reference of the hysteresis tests (tests/test_hysteresis_host.py, tests/test_gpu_hysteresis.py), on scipy.ndimage.label alone
with explicit 4- and 8-structures.  Per class: label the candidates, keep the labels that occur under a seed, apply min_area from
np.bincount.  It restates the algorithm of skimage.filters.apply_hysteresis_threshold (which is not a dependency) and shares nothing
with the package's union-find.  With from_logits the scores are the float64 softmax / sigmoid rounded to fp32 (the convention of
tests/curves_ref.py).  Every comparison built on it is exact, which the generator earns with a MARGIN: every selected score of a
generated case lies at least 1e-3 away from every threshold in use, where an fp32 softmax differs from the float64 one near 1e-7.

The generator builds score maps FROM a label map.  Raw values, each with a uniform jitter of +-0.05:
    a pixel of class c >= 1 (a candidate)   0.5 in channel c, 0.65 in the background channel -- the weak defect pixel whose arg-max
                                            is the background -- and 0.05 in the other channels;
    a random 3 % of those (the seeds)       0.85 in channel c, 0.05 everywhere else;
    every other pixel                       0.85 in the background channel, 0.05 in the others;
then every pixel is normalised to sum 1 (raw values are floored at 0.002, so that the logits log p are finite).  That puts candidates
into [0.33, 0.48], seeds above 0.72 and everything else below 0.12: low = 0.25 and high = 0.5 separate them with room to spare.  A
one-channel map is the class-1 channel of the two-channel construction (labels >= 1 all count as class 1); its logit is log p/(1-p)."""
import functools

import numpy as np
from scipy import ndimage

import components_ref as CR

F32 = np.float32
S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
S8 = np.ones((3, 3), dtype=int)
LOW, HIGH, MARGIN = 0.25, 0.5, 1e-3
PER_CLASS = ((0.2, 0.25, 0.3), (0.5, 0.6, 0.7))          # per-class thresholds for classes 1, 2, 3 of the generated maps


def _structure(connectivity):
    return S8 if connectivity == 8 else S4


def probabilities(S, from_logits):
    S = np.asarray(S, dtype=F32)
    if not from_logits:
        return S
    z = S.astype(np.float64)
    if S.shape[1] == 1:
        return (1.0 / (1.0 + np.exp(-z))).astype(F32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F32)


def _selection(C, classes, background):
    if classes is None:
        classes = [1] if C == 1 else [c for c in range(C) if c != background]
    return [int(c) for c in classes]


def _per_class(v, n):
    return np.asarray([v] * n if np.isscalar(v) else list(v), dtype=F32)


def classify(scores, low, high, from_logits=False, classes=None, background=0):
    """(cls int64 [B,H,W]: the pixel's class among the selected ones, cand bool, seed bool), thresholds in the order of `classes`."""
    p = probabilities(scores, from_logits)
    C = p.shape[1]
    cl = _selection(C, classes, background)
    lo, hi = _per_class(low, len(cl)), _per_class(high, len(cl))
    order = np.argsort(cl, kind="stable")                 # ascending classes: the first maximum is the lowest class
    cl, lo, hi = np.asarray(cl)[order], lo[order], hi[order]
    sel = p[:, [0] * len(cl)] if C == 1 else p[:, cl]
    bad = np.isnan(sel).any(axis=1)
    k = np.argmax(np.where(np.isnan(sel), -np.inf, sel), axis=1)
    best = np.take_along_axis(sel, k[:, None], axis=1)[:, 0]
    with np.errstate(invalid="ignore"):
        cand, seed = ~bad & (best >= lo[k]), ~bad & (best >= hi[k])
    return cl[k].astype(np.int64), cand, seed


def _keep(plane, seed, connectivity, min_area):
    lab, n = ndimage.label(plane, structure=_structure(connectivity))
    keep = np.zeros(n + 1, dtype=bool)
    keep[np.unique(lab[seed & plane])] = True
    keep &= np.bincount(lab.reshape(-1), minlength=n + 1) >= min_area
    keep[0] = False
    return keep[lab]


def hysteresis(scores, low, high, from_logits=False, classes=None, background=0, connectivity=8, min_area=1):
    """scores [B,C,H,W] -> int64 [B,H,W]: the class on the pixels of seeded candidate components, `background` elsewhere."""
    cls, cand, seed = classify(scores, low, high, from_logits, classes, background)
    out = np.full(cls.shape, background, dtype=np.int64)
    for b in range(cls.shape[0]):
        for c in np.unique(cls[b][cand[b]]):
            out[b][_keep(cand[b] & (cls[b] == c), seed[b], connectivity, min_area)] = c
    return out


def reconstruct(mask, markers, num_classes, classes=None, background=0, connectivity=8, min_area=1):
    m = np.array(mask)
    cl = [c for c in range(num_classes) if c != background] if classes is None else [int(c) for c in classes]
    out = m.copy()
    for b in range(m.shape[0]):
        for c in cl:
            plane = m[b] == c
            out[b][plane & ~_keep(plane, np.asarray(markers[b]) != 0, connectivity, min_area)] = background
    return out


def threshold_mask(scores, t, from_logits=False, classes=None, background=0):
    """The plain one-threshold mask: the pixel's class where its score reaches t (per class), `background` elsewhere."""
    cls, cand, _ = classify(scores, t, t, from_logits, classes, background)
    return np.where(cand, cls, background)


def margin(scores, thresholds, from_logits=False, classes=None, background=0):
    """The smallest distance of a selected score (float64 softmax with from_logits) from a threshold in use."""
    S = np.asarray(scores, dtype=np.float64)
    C = S.shape[1]
    if from_logits:
        if C == 1:
            S = 1.0 / (1.0 + np.exp(-S))
        else:
            e = np.exp(S - S.max(axis=1, keepdims=True))
            S = e / e.sum(axis=1, keepdims=True)
    cl = _selection(C, classes, background)
    sel = S[:, [0] * len(cl)] if C == 1 else S[:, cl]
    return min(float(np.abs(sel - float(t)).min()) for t in np.unique(np.asarray(thresholds, dtype=np.float64)))


def informative(ref, scores, low, high, from_logits=False, classes=None, background=0):
    """Something was dropped (the result is not the low-threshold mask), something grew beyond its seeds (nor the high-threshold
    mask), and something is left."""
    lo = threshold_mask(scores, low, from_logits, classes, background)
    hi = threshold_mask(scores, high, from_logits, classes, background)
    return bool((ref != lo).any() and (ref != hi).any() and (ref != background).any())


# ------------------------------------------------------------------------------------------------ generators
def scores_from_labels(m, C=4, seed=0, seeds=None):
    """(probabilities fp32 [B,C,H,W], logits fp32 [B,C,H,W]) built from the label map m [B,H,W] by the recipe of the module's text.
    seeds: a bool [B,H,W] map that replaces the random 3 % (only candidate pixels among it count)."""
    m = np.asarray(m)
    rng = np.random.default_rng(seed)
    B, H, W = m.shape
    Cn = max(C, 2)
    lab = np.where((m >= 1) & (m < Cn), m, 0) if C > 1 else np.where((m >= 1) & (m < 255), 1, 0)
    cand = lab > 0
    strong = cand & (rng.random((B, H, W)) < 0.03) if seeds is None else cand & np.asarray(seeds, dtype=bool)
    raw = np.full((B, Cn, H, W), 0.05)
    raw[:, 0] = np.where(cand, np.where(strong, 0.05, 0.65), 0.85)
    own = np.where(strong, 0.85, 0.5)
    for c in range(1, Cn):
        raw[:, c] = np.where(lab == c, own, raw[:, c])
    raw = np.maximum(raw + rng.uniform(-0.05, 0.05, raw.shape), 0.002)
    p = raw / raw.sum(axis=1, keepdims=True)
    if C == 1:
        p1 = p[:, 1:2]
        return p1.astype(F32), np.log(p1 / (1.0 - p1)).astype(F32)
    return p.astype(F32), np.log(p).astype(F32)


@functools.lru_cache(maxsize=None)
def _case(shape, C, from_logits):
    p, z = scores_from_labels(CR.rings(*shape), C)
    s = z if from_logits else p
    for lo, hi in ((LOW, HIGH), PER_CLASS):
        if C == 1 and not np.isscalar(lo):
            continue
        assert margin(s, np.concatenate([np.atleast_1d(lo), np.atleast_1d(hi)]), from_logits) >= MARGIN, ("margin", shape, C)
    s.setflags(write=False)
    return s


def case(shape, C=4, from_logits=False):
    """The generated scores (logits with from_logits) of components_ref.rings(*shape); the margin condition is asserted here, once.
    Read-only and cached."""
    return _case(tuple(shape), C, bool(from_logits))


@functools.lru_cache(maxsize=None)
def _expected(shape, C, from_logits, per_class, connectivity, min_area, check):
    s = case(shape, C, from_logits)
    lo, hi = PER_CLASS if per_class else (LOW, HIGH)
    ref = hysteresis(s, lo, hi, from_logits, connectivity=connectivity, min_area=min_area)
    if check:
        assert informative(ref, s, lo, hi, from_logits), ("a vacuous case", shape, C, connectivity)
    ref.setflags(write=False)
    return ref


def expected(shape, C=4, from_logits=False, per_class=False, connectivity=8, min_area=1, check=True):
    """The reference result of case(shape, C, from_logits) at the scalar or the per-class thresholds; check: the informative
    condition is asserted.  Read-only and cached: shared by the tests that need it."""
    return _expected(tuple(shape), C, bool(from_logits), bool(per_class), connectivity, min_area, bool(check))

"""Float64 restatements (torch double on the CPU, autograd) of the reference's supervised loss family, written from its formulas:
utilities/pytorch_losses.py ce_loss (:31-51), dice_loss (:54-89), jaccard_loss (:92-128), tversky_loss (:131-175) and
utilities/losses_1.py FocalLoss (:63-97), DiceLoss (:100-136) -- plus the defined extension of csrc/loss_seg.hip: a pixel whose label
equals `ignore` enters no term (the region sums exclude it, focal divides by the number of valid pixels); a label outside [0, C) that
is not `ignore` enters no term either.  With nothing ignored these are the reference's own expressions."""
import torch
import torch.nn.functional as F

TERMS = ("ce", "focal", "dice", "jaccard", "tversky", "dice_sq")


def _masks(true, C, ignore):
    inside = (true >= 0) & (true < C)
    valid = inside if ignore is None else inside & (true != ignore)
    safe = torch.where(valid, true, torch.zeros_like(true))
    return valid, safe


def _region(true, logits, ignore):
    """probas and one-hot labels [B,C,H,W] with the ignored pixels zeroed in both (pytorch_losses.py:81-87 otherwise)."""
    C = logits.shape[1]
    valid, safe = _masks(true, C, ignore)
    m = valid.unsqueeze(1).to(logits.dtype)
    one_hot = torch.eye(C, dtype=logits.dtype)[safe].permute(0, 3, 1, 2) * m
    return F.softmax(logits, dim=1) * m, one_hot


def ce_loss(true, logits, weights=None, ignore=None):
    C = logits.shape[1]
    valid, safe = _masks(true, C, ignore)
    target = torch.where(valid, safe, torch.full_like(safe, -100))
    w = None if weights is None else torch.as_tensor(weights, dtype=logits.dtype)
    return F.cross_entropy(logits, target, weight=w, ignore_index=-100)


def focal_loss(true, logits, gamma=2.0, alpha=None, size_average=True, ignore=None, detach_pt=True):
    """losses_1.py:74-97.  detach_pt=False: the full derivative through (1 - p_t)^gamma, which the reference does NOT take (:85)."""
    C = logits.shape[1]
    valid, safe = _masks(true, C, ignore)
    logpt = F.log_softmax(logits, dim=1).gather(1, safe.unsqueeze(1)).squeeze(1)
    pt = logpt.detach().exp() if detach_pt else logpt.exp()
    if alpha is not None:
        logpt = logpt * torch.as_tensor(alpha, dtype=logits.dtype)[safe]
    loss = (-1 * (1 - pt) ** gamma * logpt)[valid]
    return loss.mean() if size_average else loss.sum()


def dice_loss(true, logits, eps=1e-7, ignore=None):
    p, t = _region(true, logits, ignore)
    inter, card = (p * t).sum((0, 2, 3)), (p + t).sum((0, 2, 3))
    return 1 - (2.0 * inter / (card + eps)).mean()


def jaccard_loss(true, logits, eps=1e-7, ignore=None):
    p, t = _region(true, logits, ignore)
    inter, card = (p * t).sum((0, 2, 3)), (p + t).sum((0, 2, 3))
    return 1 - (inter / (card - inter + eps)).mean()


def tversky_loss(true, logits, alpha, beta, eps=1e-7, ignore=None):
    p, t = _region(true, logits, ignore)
    valid = _masks(true, logits.shape[1], ignore)[0].unsqueeze(1).to(logits.dtype)
    inter = (p * t).sum((0, 2, 3))
    fps, fns = (p * (valid - t)).sum((0, 2, 3)), ((valid - p) * t).sum((0, 2, 3))
    return 1 - (inter / (inter + alpha * fps + beta * fns + eps)).mean()


def dice_sq_loss(true, logits, weight=None, ignore=None, smooth=1e-5):
    """losses_1.DiceLoss(C)(logits, true, weight, softmax=True)."""
    C = logits.shape[1]
    p, t = _region(true, logits, ignore)
    w = [1.0] * C if weight is None else [float(x) for x in weight]
    loss = 0.0
    for i in range(C):
        inter, y_sum, z_sum = (p[:, i] * t[:, i]).sum(), (t[:, i] * t[:, i]).sum(), (p[:, i] * p[:, i]).sum()
        loss = loss + (1 - (2 * inter + smooth) / (z_sum + y_sum + smooth)) * w[i]
    return loss / C


def seg_terms(true, logits, class_weight=None, ignore=None, focal_gamma=2.0, focal_alpha=None, focal_mean=True, tversky=(0.5, 0.5),
              dice_sq_weight=None, eps=1e-7, detach_pt=True):
    """All six terms by name."""
    return {"ce": ce_loss(true, logits, class_weight, ignore),
            "focal": focal_loss(true, logits, focal_gamma, focal_alpha, focal_mean, ignore, detach_pt),
            "dice": dice_loss(true, logits, eps, ignore), "jaccard": jaccard_loss(true, logits, eps, ignore),
            "tversky": tversky_loss(true, logits, tversky[0], tversky[1], eps, ignore),
            "dice_sq": dice_sq_loss(true, logits, dice_sq_weight, ignore)}


def fixture_cases(g):
    """The entries of g11_seglosses.npz as (case prefix, entry name, key of the labels to use, keyword arguments of `seg_terms`); the
    value is stored under prefix + name, the gradient (where stored) under prefix + "d" + name, the term is `term_of(name)`."""
    out = []
    for i in range(3):
        pre = f"c{i}_"
        alpha = [float(a) for a in g[pre + "alpha"]]
        out += [(pre, "ce", "labels_ign", dict(class_weight=g[pre + "ce_w"].tolist(), ignore=255)),
                (pre, "jaccard", "labels", {}),
                (pre, "tversky", "labels", dict(tversky=(0.3, 0.7))),
                (pre, "focal_g2", "labels", dict(focal_gamma=2.0, focal_alpha=alpha)),
                (pre, "focal_g15", "labels", dict(focal_gamma=1.5, focal_alpha=alpha)),
                (pre, "focal_sum", "labels", dict(focal_gamma=2.0, focal_mean=False)),
                (pre, "dice_sq", "labels", dict(dice_sq_weight=g[pre + "dsq_w"].tolist()))]
    return out


def term_of(name):
    return "focal" if name.startswith("focal") else name


# ---- the fixture's entries through the package (shared by the host and the GPU tests) ------------------------------------------------

def entry_point(name, g, pre, y, z):
    """The fixture entry `name` through the reference-signature entry point of uaps_amd.seg_losses."""
    from uaps_amd import seg_losses as S
    alpha = [float(a) for a in g[pre + "alpha"]]
    if name == "ce":
        return S.ce_loss(y.unsqueeze(1), z, torch.tensor(g[pre + "ce_w"]), ignore=255)
    if name == "jaccard":
        return S.jaccard_loss(y.unsqueeze(1), z)
    if name == "tversky":
        return S.tversky_loss(y, z, 0.3, 0.7)
    if name == "focal_g2":
        return S.FocalLoss(gamma=2, alpha=alpha)(z, y)
    if name == "focal_g15":
        return S.FocalLoss(gamma=1.5, alpha=alpha)(z, y)
    if name == "focal_sum":
        return S.FocalLoss(gamma=2, alpha=None, size_average=False)(z, y)
    if name == "dice_sq":
        return S.DiceLoss(z.shape[1])(z, y.unsqueeze(1), weight=[float(a) for a in g[pre + "dsq_w"]], softmax=True)
    raise KeyError(name)


def seg_loss_for(name, g, pre):
    """The same entry as a one-term SegLoss."""
    from uaps_amd import seg_losses as S
    alpha = [float(a) for a in g[pre + "alpha"]]
    return {"ce": lambda: S.SegLoss({"ce": 1.0}, class_weight=g[pre + "ce_w"].tolist(), ignore_index=255),
            "jaccard": lambda: S.SegLoss({"jaccard": 1.0}),
            "tversky": lambda: S.SegLoss({"tversky": 1.0}, tversky=(0.3, 0.7)),
            "focal_g2": lambda: S.SegLoss({"focal": 1.0}, focal_gamma=2, focal_alpha=alpha),
            "focal_g15": lambda: S.SegLoss({"focal": 1.0}, focal_gamma=1.5, focal_alpha=alpha),
            "focal_sum": lambda: S.SegLoss({"focal": 1.0}, focal_size_average=False),
            "dice_sq": lambda: S.SegLoss({"dice_sq": 1.0}, dice_sq_weight=g[pre + "dsq_w"].tolist())}[name]()

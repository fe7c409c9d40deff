"""An independent statement of the boundary table of uaps_amd/surface.py on scipy: surfaces by binary_erosion with the 4-connected
cross, exact squared distances as rint(distance_transform_edt(~other_surface) ** 2) (float64: exact up to 2 * 4095^2, checked against
brute force), the table's columns with Python integers (math.isqrt), np.percentile for the float check; and the patterns the tests of
both paths share."""
import functools
import math

import numpy as np
import torch
from scipy import ndimage

DEV = torch.device("cuda:0")
COLUMNS = ("n_pred", "n_gt", "max_pg", "max_gp", "sum16_pg", "sum16_gp", "within_pg", "within_gp", "rank_lo", "rank_hi", "q_lo", "q_hi")
NO_FEATURE = 2 ** 30
CROSS = ndimage.generate_binary_structure(2, 1)


def surface(m, c):
    fg = m == c
    return fg ^ ndimage.binary_erosion(fg, structure=CROSS, border_value=0)


def edt_sq(mask):
    """int64: the squared distance of every pixel to the nearest zero pixel of `mask`; NO_FEATURE everywhere without one."""
    mask = np.asarray(mask) != 0
    if mask.all():
        return np.full(mask.shape, NO_FEATURE, dtype=np.int64)
    return np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)


def directed(m_pred, m_gt, c):
    """(d2_pg, d2_gp) int64 arrays, or None for a pair that is not valid."""
    sp, sg = surface(m_pred, c), surface(m_gt, c)
    if not sp.any() or not sg.any():
        return int(sp.sum()), int(sg.sum()), None, None
    return int(sp.sum()), int(sg.sum()), edt_sq(~sg)[sp], edt_sq(~sp)[sg]


def tol_d2(tolerance):
    return None if tolerance is None else int(math.floor(float(tolerance) * float(tolerance)))


def table(pred, target, C, percentile=95.0, tolerance=None, tol_sq=None):
    """int64 [B,C,12] with Python-integer arithmetic.  tol_sq: the squared tolerance itself, in place of floor(tolerance^2)."""
    B = pred.shape[0]
    t2 = tol_d2(tolerance) if tol_sq is None else int(tol_sq)
    out = np.zeros((B, C, 12), dtype=np.int64)
    for b in range(B):
        for c in range(C):
            n_p, n_g, pg, gp = directed(pred[b], target[b], c)
            row = [n_p, n_g] + [0] * 10
            if pg is not None:
                pgl, gpl = [int(v) for v in pg], [int(v) for v in gp]
                row[2], row[3] = max(pgl), max(gpl)
                row[4], row[5] = sum(math.isqrt(v << 32) for v in pgl), sum(math.isqrt(v << 32) for v in gpl)
                if t2 is not None:
                    row[6], row[7] = sum(v <= t2 for v in pgl), sum(v <= t2 for v in gpl)
                pooled = sorted(pgl + gpl)
                N = len(pooled)
                h = float(N - 1) * (percentile / 100.0)
                lo = int(math.floor(h))
                hi = min(lo + 1, N - 1)
                row[8:12] = [lo, hi, pooled[lo], pooled[hi]]
            out[b, c] = row
    return out


def float_metrics(pred_b, target_b, c, percentile=95.0, tolerance=None):
    """hd, hd95, asd_pg, asd_gp, nsd of one valid pair in float64, the way a medpy user computes them."""
    _, _, pg, gp = directed(pred_b, target_b, c)
    dp, dg = np.sqrt(pg.astype(np.float64)), np.sqrt(gp.astype(np.float64))
    out = {"hd": max(dp.max(), dg.max()), "hd95": float(np.percentile(np.hstack((dp, dg)), percentile)),
           "asd_pg": float(dp.mean()), "asd_gp": float(dg.mean())}
    if tolerance is not None:
        out["nsd"] = float(((pg <= tol_d2(tolerance)).sum() + (gp <= tol_d2(tolerance)).sum()) / (len(pg) + len(gp)))
    return out


# ------------------------------------------------------------------------------------------------ patterns: (pred, target) int64 [B,H,W]
def blobs(B, H, W, C=4, seed=1, n=6):
    """Random rectangles per class; the prediction is the target with rectangles of its own added."""
    rng = np.random.default_rng(seed)

    def draw(base, k):
        m = base.copy()
        for b in range(B):
            for _ in range(k):
                h, w = rng.integers(1, max(2, H // 2 + 1)), rng.integers(1, max(2, W // 2 + 1))
                y, x = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
                m[b, y:y + h, x:x + w] = rng.integers(0, C)
        return m
    target = draw(np.zeros((B, H, W), dtype=np.int64), n)
    return draw(target, max(1, n // 2)), target


def class_noise(B, H, W, C=4, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, C, (B, H, W)).astype(np.int64), rng.integers(0, C, (B, H, W)).astype(np.int64)


def filled(B, H, W, C=4, seed=2):
    """One class fills the prediction (its surface is the edge ring); the target is class noise."""
    return np.full((B, H, W), min(1, C - 1), dtype=np.int64), class_noise(B, H, W, C, seed)[1]


def absent(B, H, W, C=4, seed=3):
    """The last class is missing from the prediction and class 0 from the target: pairs that are not valid."""
    p, t = class_noise(B, H, W, C, seed)
    p[p == C - 1] = 0
    if C > 1:
        t[t == 0] = 1
    return p, t


def same(B, H, W, C=4, seed=4):
    p = blobs(B, H, W, C, seed)[1]
    return p, p.copy()


def shifted(B, H, W, C=4):
    """A rectangle of class 1 and the same rectangle moved by (3, 4): hd is exactly 5 where both fit inside the image."""
    p, t = np.zeros((B, H, W), dtype=np.int64), np.zeros((B, H, W), dtype=np.int64)
    h, w = max(1, min(6, H - 3)), max(1, min(9, W - 4))
    t[:, 0:h, 0:w] = min(1, C - 1)
    p[:, 3:3 + h, 4:4 + w] = min(1, C - 1)
    return p, t


def corner_pixels(B, H, W, C=4):
    """One pixel of class 1 in opposite corners: d2 = (H - 1)^2 + (W - 1)^2 both ways."""
    p, t = np.zeros((B, H, W), dtype=np.int64), np.zeros((B, H, W), dtype=np.int64)
    p[:, 0, 0] = min(1, C - 1)
    t[:, H - 1, W - 1] = min(1, C - 1)
    return p, t


PATTERNS = {"blobs": blobs, "noise": class_noise, "filled": filled, "absent": absent, "same": same, "shifted": shifted,
            "corners": corner_pixels}


@functools.lru_cache(maxsize=None)
def case(name, shape, C=4, seed=None):
    """((pred, target), reference table at percentile 95 without a tolerance), computed once and shared; treat as read-only."""
    B, H, W = shape
    fn = PATTERNS[name]
    pt = fn(B, H, W, C) if seed is None else fn(B, H, W, C, seed)
    for a in pt:
        a.setflags(write=False)
    return pt, table(pt[0], pt[1], C)


def valid_fraction(tab):
    return float(((tab[..., 0] > 0) & (tab[..., 1] > 0)).mean())

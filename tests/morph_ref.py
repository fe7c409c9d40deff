"""An independent restatement of uaps_amd.morphology for the tests: scipy.ndimage.binary_erosion / binary_dilation with explicit
footprint arrays (border_value 1 / 0), and the three-branch combine rule applied pixel class by pixel class, step by step.  Nothing
here shares code with the package's numpy path (which counts row runs on prefix sums)."""
import functools

import numpy as np
from scipy import ndimage

OPS = ("erode", "dilate", "open", "close", "boundary")
FOOTPRINTS = ("square", "cross", "disk")


def footprint(kind, r):
    """bool [2r+1, 2r+1]: the offsets (dy, dx) of the structuring element, centre at [r, r]."""
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    if kind == "square":
        return np.ones((2 * r + 1, 2 * r + 1), dtype=bool)
    if kind == "cross":
        return np.abs(dy) + np.abs(dx) <= r
    if kind == "disk":
        return dy * dy + dx * dx <= r * r               # |dx| <= floor(sqrt(r^2 - dy^2)), in integers
    raise ValueError(kind)


def erode(plane, S):
    return ndimage.binary_erosion(plane, structure=S, border_value=1)


def dilate(plane, S):
    return ndimage.binary_dilation(plane, structure=S, border_value=0)


def step_plane(plane, op, S):
    if op == "erode":
        return erode(plane, S)
    if op == "dilate":
        return dilate(plane, S)
    if op == "open":
        return dilate(erode(plane, S), S)
    if op == "close":
        return erode(dilate(plane, S), S)
    if op == "boundary":
        return plane & ~erode(plane, S)
    raise ValueError(op)


def step_image(img, op, S, classes, background):
    res = {c: step_plane(img == c, op, S) for c in classes}
    out = img.copy()
    stays = np.zeros(img.shape, dtype=bool)
    for c in classes:
        stays |= (img == c) & res[c]                    # 1: a selected class that its own result keeps
    stays |= (img != background) & ~np.isin(img, list(classes))     # 2: an obstacle passes through
    out[~stays] = background                            # 3: background or just removed ...
    for c in sorted(classes, reverse=True):             # ... the smallest class that covers it (written last, so it wins)
        out[~stays & res[c]] = c
    return out


def morphology(mask, steps, num_classes, classes=None, background=0):
    """int64 [B,H,W] -> int64 [B,H,W]."""
    classes = [c for c in range(num_classes) if c != background] if classes is None else list(classes)
    out = np.array(mask, dtype=np.int64, copy=True)
    for op, kind, r in steps:
        S = footprint(kind, r)
        for b in range(out.shape[0]):
            out[b] = step_image(out[b], op, S, classes, background)
    return out


@functools.lru_cache(maxsize=None)
def discs(B, H, W, C, r, seed=0):
    """int64 [B,H,W] (read-only): six filled discs per image of classes 1 .. C-1, radii in [2r+1, 3r+2], centres up to r pixels OUTSIDE
    the frame (masks touch all four borders), then salt of random classes and pepper to background, each at density 0.3 / (2r+1)^2 --
    scaled with r so that an erosion of radius r still leaves something and compares something."""
    rng = np.random.default_rng(seed * 7919 + r * 131 + H * 17 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        for k in range(6):
            rad = int(rng.integers(2 * r + 1, 3 * r + 3))
            if k < 4:                                   # one disc over each border, its centre outside the frame
                off = int(rng.integers(1, r + 1))
                cy, cx = ((-off, int(rng.integers(0, W))), (H - 1 + off, int(rng.integers(0, W))),
                          (int(rng.integers(0, H)), -off), (int(rng.integers(0, H)), W - 1 + off))[k]
            else:
                cy, cx = int(rng.integers(-r, H + r)), int(rng.integers(-r, W + r))
            m[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = 1 + (k + b) % (C - 1)
    density = 0.3 / (2 * r + 1) ** 2
    salt = rng.random((B, H, W)) < density
    m[salt] = rng.integers(1, C, size=int(salt.sum()))
    m[rng.random((B, H, W)) < density] = 0
    m.setflags(write=False)
    return m


def informative(ref, inp):
    """The three conditions every parametrised case asserts before it compares: the reference result differs from the input, is
    not empty and is not full."""
    return bool((ref != inp).any()) and bool((ref != 0).any()) and bool((ref == 0).any())

"""The reference of the component clean-up tests (tests/test_components_host.py, tests/test_gpu_components.py), on scipy.ndimage alone:
`label` with explicit structures, np.bincount for the areas, border membership from the four edges of the label image,
`binary_fill_holes` as a second opinion, and the combine rule written out.  It shares nothing with the package's numpy path (a
union-find).  Every comparison built on it is exact."""
import functools

import numpy as np
from scipy import ndimage

import instances_ref as IR

S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
S8 = np.ones((3, 3), dtype=int)
KINDS = ("area_open", "clear_border", "fill_holes")


def _structure(connectivity):
    return S8 if connectivity == 8 else S4


def _edge_labels(lab):
    """The labels (0 among them, possibly) that occur on the four edges of a label image."""
    return np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))


def _default_classes(num_classes, classes, background):
    return sorted(c for c in range(num_classes) if c != background) if classes is None else sorted(int(c) for c in classes)


def holes_of(P, connectivity, n):
    """The pixels of the holes of the binary plane P with at most n pixels (None: all): components of ~P under the complementary
    structure that do not touch the image border."""
    comp = _structure(4 if connectivity == 8 else 8)
    lab, k = ndimage.label(~P, structure=comp)
    area = np.bincount(lab.reshape(-1), minlength=k + 1)
    keep = np.ones(k + 1, dtype=bool)
    keep[0] = False
    keep[_edge_labels(lab)] = False
    if n is None:
        assert np.array_equal(keep[lab], ndimage.binary_fill_holes(P, structure=comp) & ~P)      # the second opinion
    else:
        keep &= area <= n
    return keep[lab]


def step_image(m, step, classes, background, connectivity):
    out = m.copy()
    if step[0] == "fill_holes":
        free = m == background                          # only background pixels are ever rewritten
        for c in classes:                               # ascending: the smallest class takes a shared pixel
            claim = free & holes_of(m == c, connectivity, step[1])
            out[claim] = c
            free &= ~claim
        return out
    for c in classes:
        lab, k = ndimage.label(m == c, structure=_structure(connectivity))
        drop = np.zeros(k + 1, dtype=bool)
        if step[0] == "area_open":
            drop = np.bincount(lab.reshape(-1), minlength=k + 1) < step[1]
        else:
            drop[_edge_labels(lab)] = True
        drop[0] = False
        out[drop[lab]] = background
    return out


def components(mask, steps, num_classes, classes=None, background=0, connectivity=8):
    """mask int64 [B,H,W] array -> the chain applied step by step, image by image."""
    cl = _default_classes(num_classes, classes, background)
    m = np.array(mask)
    for s in steps:
        s = tuple(s)
        m = np.stack([step_image(m[b], s, cl, background, connectivity) for b in range(m.shape[0])])
    return m


def informative(ref, m, background=0):
    """The step changed the input and left neither an empty nor a full mask: a test that compares two unchanged masks shows nothing."""
    return bool((ref != m).any() and (ref != background).any() and (ref == background).any())


# ------------------------------------------------------------------------------------------------ generators
@functools.lru_cache(maxsize=None)
def _rings(B, H, W, C, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((B, H, W), dtype=np.int64)
    y, x = np.mgrid[0:H, 0:W]
    big = max(3.0, min(max(H, W) / 4.0, 14.0))
    for b in range(B):
        for k in range(10):
            cy, cx = rng.integers(-4, H + 4), rng.integers(-4, W + 4)
            ro = rng.uniform(3.0, big)
            ri = ro - rng.uniform(1.5, 3.5)
            d2 = (y - cy) ** 2 + (x - cx) ** 2
            m[b][(d2 <= ro * ro) & (d2 >= ri * ri)] = 1 + (k + b) % (C - 1)
        noise = rng.random((H, W))
        m[b][noise < 0.01] = 0                                                          # pepper
        salt = (noise > 0.99)
        m[b][salt] = rng.integers(1, C, (H, W))[salt]
        for _ in range(3):
            m[b, rng.integers(0, H), rng.integers(0, W)] = 255
        if H >= 3 and W >= 3:                                                           # a 3 x 3 block with a pinhole: a one-pixel
            m[b, H // 2 - 1:H // 2 + 2, W // 2 - 1:W // 2 + 2] = 1                      # hole under either connectivity
            m[b, H // 2, W // 2] = 0
    m.setflags(write=False)
    return m


def rings(B, H, W, C=4, seed=0):
    """About ten annuli an image of classes 1..C-1, some centred up to 4 px outside the frame, salt and pepper at about 2 %, and a
    few 255 pixels, and a 3 x 3 block with a pinhole in the middle.  Read-only and cached: copy before changing it."""
    return _rings(B, H, W, C, seed)


def open_spiral(H, W, cls=1):
    return IR.spiral(H, W, cls)


def closed_spiral(H, W, cls=1):
    """instances_ref.spiral with its mouth sealed: the corridor between the walls, which opens at (1, 0), becomes ONE large hole."""
    m = np.array(IR.spiral(H, W, cls))
    assert m[0, 1, 0] == 0 and m[0, 0, 0] == cls and m[0, 2, 0] == cls
    m[0, 1, 0] = cls
    return m


def comb(H, W, cls=2):
    return IR.comb(H, W, cls)


def checkerboard(H, W, cls=1):
    return IR.checkerboard(H, W, cls)


def nested_rings(H=21, W=23):
    """A ring of class 2 around a ring of class 1 (square rings, two pixels thick, one pixel of background between them)."""
    m = np.zeros((1, H, W), dtype=np.int64)
    m[0, 2:H - 2, 2:W - 2] = 2
    m[0, 4:H - 4, 4:W - 4] = 0
    m[0, 5:H - 5, 5:W - 5] = 1
    m[0, 7:H - 7, 7:W - 7] = 0
    return m


def frame(H, W, cls=1):
    """A one-pixel frame along the whole image border."""
    m = np.zeros((1, H, W), dtype=np.int64)
    m[0, 0], m[0, -1], m[0, :, 0], m[0, :, -1] = cls, cls, cls, cls
    return m

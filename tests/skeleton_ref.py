"""The reference of the skeleton tests: Guo and Hall's thinning (CACM 32(3), 1989, algorithm A1) written per pixel from its definition,
and brute-force skeleton statistics per label.  It shares nothing with uaps_amd/skeleton.py: the deletion rule lives in two 256-entry
tables built by enumerating the neighbourhoods in plain Python, and a sub-iteration is an explicit loop over the foreground pixels
(`thin_pixels`) -- or, for the larger cases, the same tables looked up at a neighbourhood code formed with scipy.ndimage.correlate
(`thin`); test_skeleton_host.py checks the two against each other.

Neighbours P2..P9 = N, NE, E, SE, S, SW, W, NW; bit i of a neighbourhood code is P(i + 2); outside the image is background."""
import numpy as np
from scipy import ndimage

OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))       # P2 .. P9 as (dy, dx)


def _deletable(code: int, second: bool) -> bool:
    P = {i + 2: (code >> i) & 1 for i in range(8)}
    C = (int(not P[2] and (P[3] or P[4])) + int(not P[4] and (P[5] or P[6])) + int(not P[6] and (P[7] or P[8]))
         + int(not P[8] and (P[9] or P[2])))
    N1 = int(P[9] or P[2]) + int(P[3] or P[4]) + int(P[5] or P[6]) + int(P[7] or P[8])
    N2 = int(P[2] or P[3]) + int(P[4] or P[5]) + int(P[6] or P[7]) + int(P[8] or P[9])
    N = min(N1, N2)
    if second:
        third = (P[6] or P[7] or not P[9]) and P[8]
    else:
        third = (P[2] or P[3] or not P[5]) and P[4]
    return C == 1 and 2 <= N <= 3 and not third


TABLES = tuple(np.array([_deletable(code, second) for code in range(256)], dtype=bool) for second in (False, True))
_WEIGHTS = np.zeros((3, 3), dtype=np.int32)
for _i, (_dy, _dx) in enumerate(OFFSETS):
    _WEIGHTS[1 + _dy, 1 + _dx] = 1 << _i


def sub_iteration_pixels(plane: np.ndarray, second: bool) -> np.ndarray:
    """One sub-iteration as an explicit loop over the foreground pixels."""
    H, W = plane.shape
    out = plane.copy()
    for y, x in np.argwhere(plane):
        code = 0
        for i, (dy, dx) in enumerate(OFFSETS):
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and plane[yy, xx]:
                code |= 1 << i
        if TABLES[int(second)][code]:
            out[y, x] = False
    return out


def sub_iteration(plane: np.ndarray, second: bool) -> np.ndarray:
    """The same through a neighbourhood code per pixel (correlation with the bit weights, zero outside) and the table."""
    code = ndimage.correlate(plane.astype(np.int32), _WEIGHTS, mode="constant", cval=0)
    return plane & ~TABLES[int(second)][code]


def thin_plane(plane: np.ndarray, max_iters: int, step=sub_iteration):
    """(result, iterations that removed something, is the result a fixed point) after at most max_iters iterations."""
    p = plane.astype(bool)
    done = 0
    for _ in range(max_iters):
        q = step(step(p, False), True)
        if np.array_equal(p, q):
            return p, done, True
        p, done = q, done + 1
    return p, done, bool(np.array_equal(step(step(p, False), True), p))


def thin(mask: np.ndarray, classes, background: int = 0, max_iters: int = 64, step=sub_iteration):
    """The label-map rule on an int64 [B,H,W] map: every class of `classes` thinned on its own plane, removed pixels -> background,
    everything else untouched.  Returns (map, iterations [B] -- the largest count among the classes -- and fixed point [B])."""
    out = mask.copy()
    iters = np.zeros(mask.shape[0], dtype=np.int64)
    fixed = np.ones(mask.shape[0], dtype=bool)
    for b in range(mask.shape[0]):
        for c in classes:
            plane = mask[b] == c
            res, n, ok = thin_plane(plane, max_iters, step)
            out[b][plane & ~res] = background
            iters[b] = max(iters[b], n)
            fixed[b] &= ok
    return out, iters, fixed


def stats(labels: np.ndarray, skel: np.ndarray, classes, plane, M: int) -> np.ndarray:
    """int64 [B,M,7] (n_skel, n_orth, n_diag, n_end, n_branch, d2max, d2sum): a brute-force loop per label and pixel."""
    B, H, W = labels.shape
    table = np.zeros((B, M, 7), dtype=np.int64)
    classes = set(int(c) for c in classes)
    for b in range(B):
        pix = {}
        for y in range(H):
            for x in range(W):
                k = int(labels[b, y, x])
                if 1 <= k <= M and int(skel[b, y, x]) in classes:
                    pix.setdefault(k, set()).add((y, x))
        for k, S in pix.items():
            row = table[b, k - 1]
            for (y, x) in S:
                ring = [(y + dy, x + dx) in S for dy, dx in OFFSETS]
                row[0] += 1
                row[1] += int((y, x + 1) in S) + int((y + 1, x) in S)                       # each edge link by its first end
                row[2] += int((y + 1, x + 1) in S and (y, x + 1) not in S and (y + 1, x) not in S)
                row[2] += int((y + 1, x - 1) in S and (y, x - 1) not in S and (y + 1, x) not in S)
                row[3] += int(sum(ring) == 1)
                row[4] += int(sum(1 for i in range(8) if not ring[i] and ring[(i + 1) % 8]) >= 3)
                if plane is not None:
                    v = max(int(plane[b, y, x]), 0)
                    row[5] = max(row[5], v)
                    row[6] += v
    return table


# ---- the cases of the tests: fillings of an H x W frame -----------------------------------------------------------------------------
SHAPES = ((1, 1), (2, 2), (1, 70), (70, 1), (3, 200), (37, 53), (64, 64), (65, 129))
LINE_SHAPES = ((1, 1), (1, 70), (70, 1))       # nothing to thin: compared without the "differs from its input" claim


def _dilate(a: np.ndarray) -> np.ndarray:
    return ndimage.binary_dilation(a, structure=np.ones((3, 3), dtype=bool))


def filling(name: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """An int64 [1,H,W] label map (classes 1 and, for "two", 2 and an ignore stripe of 255)."""
    rng = np.random.default_rng(seed * 1000003 + H * 4099 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    if name.startswith("noise"):
        m = (rng.random((H, W)) < float(name[5:])).astype(np.int64)
    elif name == "discs":
        m = np.zeros((H, W), dtype=np.int64)
        for _ in range(6):
            cy, cx, r = rng.integers(-4, H + 4), rng.integers(-4, W + 4), rng.integers(2, max(3, min(H, W) // 3 + 2))
            d2 = (yy - cy) ** 2 + (xx - cx) ** 2
            m[d2 <= r * r] = 1
        for _ in range(3):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(3, max(4, min(H, W) // 2 + 3))
            d2 = (yy - cy) ** 2 + (xx - cx) ** 2
            m[(d2 <= r * r) & (d2 >= (r - 2) * (r - 2))] = 1
    elif name == "salt":
        m = _dilate(_dilate(rng.random((H, W)) < 0.02)).astype(np.int64)
    elif name == "full":
        m = np.ones((H, W), dtype=np.int64)
    elif name == "two":
        m = np.where(xx < W // 2, 1, 2).astype(np.int64)
        m[rng.random((H, W)) < 0.15] = 0
        m[:, W // 3] = 255
    else:
        raise KeyError(name)
    return m[None]


FILLINGS = ("noise0.35", "noise0.5", "noise0.65", "noise0.9", "discs", "salt", "full", "two")


def classes_of(name: str):
    return (1, 2) if name == "two" else (1,)

"""The reference of the shape-descriptor tests (tests/test_shapes_host.py, tests/test_gpu_shapes.py): brute force, one label at a time.
np.nonzero for the sums, the four shifted views of the zero-padded plane `labels == k` for the bit quads, scipy.ndimage.label of the
padded complement for the holes, and direct float64 central moments sum (x - mean)^2 for the derived values.  It shares nothing with
the package's numpy path (np.add.at over all labels at once, owner corners).  The instances come from tests/instances_ref.py (scipy).
Also the case table both test files run, and the names of the kernels the cases reach."""
import functools

import numpy as np
from scipy import ndimage

import components_ref as CR
import instances_ref as IR

COLUMNS = ("sy", "sx", "syy", "sxy", "sxx", "q1", "q2", "q3", "qd", "pmax", "psum")
LDS_ROWS = 256                                          # UAPS_SHAPE_LDS_ROWS: above it the direct flush form runs
MS = (1, 3, LDS_ROWS, LDS_ROWS + 1)
# <PLANE, LDS>: every case runs with and without a plane, at M on both sides of LDS_ROWS
KERNELS = ("shape_zero_kernel",) + tuple(f"shape_accumulate_kernel<{p}, {l}>" for p in ("false", "true") for l in ("false", "true"))


def table(labels, plane, M):
    """labels int32 [B,H,W], plane int32 [B,H,W] or None -> int64 [B,M,11]."""
    B, H, W = labels.shape
    out = np.zeros((B, M, 11), dtype=np.int64)
    for b in range(B):
        top = int(min(M, labels[b].max(initial=0)))
        for k in range(1, top + 1):
            P = labels[b] == k
            if not P.any():
                continue
            y, x = (v.astype(np.int64) for v in np.nonzero(P))
            row = out[b, k - 1]
            row[0:5] = y.sum(), x.sum(), (y * y).sum(), (x * y).sum(), (x * x).sum()
            pad = np.zeros((H + 2, W + 2), dtype=np.int64)
            pad[1:-1, 1:-1] = P
            a, bb, c, d = pad[:-1, :-1], pad[:-1, 1:], pad[1:, :-1], pad[1:, 1:]
            n = a + bb + c + d
            diag = (n == 2) & (a == d)                  # two pixels, and the corners of a diagonal agree: a diagonal pair
            row[5], row[6], row[7], row[8] = (n == 1).sum(), ((n == 2) & ~diag).sum(), (n == 3).sum(), diag.sum()
            if plane is not None:
                p = np.maximum(plane[b][P].astype(np.int64), 0)
                row[9], row[10] = p.max(), p.sum()
    return out


def holes(P, connectivity):
    """The components of the complement of the binary plane P that do not reach the padding, under the complementary connectivity."""
    pad = np.ones((P.shape[0] + 2, P.shape[1] + 2), dtype=bool)
    pad[1:-1, 1:-1] = ~P
    _, n = ndimage.label(pad, structure=CR.S4 if connectivity == 8 else CR.S8)
    return n - 1


def crack_perimeter(P):
    """Pixel edges between P and anything else, the frame included."""
    pad = np.zeros((P.shape[0] + 2, P.shape[1] + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = P
    return int((pad[1:] != pad[:-1]).sum() + (pad[:, 1:] != pad[:, :-1]).sum())


def central(P):
    """Direct float64 central moments of one plane: dict var_x, var_y, cov_xy, l1, l2 (the eigenvalues by the textbook formula, with
    its subtraction)."""
    y, x = (v.astype(np.float64) for v in np.nonzero(P))
    dy, dx = y - y.mean(), x - x.mean()
    vx, vy, cxy = (dx * dx).mean(), (dy * dy).mean(), (dx * dy).mean()
    half, root = (vx + vy) / 2.0, np.sqrt(((vx - vy) / 2.0) ** 2 + cxy * cxy)
    return {"var_x": vx, "var_y": vy, "cov_xy": cxy, "l1": half + root, "l2": half - root, "centroid_y": y.mean(), "centroid_x": x.mean()}


# ------------------------------------------------------------------------------------------------ fillings: class masks [B,H,W]
def _empty(B, H, W):
    return np.zeros((B, H, W), dtype=np.int64)


def _full(B, H, W):
    return np.ones((B, H, W), dtype=np.int64)


def _checker(B, H, W):
    return np.repeat(IR.checkerboard(H, W), B, axis=0)


def _touch(B, H, W):
    """Classes 1 and 2 in blocks that share edges, and class 3 blocks that meet class 1 only at corners."""
    y, x = np.mgrid[0:H, 0:W]
    m = np.where((y // 2 + x // 3) % 2 == 0, 1, 2)
    m = np.where((y % 4 == 3) & (x % 5 == 4), 3, m)
    m = np.where((y % 4 == 2) & (x % 5 == 3), 0, m)
    return np.repeat(m[None].astype(np.int64), B, axis=0)


def _diagonals(B, H, W):
    y, x = np.mgrid[0:H, 0:W]
    m = np.where((y - x) % 7 == 0, 1, 0)
    m = np.where((y + x) % 11 == 5, 2, m)
    return np.repeat(m[None].astype(np.int64), B, axis=0)


def _edges(B, H, W):
    """Components on all four frame edges and in the corners, and one in the middle."""
    m = np.zeros((B, H, W), dtype=np.int64)
    m[:, 0, ::3] = 1
    m[:, -1, 1::4] = 2
    m[:, ::2, 0] = 3
    m[:, 1::3, -1] = 1
    m[:, 0, 0] = m[:, 0, -1] = m[:, -1, 0] = m[:, -1, -1] = 2
    m[:, H // 2, W // 2] = 3
    return m


def _noise(B, H, W):
    return IR.noise(B, H, W, 0.6, seed=5)


def _rings(B, H, W):
    return np.array(CR.rings(B, H, W))


FILLINGS = {"empty": (_empty, 8), "full": (_full, 8), "checker4": (_checker, 4), "touch": (_touch, 8), "touch4": (_touch, 4),
            "diagonals": (_diagonals, 8), "diagonals4": (_diagonals, 4), "edges": (_edges, 8), "noise": (_noise, 8), "rings": (_rings, 4)}
# (1,1,1), (1,1,65): a row crossing a wave; (3,17,129): more rows than a workgroup's 8 items and three groups a row; (1,2,2100): a
# row longer than an item's carried span in both flush forms (4 x 64 pixels in the LDS form, 16 x 64 in the direct one)
SHAPES = ((1, 1, 1), (1, 1, 65), (2, 3, 64), (1, 5, 63), (3, 17, 129), (1, 2, 2100))
FIXED = {"ring": lambda: (CR.frame(9, 70)[:, :, :], 8), "nested_rings": lambda: (CR.nested_rings(), 8),
         "nested_one_label4": lambda: (np.minimum(CR.nested_rings(), 1), 4), "comb": lambda: (IR.comb(19, 131), 4),
         "spiral": lambda: (IR.spiral(21, 67), 8)}
CASES = [(f"{name}-{B}x{H}x{W}", name, (B, H, W)) for name in FILLINGS for (B, H, W) in SHAPES] + [(name, name, None) for name in FIXED]
CASE_IDS = [c[0] for c in CASES]


class Case:
    """mask, connectivity, and per M the scipy instances (labels, count, table) of it; plane: int32 with negative values and 2^31 - 1."""

    def __init__(self, cid, name, shape):
        self.id = cid
        if shape is None:
            self.mask, self.connectivity = FIXED[name]()
        else:
            self.mask, self.connectivity = FILLINGS[name][0](*shape), FILLINGS[name][1]
        self.mask = np.ascontiguousarray(self.mask, dtype=np.int64)
        rng = np.random.default_rng(11)
        self.plane = rng.integers(-1000, 1000, self.mask.shape).astype(np.int32)
        self.plane[rng.random(self.mask.shape) < 0.05] = 2 ** 31 - 1
        self.plane[rng.random(self.mask.shape) < 0.05] = -2 ** 31
        self._inst, self._table = {}, {}

    def instances(self, M):
        if M not in self._inst:
            self._inst[M] = IR.label_batch(self.mask, connectivity=self.connectivity, max_instances=M)
        return self._inst[M]

    def table(self, M, with_plane):
        key = (M, with_plane)
        if key not in self._table:
            t = table(self.instances(M)[0], self.plane if with_plane else None, M)
            t.setflags(write=False)
            self._table[key] = t
        return self._table[key]


@functools.lru_cache(maxsize=None)
def case(cid):
    for c in CASES:
        if c[0] == cid:
            return Case(*c)
    raise KeyError(cid)
